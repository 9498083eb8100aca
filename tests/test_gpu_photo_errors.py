"""GPU tests of what the photometric equalisation rejects (lfbm5d_photo_*, include/lfbm5d_photo.h): every rejected argument returns 1
with its message and writes nothing: NULL buffers, overlapping input and output, C, W / H, the angular arguments, every parameter out
of range, a mask without a non-empty SAI, gains that are not finite and positive, a context with a shard."""
import ctypes as C

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core
import photo_cases as K

GEO = (L.ROWMAJOR, 3, 2, 40, 21, 3)


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    import torch
    c = K.case("2x3-row")
    return torch.from_numpy(c["lf"]).cuda(), c["mask"]


@pytest.mark.gpu
@pytest.mark.parametrize("kw,word", [
    (dict(max_disparity=9), "max_disparity"), (dict(box_radius=8), "box_radius"), (dict(ang_radius=0), "ang_radius"),
    (dict(ang_radius=3), "ang_radius"), (dict(steps=0), "steps"), (dict(steps=3), "steps"), (dict(min_sources=1), "min_sources"),
    (dict(min_sources=25), "min_sources"), (dict(max_rounds=0), "max_rounds"), (dict(max_rounds=65), "max_rounds"),
    (dict(per_channel=2), "per_channel"), (dict(anchor=6), "anchor"), (dict(min_count=0), "min_count"), (dict(tol=-1.0), "tol"),
    (dict(tol=float("nan")), "tol"), (dict(tol=float("inf")), "tol"), (dict(lo=-1.0), "lo and hi"), (dict(lo=5.0, hi=4.0), "lo and hi"),
    (dict(hi=float("inf")), "lo and hi"), (dict(hi=float("nan")), "lo and hi"), (dict(lo=float("nan")), "lo and hi")], ids=str)
def test_every_parameter_out_of_range_is_rejected(ctx, data, kw, word):
    import torch
    d, mask = data
    out = torch.zeros_like(d)
    with pytest.raises(L.LfBm5dError, match="lfbm5d_photo_device: .*" + word):
        ctx.equalise(d, mask, *GEO, out=out, **kw)
    assert not out.any().item()                                                     # nothing was written


@pytest.mark.gpu
def test_an_empty_anchor_is_rejected(ctx, data):
    d, mask = data
    m = mask.copy()
    m[1] = 0
    with pytest.raises(L.LfBm5dError, match="anchor"):
        ctx.equalise(d, m, *GEO, anchor=1)
    assert ctx.equalise(d, m, *GEO, anchor=0).gain[0].tolist() == [1.0, 1.0, 1.0]


@pytest.mark.gpu
def test_rejected_geometry_and_buffers(ctx, data):
    import torch
    d, mask = data
    out = torch.zeros_like(d)
    with pytest.raises(L.LfBm5dError, match="chnls"):
        ctx.equalise(d, mask, L.ROWMAJOR, 3, 2, 60, 21, 2, out=out)
    with pytest.raises(L.LfBm5dError, match="at least 2"):
        ctx.equalise(d, mask, L.ROWMAJOR, 3, 2, 1, 21 * 40, 3, out=out)
    with pytest.raises(L.LfBm5dError, match="ang_major"):
        ctx.equalise(d, mask, 0, 3, 2, 40, 21, 3, out=out)
    with pytest.raises(L.LfBm5dError, match="awidth and aheight"):
        ctx.equalise(d, mask, L.ROWMAJOR, 0, 2, 40, 21, 3, out=out)
    with pytest.raises(L.LfBm5dError, match="no non-empty SAI"):
        ctx.equalise(d, np.zeros(6, np.uint32), *GEO, out=out)
    with pytest.raises(L.LfBm5dError, match="must not overlap"):
        ctx.equalise(d, mask, *GEO, out=d)
    big = torch.zeros(d.numel() + 40 * 21, dtype=torch.float32, device="cuda")
    with pytest.raises(L.LfBm5dError, match="must not overlap"):                     # a partial overlap
        ctx.equalise(big[:d.numel()].view(6, -1), mask, *GEO, out=big[40 * 21:].view(6, -1))
    assert not out.any().item() and not big.any().item()
    lib, h = core.lib(), ctx._h
    up, dp = C.POINTER(C.c_uint), C.POINTER(C.c_double)
    P, res = L.photo_params(), core.PhotoResultStruct()
    gain, state = np.zeros((6, 3), np.float64), np.zeros(6, np.uint32)
    p, o, mp, gp, sp = C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr()), mask.ctypes.data_as(up), gain.ctypes.data_as(dp), state.ctypes.data_as(up)
    for args in ((None, p, mp, o, gp, sp), (C.byref(P), None, mp, o, gp, sp), (C.byref(P), p, None, o, gp, sp), (C.byref(P), p, mp, None, gp, sp),
                 (C.byref(P), p, mp, o, None, sp), (C.byref(P), p, mp, o, gp, None)):
        assert lib.lfbm5d_photo_device(h, *args, None, *GEO, C.byref(res)) == 1
        assert "lfbm5d_photo_device: NULL" in lib.lfbm5d_last_error(h).decode()
    ptrs = (C.c_void_p * 6)()                                                        # non-empty SAIs without a pointer
    assert lib.lfbm5d_photo_host_sai(h, C.byref(P), ptrs, mp, ptrs, gp, sp, None, *GEO, C.byref(res)) == 1
    assert "lfbm5d_photo_host_sai: NULL" in lib.lfbm5d_last_error(h).decode()
    assert lib.lfbm5d_photo_host_sai(h, C.byref(P), None, mp, ptrs, gp, sp, None, *GEO, C.byref(res)) == 1
    assert lib.lfbm5d_photo_device(None, C.byref(P), p, mp, o, gp, sp, None, *GEO, C.byref(res)) == 1
    assert not out.any().item()
    assert lib.lfbm5d_photo_device(h, C.byref(P), p, mp, o, gp, sp, None, *GEO, None) == 0   # everything optional is optional
    assert list(state) == [1] * 6 and (gain > 0).all() and out.any().item()


@pytest.mark.gpu
def test_rejected_apply_calls(ctx, data):
    import torch
    d, mask = data
    lib, h = core.lib(), ctx._h
    up, dp = C.POINTER(C.c_uint), C.POINTER(C.c_double)
    out = torch.zeros_like(d)
    gain = np.ones((6, 3), np.float64)
    p, o, mp, gp = C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr()), mask.ctypes.data_as(up), gain.ctypes.data_as(dp)
    tail = (3, 2, 40, 21, 3)
    for args in ((None, mp, gp, 0, o), (p, None, gp, 0, o), (p, mp, None, 0, o), (p, mp, gp, 0, None)):
        assert lib.lfbm5d_photo_apply_device(h, *args, *tail) == 1
        assert "lfbm5d_photo_apply_device: NULL" in lib.lfbm5d_last_error(h).decode()
    for bad_tail, word in (((3, 2, 40, 21, 2), "chnls"), ((3, 2, 0, 21, 3), "width and height"), ((0, 2, 40, 21, 3), "awidth and aheight")):
        assert lib.lfbm5d_photo_apply_device(h, p, mp, gp, 0, o, *bad_tail) == 1
        assert word in lib.lfbm5d_last_error(h).decode()
    assert lib.lfbm5d_photo_apply_device(h, p, mp, gp, 2, o, *tail) == 1 and "invert" in lib.lfbm5d_last_error(h).decode()
    for v in (0.0, -1.0, float("nan"), float("inf")):
        g = gain.copy()
        g[3, 2] = v
        with pytest.raises(L.LfBm5dError, match="finite and positive"):
            ctx.apply_gains(d, g, chnls=3, mask=mask, out=out)
    g = gain.copy()
    g[3, 2] = 0.0                                                                    # ... but not in an empty SAI
    m = mask.copy()
    m[3] = 0
    ctx.apply_gains(d, g, chnls=3, mask=m, out=out)
    assert out[[0, 1, 2, 4, 5]].equal(d[[0, 1, 2, 4, 5]]) and not out[3].any().item()
    out.zero_()
    with pytest.raises(L.LfBm5dError, match="no non-empty SAI"):
        ctx.apply_gains(d, gain, chnls=3, mask=np.zeros(6, np.uint32), out=out)
    big = torch.zeros(d.numel() + 4, dtype=torch.float32, device="cuda")
    with pytest.raises(L.LfBm5dError, match="d_out must be d_in or not overlap it"):
        ctx.apply_gains(big[:d.numel()].view(6, -1), gain, chnls=3, out=big[4:].view(6, -1))
    ptrs = (C.c_void_p * 6)()
    assert lib.lfbm5d_photo_apply_host_sai(h, ptrs, mp, gp, 0, ptrs, *tail) == 1
    assert "lfbm5d_photo_apply_host_sai: NULL" in lib.lfbm5d_last_error(h).decode()
    with pytest.raises(L.LfBm5dError, match="apply_gains"):
        ctx.apply_gains(d, np.ones((5, 3)), chnls=3)
    assert not out.any().item()


@pytest.mark.gpu
def test_a_context_with_a_shard_is_rejected(data):
    d, mask = data
    sharded = L.Context(0)
    try:
        sharded.set_shard(0, 2)
        with pytest.raises(L.LfBm5dError, match="one GPU"):
            sharded.equalise(d, mask, *GEO)
        with pytest.raises(L.LfBm5dError, match="one GPU"):
            sharded.apply_gains(d, np.ones((6, 3)), chnls=3)
    finally:
        sharded.close()
