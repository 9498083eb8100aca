"""GPU tests of what the joint repair rejects (lfbm5d_repair_*, include/lfbm5d_repair.h): every rejected argument returns 1 with its
message and writes nothing: NULL buffers, overlapping buffers, C, W / H, the angular arguments, every parameter out of range, a missing
SAI masked empty, a mask without a non-empty SAI, nothing to repair, a loop schedule out of range, a context with a shard."""
import ctypes as C

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core
import repair_cases as K

GEO = (L.ROWMAJOR, 3, 2, 40, 21, 3)
HT = (8, 8, 3, 8, 3, "dct", "sadct", "haar")


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    import torch
    c = K.case("2x3-row")
    return torch.from_numpy(c["lf"]).cuda(), torch.from_numpy(c["flags"]).cuda(), c["missing"], c["mask"]


@pytest.mark.gpu
@pytest.mark.parametrize("kw,word", [
    (dict(max_disparity=9), "max_disparity must be 0..8"), (dict(box_radius=8), "box_radius must be 0..7"),
    (dict(ang_radius=0), "ang_radius must be 1 or 2"), (dict(ang_radius=3), "ang_radius must be 1 or 2"),
    (dict(min_valid=0), "min_valid must be 1..24"), (dict(min_valid=25), "min_valid must be 1..24")], ids=str)
def test_every_parameter_out_of_range_is_rejected(ctx, data, kw, word):
    import torch
    d, fl, miss, mask = data
    out = torch.zeros_like(d)
    with pytest.raises(L.LfBm5dError, match="lfbm5d_repair_fill_device: " + word):
        ctx.repair_fill(d, fl, miss, mask, *GEO, out=out, **kw)
    assert not out.any().item()                                                     # nothing was written


@pytest.mark.gpu
@pytest.mark.parametrize("kw,word", [
    (dict(iterations=1001), "iterations must be at most 1000"), (dict(sigma_start=0.0), "sigma_start and sigma_end must be positive"),
    (dict(sigma_end=-1.0), "sigma_start and sigma_end must be positive"), (dict(sigma_start=float("inf")), "sigma_start and sigma_end"),
    (dict(sigma_start=4.0, sigma_end=5.0), "sigma_end must not exceed sigma_start"),
    (dict(sigma_noise=-1.0), "sigma_noise must be finite and not negative"), (dict(sigma_noise=float("nan")), "sigma_noise")], ids=str)
def test_a_schedule_out_of_range_is_rejected(ctx, data, kw, word):
    import torch
    d, fl, miss, mask = data
    out = torch.zeros_like(d)
    P = core.make_params(20.0, 2.7, *HT)
    with pytest.raises(L.LfBm5dError, match="lfbm5d_repair_device: " + word):
        ctx.repair(d, fl, miss, mask, P, L.ROWMAJOR, 3, 2, 1, 40, 21, 3, out=out, **kw)
    assert not out.any().item()


@pytest.mark.gpu
def test_rejected_geometry_buffers_and_lists(ctx, data):
    import torch
    d, fl, miss, mask = data
    out = torch.zeros_like(d)
    with pytest.raises(L.LfBm5dError, match="chnls must be 1 or 3"):
        ctx.repair_fill(d, fl, miss, mask, L.ROWMAJOR, 3, 2, 60, 21, 2, out=out)
    with pytest.raises(L.LfBm5dError, match="width and height must be at least 2"):
        ctx.repair_fill(d, fl, miss, mask, L.ROWMAJOR, 3, 2, 1, 21 * 40, 3, out=out)
    with pytest.raises(L.LfBm5dError, match="ang_major must be"):
        ctx.repair_fill(d, fl, miss, mask, 0, 3, 2, 40, 21, 3, out=out)
    with pytest.raises(L.LfBm5dError, match="awidth and aheight must be at least 1"):
        ctx.repair_fill(d, fl, miss, mask, L.ROWMAJOR, 0, 2, 40, 21, 3, out=out)
    with pytest.raises(L.LfBm5dError, match="the mask has no non-empty SAI"):
        ctx.repair_fill(d, fl, None, np.zeros(6, np.uint32), *GEO, out=out)
    m = mask.copy()
    m[4] = 0
    with pytest.raises(L.LfBm5dError, match="a missing SAI is masked empty"):
        ctx.repair_fill(d, fl, miss, m, *GEO, out=out)
    with pytest.raises(L.LfBm5dError, match="lfbm5d_repair_fill_device: nothing to repair"):
        ctx.repair_fill(d, None, None, mask, *GEO, out=out)
    with pytest.raises(L.LfBm5dError, match="nothing to repair"):
        ctx.repair_fill(d, torch.zeros_like(fl), np.zeros(6, np.uint32), mask, *GEO, out=out)
    with pytest.raises(L.LfBm5dError, match="d_out must not overlap d_in"):
        ctx.repair_fill(d, fl, miss, mask, *GEO, out=d)
    big = torch.zeros(d.numel() + 40 * 21, dtype=torch.float32, device="cuda")
    with pytest.raises(L.LfBm5dError, match="d_out must not overlap d_in"):          # a partial overlap
        ctx.repair_fill(big[:d.numel()].view(6, -1), fl, miss, mask, *GEO, out=big[40 * 21:].view(6, -1))
    with pytest.raises(L.LfBm5dError, match="d_codes must not overlap"):
        ctx.repair_fill(d, fl, miss, mask, *GEO, out=out, codes_out=fl)
    bytes_ = torch.zeros(d.numel() + 6 * 40 * 21, dtype=torch.uint8, device="cuda")
    with pytest.raises(L.LfBm5dError, match="d_disp must not overlap"):
        ctx.repair_fill(d, fl, miss, mask, *GEO, out=out, codes_out=bytes_[:d.numel()].view(6, -1),
                        disparity_out=bytes_[d.numel() - 8:d.numel() - 8 + 6 * 40 * 21].view(torch.int8).view(6, -1))
    assert not out.any().item() and not big.any().item() and not bytes_.any().item()
    lib, h = core.lib(), ctx._h
    up = C.POINTER(C.c_uint)
    P, res, HP = L.repair_params(), core.RepairResultStruct(), core.make_params(20.0, 2.7, *HT)
    p, f, o = C.c_void_p(d.data_ptr()), C.c_void_p(fl.data_ptr()), C.c_void_p(out.data_ptr())
    mp, sp = mask.ctypes.data_as(up), miss.ctypes.data_as(up)
    for args in ((None, p, f, mp, sp, o), (C.byref(P), None, f, mp, sp, o), (C.byref(P), p, f, None, sp, o), (C.byref(P), p, f, mp, sp, None)):
        assert lib.lfbm5d_repair_fill_device(h, *args, None, None, *GEO, C.byref(res)) == 1
        assert "lfbm5d_repair_fill_device: NULL pointer for a required buffer" in lib.lfbm5d_last_error(h).decode()
    assert lib.lfbm5d_repair_device(h, C.byref(P), None, p, f, mp, sp, o, None, None, L.ROWMAJOR, 3, 2, 1, 40, 21, 3, C.byref(res)) == 1
    assert "lfbm5d_repair_device: NULL pointer for a required buffer" in lib.lfbm5d_last_error(h).decode()
    ptrs = (C.c_void_p * 6)()                                                        # non-empty SAIs without a pointer
    assert lib.lfbm5d_repair_host_sai(h, C.byref(P), C.byref(HP), ptrs, None, mp, sp, ptrs, None, None, L.ROWMAJOR, 3, 2, 1, 40, 21, 3,
                                      C.byref(res)) == 1
    assert "lfbm5d_repair_host_sai: NULL pointer for a non-empty SAI" in lib.lfbm5d_last_error(h).decode()
    assert lib.lfbm5d_repair_host_sai(h, C.byref(P), C.byref(HP), None, None, mp, sp, ptrs, None, None, L.ROWMAJOR, 3, 2, 1, 40, 21, 3,
                                      C.byref(res)) == 1
    assert "lfbm5d_repair_host_sai: NULL pointer for a required buffer" in lib.lfbm5d_last_error(h).decode()
    assert lib.lfbm5d_repair_fill_device(None, C.byref(P), p, f, mp, sp, o, None, None, *GEO, C.byref(res)) == 1
    assert not out.any().item()
    assert lib.lfbm5d_repair_fill_device(h, C.byref(P), p, f, mp, None, o, None, None, *GEO, None) == 0   # everything optional is optional
    assert out.any().item()


@pytest.mark.gpu
def test_a_context_with_a_shard_is_rejected(data):
    d, fl, miss, mask = data
    sharded = L.Context(0)
    try:
        sharded.set_shard(0, 2)
        with pytest.raises(L.LfBm5dError, match="the joint repair runs on one GPU"):
            sharded.repair_fill(d, fl, miss, mask, *GEO)
    finally:
        sharded.close()
