"""What the clipping-aware entry points refuse (lfbm5d_clip_*, lfbm5d_noise_level_clipped_*, lfbm5d_declip_*, lfbm5d_denoise_clipped_*,
include/lfbm5d.h), each with a message: contexts with a shard, bad ranges and sigmas, NULL buffers and planes, sizes below 2, masks
without a SAI."""
import ctypes as C

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core, synth

H = W = 64
MASK = np.ones(9, np.uint32)
P1 = core.make_params(25.0, 2.7, 8, 18, 6, 16, 4, "id", "sadct", "haar")
P2 = core.make_params(25.0, 2.7, 16, 18, 6, 8, 4, "dct", "sadct", "haar")
TAIL = (L.ROWMAJOR, 3, 3, 1, 1, W, H, 3)
INF, NAN = float("inf"), float("nan")
BAD_RANGES = [(5.0, 5.0), (255.0, 0.0), (NAN, 255.0), (0.0, NAN), (-INF, 255.0), (0.0, INF), (1.0, 1.0 + 1e-12)]


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lf():
    import torch
    x = synth.clip_round(synth.add_noise_mt19937(synth.make_lf(3, 3, H, W).astype(np.float32).reshape(9, -1), 20.0, seed=4))
    return torch.from_numpy(x).cuda()


def _calls(c, d, out, out2):
    """Every device-form call of the stage with its range and sigma as keywords to replace."""
    return {"clip_histogram": lambda lo=0.0, hi=255.0, sigma=25.0, mask=MASK, w=W, h=H, ch=3: c.clip_histogram(d, mask, w, h, ch, lo, hi),
            "noise_level_clipped": lambda lo=0.0, hi=255.0, sigma=25.0, mask=MASK, w=W, h=H, ch=3: c.noise_level_clipped(d, mask, w, h, ch, lo, hi),
            "declip": lambda lo=0.0, hi=255.0, sigma=25.0, mask=MASK, w=W, h=H, ch=3: c.declip(sigma, d, mask, out, w, h, ch, lo, hi),
            "denoise_clipped": lambda lo=0.0, hi=255.0, sigma=25.0, mask=MASK, w=W, h=H, ch=3:
                c.denoise_clipped(sigma, P1, P2, d, mask, out, out2, L.ROWMAJOR, 3, 3, 1, 1, w, h, ch, lo, hi)}


@pytest.mark.gpu
def test_contexts_with_a_shard_are_refused(lf):
    import torch
    c = L.Context(0)
    try:
        c.set_shard(0, 2)
        for name, call in _calls(c, lf, torch.zeros_like(lf), torch.zeros_like(lf)).items():
            with pytest.raises(L.LfBm5dError, match="the clipping-aware routines run on one GPU") as e:
                call()
            assert str(e.value).startswith("lfbm5d_"), name
    finally:
        c.close()


@pytest.mark.gpu
def test_bad_ranges_sigmas_shapes_and_masks(ctx, lf):
    import torch
    out, out2 = torch.full_like(lf, -3.0), torch.full_like(lf, -3.0)
    before = lf.clone()
    calls = _calls(ctx, lf, out, out2)
    for name, call in calls.items():
        for lo, hi in BAD_RANGES:
            with pytest.raises(L.LfBm5dError, match="the range needs lo < hi, both finite"):
                call(lo=lo, hi=hi)
        for kw, text in ((dict(ch=2), "chnls must be 1 or 3"), (dict(w=1), "width and height must be at least 2"),
                         (dict(h=1), "width and height must be at least 2"), (dict(mask=np.zeros(9, np.uint32)), "no non-empty SAI")):
            with pytest.raises(L.LfBm5dError, match=text):
                call(**kw)
    for sigma in (NAN, INF, -INF):
        with pytest.raises(L.LfBm5dError, match="sigma must be finite"):
            calls["declip"](sigma=sigma)
        with pytest.raises(L.LfBm5dError, match="sigma must be finite"):
            calls["denoise_clipped"](sigma=sigma)
    for sigma in (0.0, -1.0, 1e-320):
        with pytest.raises(L.LfBm5dError, match="sigma must be finite and positive"):
            calls["declip"](sigma=sigma)
    # nothing was written, nothing was changed
    assert (out == -3.0).all() and (out2 == -3.0).all() and torch.equal(lf, before)


@pytest.mark.gpu
def test_null_buffers_and_planes(ctx, lf):
    lib, h = core.lib(), ctx._h
    mp = MASK.ctypes.data_as(C.POINTER(C.c_uint))
    p = C.c_void_p(lf.data_ptr())
    res, used = core.ClipEstimateStruct(), C.c_double()
    ull = (C.c_ulonglong * (3 * 64 * 322))()
    up = C.cast(ull, C.POINTER(C.c_ulonglong))
    msg = lambda: lib.lfbm5d_last_error(h).decode()
    assert lib.lfbm5d_clip_histogram_device(h, None, mp, 9, W, H, 3, 0.0, 255.0, up, up, up, up, None, None) == 1 and "NULL" in msg()
    assert lib.lfbm5d_clip_histogram_device(h, p, None, 9, W, H, 3, 0.0, 255.0, up, up, up, up, None, None) == 1 and "NULL" in msg()
    assert lib.lfbm5d_clip_histogram_device(h, p, mp, 9, W, H, 3, 0.0, 255.0, up, up, None, up, None, None) == 1 and "NULL" in msg()
    assert lib.lfbm5d_noise_level_clipped_device(h, None, mp, 9, W, H, 3, 0.0, 255.0, C.byref(res)) == 1 and "NULL" in msg()
    assert lib.lfbm5d_noise_level_clipped_device(h, p, mp, 9, W, H, 3, 0.0, 255.0, None) == 1 and "NULL" in msg()
    assert lib.lfbm5d_noise_level_clipped_host_sai(h, None, mp, 9, W, H, 3, 0.0, 255.0, C.byref(res)) == 1 and "NULL" in msg()
    assert lib.lfbm5d_noise_level_clipped_host_sai(h, (C.c_void_p * 9)(), mp, 9, W, H, 3, 0.0, 255.0, C.byref(res)) == 1
    assert "NULL pointer for a non-empty SAI" in msg()
    assert lib.lfbm5d_declip_device(h, 25.0, 0.0, 255.0, None, mp, p, 9, W, H, 3) == 1 and "NULL" in msg()
    assert lib.lfbm5d_declip_device(h, 25.0, 0.0, 255.0, p, mp, None, 9, W, H, 3) == 1 and "NULL" in msg()
    assert lib.lfbm5d_declip_device(h, 25.0, 0.0, 255.0, p, None, p, 9, W, H, 3) == 1 and "NULL" in msg()
    host = [np.zeros(3 * H * W, np.float32) for _ in range(9)]
    full = (C.c_void_p * 9)(*[a.ctypes.data for a in host])
    holed = (C.c_void_p * 9)(*[a.ctypes.data for a in host])
    holed[4] = None
    assert lib.lfbm5d_declip_host_sai(h, 25.0, 0.0, 255.0, full, mp, holed, 9, W, H, 3) == 1 and "NULL pointer for a non-empty SAI" in msg()
    assert lib.lfbm5d_declip_host_sai(h, 25.0, 0.0, 255.0, holed, mp, full, 9, W, H, 3) == 1 and "NULL pointer for a non-empty SAI" in msg()
    assert lib.lfbm5d_declip_host_sai(h, 25.0, 0.0, 255.0, full, mp, None, 9, W, H, 3) == 1 and "NULL" in msg()
    tail = (L.ROWMAJOR, 3, 3, 1, 1, W, H, 3)
    head = (h, 25.0, 0.0, 255.0, C.byref(res), C.byref(used))
    assert lib.lfbm5d_denoise_clipped_device(*head, None, C.byref(P2), p, mp, p, p, *tail) == 1 and "NULL" in msg()
    assert lib.lfbm5d_denoise_clipped_device(*head, C.byref(P1), C.byref(P2), None, mp, p, p, *tail) == 1 and "NULL" in msg()
    assert lib.lfbm5d_denoise_clipped_device(*head, C.byref(P1), C.byref(P2), p, mp, p, None, *tail) == 1 and "NULL" in msg()
    assert lib.lfbm5d_denoise_clipped_host_sai(*head, C.byref(P1), C.byref(P2), full, mp, holed, full, *tail) == 1
    assert "NULL pointer for a non-empty SAI" in msg()
    assert lib.lfbm5d_denoise_clipped_host_sai(*head, C.byref(P1), C.byref(P2), holed, mp, full, full, *tail) == 1
    assert "NULL pointer for a non-empty SAI" in msg()
    assert lib.lfbm5d_denoise_clipped_host_sai(*head, C.byref(P1), C.byref(P2), full, mp, full, None, *tail) == 1 and "NULL" in msg()
    # without a context there is nothing to carry a message
    assert lib.lfbm5d_declip_device(None, 25.0, 0.0, 255.0, p, mp, p, 9, W, H, 3) == 1
    assert lib.lfbm5d_noise_level_clipped_device(None, p, mp, 9, W, H, 3, 0.0, 255.0, C.byref(res)) == 1
