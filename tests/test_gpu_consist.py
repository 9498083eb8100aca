"""GPU tests of the consistency check (lfbm5d_consist_*, include/lfbm5d.h): flags, states, histograms, scales, thresholds, counts, rounds and
disparities equal the numpy model (tests/consist_model.py) bit for bit on the cases of tests/consist_cases.py -- planted defects and a noise
SAI (two rounds), empty and excluded SAIs at both angular radii, degenerate angular axes with untested SAIs, defects across every tile
edge and corner, non-finite values, both angular orders -- at (D, r) = (0, 0), (3, 3), (8, 7); planes that must not be written keep a
sentinel and a second call returns the same bits; the host forms and the C++ drop-in return the device form's bits; rejected calls; and
the chains consist -> inpaint and consist -> view_synth equal the same stages called with the model's map and list."""
import ctypes as C
import os

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core, synth
import consist_cases as K
import consist_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
HT = (8, 8, 3, 8, 3, "dct", "sadct", "haar")


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(ctx, c, D, r, lf=None, **more):
    import torch
    A = c["aw"] * c["ah"]
    flags = torch.full((A, c["C"] * c["H"] * c["W"]), K.FLAG_SENTINEL, dtype=torch.uint8, device="cuda")
    disp = torch.full((A, c["H"] * c["W"]), K.DISP_SENTINEL, dtype=torch.int8, device="cuda")
    d = _dev(c["lf"]) if lf is None else lf
    got = ctx.consist(d, c["mask"], c["ang_major"], c["aw"], c["ah"], c["W"], c["H"], c["C"], exclude=c["exclude"], flags_out=flags,
                      disparity_out=disp, fill_nonfinite=False, max_disparity=D, box_radius=r, **dict(c["params"], **more))
    assert got.flags is flags and got.disparity is disp
    return got, d


def _assert_equal(got, want, C_, tag):
    assert np.array_equal(got.flags.cpu().numpy(), want["flags"]), tag
    assert np.array_equal(got.disparity.cpu().numpy(), want["disp"]), tag
    assert list(got.state) == list(want["state"]), tag
    assert np.array_equal(got.hist, want["hist"]), tag
    assert list(got.scale_channel) == list(want["scale_channel"][:C_]), tag          # doubles, bit for bit
    assert np.array_equal(np.array(got.threshold, np.float32).view(np.uint32), want["threshold"][:C_].view(np.uint32)), tag
    assert np.array_equal(got.scale_sai.view(np.uint64), want["scale_sai"].view(np.uint64)), tag
    assert list(got.flagged) == list(want["counts"][:C_, 0]) and list(got.nonfinite) == list(want["counts"][:C_, 1]), tag
    assert (list(got.bad), list(got.untested), got.rounds, got.pixels, got.skipped) == \
           (want["bad"], want["untested"], want["rounds"], want["pixels"], want["skipped"]), tag


@pytest.mark.gpu
@pytest.mark.parametrize("D,r", K.DRS)
@pytest.mark.parametrize("name", K.NAMES)
def test_consist_equals_the_model(ctx, name, D, r):
    c, want = K.case(name), K.model(name, D, r)
    got, d = _run(ctx, c, D, r)
    tag = f"{name} D={D} r={r}"
    assert np.array_equal(d.cpu().numpy().view(np.uint32), c["lf"].view(np.uint32)), tag   # the input is only read
    _assert_equal(got, want, c["C"], tag)
    empty = np.nonzero(c["mask"] == 0)[0]
    assert (got.flags.cpu().numpy()[empty] == K.FLAG_SENTINEL).all()                 # empty SAIs keep the sentinel
    again, _ = _run(ctx, c, D, r, lf=d)
    _assert_equal(again, want, c["C"], tag + " (second call)")
    # what the cases are there for
    if name == "textured":
        assert want["rounds"] == 2 and want["bad"] == [5]
        if (D, r) == (3, 3):
            f = want["flags"].reshape(9, 3, 37, 70)
            assert f[4, :, 10:15, 20:25].all() and f[2, :, 15, 40].all()             # the planted defects are found
    if name.startswith("5x5"):
        assert want["state"][7] == M.EMPTY and want["state"][18] == M.EXCLUDED
    if name in ("1x3", "3x1"):
        assert want["untested"] == [0, 2] and want["tested"] == [1]
    if name == "nan":
        assert want["skipped"] == 18 + 3 + 1 and int(want["counts"][:, 1].sum()) == 22
    if name.startswith("tiles") and (D, r) == (3, 3):
        H, W = c["H"], c["W"]
        f = want["flags"].reshape(9, c["C"], H, W)
        for st, y, x, h, w in K.tile_spots(9, H, W):                                 # flagged values on every side of the tile edges
            assert f[st, :, max(y, 0):y + h, max(x, 0):x + w].all(), (st, y, x)


@pytest.mark.gpu
def test_both_angular_orders_agree(ctx):
    row, col = K.model("2x3-row", 3, 3), K.model("2x3-col", 3, 3)
    perm = [(st % 2) * 3 + st // 2 for st in range(6)]
    assert np.array_equal(col["flags"], row["flags"][perm]) and np.array_equal(col["disp"], row["disp"][perm])
    got, _ = _run(ctx, K.case("2x3-col"), 3, 3)
    assert np.array_equal(got.flags.cpu().numpy(), row["flags"][perm])


@pytest.mark.gpu
def test_rounds_and_switches(ctx):
    c = K.case("textured")
    for more in (dict(sai_factor=0.0), dict(max_rounds=1), dict(min_sources=4), dict(min_sources=9), dict(spread=1.0, k=4.0, min_threshold=3.0)):
        got, _ = _run(ctx, c, 3, 3, **more)
        want = M.consist(c["lf"], c["mask"], c["ang_major"], 3, 3, 70, 37, 3, D=3, r=3, flags=np.full(c["lf"].shape, K.FLAG_SENTINEL, np.uint8),
                         disp=np.full((9, 37 * 70), K.DISP_SENTINEL, np.int8), **dict(c["params"], **more))
        _assert_equal(got, want, 3, str(more))
    off, _ = _run(ctx, c, 3, 3, sai_factor=0.0)
    assert off.rounds == 1 and off.bad == ()
    one, _ = _run(ctx, c, 3, 3, max_rounds=1)
    assert one.rounds == 2 and one.bad == (5,)
    corners, _ = _run(ctx, c, 3, 3, min_sources=4)
    assert set(corners.untested) >= {0, 6} and not corners.flags[[0, 6]].any().item()
    none, _ = _run(ctx, c, 3, 3, min_sources=9)
    assert none.pixels == 0 and len(none.untested) == 9 and not none.flags.any().item()


@pytest.mark.gpu
def test_host_forms_and_the_drop_in_return_the_device_forms_bits(ctx):
    for name in ("textured", "5x5-R1"):
        c = K.case(name)
        A, C_, W, H = c["aw"] * c["ah"], c["C"], c["W"], c["H"]
        kw = dict(max_disparity=3, box_radius=3, **c["params"])
        geo = (c["ang_major"], c["aw"], c["ah"], W, H, C_)
        dev = ctx.consist(_dev(c["lf"]), c["mask"], *geo, exclude=c["exclude"], return_disparity=True, **kw)
        d_flags, d_disp = dev.flags.cpu().numpy(), dev.disparity.cpu().numpy()
        live = c["mask"] != 0
        assert not d_flags[~live].any()                                             # a fresh flag tensor is zero in empty SAIs
        h = ctx.consist(c["lf"].copy(), c["mask"], *geo, exclude=c["exclude"], return_disparity=True, **kw)      # a flat host array
        assert isinstance(h.flags, np.ndarray) and np.array_equal(h.flags[live], d_flags[live]) and np.array_equal(h.disparity, d_disp)
        assert list(h.state) == list(dev.state) and np.array_equal(h.hist, dev.hist) and np.array_equal(h.scale_sai, dev.scale_sai)
        assert h[3:5] == dev[3:5] and h[7:] == dev[7:]
        sais = [c["lf"][i].copy() if live[i] else None for i in range(A)]               # one array per SAI, None for empty ones
        l = L.consist(sais, c["mask"], *geo, ctx=ctx, exclude=c["exclude"], **kw)
        assert all(np.array_equal(l.flags[i], d_flags[i]) for i in range(A) if live[i]) and l.disparity is None and l[7:] == dev[7:]
        t = L.consist(_dev(c["lf"]), c["mask"], *geo, ctx=ctx, exclude=c["exclude"], **kw)                        # the module-level torch form
        assert np.array_equal(t.flags.cpu().numpy(), d_flags) and t[7:] == dev[7:]
        p = c["params"]
        cpp = core.consist_probe(c["lf"], c["mask"], c["aw"], c["ah"], W, H, C_, exclude=c["exclude"], max_disparity=3, box_radius=3,
                                 ang_radius=p["ang_radius"], min_sources=p["min_sources"], max_rounds=p["max_rounds"], k=p["k"], spread=p["spread"],
                                 sai_factor=p["sai_factor"], ang_major=c["ang_major"])
        # consist_LF has no min_scale argument: it runs at the library's default, which these cases' parameters spell out
        assert L.consist_params().min_scale == p["min_scale"]
        assert np.array_equal(cpp[0][live], d_flags[live]) and list(cpp[1]) == list(dev.state)
        assert cpp[2:7] == (sum(dev.flagged), sum(dev.nonfinite), len(dev.bad), len(dev.untested), dev.rounds)
        assert list(cpp[7][:C_]) == list(dev.scale_channel)


@pytest.mark.gpu
def test_non_finite_values_are_filled_first_by_the_wrapper(ctx):
    """With fill_nonfinite (the default) the check runs on inpaint_fill's output under an empty map and the holes get code 2."""
    import torch
    c = K.case("nan")
    geo = (c["ang_major"], 3, 3, 70, 37, 3)
    kw = dict(max_disparity=3, box_radius=3, **c["params"])
    d = _dev(c["lf"])
    holes = ~np.isfinite(c["lf"])
    got = ctx.consist(d, c["mask"], *geo, **kw)
    filled = ctx.inpaint_fill(d, torch.zeros(d.shape, dtype=torch.uint8, device="cuda"), c["mask"], 70, 37, 3).out
    assert bool(torch.isfinite(filled).all().item())
    want = M.consist(filled.cpu().numpy(), c["mask"], *geo, D=3, r=3, **c["params"])
    f = want["flags"].copy()
    f[holes] = 2
    assert np.array_equal(got.flags.cpu().numpy(), f) and got.skipped == 0 and (got.flags.cpu().numpy() == 2).sum() == holes.sum() == 22
    host = ctx.consist(c["lf"].copy(), c["mask"], *geo, **kw)
    assert np.array_equal(host.flags, f)
    assert np.array_equal(d.cpu().numpy().view(np.uint32), c["lf"].view(np.uint32))      # the input is only read


@pytest.mark.gpu
def test_rejected_calls(ctx):
    import torch
    c = K.case("2x3-row")
    d = _dev(c["lf"])
    mask = c["mask"]
    flags = torch.zeros(d.shape, dtype=torch.uint8, device="cuda")
    geo = (L.ROWMAJOR, 3, 2, 40, 21, 3)
    for kw, word in ((dict(max_disparity=9), "max_disparity"), (dict(box_radius=8), "box_radius"), (dict(ang_radius=0), "ang_radius"),
                     (dict(ang_radius=3), "ang_radius"), (dict(min_sources=1), "min_sources"), (dict(min_sources=25), "min_sources"),
                     (dict(max_rounds=0), "max_rounds"), (dict(k=-1.0), "min_threshold"), (dict(min_threshold=float("nan")), "min_threshold"),
                     (dict(spread=-1.0), "spread"), (dict(sai_factor=-0.5), "sai_factor"), (dict(min_scale=float("inf")), "min_scale")):
        with pytest.raises(L.LfBm5dError, match=word):
            ctx.consist(d, mask, *geo, flags_out=flags, **kw)
    with pytest.raises(L.LfBm5dError, match="chnls"):
        ctx.consist(d, mask, L.ROWMAJOR, 3, 2, 60, 21, 2, flags_out=flags)
    with pytest.raises(L.LfBm5dError, match="at least 2"):
        ctx.consist(d, mask, L.ROWMAJOR, 3, 2, 1, 21 * 40, 3, flags_out=flags)
    with pytest.raises(L.LfBm5dError, match="ang_major"):
        ctx.consist(d, mask, 0, 3, 2, 40, 21, 3, flags_out=flags)
    with pytest.raises(L.LfBm5dError, match="no non-empty SAI"):
        ctx.consist(d, np.zeros(6, np.uint32), *geo, flags_out=flags, fill_nonfinite=False)
    assert not flags.any().item()                                                   # nothing was written by a rejected call
    lib, h = core.lib(), ctx._h
    up = C.POINTER(C.c_uint)
    P, res = L.consist_params(min_sources=2), core.ConsistResultStruct()
    state = np.zeros(6, np.uint32)
    p, f, mp, sp = C.c_void_p(d.data_ptr()), C.c_void_p(flags.data_ptr()), mask.ctypes.data_as(up), state.ctypes.data_as(up)
    for args in ((None, p, mp, None, f, sp), (C.byref(P), None, mp, None, f, sp), (C.byref(P), p, None, None, f, sp),
                 (C.byref(P), p, mp, None, None, sp), (C.byref(P), p, mp, None, f, None)):
        assert lib.lfbm5d_consist_device(h, *args, None, None, None, *geo, C.byref(res)) == 1
        assert "NULL" in lib.lfbm5d_last_error(h).decode()
    ptrs = (C.c_void_p * 6)()                                                        # non-empty SAIs without a pointer
    assert lib.lfbm5d_consist_host_sai(h, C.byref(P), ptrs, mp, None, ptrs, sp, None, None, None, *geo, C.byref(res)) == 1
    assert "NULL" in lib.lfbm5d_last_error(h).decode()
    assert lib.lfbm5d_consist_device(h, C.byref(P), p, mp, None, f, sp, None, None, None, *geo, None) == 0   # everything optional is optional
    assert list(state) == [1] * 6
    sharded = L.Context(0)
    try:
        sharded.set_shard(0, 2)
        with pytest.raises(L.LfBm5dError, match="one GPU"):
            sharded.consist(d, mask, *geo)
    finally:
        sharded.close()


@pytest.mark.gpu
def test_chains_into_inpaint_and_view_synth(ctx):
    """64 x 64 golden crop with add_defects written as 0 / 255 and the corner SAI replaced by noise: the flags go to inpaint (fill only),
    the bad SAIs to view_synth (K = 0), and both equal the same stages called with the model's map and list."""
    clean = np.load(GOLDEN)[:, :, 80:144, 80:144].astype(np.float32)
    fl = synth.add_defects(clean.shape, seed=2)
    y = np.where(fl, np.where(clean > 127.0, np.float32(0.0), np.float32(255.0)), clean).astype(np.float32)
    y = synth.degrade_sai(y, 8, "noise", seed=3).reshape(9, -1)
    mask = np.ones(9, np.uint32)
    geo = (L.ROWMAJOR, 3, 3, 64, 64, 3)
    kw = dict(K.PARAMS)
    want = M.consist(y, mask, *geo, D=4, r=3, **kw)
    assert want["bad"] == [8] and want["flags"].any()
    d = _dev(y)
    got = ctx.consist(d, mask, *geo, max_disparity=4, box_radius=3, **kw)
    assert np.array_equal(got.flags.cpu().numpy(), want["flags"]) and list(got.bad) == want["bad"]
    assert np.array_equal(got.missing, (want["state"] == M.BAD).astype(np.uint32))
    P = core.make_params(0.0, 2.7, *HT)
    tail = (L.ROWMAJOR, 3, 3, 1, 64, 64, 3)
    a = ctx.inpaint(d, got.flags, mask, P, *tail, iterations=0)
    b = ctx.inpaint(d, _dev(want["flags"]), mask, P, *tail, iterations=0)
    assert np.array_equal(a.out.cpu().numpy().view(np.uint32), b.out.cpu().numpy().view(np.uint32)) and a[2:] == b[2:]
    va = ctx.view_synth(a.out, mask, got.missing, P, *tail, iterations=0)
    vb = ctx.view_synth(b.out, mask, (want["state"] == M.BAD).astype(np.uint32), P, *tail, iterations=0)
    assert np.array_equal(va.out.cpu().numpy().view(np.uint32), vb.out.cpu().numpy().view(np.uint32)) and va[2:] == vb[2:]
    hit = (want["flags"].reshape(fl.shape) != 0) & fl
    print(f"64 x 64 crop: {int(want['flags'].astype(bool).sum())} values flagged, {int(hit[:8].sum())} of {int(fl[:8].sum())} planted values of the "
          f"tested SAIs among them; bad SAIs {want['bad']}; synthesised SAI 8 at {M.V.psnr(va.out.cpu().numpy()[8], clean.reshape(9, -1)[8]):.2f} dB")
