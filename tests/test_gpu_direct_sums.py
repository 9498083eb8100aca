"""GPU tests of the direct sums of the graph form (round 8): a window of the graph has exactly one pass, so its aggregation works
straight on the light field's num / den -- tiles over the W x H interior only, from (nHW, nHW) of the padded frame -- instead of
on mirror-padded copies that k_window_begin fills and k_window_end copies back; k_window_end is left with the coverage count.
Option window_sums_padded (LFBM5D_WINDOW_SUMS_PADDED) restores the padded copies.  The bar is bit-identity of the three outputs and
of the window sequence between the two forms, for the two-step job and for the two calls, and an exact coverage count:
stats.windows == stats.passes, i.e. no job was silently redone in the sequential form."""
import numpy as np
import pytest
import torch

import helpers as Hh

pytestmark = pytest.mark.gpu

ENV = ("LFBM5D_EMULATE_WORLD", "LFBM5D_DATA_DRIVEN_SCHEDULE", "LFBM5D_STEP_SHARDING", "LFBM5D_LANES", "LFBM5D_MAX_WINDOWS", "LFBM5D_FUSED",
       "LFBM5D_BAND_MB", "LFBM5D_FORCE_REDO", "LFBM5D_WINDOW_SUMS_PADDED", "LFBM5D_HOST_BLOCKING")

# (N, nSim, nDisp, k, p, tau_2D, tau_4D, tau_5D)
HT16 = (4, 6, 2, 16, 4, "id", "sadct", "haar")      # k = 16: 16 x 4 tiles; nHW = 8 is half a tile width, so the tile grid really shifts
WIEN8 = (8, 6, 2, 8, 4, "dct", "sadct", "haar")     # k = 8: 8 x 8 windowed tiles, four candidates per lane
HT12 = (4, 6, 2, 12, 4, "dct", "sadct", "haar")     # k = 12: 16 x 4 windowed tiles
WIEN6 = (8, 6, 2, 6, 3, "dct", "sadct", "haar")     # k = 6: 8 x 8 tiles without a window


@pytest.fixture(scope="module")
def ctx():
    import lfbm5d_amd as L
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def clean_options(ctx, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    yield
    for k in ("window_sums_padded", "force_redo", "emulate_world", "band_mb", "lanes"):
        ctx.set_option(k, None)


_LF = {}


def _lf(ah, aw, Hs, Ws, grey=False):
    key = (ah, aw, Hs, Ws, grey)
    if key not in _LF:
        lf = Hh.textured_lf(ah, aw, Hs, Ws)
        if grey:
            lf = lf[:, :1]
        noisy = Hh.noisy_lf(lf, 25.0)[1]
        noisy.setflags(write=False)
        _LF[key] = noisy
    return _LF[key]


def _params(pk1, pk2, cs="opp"):
    from lfbm5d_amd import core
    return core.make_params(25.0, 2.7, *pk1, color_space=cs), core.make_params(25.0, 2.7, *pk2, color_space=cs)


def _job(ctx, P1, P2, noisy, mask, aw, ah, Ws, Hs, mj, Cc=3):
    d_n = torch.from_numpy(np.array(noisy)).cuda()
    d_b, d_d = torch.zeros_like(d_n), torch.zeros_like(d_n)
    ctx.reset_stats()
    ctx.denoise(P1, P2, d_n, mask, d_b, d_d, mj, aw, ah, 1, 1, Ws, Hs, Cc)
    return d_n.cpu().numpy(), d_b.cpu().numpy(), d_d.cpu().numpy(), ctx.last_windows(), ctx.stats()


def _calls(ctx, P1, P2, noisy, mask, aw, ah, Ws, Hs, mj, Cc=3):
    d_n = torch.from_numpy(np.array(noisy)).cuda()
    d_b, d_d = torch.zeros_like(d_n), torch.zeros_like(d_n)
    ctx.reset_stats()
    ctx.step1(P1, d_n, mask, d_b, mj, aw, ah, 1, Ws, Hs, Cc)
    w1 = ctx.last_windows()
    ctx.step2(P2, d_n, mask, d_b, d_d, mj, aw, ah, 1, Ws, Hs, Cc)
    return d_n.cpu().numpy(), d_b.cpu().numpy(), d_d.cpu().numpy(), np.concatenate([w1, ctx.last_windows()]), ctx.stats()


def _both_forms(ctx, run, *args):
    """`run` with the direct sums (default) and with the padded copies: (outputs, windows, stats) of each."""
    ctx.set_option("window_sums_padded", None)
    assert ctx.get_option("window_sums_padded") == "0"
    d = run(ctx, *args)
    ctx.set_option("window_sums_padded", 1)
    p = run(ctx, *args)
    ctx.set_option("window_sums_padded", None)
    return d, p


def _same(d, p, what):
    assert np.array_equal(d[3], p[3]), what
    for i, name in enumerate(("noisy", "basic", "denoised")):
        assert np.array_equal(d[i], p[i]), (what, name)


@pytest.mark.parametrize("holes", [(), (0,)], ids=["full", "empty-sai"])
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("major", ["row", "col"])
def test_direct_sums_equal_padded_sums_5x5(ctx, major, lanes, holes):
    """Colour 5 x 5 light field of 61 x 70 pixels: H and W divide by neither 4, 8 nor 16 (partial tiles at the far edges, the count
    region's edge inside a tile), five windows that share SAIs (sums carry from window to window); k = 16 then k = 8.  With one
    empty SAI -- the corner (0, 0): inside the window centred on (1, 1), never a window's centre, so the job stays in the graph form --
    the shape-adaptive kernels and the tiles of a skipped slot take part."""
    import lfbm5d_amd as L
    ah = aw = 5
    Hs, Ws = 61, 70
    mj = L.ROWMAJOR if major == "row" else L.COLMAJOR
    noisy = _lf(ah, aw, Hs, Ws)
    mask = np.ones(ah * aw, np.uint32)
    mask[list(holes)] = 0
    P1, P2 = _params(HT16, WIEN8)
    ctx.set_option("lanes", lanes)
    d, p = _both_forms(ctx, _job, P1, P2, noisy, mask, aw, ah, Ws, Hs, mj)
    _same(d, p, "job")
    for r in (d, p):
        assert r[4].windows == r[4].passes == len(r[3]) > 0      # exact coverage count: nothing was redone
    assert not np.array_equal(d[2][mask != 0], np.zeros_like(d[2][mask != 0]))
    dc, pc = _both_forms(ctx, _calls, P1, P2, noisy, mask, aw, ah, Ws, Hs, mj)
    _same(dc, pc, "calls")
    _same(d, dc, "job against calls")
    for r in (dc, pc):
        assert r[4].windows == r[4].passes == len(r[3])


@pytest.mark.parametrize("pk", [(HT12, WIEN6), (WIEN6[:5] + ("id", "sadct", "haar"), HT12[:5] + ("dct", "sadct", "haar"))], ids=["k12-k6", "k6-k12"])
def test_direct_sums_other_tile_variants_3x3(ctx, pk):
    """Colour 3 x 3, 48 x 52, k = 12 (16 x 4 windowed tiles) and k = 6 (8 x 8 tiles, all-ones window), each as either step."""
    import lfbm5d_amd as L
    ah = aw = 3
    Hs, Ws = 48, 52
    noisy = _lf(ah, aw, Hs, Ws)
    mask = np.ones(ah * aw, np.uint32)
    P1, P2 = _params(*pk)
    d, p = _both_forms(ctx, _job, P1, P2, noisy, mask, aw, ah, Ws, Hs, L.ROWMAJOR)
    _same(d, p, "job")
    for r in (d, p):
        assert r[4].windows == r[4].passes == len(r[3]) == 2


@pytest.mark.parametrize("opt,value", [("emulate_world", 2), ("band_mb", 1), ("agg_64bit", 1), ("agg_scalar_scan", 1)])
def test_direct_sums_under_ranks_bands_and_scan_variants(ctx, opt, value):
    """The 5 x 5 case with two emulated ranks (each rank its own light-field sums, SAIs exchanged as device copies), with every pass cut
    into bands of 1 MB of filtered patches (each band's launch adds to the light field's sums: the sums do not depend on the cut), and
    on the aggregation's 64-bit and one-candidate-per-lane variants: every one equals the padded form and the plain default."""
    import lfbm5d_amd as L
    ah = aw = 5
    Hs, Ws = 61, 70
    noisy = _lf(ah, aw, Hs, Ws)
    mask = np.ones(ah * aw, np.uint32)
    P1, P2 = _params(HT16, WIEN8)
    ref = _job(ctx, P1, P2, noisy, mask, aw, ah, Ws, Hs, L.ROWMAJOR)
    try:
        ctx.set_option(opt, value)
        d, p = _both_forms(ctx, _job, P1, P2, noisy, mask, aw, ah, Ws, Hs, L.ROWMAJOR)
    finally:
        ctx.set_option(opt, None)
    _same(d, p, opt)
    _same(d, ref, opt + " against the default")
    for r in (d, p):
        assert r[4].windows == r[4].passes == len(r[3])
    if opt == "band_mb":
        assert d[4].launches_aggregate > d[4].passes      # the passes really ran band by band


def test_forced_redo_and_greyscale_take_the_sequential_form(ctx):
    """force_redo: the graph runs (direct or padded), is declared incomplete, and the job is redone as the two calls from the light
    field as it arrived -- the result equals the undisturbed job's.  A greyscale light field never enters the graph: windows take
    further passes (stats.passes > stats.windows) on padded sums, whatever the option says."""
    import lfbm5d_amd as L
    ah = aw = 5
    Hs, Ws = 61, 70
    noisy = _lf(ah, aw, Hs, Ws)
    mask = np.ones(ah * aw, np.uint32)
    P1, P2 = _params(HT16, WIEN8)
    ref = _job(ctx, P1, P2, noisy, mask, aw, ah, Ws, Hs, L.ROWMAJOR)
    try:
        ctx.set_option("force_redo", 1)
        d, p = _both_forms(ctx, _job, P1, P2, noisy, mask, aw, ah, Ws, Hs, L.ROWMAJOR)
    finally:
        ctx.set_option("force_redo", None)
    _same(d, p, "force_redo")
    for i in range(3):                                          # (last_windows() is the second call's alone after a redo)
        assert np.array_equal(d[i], ref[i]), i
    for r in (d, p):
        assert r[4].passes > r[4].windows > 0                   # the graph's passes, then the redo's windows
    ah = aw = 3
    Hs, Ws = 48, 52
    grey = _lf(ah, aw, Hs, Ws, grey=True)
    mask = np.ones(ah * aw, np.uint32)
    d, p = _both_forms(ctx, _job, P1, P2, grey, mask, aw, ah, Ws, Hs, L.ROWMAJOR, 1)
    _same(d, p, "greyscale")
    for r in (d, p):
        assert r[4].passes > r[4].windows > 0


def test_option_reads_empty_as_off(ctx, monkeypatch):
    """LFBM5D_WINDOW_SUMS_PADDED: an empty value means off (unlike the presence flags of rounds 1-5)."""
    monkeypatch.setenv("LFBM5D_WINDOW_SUMS_PADDED", "1")
    ctx.reset_stats()
    assert ctx.get_option("window_sums_padded") == "1"
    monkeypatch.setenv("LFBM5D_WINDOW_SUMS_PADDED", "")
    ctx.reset_stats()
    assert ctx.get_option("LFBM5D_WINDOW_SUMS_PADDED") == "0"
    monkeypatch.delenv("LFBM5D_WINDOW_SUMS_PADDED")
    ctx.reset_stats()
    assert ctx.get_option("window_sums_padded") == "0"
