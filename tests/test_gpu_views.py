"""GPU tests of the jobs with per-view noise levels (lfbm5d_*_views_*, include/lfbm5d_views.h).  The kernels are untouched -- a pass
still has one sigma -- so every check but the last is bit-identity against the plain job: a uniform table IS the plain job; a window
of a table job IS the plain job with that window's sigma; the sigmas applied are the numpy model's (tests/views_model.py); the
schedule forms agree with each other; the table does not outlive its call.  The last check is the point of the feature: on views of
different noise levels the table job beats the plain job run with the true pooled sigma."""
import functools

import numpy as np
import pytest
import torch

import helpers as Hh
import views_model as M

pytestmark = pytest.mark.gpu

ENV = ("LFBM5D_EMULATE_WORLD", "LFBM5D_DATA_DRIVEN_SCHEDULE", "LFBM5D_STEP_SHARDING", "LFBM5D_LANES", "LFBM5D_MAX_WINDOWS", "LFBM5D_FUSED")
PK1 = (4, 6, 2, 8, 4, "id", "sadct", "haar")
PK2 = (8, 6, 2, 8, 4, "dct", "sadct", "haar")
HOLES = (0, 11, 40, 62)


@pytest.fixture(scope="module")
def ctx():
    import lfbm5d_amd as L
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _plain_environment(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


@functools.lru_cache(maxsize=None)
def _lf(ah, aw, Hs=64, Ws=64, sigma=25.0):
    """(clean, noisy) [A][3*H*W] float32 with uniform noise; shared, never written."""
    clean, noisy = Hh.noisy_lf(Hh.textured_lf(ah, aw, Hs, Ws), sigma)
    clean.setflags(write=False)
    noisy.setflags(write=False)
    return clean, noisy


def _params(sigma, cs="opp"):
    from lfbm5d_amd import core
    return core.make_params(sigma, 2.7, *PK1, color_space=cs), core.make_params(sigma, 2.7, *PK2, color_space=cs)


def _mask(n, holes=()):
    m = np.ones(n, np.uint32)
    m[list(holes)] = 0
    return m


def _plain(ctx, sigma, noisy, mask, aw, ah, an, mj, W=64, H=64):
    """The existing job with one sigma: (noisy, basic, denoised, windows, window sigmas)."""
    P1, P2 = _params(sigma)
    d_n = torch.from_numpy(np.array(noisy)).cuda()
    d_b, d_d = torch.zeros_like(d_n), torch.zeros_like(d_n)
    ctx.denoise(P1, P2, d_n, mask, d_b, d_d, mj, aw, ah, an[0], an[1], W, H, 3)
    return d_n.cpu().numpy(), d_b.cpu().numpy(), d_d.cpu().numpy(), ctx.last_windows(), ctx.last_window_sigmas()


def _views(ctx, table, noisy, mask, aw, ah, an, mj, W=64, H=64):
    """The table job (P.sigma = 99: ignored): (noisy, basic, denoised, windows, window sigmas, table used)."""
    P1, P2 = _params(99.0)
    d_n = torch.from_numpy(np.array(noisy)).cuda()
    d_b, d_d = torch.zeros_like(d_n), torch.zeros_like(d_n)
    used = ctx.denoise_views(table, P1, P2, d_n, mask, d_b, d_d, mj, aw, ah, an[0], an[1], W, H, 3)
    return d_n.cpu().numpy(), d_b.cpu().numpy(), d_d.cpu().numpy(), ctx.last_windows(), ctx.last_window_sigmas(), used


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))


@pytest.mark.parametrize("lanes", ["1", "3"])
@pytest.mark.parametrize("case", [("5x5", 5, 5, ()), ("7x9-holes", 7, 9, HOLES)], ids=lambda c: c[0])
def test_uniform_table_is_the_plain_job(ctx, monkeypatch, case, lanes):
    import lfbm5d_amd as L
    name, ah, aw, holes = case
    _, noisy = _lf(ah, aw)
    mask = _mask(ah * aw, holes)
    monkeypatch.setenv("LFBM5D_LANES", lanes)
    ref = _plain(ctx, 25.0, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR)
    table = np.full(ah * aw, 25.0)
    table[list(holes)] = np.nan                                       # entries of empty SAIs are ignored
    got = _views(ctx, table, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR)
    assert _same(got, ref), (name, lanes)
    assert len(ref[3]) > 2 and np.array_equal(got[4], ref[4]) and (ref[4] == np.float32(25.0)).all() and len(ref[4]) == len(ref[3])
    assert np.array_equal(got[5][mask != 0], np.full(int(mask.sum()), 25.0)) and (got[5][mask == 0] == 0).all()


def test_one_window_is_the_plain_job_with_its_sigma(ctx):
    import lfbm5d_amd as L
    _, noisy = _lf(3, 3)
    mask = _mask(9)
    table = np.array([12.0, 31.5, 18.25, 40.0, 9.5, 22.0, 27.75, 14.0, 35.0])
    ws = L.window_sigma(table, 3, 3, 1, 1, 1)
    assert ws == M.window_sigma(table, mask, 1, 1, 1, 3, 3, L.ROWMAJOR) and ws not in table.astype(np.float32)
    got = _views(ctx, table, noisy, mask, 3, 3, (1, 1), L.ROWMAJOR)
    ref = _plain(ctx, float(ws), noisy, mask, 3, 3, (1, 1), L.ROWMAJOR)
    assert _same(got, ref)
    assert np.array_equal(got[4].view(np.uint32), np.array([ws, ws], np.float32).view(np.uint32))
    assert not np.array_equal(got[2], _plain(ctx, 25.0, noisy, mask, 3, 3, (1, 1), L.ROWMAJOR)[2])    # ... and the sigma matters


@pytest.mark.parametrize("tiles", [1, 4])
def test_first_window_of_several_is_the_plain_job_with_its_sigma(ctx, monkeypatch, tiles):
    import lfbm5d_amd as L
    ah, aw = 7, 9
    _, noisy = _lf(ah, aw)
    mask = _mask(ah * aw)
    table = M.radial_table(aw, ah, 15.0, 0.4)
    ws = M.window_sigma(table, mask, ah // 2, aw // 2, 1, aw, ah, L.ROWMAJOR)          # the first window of either step: the centre's
    monkeypatch.setenv("LFBM5D_MAX_WINDOWS", "1")
    try:
        ctx.set_tiles(tiles)
        got = _views(ctx, table, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR)
        ref = _plain(ctx, float(ws), noisy, mask, aw, ah, (1, 1), L.ROWMAJOR)
    finally:
        ctx.set_tiles(1)
    assert _same(got, ref), tiles
    # (tile mode runs the two calls: the windows on record are the second step's)
    assert len(got[3]) == (2 if tiles == 1 else 1) and (got[4].view(np.uint32) == np.float32(ws).view(np.uint32)).all()
    assert not np.array_equal(got[2], noisy)


SIGMA_CASES = [
    ("7x9-holes", 7, 9, HOLES, "row", (1, 1)),
    ("7x9-holes-col", 7, 9, HOLES, "col", (1, 1)),
    ("7x9-an-2-1", 7, 9, (), "row", (2, 1)),
    ("7x9-holes-col-an-2-1", 7, 9, HOLES, "col", (2, 1)),
]


@pytest.mark.parametrize("case", SIGMA_CASES, ids=[c[0] for c in SIGMA_CASES])
def test_recorded_window_sigmas_equal_the_model(ctx, case):
    import lfbm5d_amd as L
    from lfbm5d_amd import core
    name, ah, aw, holes, major, an = case
    mj = L.ROWMAJOR if major == "row" else L.COLMAJOR
    _, noisy = _lf(ah, aw)
    mask = _mask(ah * aw, holes)
    table = M.radial_table(aw, ah, 15.0, 0.4, mj)
    got = _views(ctx, table, noisy, mask, aw, ah, an, mj)
    want = np.concatenate([M.window_sigmas(table, mask, aw, ah, a, mj) for a in an])
    plan = np.concatenate([core.plan_windows(aw, ah, a, mj, mask) for a in an])
    assert np.array_equal(got[3], plan)
    assert np.array_equal(got[4].view(np.uint32), want.view(np.uint32)), name
    assert len(set(want.tolist())) > 3


def test_schedule_forms_agree(ctx, monkeypatch):
    """One lane, three lanes, the two calls behind the job's entry point, the two step entry points, and 2, 3 and 4 ranks played on
    this GPU: one result."""
    import lfbm5d_amd as L
    ah, aw = 7, 9
    _, noisy = _lf(ah, aw)
    mask = _mask(ah * aw, HOLES)
    table = M.radial_table(aw, ah, 15.0, 0.4)
    monkeypatch.setenv("LFBM5D_LANES", "1")
    ref = _views(ctx, table, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR)
    assert not _same(ref, _plain(ctx, 25.0, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR))
    monkeypatch.setenv("LFBM5D_LANES", "3")
    assert _same(_views(ctx, table, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR), ref)
    monkeypatch.delenv("LFBM5D_LANES")
    monkeypatch.setenv("LFBM5D_FUSED", "0")
    two = _views(ctx, table, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR)
    assert all(np.array_equal(x, y) for x, y in zip(two[:3], ref[:3]))
    assert np.array_equal(two[4].view(np.uint32), ref[4][len(ref[4]) // 2:].view(np.uint32))   # (the second call's windows are on record)
    monkeypatch.delenv("LFBM5D_FUSED")
    # step1_views followed by step2_views
    P1, P2 = _params(99.0)
    d_n = torch.from_numpy(np.array(noisy)).cuda()
    d_b, d_d = torch.zeros_like(d_n), torch.zeros_like(d_n)
    u1 = ctx.step1_views(table, P1, d_n, mask, d_b, L.ROWMAJOR, aw, ah, 1, 64, 64, 3)
    s1 = ctx.last_window_sigmas()
    u2 = ctx.step2_views(table, P2, d_n, mask, d_b, d_d, L.ROWMAJOR, aw, ah, 1, 64, 64, 3)
    s2 = ctx.last_window_sigmas()
    assert np.array_equal(d_n.cpu().numpy(), ref[0]) and np.array_equal(d_b.cpu().numpy(), ref[1]) and np.array_equal(d_d.cpu().numpy(), ref[2])
    assert np.array_equal(np.concatenate([s1, s2]).view(np.uint32), ref[4].view(np.uint32))
    assert np.array_equal(u1, ref[5]) and np.array_equal(u2, ref[5])
    for n in (2, 3, 4):
        monkeypatch.setenv("LFBM5D_EMULATE_WORLD", str(n))
        got = _views(ctx, table, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR)
        assert _same(got, ref) and np.array_equal(got[4].view(np.uint32), ref[4].view(np.uint32)), n


def test_greyscale_windows_take_their_further_passes_at_the_window_sigma(ctx):
    """Greyscale light fields run window after window with data-driven further passes (the two calls behind the job's entry point):
    every pass of a window runs at the window's sigma."""
    import lfbm5d_amd as L

    def job(noisy, ah, aw, table, sigma):
        P1, P2 = _params(sigma)
        d_n = torch.from_numpy(noisy).cuda()
        d_b, d_d = torch.zeros_like(d_n), torch.zeros_like(d_n)
        ctx.reset_stats()
        tail = (_mask(ah * aw), d_b, d_d, L.ROWMAJOR, aw, ah, 1, 1, 48, 48, 1)
        if table is None:
            ctx.denoise(P1, P2, d_n, *tail)
        else:
            ctx.denoise_views(table, P1, P2, d_n, *tail)
        s = ctx.stats()
        return d_n.cpu().numpy(), d_b.cpu().numpy(), d_d.cpu().numpy(), ctx.last_windows(), ctx.last_window_sigmas(), s.passes, s.windows
    # one window, any table: the plain job at the window's sigma, further passes included
    _, noisy = Hh.noisy_lf(Hh.textured_lf(3, 3, 48, 48)[:, :1], 25.0)
    table = np.array([12.0, 31.5, 18.25, 40.0, 9.5, 22.0, 27.75, 14.0, 35.0])
    ref = job(noisy, 3, 3, None, float(L.window_sigma(table, 3, 3, 1, 1, 1)))
    assert ref[5] > ref[6]                                            # further passes do happen here
    assert _same(job(noisy, 3, 3, table, 99.0), ref)
    # several windows: a uniform table is the plain job, a radial one runs every window at the model's sigma
    ah, aw = 3, 5
    _, noisy = Hh.noisy_lf(Hh.textured_lf(ah, aw, 48, 48)[:, :1], 25.0)
    ref = job(noisy, ah, aw, None, 25.0)
    assert ref[5] > ref[6] and _same(job(noisy, ah, aw, np.full(ah * aw, 25.0), 99.0), ref)
    table = M.radial_table(aw, ah, 15.0, 0.4)
    got = job(noisy, ah, aw, table, 99.0)
    assert np.array_equal(got[4].view(np.uint32), M.window_sigmas(table, _mask(ah * aw), aw, ah, 1, L.ROWMAJOR).view(np.uint32))   # (the second call's)
    assert not np.array_equal(got[2], ref[2])


def test_host_form_and_the_drop_in_equal_the_device_form(ctx):
    import lfbm5d_amd as L
    from lfbm5d_amd import core
    ah, aw = 5, 5
    _, noisy = _lf(ah, aw)
    mask = _mask(ah * aw, (3,))
    table = M.radial_table(aw, ah, 20.0, 0.5)
    ref = _views(ctx, table, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR)
    P1, P2 = _params(99.0)
    h_n = np.array(noisy)
    h_b, h_d = np.zeros_like(h_n), np.zeros_like(h_n)
    used = ctx.denoise_views(table, P1, P2, h_n, mask, h_b, h_d, L.ROWMAJOR, aw, ah, 1, 1, 64, 64, 3)
    keep = mask != 0
    assert np.array_equal(h_n[keep], ref[0][keep]) and np.array_equal(h_b[keep], ref[1][keep]) and np.array_equal(h_d[keep], ref[2][keep])
    assert np.array_equal(used, ref[5])
    n, b, d, used, ws = core.denoise_views_probe(np.array(noisy), mask, table, aw, ah, 64, 64, 3, 2.7, PK1, PK2)
    assert np.array_equal(n[keep], ref[0][keep]) and np.array_equal(b[keep], ref[1][keep]) and np.array_equal(d[keep], ref[2][keep])
    assert np.array_equal(used, ref[5]) and np.array_equal(ws.view(np.uint32), ref[4].view(np.uint32))


def test_bm3d_lf_views_filters_every_sai_with_its_own_sigma(ctx):
    from lfbm5d_amd import core
    _, noisy = _lf(3, 3)
    mask = _mask(9, (2,))
    table = np.array([12.0, 31.5, 18.25, 40.0, 9.5, 22.0, 27.75, 14.0, 35.0])
    bm = lambda s: (core.make_bm3d_params(s, 2.7, 8, 6, 8, 3, "bior"), core.make_bm3d_params(s, 2.7, 8, 6, 8, 3, "dct"))
    d_n = torch.from_numpy(np.array(noisy)).cuda()
    d_b, d_d = torch.zeros_like(d_n), torch.zeros_like(d_n)
    hard, wien = bm(99.0)
    wien.sigma = 77.0                                                  # both ignored
    used = ctx.bm3d_lf_views(table, hard, wien, d_n, mask, d_b, d_d, 64, 64, 3)
    assert np.array_equal(used[mask != 0], table[mask != 0]) and used[2] == 0
    for v in range(9):
        if not mask[v]:
            continue
        one = np.zeros(9, np.uint32)
        one[v] = 1
        e_n = torch.from_numpy(np.array(noisy)).cuda()
        e_b, e_d = torch.zeros_like(e_n), torch.zeros_like(e_n)
        ctx.bm3d_lf(*bm(float(table[v])), e_n, one, e_b, e_d, 64, 64, 3)
        assert torch.equal(e_n[v], d_n[v]) and torch.equal(e_b[v], d_b[v]) and torch.equal(e_d[v], d_d[v]), v
    assert not torch.equal(d_d[0], d_d[1])


def test_table_does_not_outlive_its_call(ctx):
    import lfbm5d_amd as L
    ah, aw = 5, 5
    _, noisy = _lf(ah, aw)
    mask = _mask(ah * aw, (3,))
    table = M.radial_table(aw, ah, 15.0, 0.4)
    fresh = L.Context(0)
    try:
        ref = _plain(fresh, 25.0, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR)
    finally:
        fresh.close()
    with_table = _views(ctx, table, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR)
    assert not np.array_equal(with_table[2], ref[2])
    after = _plain(ctx, 25.0, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR)
    assert _same(after, ref) and (after[4] == np.float32(25.0)).all()
    # a call that fails on its table leaves nothing behind either; the empty SAI's entry may be anything
    for bad in (np.nan, 0.0, -4.0, np.inf):
        t = table.copy()
        t[3] = bad
        assert _same(_views(ctx, t, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR), with_table)
        t[17] = bad
        with pytest.raises(L.LfBm5dError, match=r"sigma_sai\[17\]"):
            _views(ctx, t, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR)
        assert _same(_plain(ctx, 25.0, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR), ref), bad
    # ... nor does a job that fails behind a good table (an angular window larger than the light field)
    with pytest.raises(L.LfBm5dError):
        _views(ctx, table, noisy, mask, aw, ah, (3, 3), L.ROWMAJOR)
    assert _same(_plain(ctx, 25.0, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR), ref)


def test_null_table_takes_the_per_sai_estimate(ctx):
    import lfbm5d_amd as L
    ah, aw = 5, 5
    clean, _ = _lf(ah, aw)
    mask = _mask(ah * aw, (3,))
    true = M.radial_table(aw, ah, 15.0, 0.4)
    noisy = L.add_view_noise(clean, true, seed=3)
    est = ctx.noise_level(torch.from_numpy(noisy).cuda(), mask, 64, 64, 3, per_sai=True).sigma_sai
    got = _views(ctx, None, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR)
    assert np.array_equal(got[5].view(np.uint64), est.view(np.uint64)) and got[5][3] == 0
    assert _same(_views(ctx, est, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR), got)
    keep = mask != 0
    print("per-SAI estimate / true sigma: min %.3f max %.3f" % ((est[keep] / true[keep]).min(), (est[keep] / true[keep]).max()))
    assert len(set(got[4].tolist())) > 1


def _psnr_sai(x, clean):
    mse = ((x.astype(np.float64) - clean.astype(np.float64)) ** 2).mean(axis=1)
    return 10.0 * np.log10(255.0 ** 2 / mse)


def test_true_table_beats_the_true_pooled_sigma(ctx):
    """textured_lf(7, 7, 64, 64) under the noise a devignetted capture carries, sigma_v = 15 / vignette(edge 0.4): the mean PSNR over
    the views of the table job is higher than that of the existing job run with the true pooled (root mean square) sigma.  The
    yardstick is the existing job; the condition is gain > 0.  Measured on an MI355X (profiles/views.txt): +0.52 dB, 35.126 -> 35.648;
    per ring of views from the centre outwards +1.98, +1.45, +0.43, +0.21 dB."""
    import lfbm5d_amd as L
    from lfbm5d_amd import synth
    ah = aw = 7
    clean = np.ascontiguousarray(Hh.textured_lf(ah, aw, 64, 64).astype(np.float32)).reshape(ah * aw, -1)
    table = 15.0 / synth.vignette_gains(aw, ah, 0.4)
    assert np.array_equal(table, M.radial_table(aw, ah, 15.0, 0.4))
    noisy = L.add_view_noise(clean, table, seed=1)
    mask = _mask(ah * aw)
    pooled = float(np.sqrt((table ** 2).mean()))
    plain = _psnr_sai(_plain(ctx, pooled, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR)[2], clean)
    views = _psnr_sai(_views(ctx, table, noisy, mask, aw, ah, (1, 1), L.ROWMAJOR)[2], clean)
    s, t = np.mgrid[0:ah, 0:aw]
    ring = np.maximum(abs(s - ah // 2), abs(t - aw // 2)).reshape(-1)
    for r in range(ah // 2 + 1):
        print("ring %d: sigma %.2f..%.2f  plain %.3f dB  views %.3f dB  gain %+.3f dB" % (
            r, table[ring == r].min(), table[ring == r].max(), plain[ring == r].mean(), views[ring == r].mean(),
            (views - plain)[ring == r].mean()))
    print("pooled sigma %.3f  mean PSNR plain %.4f dB  views %.4f dB  gain %+.4f dB" % (pooled, plain.mean(), views.mean(), views.mean() - plain.mean()))
    assert views.mean() - plain.mean() > 0
