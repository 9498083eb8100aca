"""The register-resident selection on an unfilled score table (k_self_select_regs, lfbm5d_pass.hip) against the form of rounds 1-8
(option select_prefill: `scores` filled with 2 thr in front of the table kernel, k_self_select): self_idx[:cnt], self_cnt, num and
den of one core pass, bit for bit.

3 x 3 light fields of 64 x 64 pixels.  With nSim = 18, nDisp = 6 the padded window is 112 x 112 and EVERY reference patch lies
within nSim of a border, so backward entries the table kernel never writes are the rule, and whatever the score buffer held before
(an earlier pass, fresh memory) sits where the old form had 2 thr."""
import numpy as np
import pytest

import helpers as Hh
from test_gpu_parity import gpu_pass

pytestmark = pytest.mark.gpu

CROP = 64


@pytest.fixture(scope="module")
def ctx():
    import lfbm5d_amd as L
    c = L.Context(0)
    yield c
    c.close()


def _window(pk, sigma=25.0, seed=1, scale=1.0, flat=False):
    lf = Hh.source_lf(crop=CROP)
    if flat:
        noisy = np.full((lf.shape[0], lf[0].size), 128.0, np.float32)
    else:
        _, noisy = Hh.noisy_lf(lf, sigma, seed=seed)
        noisy = np.ascontiguousarray((noisy * scale).astype(np.float32))
    win, Wb, Hb = Hh.padded_window(noisy, CROP, CROP, lf.shape[1], pk[1] + pk[2])
    return win, Wb, Hb, lf.shape[1]


def _pass(ctx, old, step, sigma, pk, win, Wb, Hb, Cc, want_fast=True):
    """One pass in either form: (num, den, idx masked to its used entries, cnt, refs)."""
    basic = np.ascontiguousarray(0.5 * win + 0.5 * np.roll(win, 1, axis=1)) if step == 2 else None
    ctx.set_option("select_prefill", 1 if old else None)
    try:
        num, den = gpu_pass(ctx, step, sigma, pk, win, basic, Wb, Hb, Cc)
        if want_fast:
            assert ctx.last_scan_version() >= 2     # the ring-sharing table kernel: the default form leaves the fill out
        refs, idx, cnt, _, _ = ctx.last_bm(pk[0], win.shape[0], Wb * Hb)
    finally:
        ctx.set_option("select_prefill", None)
    used = np.arange(idx.shape[1])[None, :] < cnt[:, None]
    return num, den, np.where(used, idx, 0), cnt, refs


def _same(a, b):
    for x, y, what in zip(a, b, ("num", "den", "self_idx", "self_cnt", "refs")):
        assert x.dtype == y.dtype and x.shape == y.shape, what
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, int((x.view(np.uint32) != y.view(np.uint32)).sum()))


# name, step, (N, nSim, nDisp, k, p, tau_2D, tau_4D, tau_5D).  p = 3 and 5 put the forced last grid row / column off the pattern
# nHW + i p; nSim = 3: 49 candidates, fewer than a wavefront's lanes; nSim = 18: 1 369 candidates, 22 rows per lane
CASES = [
    ("ht-k16-n8-p4", 1, (8, 18, 6, 16, 4, "id", "sadct", "haar")),
    ("wien-k8-n16-p4", 2, (16, 18, 6, 8, 4, "dct", "sadct", "haar")),
    ("ht-k8-n2-p3", 1, (2, 18, 6, 8, 3, "id", "sadct", "haar")),
    ("wien-k8-n32-p5", 2, (32, 18, 6, 8, 5, "dct", "sadct", "haar")),
    ("ht-k16-n16-p3", 1, (16, 18, 6, 16, 3, "id", "sadct", "haar")),
    ("wien-k16-n2-p5", 2, (2, 18, 6, 16, 5, "dct", "sadct", "haar")),
    ("ht-k8-n8-p5", 1, (8, 18, 6, 8, 5, "id", "sadct", "haar")),
    ("ht-k16-n32-p5-nsim3", 1, (32, 3, 6, 16, 5, "id", "sadct", "haar")),
    ("wien-k8-n8-p4-nsim3", 2, (8, 3, 6, 8, 4, "dct", "sadct", "haar")),
    ("ht-k8-n16-p3-nsim3", 1, (16, 3, 6, 8, 3, "id", "sadct", "haar")),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_default_selection_equals_the_prefilled_form(ctx, case):
    _, step, pk = case
    win, Wb, Hb, Cc = _window(pk)
    new = _pass(ctx, False, step, 25.0, pk, win, Wb, Hb, Cc)
    old = _pass(ctx, True, step, 25.0, pk, win, Wb, Hb, Cc)
    _same(new, old)
    assert (new[3] == pk[0]).any()     # full groups: more candidates pass than a group takes


@pytest.mark.parametrize("k,N", [(8, 16), (16, 8)])
def test_flat_image_all_ties(ctx, k, N):
    """Every score is 0: the selection is scan order alone, and every candidate ties with the pruning bound."""
    pk = (N, 18, 6, k, 4, "id", "sadct", "haar")
    win, Wb, Hb, Cc = _window(pk, flat=True)
    new = _pass(ctx, False, 1, 25.0, pk, win, Wb, Hb, Cc)
    old = _pass(ctx, True, 1, 25.0, pk, win, Wb, Hb, Cc)
    _same(new, old)
    assert (new[3] == N).all()


def test_few_candidates_pass_the_threshold(ctx):
    """The window scaled until the threshold is low against the noise: groups of the duplicated reference alone (self_cnt 2: the
    `cnt == 0` rule and nSx = 1 both write that; a finite table cannot reach cnt == 0 itself, a patch's distance to itself is an
    exact 0), groups truncated to a power of two below N, and full ones."""
    pk = (16, 18, 6, 8, 4, "id", "sadct", "haar")
    win, Wb, Hb, Cc = _window(pk, scale=2.2)
    new = _pass(ctx, False, 1, 25.0, pk, win, Wb, Hb, Cc)
    old = _pass(ctx, True, 1, 25.0, pk, win, Wb, Hb, Cc)
    _same(new, old)
    cnt = new[3]
    assert (cnt == 2).any() and ((cnt > 2) & (cnt < 16)).any() and np.isin(cnt, (2, 4, 8, 16)).all()


def test_nothing_is_taken_from_an_earlier_pass(ctx):
    """Stale buffer: a pass at sigma 40, then on the same context one at sigma 10 with another noise seed and another step p --
    thr and the number of reference patches both change.  The second pass's tables and sums equal those of a fresh context
    running the prefilled form."""
    import lfbm5d_amd as L
    pk1, pk2 = (16, 18, 6, 8, 4, "id", "sadct", "haar"), (16, 18, 6, 8, 3, "id", "sadct", "haar")
    w1 = _window(pk1, sigma=40.0, seed=1)
    w2 = _window(pk2, sigma=10.0, seed=2)
    _pass(ctx, False, 1, 40.0, pk1, *w1)
    new = _pass(ctx, False, 1, 10.0, pk2, *w2)
    fresh = L.Context(0)
    try:
        old = _pass(fresh, True, 1, 10.0, pk2, *w2)
    finally:
        fresh.close()
    _same(new, old)


def test_last_scores_reads_like_a_filled_table(ctx):
    """lfbm5d_last_scores after a default pass (k = 8, fast path) is the prefilled form's table, entry for entry."""
    pk = (16, 18, 6, 8, 4, "id", "sadct", "haar")
    win, Wb, Hb, Cc = _window(pk)
    ncand = (2 * pk[1] + 1) ** 2
    other = (16, 18, 6, 8, 5, "id", "sadct", "haar")
    _pass(ctx, True, 1, 40.0, other, *_window(other, sigma=40.0))     # (the buffer holds another geometry's fill and scores)
    new = _pass(ctx, False, 1, 25.0, pk, win, Wb, Hb, Cc)
    s_new = ctx.last_scores(len(new[4]) * ncand)
    old = _pass(ctx, True, 1, 25.0, pk, win, Wb, Hb, Cc)
    s_old = ctx.last_scores(len(old[4]) * ncand)
    assert s_new.size == len(new[4]) * ncand == s_old.size
    assert np.array_equal(s_new.view(np.uint32), s_old.view(np.uint32))
    thr2 = np.float32(2 * Hh.tau_match(25.0, Cc, 1) * 8 * 8)
    assert (s_old == thr2).mean() > 0.1     # unwritten entries are the rule in this window
