"""Hard-threshold decisions of the fast 3x3 chain against the reference-order form (run with -m gpu on an MI355X).

k_group_id_haar_fast (lfbm5d_group_ht.hip, the hard-thresholding step of 3x3 windows with tau_2D = id, Haar fibres and the
angular DCT / SADCT) compares an unnormalised transform chain with rescaled thresholds; a wave with a coefficient inside the
guard band of its threshold hands its (group, channel) to the list launch, which redoes it in reference-order arithmetic.  The
option ht_reference_order (LFBM5D_HT_REF_ORDER) runs the whole window in reference-order arithmetic (k_group_id_haar).  Same
window, both forms: every threshold decision must be the same, so the group weights 1 / (sigma^2 survivors) and `den` are
bit-identical and the filtered values agree to an ulp or two.  The matrix covers every kernel shape the fast chain takes
(nSx = 1, 2, 4, 8; one to four waves per group; DCT and SADCT; colour and grey; SD weights; a subset pass) at the noise levels
and data ranges where a guard band relative to the threshold alone is too narrow (tests/test_ht_guard_model.py models it).

The last cases take the 16x16 hard-threshold kernels and the general kernel, which have no fast form, to the CPU oracle at
sigma = 5 with the bounds of tests/test_gpu_parity.py (non-strict form: at most 1 % of (group, channel) pairs off by one
survivor)."""
import numpy as np
import pytest

import helpers as Hh
from oracle import oracle as O
from test_gpu_parity import _check_pass, gpu_pass

pytestmark = pytest.mark.gpu

ID8 = (8, 6, 2, 8, 3, "id", "sadct", "haar")          # the README hard-thresholding configuration, k = 8
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def ctx():
    import lfbm5d_amd as L
    c = L.Context(0)
    yield c
    c.close()


def make_window(sigma, pk, crop, grey=False, scale=1.0, offset=0.0, seed=1):
    """The golden light field cropped, as x * scale + offset, plus seeded Gaussian noise; colour-transformed and padded."""
    lf = Hh.source_lf(crop=crop).astype(np.float32)
    if grey:
        lf = lf[:, :1]
    lf = lf * np.float32(scale) + np.float32(offset)
    A, Cc = lf.shape[:2]
    noisy = O.add_noise_lf(np.ascontiguousarray(lf.reshape(A, -1)), sigma, seed=seed)
    ch, cw = (crop, crop) if np.isscalar(crop) else crop
    win, Wb, Hb = Hh.padded_window(noisy, cw, ch, Cc, pk[1] + pk[2])
    return win, Wb, Hb, Cc


# name, sigma, params, crop, grey, scale, offset, useSD; NEEDS_GUARD: cases that must send at least one (group, channel) through
# the guard band (low sigma, a 16x wider range), or they would not test it
CASES = [(f"s{s:g}-{'grey' if g else 'rgb'}", s, ID8, 64, g, 1.0, 0.0, 0) for s in (0.5, 1.0, 2.0, 5.0, 10.0, 25.0, 50.0) for g in (False, True)] + [
    ("x16-s25", 25.0, ID8, 64, False, 16.0, 0.0, 0),
    ("x256-s400", 400.0, ID8, 64, False, 256.0, 0.0, 0),                  # sigma / range of the headline
    ("bright-flat-s5", 5.0, ID8, 64, False, 0.25, 190.0, 0),
    ("x4-n8-few-s5", 5.0, ID8, 64, False, 4.0, 0.0, 0),                   # N = 8, many groups with fewer matches
    ("n1-s2", 2.0, (1, 6, 2, 8, 3, "id", "sadct", "haar"), 64, False, 1.0, 0.0, 0),
    ("n2-s2", 2.0, (2, 6, 2, 8, 3, "id", "sadct", "haar"), 64, False, 1.0, 0.0, 0),
    ("n4-s2", 2.0, (4, 6, 2, 8, 3, "id", "sadct", "haar"), 64, False, 1.0, 0.0, 0),
    ("k4-s2", 2.0, (8, 5, 2, 4, 2, "id", "sadct", "haar"), 48, False, 1.0, 0.0, 0),
    ("k12-s2", 2.0, (8, 6, 2, 12, 4, "id", "sadct", "haar"), 72, False, 1.0, 0.0, 0),
    ("k16-s2", 2.0, (8, 8, 3, 16, 4, "id", "sadct", "haar"), 96, False, 1.0, 0.0, 0),
    ("dct-s2", 2.0, (8, 6, 2, 8, 4, "id", "dct", "haar"), 64, False, 1.0, 0.0, 0),
    ("dct-x16-s25", 25.0, (8, 6, 2, 8, 4, "id", "dct", "haar"), 64, False, 16.0, 0.0, 0),
    ("usesd-s2", 2.0, ID8, 64, False, 1.0, 0.0, 1),
]
NEEDS_GUARD = {"s1-rgb", "s1-grey", "s2-rgb", "s2-grey", "x16-s25"}


def run_both(ctx, monkeypatch, sigma, pk, win, Wb, Hb, Cc, useSD=0, num=None, den=None, proc=None, pst=4):
    """The same pass twice: fast chain (default), then reference order; per run num, den, weights, group list, block matching."""
    out = []
    for ref in (False, True):
        if ref:
            monkeypatch.setenv("LFBM5D_HT_REF_ORDER", "1")
        else:
            monkeypatch.delenv("LFBM5D_HT_REF_ORDER", raising=False)
        n, d = gpu_pass(ctx, 1, sigma, pk, win, None, Wb, Hb, Cc, useSD=useSD, pst=pst,
                        num=None if num is None else num.copy(), den=None if den is None else den.copy(), proc=proc)
        refs, idx, cnt, best, shape = ctx.last_bm(pk[0], 9, Wb * Hb)
        R = len(refs)
        out.append(dict(num=n, den=d, w=ctx.last_weights(R, Cc), lst=ctx.last_group_list(), refs=refs, idx=idx, cnt=cnt,
                        best=best, shape=shape, R=R))
    monkeypatch.delenv("LFBM5D_HT_REF_ORDER", raising=False)
    return out


def guard_entries(lst):
    """entries the fast chain listed (one channel bit), as opposed to the shape pre-pass's (mask 7)"""
    return int(((lst >> 29) != 7).sum())


def check_same_decisions(name, f, r, win, Cc, useSD, range_scale):
    for key in ("refs", "idx", "cnt", "best", "shape"):   # same inputs, same block-matching kernels
        assert np.array_equal(f[key], r[key]), (name, key)
    R = f["R"]
    if useSD:
        # SD weights come from tree sums of the filtered values: close, and the survivors (den != 0) the same
        np.testing.assert_allclose(f["w"], r["w"], rtol=1e-5, atol=0, err_msg=name)
        assert np.array_equal(f["den"] != 0, r["den"] != 0), name
        np.testing.assert_allclose(f["den"], r["den"], rtol=1e-5, atol=0, err_msg=name)
    else:
        bad = np.argwhere(f["w"].view(np.uint32) != r["w"].view(np.uint32))
        assert len(bad) == 0, f"{name}: {len(bad)} of {R * Cc} (group, channel) weights differ, first {bad[:5].tolist()}"
        assert np.array_equal(f["den"].view(np.uint32), r["den"].view(np.uint32)), name
    # Filtered values: the two forms' differ by an ulp or two of the group's coefficients, i.e. by up to ~1e-6 of the data range
    # per value, whatever its own size.  So num = sum of weight * value within 4 ulp relative plus 1e-6 of the 8-bit range
    # (scaled with the data) times den, and the estimates within 1e-6 of the range.  Measured with every decision agreeing:
    # estimates up to 1.8e-4 grey levels apart (16x16 patches, sigma 2), num up to 6 ulp where num is small against den.
    # A flipped decision moves an estimate by a good fraction of a grey level (and fails the weight / den checks above).
    tol = 2.55e-4 * range_scale
    np.testing.assert_array_less(np.abs(f["num"] - r["num"]), 4 * EPS32 * np.abs(r["num"]) + tol * np.abs(r["den"]) + 1e-30, err_msg=name)
    ef, er = Hh.estimate(f["num"], f["den"], win), Hh.estimate(r["num"], r["den"], win)
    assert np.abs(ef - er).max() < tol, (name, float(np.abs(ef - er).max()))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fast_chain_decides_like_the_reference_order(ctx, monkeypatch, case):
    name, sigma, pk, crop, grey, scale, offset, useSD = case
    win, Wb, Hb, Cc = make_window(sigma, pk, crop, grey=grey, scale=scale, offset=offset)
    f, r = run_both(ctx, monkeypatch, sigma, pk, win, Wb, Hb, Cc, useSD=useSD)
    R, ng = f["R"], guard_entries(f["lst"])
    nsx = np.bincount(np.minimum(f["cnt"], 8), minlength=9)[[1, 2, 4, 8]] if pk[0] == 8 else None
    print(f"{name}: guard-band (group, channel) pairs {ng} of {R * Cc} ({100.0 * ng / max(1, R * Cc):.2f} %), "
          f"shape-adaptive groups {len(f['lst']) - ng}" + (f", match counts 1/2/4/8+ {nsx.tolist()}" if nsx is not None else ""))
    assert guard_entries(r["lst"]) == 0   # the reference-order run lists nothing but shape-adaptive groups
    if name in NEEDS_GUARD:
        assert ng >= 1, f"{name}: no (group, channel) went through the guard band: the case does not test it"
    if name == "x4-n8-few-s5":
        assert (f["cnt"] < 8).any() and (f["cnt"] == 8).any(), np.bincount(f["cnt"]).tolist()
    check_same_decisions(name, f, r, win, Cc, useSD, max(1.0, scale))


def test_fast_chain_decides_like_the_reference_order_in_a_subset_pass(ctx, monkeypatch):
    """pst != cst: greyscale window at sigma = 2, the centre pass first, then the den-aware pass of another SAI"""
    pk = ID8
    win, Wb, Hb, Cc = make_window(2.0, pk, 72, grey=True)
    num0, den0 = gpu_pass(ctx, 1, 2.0, pk, win, None, Wb, Hb, Cc)
    proc = np.zeros(9, np.uint32)
    proc[4] = 1
    for pst in (8, 1):
        f, r = run_both(ctx, monkeypatch, 2.0, pk, win, Wb, Hb, Cc, num=num0, den=den0, proc=proc, pst=pst)
        assert 0 < f["R"]
        ng = guard_entries(f["lst"])
        print(f"subset pst {pst}: guard-band (group, channel) pairs {ng} of {f['R']}")
        check_same_decisions(f"subset-pst{pst}", f, r, win, Cc, 0, 1.0)
        assert np.array_equal(f["num"][4], num0[4])


# the HT kernels without a fast form, against the CPU oracle at a low noise level (non-strict bounds of test_gpu_parity.py)
LOW_SIGMA_ORACLE = [
    ("ht-k16-bior-n8-s5", 1, 5.0, (8, 8, 3, 16, 4, "bior", "sadct", "haar"), 96, 0),
    ("ht-k16-dct-n8-s5", 1, 5.0, (8, 8, 3, 16, 4, "dct", "sadct", "haar"), 96, 0),
    ("ht-k10-dct-s5", 1, 5.0, (4, 6, 2, 10, 4, "dct", "sadct", "haar"), 72, 0),
]


@pytest.mark.parametrize("case", LOW_SIGMA_ORACLE, ids=[c[0] for c in LOW_SIGMA_ORACLE])
def test_reference_order_kernels_match_oracle_at_low_sigma(ctx, case):
    _check_pass(ctx, case, strict=False)
