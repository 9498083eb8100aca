"""CPU tests of the oracle's leaf routines: against the compiled reference (outputs of lib_transforms.cpp and
mt19937ar.c, compiled unmodified, on fixed inputs: tests/golden/ref_leaf_vectors.npz, written by
tools/make_golden_leaf.py), against scipy's DCT (the published REDFT10/REDFT01 definitions) and against
structural properties the reference relies on."""
import os

import numpy as np
import pytest
import scipy.fft

from oracle import oracle as O

L = O.lib()
rng = np.random.default_rng(7)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def R():
    """The compiled reference leaf routines' outputs on fixed inputs (tests/golden/ref_leaf_vectors.npz)."""
    with np.load(os.path.join(GOLDEN, "ref_leaf_vectors.npz")) as z:
        return dict(z)


@pytest.mark.parametrize("n", [1, 2, 4, 8, 16, 32])
def test_haar_hadamard_bit_exact_vs_reference(R, n):
    vs = R[f"haar_in_{n}"]
    assert vs.shape == (20, n)
    for i, v in enumerate(vs):
        for mine, key in ((L.orc_haar_forward, "haar_fwd"), (L.orc_haar_inverse, "haar_inv"), (L.orc_hadamard, "hadamard")):
            a = v.copy()
            mine(a, n)
            assert np.array_equal(a, R[f"{key}_{n}"][i])


@pytest.mark.parametrize("n", [2, 4, 8, 16])
def test_bior_bit_exact_vs_reference(R, n):
    imgs = R[f"bior_in_{n}"]
    assert imgs.shape == (5, n + 3, n + 5)
    for i, img in enumerate(imgs):
        stride = img.shape[1]
        a = np.zeros(n * n, np.float32)
        L.orc_bior_forward(np.ascontiguousarray(img).reshape(-1), stride, a, n)
        assert np.array_equal(a, R[f"bior_fwd_{n}"][i])
        L.orc_bior_inverse(a, n)
        assert np.array_equal(a, R[f"bior_inv_{n}"][i])
        if n <= 4:   # the reference's pair reconstructs exactly only up to 4x4 (measured: not for 8/16)
            np.testing.assert_allclose(a.reshape(n, n), img[:n, :n], atol=2e-3)


def test_mt19937_res53_bit_exact_vs_reference(R):
    assert list(R["mt_seeds"]) == [1, 5489, 123456789] and R["mt_res53"].shape == (3, 2000)
    for seed, b in zip(R["mt_seeds"], R["mt_res53"]):
        L.orc_mt_seed(int(seed))
        a = [L.orc_mt_res53() for _ in range(len(b))]
        assert a == list(b)


def test_mt19937_known_answer():
    # first outputs of MT19937 with the default seed 5489 (Matsumoto & Nishimura reference output)
    L.orc_mt_seed(5489)
    assert [L.orc_mt_int32() for _ in range(3)] == [3499211612, 581869302, 3890346734]


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 12, 16])
def test_redft_matches_published_definition(n):
    x = (rng.normal(size=n) * 50).astype(np.float32)
    y = np.zeros(n, np.float32)
    L.orc_redft10(x, y, n)
    np.testing.assert_allclose(y, scipy.fft.dct(x.astype(np.float64), type=2), rtol=1e-6, atol=1e-4)
    L.orc_redft01(x, y, n)
    np.testing.assert_allclose(y, scipy.fft.dct(x.astype(np.float64), type=3), rtol=1e-6, atol=1e-4)


@pytest.mark.parametrize("k", [8, 12, 16])
def test_patch_dct_is_orthonormal_dct2(k):
    x = (rng.normal(size=(k, k)) * 50 + 100).astype(np.float32)
    y = np.zeros(k * k, np.float32)
    L.orc_dct2d_forward(x.reshape(-1), k, y, k)
    ref = scipy.fft.dctn(x.astype(np.float64), type=2, norm="ortho")
    np.testing.assert_allclose(y.reshape(k, k), ref, rtol=1e-5, atol=1e-3)
    L.orc_dct2d_inverse(y, k)
    np.testing.assert_allclose(y.reshape(k, k), x, atol=1e-3)


def test_angular_dct_is_orthonormal_and_sadct_full_shape_is_sqrt2_times_it():
    v = (rng.normal(size=9) * 30).astype(np.float32)
    a = v.copy()
    L.orc_dct4d_forward(a, 3, 3)
    np.testing.assert_allclose(a.reshape(3, 3), scipy.fft.dctn(v.reshape(3, 3).astype(np.float64), type=2, norm="ortho"),
                               rtol=1e-5, atol=1e-4)
    b = v.copy()
    md = np.zeros(9, np.uint32)
    L.orc_sadct_forward(b, np.ones(9, np.uint32), 3, 3, md)
    np.testing.assert_allclose(b, a * np.sqrt(2), rtol=1e-5, atol=1e-4)
    L.orc_dct4d_inverse(a, 3, 3)
    np.testing.assert_allclose(a, v, atol=1e-4)


def test_sadct_round_trip_all_512_masks():
    for m in range(1, 512):
        mask = np.array([(m >> i) & 1 for i in range(9)], np.uint32)
        v = (rng.normal(size=9) * 50).astype(np.float32)
        w = v.copy()
        md = np.zeros(9, np.uint32)
        L.orc_sadct_forward(w, mask, 3, 3, md)
        assert md.sum() == mask.sum()
        assert np.all(w[md == 0] == 0)
        # support is compacted to the top-left: rows left-packed, then columns top-packed
        cols = md.reshape(3, 3).sum(0)
        assert all(md.reshape(3, 3)[:cols[t], t].all() for t in range(3))
        L.orc_sadct_inverse(w, mask, 3, 3)
        np.testing.assert_allclose(w, v * mask, atol=2e-3)


def test_kaiser_window():
    w = np.zeros(64, np.float32)
    L.orc_kaiser_window(w, 8)
    w = w.reshape(8, 8)
    assert w[0, 0] == np.float32(0.1924) and w[3, 3] == np.float32(0.9718)
    assert np.array_equal(w, w[::-1]) and np.array_equal(w, w[:, ::-1]) and np.array_equal(w, w.T)
    w16 = np.zeros(256, np.float32)
    L.orc_kaiser_window(w16, 16)
    assert np.all(w16 == 1.0)  # bm3d.cpp:1144-1146: any size other than 8/12 is unwindowed


def test_symetrize_and_index_grid():
    img = np.arange(3 * 5 * 7, dtype=np.float32)
    out = np.zeros(3 * 9 * 11, np.float32)
    L.orc_symetrize(img, out, 7, 5, 3, 2)
    ref = np.pad(img.reshape(3, 5, 7), ((0, 0), (2, 2), (2, 2)), mode="symmetric")
    assert np.array_equal(out.reshape(3, 9, 11), ref)
    back = np.zeros_like(img)
    L.orc_unsymetrize(back, out, 7, 5, 3, 2)
    assert np.array_equal(back, img)
    buf = np.zeros(200, np.uint32)
    n = L.orc_ind_initialize(304 - 16 + 1, 24, 4, buf.ctypes.data)
    assert n == 61 and buf[0] == 24 and buf[n - 1] == 264 and np.all(np.diff(buf[:n]) == 4)
    n = L.orc_ind_initialize(476 - 16 + 1, 21, 3, buf.ctypes.data)   # forced last index (utilities.cpp:710-711)
    assert buf[n - 1] == 476 - 16 + 1 - 21 - 1 and buf[n - 1] - buf[n - 2] in (1, 2, 3)


def test_sigma_table_and_colour_round_trip_is_lossy_like_the_reference():
    s = np.zeros(3, np.float32)
    assert L.orc_sigma_table(25.0, 3, O.OPP, s) == 0
    np.testing.assert_allclose(s, [25 * np.sqrt(3 * 0.333 ** 2), 25 * np.sqrt(0.5), 25 * np.sqrt(0.375)], rtol=1e-6)
    img = (rng.uniform(0, 255, size=3 * 16)).astype(np.float32)
    a = img.copy()
    L.orc_color_transform(a, O.OPP, 4, 4, 3, 1)
    L.orc_color_transform(a, O.OPP, 4, 4, 3, 0)
    d = np.abs(a - img).max()
    assert 0 < d < 0.5   # 0.333/0.666/1.333 matrices are not inverses


def test_search_window_matches_reference_semantics():
    import ctypes as C
    c, mn, mx = C.c_int(), C.c_int(), C.c_int()
    for aidx, exp in ((0, (0, 0, 2)), (8, (1, 7, 9)), (16, (2, 14, 16))):
        L.orc_search_window(aidx, 17, 1, C.byref(c), C.byref(mn), C.byref(mx))
        assert (c.value, mn.value, mx.value) == exp


def test_product_noise_generator_is_the_reference_stream():
    """lfbm5d_amd.synth.add_noise_mt19937 (what bench.py feeds the GPU) against the oracle's add_noise, which is pinned
    to the compiled mt19937ar.c above: same MT19937 stream, same Box-Muller arithmetic, bit for bit."""
    from lfbm5d_amd import synth
    rng = np.random.default_rng(3)
    clean = rng.integers(0, 256, size=(4, 3, 37, 53)).astype(np.float32)
    for seed, sigma in ((1, 25.0), (7, 50.0)):
        a = O.add_noise_lf(clean.reshape(4, -1), sigma, seed=seed).reshape(clean.shape)
        b = synth.add_noise_mt19937(clean, sigma, seed=seed)
        assert np.array_equal(a, b)
