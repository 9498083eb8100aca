"""CPU tests of the impulse repair (lfbm5d_impulse_*, include/lfbm5d.h): the exports and struct sizes, the host-only quantile against
the numpy model (tests/impulse_model.py), what the definition achieves on the golden light field, the synthetic impulses, and the CLIs'
parsing of LFBM5D_IMPULSE / LFBM5D_IMPULSE_ADD."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core, synth
import impulse_model as M
import noise_model as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")


def test_library_exports_the_impulse_entry_points():
    lib = C.CDLL(core.library_path())
    for n in ("lfbm5d_impulse_defaults", "lfbm5d_impulse_histogram_device", "lfbm5d_impulse_scale", "lfbm5d_impulse_repair_device",
              "lfbm5d_impulse_repair_flags_device", "lfbm5d_impulse_repair_host_sai"):
        assert hasattr(lib, n), n
    assert C.sizeof(core.ImpulseParamsStruct) == 5 * 8
    assert C.sizeof(core.ImpulseResultStruct) == 7 * 8 + 11 * 8
    assert core.IMPULSE_KEYS == M.Q == 386
    P = L.impulse_params()
    assert (P.k, P.min_threshold, list(P.threshold)) == (8.0, 0.0, [0.0, 0.0, 0.0])
    hdr = open(os.path.join(ROOT, "include", "lfbm5d.h")).read()
    assert "#define LFBM5D_IMPULSE_KEYS 386" in hdr
    for n in ("impulse_repair", "impulse_scale", "impulse_params", "ImpulseRepair"):
        assert n in L.__all__


@pytest.fixture(scope="module")
def golden_case():
    """The golden light field + sigma 5 Gaussian noise (default_rng(7)) + 0.5 % salt and pepper (add_impulse seed 7), the model's repair
    with k = 8 and the blind sigma of the three light fields (noise_model), computed once."""
    lf = np.load(GOLDEN).astype(np.float32).reshape(9, -1)
    mask = np.ones(9, np.uint32)
    z = (lf + np.random.default_rng(7).normal(0.0, 5.0, lf.shape)).astype(np.float32)
    d, hit = synth.add_impulse(z, 0.005, seed=7)
    r = M.repair(d, mask, 256, 256, 3, k=8.0)
    est = [N.model(x, mask, 256, 256, 3)["sigma"] for x in (z, d, r["out"])]
    return z, d, hit, r, est


def test_the_definition_on_the_golden_light_field(golden_case):
    z, d, hit, r, est = golden_case
    flagged = r["flags"] != 0
    effective = hit & (np.abs(d - z) > 3 * 5.0 + 20.0)
    recall = (flagged & effective).sum() / effective.sum()
    false_pos = (flagged & ~hit).sum() / (~hit).sum()
    print(f"recall {recall:.4f}, false positives {false_pos:.2e}, sigma undamaged {est[0]:.3f}, damaged {est[1]:.3f}, repaired {est[2]:.3f}, "
          f"thresholds {r['threshold']}, scale {r['scale']:.4f}")
    assert recall >= 0.98
    assert false_pos <= 2e-3
    assert abs(est[2] / est[0] - 1.0) <= 0.05
    assert est[1] > 1.5 * est[0]
    # bookkeeping of the model itself
    assert int(r["hist"].sum()) == r["pixels"] - r["skipped"] == d.size
    assert np.array_equal(r["flagged"], r["repaired"] + r["left"]) and int(r["flagged"].sum()) == int(flagged.sum())
    assert np.array_equal(r["out"][~flagged], d[~flagged])                    # unflagged values are copied


def test_scale_matches_the_model(golden_case):
    r = golden_case[3]
    hists = [r["hist"][0], r["hist"].sum(axis=0)]
    h = np.zeros(M.Q, np.uint64)
    h[0] = 1000                                                               # all the mass in key 0: inside [0, 2^-12)
    hists.append(h.copy())
    h[0], h[200], h[201] = 10, 7, 4                                           # an odd count: T falls inside a bin
    hists.append(h.copy())
    h[:] = 0
    h[M.Q - 1] = 5                                                            # the last key has no upper edge: its lower edge
    hists.append(h.copy())
    for h in hists:
        got, want = L.impulse_scale(h), M.scale(h)
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    assert L.impulse_scale(hists[2]) == 0.5 * 2.0 ** -12
    assert L.impulse_scale(hists[4]) == 4096.0
    empty = np.zeros(M.Q, np.uint64)
    assert M.scale(empty) is None
    with pytest.raises(L.LfBm5dError):
        L.impulse_scale(empty)
    s = C.c_double()
    lib = core.lib()
    assert lib.lfbm5d_impulse_scale(empty.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(s)) == 1
    assert lib.lfbm5d_impulse_scale(None, C.byref(s)) == 1
    with pytest.raises(L.LfBm5dError):
        L.impulse_scale(np.zeros(385, np.uint64))


def test_model_edge_cases():
    """Planted cases on a 5 x 6 plane: the mirror at a corner, a same-valued pair, a NaN centre, a NaN neighbour, a flagged 3 x 3."""
    I = np.full((5, 6), 100.0, np.float32)
    I += np.arange(30, dtype=np.float32).reshape(5, 6) % 3                     # a little texture: R of sound pixels is 0..4
    J = I.copy()
    J[0, 0] = 255.0                                                            # corner
    J[2, 2] = J[2, 3] = 0.0                                                    # horizontal pair of one value
    J[4, 5] = np.nan
    f = M.detect_plane(J, 50.0)
    want = np.zeros((5, 6), bool)
    want[0, 0] = want[2, 2] = want[2, 3] = want[4, 5] = True
    assert np.array_equal(f, want)
    out, code = M.repair_plane(J, f)
    assert np.array_equal(code != 0, want) and (code[want] == 1).all()
    assert np.isfinite(out).all() and (np.abs(out - I) <= 2.0).all()
    # R of the corner: its eight mirrored neighbours are (0,1) x2, (1,0) x2, (1,1) x4
    R, extreme = M.road(J)
    d = sorted([abs(255.0 - J[0, 1])] * 2 + [abs(255.0 - J[1, 0])] * 2 + [abs(255.0 - J[1, 1])] * 4)
    assert R[0, 0] == np.float32(sum(d[:4])) and extreme[0, 0]
    # a NaN neighbour does not make a sound pixel's R infinite (seven finite neighbours remain)
    assert np.isfinite(R[3, 4]) and not f[3, 4]
    # given flags: a fully flagged 3 x 3 leaves its centre, repairs its ring from outside
    g = np.zeros((5, 6), bool)
    g[1:4, 1:4] = True
    out, code = M.repair_plane(I, g)
    assert code[2, 2] == 2 and out[2, 2] == I[2, 2]
    ring = g.copy()
    ring[2, 2] = False
    assert (code[ring] == 1).all() and (code[~g] == 0).all()


def test_add_impulse_is_reproducible():
    clean = np.full((3, 200000), 60.0, np.float32)
    for kind in ("salt_pepper", "random", "hot"):
        a, ha = synth.add_impulse(clean, 0.01, seed=3, kind=kind)
        b, hb = synth.add_impulse(clean, 0.01, seed=3, kind=kind)
        assert a.dtype == np.float32 and ha.dtype == bool and a.shape == clean.shape
        assert np.array_equal(a, b) and np.array_equal(ha, hb)
        assert abs(ha.mean() - 0.01) < 1e-3
        assert np.array_equal(a[~ha], clean[~ha])
        c, hc = synth.add_impulse(clean, 0.01, seed=4, kind=kind)
        assert not np.array_equal(ha, hc)
    a, h = synth.add_impulse(clean, 0.01, seed=3)
    assert set(np.unique(a[h])) == {0.0, 255.0} and abs((a[h] == 255.0).mean() - 0.5) < 0.05
    a, h = synth.add_impulse(clean, 0.01, seed=3, kind="hot")
    assert (a[h] == 255.0).all()
    a, h = synth.add_impulse(clean, 0.01, seed=3, kind="random")
    assert a[h].min() >= 0.0 and a[h].max() < 255.0 and len(np.unique(a[h])) > 1000
    assert not synth.add_impulse(clean, 0.0)[1].any()
    with pytest.raises(ValueError):
        synth.add_impulse(clean, 0.01, kind="bogus")
    with pytest.raises(ValueError):
        synth.add_impulse(clean, 1.5)


def _readme_args(cli, tmp, src):
    if cli.endswith("LFBM3Ddenoising"):
        return [cli, src, "SAI", "_", "2", "2", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
                f"{tmp}/denoised", f"{tmp}/diff", "16", "16", "8", "3", "bior", "0", "32", "16", "8", "3", "dct", "0", "opp", "8",
                f"{tmp}/measures.txt"]
    return [cli, src, "SAI", "_", "3", "3", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
            f"{tmp}/denoised", f"{tmp}/diff", "8", "18", "6", "16", "4", "id", "sadct", "haar", "0", "16", "18", "6", "8", "4",
            "dct", "sadct", "haar", "0", "opp", "0", f"{tmp}/measures.txt"]


@pytest.mark.parametrize("cli", ["LFBM5Ddenoising", "LFBM3Ddenoising"])
def test_cli_parses_the_impulse_variables(tmp_path, cli):
    """Malformed values stop the command before it reads a file; well-formed ones get as far as the (missing) input files."""
    args = _readme_args(os.path.join(ROOT, "lfbm5d_amd", cli), str(tmp_path), str(tmp_path / "missing"))
    for bad in ("bogus", "", "Auto", "-1", "8x", " 8", "nan", "inf"):
        r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, LFBM5D_IMPULSE=bad))
        assert r.returncode != 0 and "LFBM5D_IMPULSE must be" in r.stdout, bad
        assert "Read input image" not in r.stdout, bad
    for bad in ("bogus", "", "-0.1", "1.5", "0.1x", "nan"):
        r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, LFBM5D_IMPULSE="auto", LFBM5D_IMPULSE_ADD=bad))
        assert r.returncode != 0 and "LFBM5D_IMPULSE_ADD must be" in r.stdout, bad
    for good in (dict(LFBM5D_IMPULSE="auto"), dict(LFBM5D_IMPULSE="6"), dict(LFBM5D_IMPULSE="0"), dict(LFBM5D_IMPULSE="7.5", LFBM5D_IMPULSE_ADD="0.005"),
                 dict(LFBM5D_IMPULSE_ADD="0")):
        r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, **good))
        assert r.returncode != 0 and "must be" not in r.stdout, good
        assert "not found or not a correct png image" in r.stdout, good
