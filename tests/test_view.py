"""CPU tests of the view synthesis (lfbm5d_view_*, include/lfbm5d.h): the exports, struct sizes and defaults, and the properties of the
numpy model (tests/view_model.py) that pin the definition: on a light field that is a pure translation per view the synthesis is the true
view bit for bit away from the border, one source is copied, no source is left, ties keep the smaller |d|."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core
import helpers
import view_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_and_binds_the_view_entry_points():
    lib = core.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfbm5d.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lfbm5d_view_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == ["lfbm5d_view_defaults", "lfbm5d_view_device", "lfbm5d_view_fill_device", "lfbm5d_view_host_sai"]
    for n in declared:
        assert hasattr(lib, n) and getattr(lib, n).argtypes is not None, n       # exported, and bound in core.py
    assert C.sizeof(core.ViewParamsStruct) == 7 * 4
    assert C.sizeof(core.ViewResultStruct) == 4 * 4 + 8 + 17 * 8
    for n in ("ViewParamsStruct", "ViewResultStruct", "ViewSynth", "view_params", "view_synth"):
        assert n in L.__all__ and hasattr(L, n), n
    assert hasattr(L.Context, "view_fill") and hasattr(L.Context, "view_synth")
    assert np.array_equal(M.RECIP[1:], (1.0 / np.arange(1, 25)).astype(np.float32)) and M.RECIP[3] == np.float32(1.0 / 3.0)


def test_defaults_work_without_a_gpu_and_lie_in_the_allowed_ranges():
    P = L.view_params()
    assert 0 <= P.max_disparity <= M.D_MAX and 0 <= P.box_radius <= M.R_MAX and P.ang_radius in (1, 2)
    assert P.iterations <= 1000 and 0.0 < P.sigma_end <= P.sigma_start and P.sigma_noise == 0.0
    P = L.view_params(max_disparity=8, box_radius=0, ang_radius=2, iterations=3, sigma_start=12.0, sigma_end=3.0, sigma_noise=2.0)
    assert (P.max_disparity, P.box_radius, P.ang_radius, P.iterations, P.sigma_start, P.sigma_end, P.sigma_noise) == (8, 0, 2, 3, 12.0, 3.0, 2.0)


def test_reflection_and_scan_order():
    assert list(M.reflect(np.arange(-7, 9), 4)) == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]     # period 6, no edge repeated
    assert list(M.reflect(np.arange(-3, 5), 2)) == [1, 0, 1, 0, 1, 0, 1, 0]
    assert M.hypotheses(0) == [0] and M.hypotheses(3) == [0, -1, 1, -2, 2, -3, 3]
    assert M.coords(5, M.ROWMAJOR, 3, 2) == (1, 2) and M.coords(5, M.COLMAJOR, 3, 2) == (1, 2) and M.coords(3, M.COLMAJOR, 3, 2) == (1, 1)
    mask, missing = np.ones(9, np.uint32), np.zeros(9, np.uint32)
    missing[[0, 1]] = 1
    mask[3] = 0
    assert M.sources(0, mask, missing, M.ROWMAJOR, 3, 3, 1) == [(4, 1, 1)]         # 1 is missing, 3 is empty
    assert [q for q, _, _ in M.sources(0, mask, missing, M.ROWMAJOR, 3, 3, 2)] == [2, 4, 5, 6, 7, 8]


def _translation_case(ah, aw, disparity, missing_sais, sound=None):
    lf = helpers.textured_lf(ah, aw, 48, 40, disparity).astype(np.float32).reshape(ah * aw, -1)
    mask = np.ones(ah * aw, np.uint32)
    missing = np.zeros(ah * aw, np.uint32)
    missing[missing_sais] = 1
    if sound is not None:
        missing[:] = 1
        missing[sound] = 0
    return lf, mask, missing


def _assert_true_view(lf, mask, missing, ah, aw, disparity, check):
    D, r = 3, 3
    damaged = lf.copy()
    damaged[missing != 0] = np.nan                                              # never read
    res = M.fill(damaged, mask, missing, M.ROWMAJOR, aw, ah, 40, 48, 3, D, r)
    b = D + r
    for m in check:
        got = res["out"][m].reshape(3, 48, 40)[:, b:-b, b:-b]
        want = lf[m].reshape(3, 48, 40)[:, b:-b, b:-b]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), m
        d = res["disp"][m].reshape(48, 40)[b:-b, b:-b]
        assert (np.abs(d) == disparity).all(), (m, np.unique(d))
    assert np.isfinite(res["out"][res["sais"]]).all() and res["left"] == 0
    return res


@pytest.mark.parametrize("disparity", [1, 2, 3])
@pytest.mark.parametrize("m", [4, 0, 1], ids=["centre", "corner", "edge"])
def test_pure_translation_gives_the_true_view(disparity, m):
    lf, mask, missing = _translation_case(3, 3, disparity, [m])
    res = _assert_true_view(lf, mask, missing, 3, 3, disparity, [m])
    assert (res["missing"], res["synthesised"], res["pixels"], int(res["hist"].sum())) == (1, 1, 48 * 40, 48 * 40)
    assert len(M.sources(m, mask, missing, M.ROWMAJOR, 3, 3, 1)) == {4: 8, 0: 3, 1: 5}[m]


@pytest.mark.parametrize("disparity", [1, 2, 3])
def test_angular_upsampling_pattern_gives_the_true_views(disparity):
    """5 x 5 with only even (s, t) sound: SAI 1 and 5 have two sources in line, SAI 6 four diagonal ones."""
    sound = [s * 5 + t for s in range(0, 5, 2) for t in range(0, 5, 2)]
    lf, mask, missing = _translation_case(5, 5, disparity, [], sound=sound)
    res = _assert_true_view(lf, mask, missing, 5, 5, disparity, [1, 5, 6])
    assert (res["missing"], res["synthesised"]) == (16, 16)
    assert [len(M.sources(m, mask, missing, M.ROWMAJOR, 5, 5, 1)) for m in (1, 5, 6)] == [2, 2, 4]


def test_one_source_is_copied_no_source_is_left():
    rng = np.random.default_rng(5)
    lf = rng.uniform(0.0, 255.0, (3, 3 * 9 * 7)).astype(np.float32)
    mask, missing = np.ones(3, np.uint32), np.array([0, 1, 0], np.uint32)
    mask[2] = 0
    res = M.fill(lf, mask, missing, M.ROWMAJOR, 3, 1, 7, 9, 3, 8, 7)            # 1 x 3 views: the source is SAI 0 alone
    assert np.array_equal(res["out"][1].view(np.uint32), lf[0].view(np.uint32)) and not res["disp"][1].any()
    assert res["hist"][8] == 63 and res["hist"].sum() == 63 and (res["synthesised"], res["left"]) == (1, 0)
    missing = np.array([1, 1, 0], np.uint32)                                    # nothing sound within reach
    res = M.fill(lf, mask, missing, M.ROWMAJOR, 3, 1, 7, 9, 3, 2, 1)
    assert (res["missing"], res["synthesised"], res["left"], res["pixels"]) == (2, 0, 2, 0) and res["left_sais"] == [0, 1]
    assert np.array_equal(res["out"].view(np.uint32), lf.view(np.uint32)) and not res["flags"].any()
    with pytest.raises(ValueError):
        M.loop(lf, mask, missing, M.ROWMAJOR, 3, 1, 7, 9, 3, 2, 1, 1, 30.0, 5.0, lambda z, s: z)
    with pytest.raises(ValueError):
        M.fill(lf, mask, np.array([0, 0, 1], np.uint32), M.ROWMAJOR, 3, 1, 7, 9, 3, 2, 1)   # a missing SAI masked empty


def test_ties_keep_the_smaller_disparity():
    lf = np.full((9, 3 * 12 * 11), 37.25, np.float32)                           # constant: E = 0 for every hypothesis
    mask, missing = np.ones(9, np.uint32), np.zeros(9, np.uint32)
    missing[4] = 1
    res = M.fill(lf, mask, missing, M.ROWMAJOR, 3, 3, 11, 12, 3, 8, 3)
    assert not res["disp"].any() and res["hist"][8] == 132
    assert (res["out"][4] == np.float32(37.25)).all()
    # a pattern of period 2 along x: d = -2 and d = +2 tie with d = 0, and d = 0 stays; +-1 are worse
    row = np.tile(np.array([10.0, 200.0], np.float32), 8)
    lf = np.tile(row, (9, 3 * 12, 1)).reshape(9, -1)
    res = M.fill(lf, mask, missing, M.ROWMAJOR, 3, 3, 16, 12, 3, 4, 2)
    assert not res["disp"].any()


def test_loop_composes_synthesis_step_and_projection():
    rng = np.random.default_rng(9)
    lf = rng.uniform(0.0, 255.0, (9, 3 * 8 * 8)).astype(np.float32)
    mask, missing = np.ones(9, np.uint32), np.zeros(9, np.uint32)
    missing[[4, 8]] = 1
    seen = []

    def step(z, sig):
        seen.append(sig)
        return z * np.float32(0.5)
    x, x0, res = M.loop(lf, mask, missing, M.ROWMAJOR, 3, 3, 8, 8, 3, 1, 1, 3, 30.0, 5.0, step, sigma_noise=10.0)
    sound = missing == 0
    assert np.array_equal(x[sound].view(np.uint32), lf[sound].view(np.uint32))
    assert np.array_equal(x[~sound], x0[~sound] * np.float32(0.125))
    assert seen == M.sigma_schedule(3, 30.0, 5.0, 10.0) and seen[0] == 30.0 and seen[-1] == 10.0


def test_the_model_gains_over_the_mean_of_the_neighbours_on_the_golden_crop():
    """Golden rows and columns 64..191, centre missing, r = 3: the mean of the neighbours (D = 0) and the sweep at D = 3, 4, 6."""
    clean = np.load(os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy"))[:, :, 64:192, 64:192].astype(np.float32).reshape(9, -1)
    mask, missing = np.ones(9, np.uint32), np.zeros(9, np.uint32)
    missing[4] = 1
    got = {D: M.psnr(M.fill(clean, mask, missing, M.ROWMAJOR, 3, 3, 128, 128, 3, D, 3)["out"][4], clean[4]) for D in (0, 3, 4, 6)}
    print(", ".join(f"D = {D}: {p:.4f} dB" for D, p in got.items()))
    for D, want in ((0, 28.03), (3, 31.53), (4, 31.88), (6, 30.31)):
        assert abs(got[D] - want) < 0.01, (D, got[D])


def _readme_args(cli, tmp, src):
    if cli.endswith("LFBM3Ddenoising"):
        return [cli, src, "SAI", "_", "2", "2", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
                f"{tmp}/denoised", f"{tmp}/diff", "16", "16", "8", "3", "bior", "0", "32", "16", "8", "3", "dct", "0", "opp", "8",
                f"{tmp}/measures.txt"]
    return [cli, src, "SAI", "_", "3", "3", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
            f"{tmp}/denoised", f"{tmp}/diff", "8", "18", "6", "16", "4", "id", "sadct", "haar", "0", "16", "18", "6", "8", "4",
            "dct", "sadct", "haar", "0", "opp", "0", f"{tmp}/measures.txt"]


@pytest.mark.parametrize("cli", ["LFBM5Ddenoising", "LFBM3Ddenoising"])
def test_cli_parses_the_missing_variables(tmp_path, cli):
    """Malformed values and the combination with LFBM5D_DEFECTS stop the command before it reads a file; well-formed ones get as far
    as the (missing) input files, and the files of the SAIs named are not asked for."""
    import subprocess
    args = _readme_args(os.path.join(ROOT, "lfbm5d_amd", cli), str(tmp_path), "none")
    for bad in ("", "2", "2_2,", "4_1", "0_1", "a_b", "2-2", " 2_2", "1_1;1_2"):
        r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, LFBM5D_MISSING=bad))
        assert r.returncode != 0 and "LFBM5D_MISSING must be" in r.stdout and "Read input image" not in r.stdout, bad
    for bad in ("bogus", "", "-1", "1.5", " 2", "2x", "1001"):
        r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, LFBM5D_MISSING="1_1", LFBM5D_MISSING_ITER=bad))
        assert r.returncode != 0 and "LFBM5D_MISSING_ITER must be" in r.stdout and "Read input image" not in r.stdout, bad
    r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, LFBM5D_MISSING="1_1", LFBM5D_DEFECTS=str(tmp_path)))
    assert r.returncode != 0 and "cannot be combined with LFBM5D_DEFECTS" in r.stdout and "Read input image" not in r.stdout
    for good, first in ((dict(LFBM5D_MISSING="1_1"), "SAI_01_02"), (dict(LFBM5D_MISSING="2_2,1_1", LFBM5D_MISSING_ITER="0"), "SAI_01_02"),
                        (dict(LFBM5D_MISSING_ITER="3"), "SAI_01_01")):
        r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, LFBM5D_IO_THREADS="1", **good))
        assert r.returncode != 0 and "must" not in r.stdout, good
        assert f"{first}.png not found or not a correct png image" in r.stdout, (good, r.stdout[-300:])
