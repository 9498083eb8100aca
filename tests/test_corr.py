"""Correlated noise on the CPU (include/lfbm5d_corr.h): the host functions against the numpy model (tests/corr_model.py), the
refusals, the figures of the blind estimate on the golden light field, the group cases' decidability, both command-line tools'
parsing of LFBM5D_NOISE_CORR (no GPU: the commands stop before they read a file), and a stand-alone program over the host code built
with AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import corr_model as CM
import group_model as M
import lfbm5d_amd as L
from lfbm5d_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "lfbm5d_amd", "LFBM5Ddenoising")
CLI3 = os.path.join(ROOT, "lfbm5d_amd", "LFBM3Ddenoising")
EPS32 = float(np.finfo(np.float32).eps)


def test_header_declares_the_feature():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfbm5d_corr.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lfbm5d_[a-z0-9_]+)\s*\(", src)))
    assert declared == ["lfbm5d_corr_check", "lfbm5d_corr_error", "lfbm5d_corr_from_kernel", "lfbm5d_corr_measure_device",
                        "lfbm5d_corr_measure_host_sai", "lfbm5d_corr_table", "lfbm5d_debug_group_corr", "lfbm5d_denoise_corr_device",
                        "lfbm5d_denoise_corr_host_sai", "lfbm5d_step1_corr_device", "lfbm5d_step2_corr_device"]
    assert '#include "lfbm5d_corr.h"' in open(os.path.join(ROOT, "include", "lfbm5d.h")).read()
    import ctypes as C
    from lfbm5d_amd import core
    assert C.sizeof(core.CorrEstimateStruct) == 49 * 8 + 2 * 8 + 2 * 8 + 2 * 4
    assert float(re.search(r"#define LFBM5D_CORR_DEFAULT_FRACTION ([0-9.]+)", src).group(1)) == 0.1


@pytest.mark.parametrize("tau,k", [("dct", 4), ("dct", 8), ("dct", 12), ("dct", 16), ("bior", 8), ("bior", 16)])
@pytest.mark.parametrize("width", [0.5, 0.8, 1.2])
def test_table_is_the_models(tau, k, width):
    """v and s within one float32 step of the float64 model (the library sums in another order: 1e-12 of that), the same entries
    clamped, the floor exactly 1 / 64."""
    acf = L.corr_from_kernel(CM.gaussian_taps(width))
    assert np.abs(acf - CM.from_kernel(CM.gaussian_taps(width))).max() < 1e-15 and CM.check(acf) is None
    s, v, clamped = L.corr_table(acf, tau, k)
    ms, mv, mclamped = CM.table(acf, tau, k)
    assert s.dtype == np.float32 and v.dtype == np.float32 and v.shape == (k * k,)
    assert clamped == mclamped
    assert np.abs(v / mv - 1).max() <= EPS32 and np.abs(s / ms - 1).max() <= EPS32
    raw = CM.table_raw(acf, tau, k)
    assert np.array_equal(v == np.float32(CM.FLOOR), raw < CM.FLOOR) and (v >= np.float32(CM.FLOOR)).all()
    if width == 1.2 and tau == "dct" and k >= 8:
        assert raw.min() < 0 and clamped > 0      # truncating a wide autocorrelation to 7 x 7 lags: some variances come out negative


def test_the_table_matters():
    """The issue's figures: the factors of an 8 x 8 DCT span 0.29..2.2 at width 0.5 (lag-1 correlation 0.26), 0.001..6.4 at 0.8 (0.67),
    and width 1.2 has a negative one (-0.12)."""
    for width, lag1, lo, hi in ((0.5, 0.26, 0.29, 2.2), (0.8, 0.67, 0.001, 6.4), (1.2, 0.84, -0.12, 12.1)):
        acf = CM.from_kernel(CM.gaussian_taps(width))
        raw = CM.table_raw(acf, "dct", 8)
        assert abs(acf[3, 4] - lag1) < 0.005 and abs(raw.min() - lo) < 0.005 and abs(raw.max() / hi - 1) < 0.01, (width, acf[3, 4], raw.min(), raw.max())


def test_white_noise_gives_exact_ones():
    for tau in ("id", "dct", "bior"):
        for k in range(2, 33):
            if tau == "bior" and k & (k - 1):
                continue
            s, v, clamped = L.corr_table(L.CORR_WHITE, tau, k)
            assert (s == 1).all() and (v == 1).all() and clamped == 0, (tau, k)
    # id: ones whatever the autocorrelation
    s, v, clamped = L.corr_table(L.corr_from_kernel(CM.gaussian_taps(0.8)), "id", 8)
    assert (s == 1).all() and (v == 1).all() and clamped == 0


def test_a_delta_kernel_is_white():
    for shape, at in (((1, 1), (0, 0)), ((7, 7), (3, 3)), ((3, 5), (2, 0)), ((7, 1), (6, 0))):
        g = np.zeros(shape)
        g[at] = -3.0
        assert np.array_equal(L.corr_from_kernel(g), L.CORR_WHITE), shape
    # a box of two taps: lag 1 is one half, exactly
    acf = L.corr_from_kernel([[1.0, 1.0]])
    assert acf[3, 4] == 0.5 and acf[3, 2] == 0.5 and acf[3, 5] == 0 and acf[4, 3] == 0 and acf[3, 3] == 1


def test_bad_autocorrelations_are_refused():
    good = L.corr_from_kernel(CM.gaussian_taps(0.8))
    for name, change, message in (("lag-0", lambda a: a.__setitem__((3, 3), 0.999), "1 at lag 0"),
                                  ("asymmetric", lambda a: a.__setitem__((3, 4), 0.1), "point-symmetric"),
                                  ("nan", lambda a: a.__setitem__((0, 0), np.nan), "finite"),
                                  ("inf", lambda a: a.__setitem__((6, 6), np.inf), "finite"),
                                  ("large", lambda a: (a.__setitem__((2, 3), 1.5), a.__setitem__((4, 3), 1.5)), "magnitude at most 1")):
        a = good.copy()
        change(a)
        assert CM.check(a) is not None, name
        with pytest.raises(L.LfBm5dError, match=message):
            L.corr_table(a, "dct", 8)
    with pytest.raises(L.LfBm5dError, match="7 x 7"):
        L.corr_table(np.ones(48), "dct", 8)
    for tau, k, message in (("dct", 1, "outside 2..32"), ("dct", 33, "outside 2..32"), ("bior", 12, "power-of-two"), ("sadct", 8, "tau_2D")):
        with pytest.raises(L.LfBm5dError, match=message):
            L.corr_table(good, tau, k)
    for taps, message in ((np.zeros((3, 3)), "all zero"), (np.ones((8, 3)), "1..7"), ([[1.0, np.nan]], "not finite")):
        with pytest.raises(L.LfBm5dError, match=message):
            L.corr_from_kernel(taps)


def test_synthesised_noise_has_the_kernels_autocorrelation():
    """add_correlated_noise keeps the marginal level and has corr_from_kernel's autocorrelation (the calibration use of the model:
    fraction 1 on a flat field); the sampling error of 3 x 128 x 128 values is a few 1e-2."""
    taps = CM.gaussian_taps(0.8)
    flat = np.full((1, 3, 128, 128), 100.0, np.float32)
    noisy = synth.add_correlated_noise(flat, 20.0, 3.0 * taps, seed=5)
    assert noisy.dtype == np.float32 and noisy.shape == flat.shape
    e = CM.measure(noisy, [1], 16, 1.0)
    assert e["selected"] == e["blocks"] == 3 * 64
    assert abs(e["sigma"] / 20.0 - 1) < 0.05 and np.abs(e["acf"] - CM.from_kernel(taps)).max() < 0.06
    assert CM.check(e["acf"]) is None


def test_blind_estimate_on_the_golden_light_field():
    """The estimate at the shipped block size and fraction (tools/corr_sweep.py writes the whole sweep to profiles/corr_defaults.txt):
    its table of the 8 x 8 DCT is closer to the true one than the all-ones table is, for Gaussian taps of width 0.5 and 0.8 at sigma
    10 and 25; the recorded figures are the ones the model gives here."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import corr_sweep
    B, fraction = corr_sweep.shipped()
    txt = open(os.path.join(ROOT, "profiles", "corr_defaults.txt")).read()
    lf = np.load(os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")).astype(np.float32)
    for width, sigma in corr_sweep.DATA:
        err, white, bias, h, v, t = corr_sweep.figures(width, sigma, B, fraction, lf)
        print("width %.1f sigma %2.0f: error %.3f (white %.3f), sigma bias %+.1f %%, lag-1 %.3f %.3f (true %.3f)" % (width, sigma, err, white, bias, h, v, t))
        assert err < white, (width, sigma, err, white)
        m = re.search(r"shipped: block %d fraction %.2f width %.1f sigma %2.0f \| error ([0-9.]+) white ([0-9.]+) sigma bias ([-+0-9.]+) %%"
                      % (B, fraction, width, sigma), txt)
        assert m, "profiles/corr_defaults.txt has no shipped row for width %.1f sigma %.0f" % (width, sigma)
        assert abs(float(m.group(1)) - err) < 2e-3 and abs(float(m.group(2)) - white) < 2e-3 and abs(float(m.group(3)) - bias) < 0.1


def test_group_cases_are_decidable():
    """The hard-threshold cases of tests/test_gpu_corr_group.py: under the non-trivial table at least 90 % of the (group, channel)
    pairs have no coefficient inside group_model.gap_of of its threshold, every pair keeps a coefficient in some group, and the
    kernel text is the table forms'."""
    acf = L.corr_from_kernel(CM.gaussian_taps(CM.TABLE_TAPS_WIDTH))
    names = set()
    for case in CM.group_cases():
        s, v, _ = L.corr_table(acf, case.tau2, case.k)
        names.update(CM.expected_kernels(case))
        if case.step != 1:
            continue
        m = CM.run(case, s, v)
        closed = float((m["ingap"] == 0).mean())
        print("%s: %.1f %% of %d pairs decidable, %.1f survivors a pair" % (case.name, 100 * closed, m["ingap"].size, m["count"].mean()))
        assert closed >= 0.9, (case.name, closed)
        assert m["count"].mean() > 1
    assert names == {"k_group_pos", "k_group_shape<false>", "k_group_shape<true>", "k_group_corr<1>", "k_group_corr<2>",
                     "k_group_big_corr<2, false>", "k_group_big_corr<1, true>", "k_group_big_corr<2, true>"}


def test_model_with_the_white_table_is_the_plain_model():
    case = CM.group_cases()[0]
    ones = np.ones(case.k * case.k, np.float32)
    a, b = CM.run(case, ones, ones), M.run(case)
    assert np.array_equal(a["filt"], b["filt"]) and np.array_equal(a["w"], b["w"]) and np.array_equal(a["count"], b["count"])
    case = CM.group_cases()[1]
    a, b = CM.run(case, ones, ones), M.run(case)
    assert np.array_equal(a["filt"], b["filt"]) and np.array_equal(a["w"], b["w"])


# ---- the command-line tools ----
def _args(cli, tmp, src):
    if cli == CLI3:
        return [cli, src, "SAI", "_", "3", "3", "1", "1", "1", "1", "row", "10", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
                f"{tmp}/denoised", f"{tmp}/diff", "16", "16", "8", "3", "bior", "0", "32", "16", "8", "3", "dct", "0", "opp", "8",
                f"{tmp}/measures.txt"]
    return [cli, src, "SAI", "_", "3", "3", "1", "1", "1", "1", "row", "10", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
            f"{tmp}/denoised", f"{tmp}/diff", "8", "8", "3", "8", "3", "dct", "sadct", "haar", "0", "16", "8", "3", "8", "3",
            "dct", "sadct", "haar", "0", "opp", "0", f"{tmp}/measures.txt"]


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if not k.startswith("LFBM5D_")}
    env.update(kw)
    return env


def _run(cli, tmp_path, src="none_here", **env):
    r = subprocess.run(_args(cli, str(tmp_path), str(tmp_path / src) if src != "none" else "none"), capture_output=True, text=True,
                       env=_env(LFBM5D_IO_THREADS="1", **env))
    assert r.returncode != 0
    return r.stdout


def test_cli_parses_the_noise_correlation_variable(tmp_path):
    acf = CM.from_kernel(CM.gaussian_taps(0.8))
    good = tmp_path / "acf.txt"
    good.write_text("\n".join(" ".join("%.17g" % x for x in row) for row in acf))
    taps = tmp_path / "taps.txt"
    taps.write_text("1 2 1\n2 4 2\n1 2 1\n")
    # good values get as far as the (missing) input files
    for value in ("auto", str(good), "kernel:" + str(taps)):
        out = _run(CLI, tmp_path, LFBM5D_NOISE_CORR=value)
        assert ".png not found or not a correct png image" in out and "LFBM5D_NOISE_CORR" not in out, (value, out[-300:])
    out = _run(CLI, tmp_path, LFBM5D_NOISE_CORR_ADD=str(taps))
    assert ".png not found or not a correct png image" in out and "LFBM5D_NOISE_CORR" not in out
    # malformed values stop the command before it reads a file
    short = tmp_path / "short.txt"
    short.write_text("1 0 0")
    asym = tmp_path / "asym.txt"
    a = acf.copy()
    a[3, 4] = 0.0
    asym.write_text(" ".join("%.17g" % x for x in a.reshape(-1)))
    words = tmp_path / "words.txt"
    words.write_text("1 2 x\n")
    ragged = tmp_path / "ragged.txt"
    ragged.write_text("1 2 1\n1 2\n")
    wide = tmp_path / "wide.txt"
    wide.write_text("1 1 1 1 1 1 1 1\n")
    zeros = tmp_path / "zeros.txt"
    zeros.write_text("0 0\n0 0\n")
    for value, message in (("", 'got ""'), (str(tmp_path / "absent.txt"), "cannot read"), (str(short), "must hold 49 numbers"),
                           (str(asym), "point-symmetric"), (str(words), "is not a number"), ("kernel:" + str(tmp_path / "absent.txt"), "cannot read"),
                           ("kernel:" + str(words), "is not a finite number"), ("kernel:" + str(ragged), "differ in length"),
                           ("kernel:" + str(wide), "1..7 rows of 1..7 taps"), ("kernel:" + str(zeros), "all zero")):
        out = _run(CLI, tmp_path, LFBM5D_NOISE_CORR=value)
        assert message in out and "Read input image" not in out and "not found" not in out, (value, out[-300:])
    for value, message in ((str(tmp_path / "absent.txt"), "cannot read"), (str(zeros), "all zero"), (str(ragged), "differ in length")):
        out = _run(CLI, tmp_path, LFBM5D_NOISE_CORR_ADD=value)
        assert "LFBM5D_NOISE_CORR_ADD" in out and message in out and "not found" not in out, (value, out[-300:])
    out = _run(CLI, tmp_path, src="none", LFBM5D_NOISE_CORR_ADD=str(taps))
    assert "LFBM5D_NOISE_CORR_ADD needs a source light field" in out
    # combinations that are errors for now
    for other in (dict(LFBM5D_SIGMA="auto"), dict(LFBM5D_SIGMA="poisson"), dict(LFBM5D_CLIP="0:255"), dict(LFBM5D_VIEW_SIGMA="auto"),
                  dict(LFBM5D_REPAIR="joint"), dict(LFBM5D_DEFECTS=str(tmp_path)), dict(LFBM5D_MISSING="1_1"), dict(LFBM5D_DETECT="auto"),
                  dict(LFBM5D_EQUALISE="auto")):
        out = _run(CLI, tmp_path, LFBM5D_NOISE_CORR="auto", **other)
        assert "Read input image" not in out and "not found" not in out, (other, out[-300:])
        if "LFBM5D_NOISE_CORR cannot be combined with " + list(other)[0] not in out:
            # (the other variable's own parser may refuse its value, or the pair, first)
            assert "LFBM5D_" in out and ("must" in out or "cannot" in out or "needs" in out), (other, out[-300:])
    out = _run(CLI, tmp_path, LFBM5D_NOISE_CORR="auto", LFBM5D_VIEW_SIGMA="auto")
    assert "LFBM5D_NOISE_CORR cannot be combined with LFBM5D_VIEW_SIGMA" in out
    out = _run(CLI, tmp_path, LFBM5D_NOISE_CORR_ADD=str(taps), LFBM5D_SIGMA="poisson")
    assert "LFBM5D_NOISE_CORR_ADD cannot be combined with LFBM5D_SIGMA=poisson" in out
    # the per-SAI BM3D command accepts the variables only to refuse them
    for var in ("LFBM5D_NOISE_CORR", "LFBM5D_NOISE_CORR_ADD"):
        out = _run(CLI3, tmp_path, **{var: "auto"})
        assert var + " is not supported by LFBM3Ddenoising" in out and "not found" not in out


def test_host_code_under_sanitizers(tmp_path):
    """tests/corr_host_check.cpp over lfbm5d_corr_host.hip (plain C++: no kernel, no HIP call), built with a host compiler and
    -fsanitize=address,undefined, run here: tables of every patch size and transform, taps of every size, the refusals."""
    exe = str(tmp_path / "corr_host_check")
    src = os.path.join(ROOT, "lfbm5d_amd", "csrc", "lfbm5d_corr_host.hip")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-Wno-unknown-pragmas", "-o", exe,
           os.path.join(ROOT, "tests", "corr_host_check.cpp"), "-x", "c++", src]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout[-1000:], r.stderr[-2000:])
