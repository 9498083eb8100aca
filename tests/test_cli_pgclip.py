"""LFBM5D_SIGMA=poisson-clipped / poisson-clipped:<a>,<b> and LFBM5D_CLIP_RANGE of both command-line tools: the values they refuse and
the variables the mode refuses (no GPU: the command stops before it reads a file), and on the GPU the README command on the golden light
field: the model line with the model given, and the estimate from the 8-bit files that run wrote."""
import os
import re
import subprocess

import numpy as np
import pytest

import lfbm5d_amd as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
CLI = os.path.join(ROOT, "lfbm5d_amd", "LFBM5Ddenoising")
CLI3 = os.path.join(ROOT, "lfbm5d_amd", "LFBM3Ddenoising")
MEAN_LEVEL = 121.4


def _args(cli, tmp, src):
    if cli == CLI3:
        return [cli, src, "SAI", "_", "3", "3", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
                f"{tmp}/denoised", f"{tmp}/diff", "16", "16", "8", "3", "bior", "0", "32", "16", "8", "3", "dct", "0", "opp", "8",
                f"{tmp}/measures.txt"]
    return [cli, src, "SAI", "_", "3", "3", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
            f"{tmp}/denoised", f"{tmp}/diff", "8", "18", "6", "16", "4", "id", "sadct", "haar", "0", "16", "18", "6", "8", "4",
            "dct", "sadct", "haar", "0", "opp", "0", f"{tmp}/measures.txt"]


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if not k.startswith("LFBM5D_")}
    env.update(kw)
    return env


@pytest.mark.parametrize("cli", [CLI, CLI3])
def test_malformed_values_stop_before_any_file_is_read(tmp_path, cli):
    args = _args(cli, str(tmp_path), str(tmp_path / "missing"))
    for bad in ("poisson-clipped:", "poisson-clipped:1", "poisson-clipped:1,", "poisson-clipped:x,1", "poisson-clipped:1,2x",
                "poisson-clipped:-1,2", "poisson-clipped:1,-2", "poisson-clipped:0,0", "poisson-clipped:1;2", "poisson-clipped: 1,2",
                "poisson-clipped:1, 2", "poisson-clipped:nan,1", "poisson-clipped:1,inf", "Poisson-clipped", "poisson-clipped ",
                "poisson_clipped", "poisson-clipped:1,2,3"):
        r = subprocess.run(args, capture_output=True, text=True, env=_env(LFBM5D_SIGMA=bad))
        assert r.returncode != 0 and "LFBM5D_SIGMA must be" in r.stdout, bad
        assert "Read input image" not in r.stdout, bad
    for bad in ("", "auto", "0", "0,", ",255", "0;255", "0,255,3", "0,255x", " 0,255", "0, 255", "255,0", "5,5", "nan,255", "0,inf"):
        r = subprocess.run(args, capture_output=True, text=True, env=_env(LFBM5D_SIGMA="poisson-clipped", LFBM5D_CLIP_RANGE=bad))
        assert r.returncode != 0 and "LFBM5D_CLIP_RANGE must be" in r.stdout, bad
        assert "Read input image" not in r.stdout, bad
    # what was rejected before the mode existed still is, with the same beginning
    for bad in ("poisson:x", "poisson:1", "25", "poisson:1,", "poisson:1,2x", "poisson:-1,2", "poisson:0,0", "poisson:1;2", "Poisson"):
        r = subprocess.run(args, capture_output=True, text=True, env=_env(LFBM5D_SIGMA=bad))
        assert r.returncode != 0 and "LFBM5D_SIGMA must be" in r.stdout, bad


@pytest.mark.parametrize("cli", [CLI, CLI3])
def test_well_formed_values_get_as_far_as_the_missing_input(tmp_path, cli):
    args = _args(cli, str(tmp_path), str(tmp_path / "missing"))
    for good in (dict(LFBM5D_SIGMA="poisson-clipped"), dict(LFBM5D_SIGMA="poisson-clipped:1,100"), dict(LFBM5D_SIGMA="poisson-clipped:0,625"),
                 dict(LFBM5D_SIGMA="poisson-clipped:0.5,4", LFBM5D_CLIP_RANGE="16,235"), dict(LFBM5D_SIGMA="poisson-clipped:8,0"),
                 dict(LFBM5D_SIGMA="poisson-clipped", LFBM5D_CLIP_RANGE="-0.5,0.5"), dict(LFBM5D_SIGMA="poisson-clipped", LFBM5D_CLIP_ADD="1")):
        r = subprocess.run(args, capture_output=True, text=True, env=_env(**good))
        assert r.returncode != 0 and "must be" not in r.stdout and "cannot be combined" not in r.stdout, good
        assert "not found or not a correct png image" in r.stdout, good


@pytest.mark.parametrize("cli", [CLI, CLI3])
def test_the_mode_refuses_clip_and_equalise_as_poisson_does(tmp_path, cli):
    args = _args(cli, str(tmp_path), str(tmp_path / "missing"))
    for mode in ("poisson-clipped", "poisson-clipped:1,100"):
        r = subprocess.run(args, capture_output=True, text=True, env=_env(LFBM5D_CLIP="auto", LFBM5D_SIGMA=mode))
        assert r.returncode != 0 and "LFBM5D_CLIP cannot be combined with LFBM5D_SIGMA=poisson" in r.stdout, mode
        assert "Read input image" not in r.stdout, mode
        for eq in ("auto", "flat"):
            r = subprocess.run(args, capture_output=True, text=True, env=_env(LFBM5D_EQUALISE=eq, LFBM5D_SIGMA=mode))
            assert r.returncode != 0 and "LFBM5D_EQUALISE cannot be combined with LFBM5D_SIGMA=poisson" in r.stdout, (mode, eq)
            assert "Read input image" not in r.stdout, (mode, eq)
    # poisson and LFBM5D_CLIP refuse each other as before
    r = subprocess.run(args, capture_output=True, text=True, env=_env(LFBM5D_CLIP="auto", LFBM5D_SIGMA="poisson"))
    assert r.returncode != 0 and "LFBM5D_CLIP cannot be combined with LFBM5D_SIGMA=poisson" in r.stdout


def _write_source_lf(tmp):
    from PIL import Image
    lf = np.load(GOLDEN)
    src = os.path.join(tmp, "sourceLF")
    os.makedirs(src)
    for s in range(3):
        for t in range(3):
            Image.fromarray(lf[s * 3 + t].transpose(1, 2, 0)).save(f"{src}/SAI_{s + 1:02d}_{t + 1:02d}.png")
    for d in ("noisy", "basic", "denoised", "diff"):
        os.makedirs(os.path.join(tmp, d))
    return src


def _model_line(stdout):
    m = re.search(r"(Estimated|Given) clipped noise model: a = ([0-9.eE+-]+), b = ([0-9.eE+-]+), range ([0-9.eE+-]+)\.\.([0-9.eE+-]+) "
                  r"\((?:(\d+) levels, censored blocks <= ([0-9.]+) %; )?sigma after stabilisation = ([0-9.eE+-]+)\)", stdout)
    assert m, stdout[-2000:]
    return m.group(1), float(m.group(2)), float(m.group(3)), float(m.group(4)), float(m.group(5)), m.group(6), m.group(7), float(m.group(8))


def _psnrs(tmp):
    txt = open(f"{tmp}/measures.txt").read()
    return {k: float(txt.split(f"-> Average PSNR {k} = ")[1].split()[0]) for k in ("noisy", "basic", "denoised")}


@pytest.mark.gpu
def test_cli_given_model_then_the_estimate_from_its_files(tmp_path):
    tmp = str(tmp_path)
    src = _write_source_lf(tmp)
    out = subprocess.run(_args(CLI, tmp, src), capture_output=True, text=True, env=_env(LFBM5D_SEED="1", LFBM5D_SIGMA="poisson-clipped:1,100"))
    assert out.returncode == 0, out.stdout[-2000:]
    kind, a, b, lo, hi, levels, pct, s = _model_line(out.stdout)
    assert (kind, a, b, lo, hi, levels) == ("Given", 1.0, 100.0, 0.0, 255.0, None)
    assert abs(s - L.pgclip_curves(1.0, 100.0).s) < 1e-4
    assert "Add noise [Poisson-Gaussian, a = 1, b = 100]" in out.stdout
    assert re.search(r"Round and clip \[range 0\.\.255\]: \d+ of 1769472 values at the bounds", out.stdout)
    vals = _psnrs(tmp)
    print("LFBM5D_SIGMA=poisson-clipped:1,100: s =", s, "PSNR", vals)
    assert vals["denoised"] > vals["basic"] > vals["noisy"] + 5.0
    assert os.path.exists(f"{tmp}/denoised/SAI_02_02.png")
    # the 8-bit files that run wrote, read back without a ground truth: the use the mode was built for
    out = subprocess.run(_args(CLI, tmp, "none"), capture_output=True, text=True, env=_env(LFBM5D_SIGMA="poisson-clipped"))
    assert out.returncode == 0, out.stdout[-2000:]
    kind, a, b, lo, hi, levels, pct, s2 = _model_line(out.stdout)
    err = (a * MEAN_LEVEL + b) / (1.0 * MEAN_LEVEL + 100.0) - 1.0
    print(f"LFBM5D_SIGMA=poisson-clipped on those files: a = {a}, b = {b} ({levels} levels, <= {pct} %), s = {s2}, "
          f"variance at {MEAN_LEVEL}: {100 * err:+.1f} %")
    assert kind == "Estimated" and (lo, hi) == (0.0, 255.0) and int(levels) >= 4 and float(pct) in (5.0, 10.0, 20.0, 40.0, 100.0)
    assert abs(err) <= 0.05
    assert abs(s2 - L.pgclip_curves(a, b).s) < 1e-3 * s2                       # (a and b as printed: 8 digits)
    # LFBM3Ddenoising: forward map, run_bm3d_LF, inverse map
    tmp3 = os.path.join(tmp, "bm3d")
    os.makedirs(tmp3)
    src3 = _write_source_lf(tmp3)
    out = subprocess.run(_args(CLI3, tmp3, src3), capture_output=True, text=True, env=_env(LFBM5D_SEED="1", LFBM5D_SIGMA="poisson-clipped:1,100"))
    assert out.returncode == 0, out.stdout[-2000:]
    assert _model_line(out.stdout)[:5] == ("Given", 1.0, 100.0, 0.0, 255.0)
    v3 = _psnrs(tmp3)
    print("LFBM3Ddenoising, LFBM5D_SIGMA=poisson-clipped:1,100: PSNR", v3)
    assert v3["denoised"] > v3["noisy"] + 5.0
