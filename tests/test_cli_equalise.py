"""LFBM5D_EQUALISE of both command lines (lfbm5d_cli.cpp): malformed values and the combinations with LFBM5D_SIGMA=poisson and LFBM5D_CLIP
stop the command before it reads a file (no GPU needed); on the GPU, the golden 3 x 3 light field as 64 x 64 files under a planted
vignette (LFBM5D_EQUALISE_ADD=0.6) gives the report line, `auto` saves results that keep the vignette and `flat` results without it;
and with the variables unset the command's output is the stored run's (tests/golden/cli_equalise_unset.json: the shape of stdout, the
noisy files and the average PSNRs of the same command, recorded on an MI355X with the binary built from the commit before the stage
existed)."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

from lfbm5d_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
STORED = os.path.join(ROOT, "tests", "golden", "cli_equalise_unset.json")
CLI = os.path.join(ROOT, "lfbm5d_amd", "LFBM5Ddenoising")
CLI3 = os.path.join(ROOT, "lfbm5d_amd", "LFBM3Ddenoising")
LINE = re.compile(r"Photometric equalisation: (\d+) of (\d+) SAIs fitted, (\d+) untested, (\d+) unfit; gains ([0-9.eE+-]+)\.\.([0-9.eE+-]+); "
                  r"(\d+) sweeps, residual ([0-9.eE+-]+)")
PSNR = re.compile(r"- (Noisy|Basic|Denoised) light field: ([0-9.]+)")
EDGE = 0.6


def _args(cli, tmp, src, aw=3, ah=3):
    if cli == CLI3:
        return [cli, src, "SAI", "_", str(aw), str(ah), "1", "1", "1", "1", "row", "10", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
                f"{tmp}/denoised", f"{tmp}/diff", "16", "16", "8", "3", "bior", "0", "32", "16", "8", "3", "dct", "0", "opp", "8",
                f"{tmp}/measures.txt"]
    return [cli, src, "SAI", "_", str(aw), str(ah), "1", "1", "1", "1", "row", "10", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
            f"{tmp}/denoised", f"{tmp}/diff", "8", "8", "3", "8", "3", "dct", "sadct", "haar", "0", "16", "8", "3", "8", "3",
            "dct", "sadct", "haar", "0", "opp", "0", f"{tmp}/measures.txt"]


def _clean_env(**more):
    env = {k: v for k, v in os.environ.items() if not k.startswith("LFBM5D_EQUALISE")}
    return dict(env, LFBM5D_IO_THREADS="1", **more)


@pytest.mark.parametrize("cli", [CLI, CLI3], ids=["LFBM5Ddenoising", "LFBM3Ddenoising"])
def test_cli_parses_the_equalise_variables(tmp_path, cli):
    src = str(tmp_path / "nowhere")

    def run(source=src, **env):
        return subprocess.run(_args(cli, str(tmp_path), source), capture_output=True, text=True, env=_clean_env(**env))
    for bad in ("", "x", "1", "Auto", "auto ", "flat,auto"):
        r = run(LFBM5D_EQUALISE=bad)
        assert r.returncode != 0 and "LFBM5D_EQUALISE must be" in r.stdout and "Read input image" not in r.stdout, bad
    for mode in ("auto", "flat"):
        r = run(LFBM5D_EQUALISE=mode, LFBM5D_SIGMA="poisson")
        assert r.returncode != 0 and "LFBM5D_EQUALISE cannot be combined with LFBM5D_SIGMA=poisson" in r.stdout and "not found" not in r.stdout
        r = run(LFBM5D_EQUALISE=mode, LFBM5D_SIGMA="poisson:0.5,4")
        assert r.returncode != 0 and "LFBM5D_EQUALISE cannot be combined with LFBM5D_SIGMA=poisson" in r.stdout and "not found" not in r.stdout
        r = run(LFBM5D_EQUALISE=mode, LFBM5D_CLIP="auto")
        assert r.returncode != 0 and "LFBM5D_EQUALISE cannot be combined with LFBM5D_CLIP" in r.stdout and "not found" not in r.stdout
    for bad in ("", "x", "0", "-0.5", "1.01", " 0.5", "0.5x", "nan", "inf"):
        r = run(LFBM5D_EQUALISE="auto", LFBM5D_EQUALISE_ADD=bad)
        assert r.returncode != 0 and "LFBM5D_EQUALISE_ADD must be" in r.stdout and "not found" not in r.stdout, bad
    r = run(source="none", LFBM5D_EQUALISE_ADD="0.6")
    assert r.returncode != 0 and "LFBM5D_EQUALISE_ADD needs a source light field" in r.stdout and "not found" not in r.stdout
    for good in (dict(LFBM5D_EQUALISE="auto"), dict(LFBM5D_EQUALISE="flat", LFBM5D_EQUALISE_ADD="0.6"), dict(LFBM5D_EQUALISE_ADD="1"),
                 dict(LFBM5D_EQUALISE="auto", LFBM5D_DISPARITY_STEPS="2"), dict(LFBM5D_EQUALISE="auto", LFBM5D_DETECT="auto", LFBM5D_SIGMA="auto")):
        r = run(**good)                                                         # well-formed: as far as the (missing) input files
        assert r.returncode != 0 and "must" not in r.stdout and "cannot" not in r.stdout and "needs" not in r.stdout, good
        assert "SAI_01_01.png not found or not a correct png image" in r.stdout, (good, r.stdout[-300:])
    r = run(LFBM5D_DISPARITY_STEPS="2")                                          # ... which still needs a sweep to apply to
    assert r.returncode != 0 and "LFBM5D_DISPARITY_STEPS needs" in r.stdout


def _crop():
    return np.load(GOLDEN)[:, :, 96:160, 96:160].copy()


def _out_dirs(tmp):
    for d in ("noisy", "basic", "denoised", "diff"):
        os.makedirs(os.path.join(tmp, d), exist_ok=True)


def _write_fixture(tmp):
    """Golden rows and columns 96..159 as 3 x 3 files of 64 x 64."""
    from PIL import Image
    lf = _crop()
    src = os.path.join(tmp, "sourceLF")
    os.makedirs(src)
    for s in range(3):
        for t in range(3):
            Image.fromarray(lf[s * 3 + t].transpose(1, 2, 0)).save(f"{src}/SAI_{s + 1:02d}_{t + 1:02d}.png")
    _out_dirs(tmp)
    return src


def _shape_of(stdout, tmp):
    """stdout with the working directory's name and every number taken out: what stays the same from run to run."""
    return re.sub(r"\n+", "\n", re.sub(r"[0-9.eE+-]+", "#", stdout.replace(tmp, "TMP").replace("\r", "\n")))


def record_unset(tmp, cli=CLI):
    """The command of the tests with every LFBM5D_EQUALISE variable unset: what tests/golden/cli_equalise_unset.json stores."""
    src = _write_fixture(tmp)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LFBM5D_EQUALISE")}
    r = subprocess.run(_args(cli, tmp, src), capture_output=True, text=True, env=dict(env, LFBM5D_SEED="1"))
    assert r.returncode == 0, r.stdout[-2000:]
    files = sorted(os.listdir(f"{tmp}/noisy"))
    psnr = {k: float(v) for k, v in PSNR.findall(r.stdout)}                      # the last block: all three
    return r, dict(stdout_shape=_shape_of(r.stdout, tmp), psnr=psnr,
                   noisy_sha256={f: hashlib.sha256(open(f"{tmp}/noisy/{f}", "rb").read()).hexdigest() for f in files})


def _sai_means(directory):
    from PIL import Image
    return np.array([[np.asarray(Image.open(f"{directory}/SAI_{s + 1:02d}_{t + 1:02d}.png")).astype(np.float64).mean() for t in range(3)]
                     for s in range(3)]).reshape(-1)


@pytest.mark.gpu
def test_cli_equalises_and_restores(tmp_path):
    tmp = str(tmp_path)
    plain, rec = record_unset(tmp)
    assert "Photometric equalisation" not in plain.stdout and "Vignette" not in plain.stdout
    stored = json.load(open(STORED))
    assert rec["stdout_shape"] == stored["stdout_shape"] and rec["noisy_sha256"] == stored["noisy_sha256"]   # unset: the stored run's output
    assert sorted(rec["psnr"]) == sorted(stored["psnr"]) == ["Basic", "Denoised", "Noisy"]
    for k, v in stored["psnr"].items():
        assert abs(rec["psnr"][k] - v) < 0.02, (k, rec["psnr"][k], v)
    src = os.path.join(tmp, "sourceLF")
    source = _sai_means(src)
    planted = synth.vignette_gains(3, 3, EDGE)
    results = {}
    for mode in ("auto", "flat"):
        out = subprocess.run(_args(CLI, tmp, src), capture_output=True, text=True,
                             env=_clean_env(LFBM5D_SEED="1", LFBM5D_EQUALISE=mode, LFBM5D_EQUALISE_ADD=str(EDGE)))
        assert out.returncode == 0, out.stdout[-2000:]
        m = LINE.search(out.stdout)
        assert m and "Vignette [corner views x 0.6]" in out.stdout, out.stdout[-2000:]
        print(mode, m.group(0))
        fitted, A, untested, unfit, gmin, gmax, sweeps, residual = m.groups()
        assert (int(fitted), int(A), int(untested), int(unfit)) == (9, 9, 0, 0) and 1 <= int(sweeps) <= 3
        # the planted range of gains: each gain is found within about 1.1 % at sigma = 0 (the crop's own views differ by 1 %), a ratio of
        # two within 2.2 %; the noise of sigma = 10 on 64 x 64 values adds little to a median: 5 %
        assert abs(float(gmin) / float(gmax) - EDGE) < 0.05 * EDGE
        assert out.stdout.index("Photometric equalisation:") < out.stdout.index("Running LFBM5D filter")
        results[mode] = {d: _sai_means(f"{tmp}/{d}") / source for d in ("basic", "denoised")}
        print(mode, "per-SAI mean of the denoised files / the source's:", " ".join(f"{v:.3f}" for v in results[mode]["denoised"]))
    for d in ("basic", "denoised"):
        assert np.abs(results["auto"][d] / planted - 1.0).max() < 0.03           # auto: the files keep every view's photometry
        flat = results["flat"][d]
        assert np.abs(flat / np.median(flat) - 1.0).max() < 0.03                 # flat: the vignette is gone
    # LFBM3Ddenoising: the same stage in front of the per-SAI filter
    tmp3 = os.path.join(tmp, "bm3d")
    _out_dirs(tmp3)
    out3 = subprocess.run(_args(CLI3, tmp3, src), capture_output=True, text=True,
                          env=_clean_env(LFBM5D_SEED="1", LFBM5D_EQUALISE="auto", LFBM5D_EQUALISE_ADD=str(EDGE)))
    assert out3.returncode == 0, out3.stdout[-2000:]
    m3 = LINE.search(out3.stdout)
    assert m3 and m3.groups()[:4] == ("9", "9", "0", "0")
    assert np.abs(_sai_means(f"{tmp3}/denoised") / source / planted - 1.0).max() < 0.03
