"""LFBM5D_VIEW_SIGMA / LFBM5D_VIEW_SIGMA_ADD of both command lines (lfbm5d_cli.cpp): malformed values and the excluded combinations stop
the command before it reads a file (no GPU needed); on the GPU, the golden 3 x 3 light field as 64 x 64 files under the noise of a
devignetted capture (LFBM5D_VIEW_SIGMA_ADD=0.5) gives the report line from the estimate and from the gains; and with the variables
unset the command's output is the stored run's (tests/golden/cli_equalise_unset.json: the shape of stdout, the noisy files and the
average PSNRs of this very command, recorded before either stage existed)."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
STORED = os.path.join(ROOT, "tests", "golden", "cli_equalise_unset.json")
CLI = os.path.join(ROOT, "lfbm5d_amd", "LFBM5Ddenoising")
CLI3 = os.path.join(ROOT, "lfbm5d_amd", "LFBM3Ddenoising")
NUM = r"([0-9.eE+-]+)"
LINE = re.compile(r"Per-view noise levels: (\d+) SAIs, sigma " + NUM + r"\.\." + NUM + r" \(pooled " + NUM + r"\), from (estimate|gains); window sigmas "
                  + NUM + r"\.\." + NUM + r"\n")
PSNR = re.compile(r"- (Noisy|Basic|Denoised) light field: ([0-9.]+)")
EDGE = 0.5


def _args(cli, tmp, src, aw=3, ah=3):
    if cli == CLI3:
        return [cli, src, "SAI", "_", str(aw), str(ah), "1", "1", "1", "1", "row", "10", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
                f"{tmp}/denoised", f"{tmp}/diff", "16", "16", "8", "3", "bior", "0", "32", "16", "8", "3", "dct", "0", "opp", "8",
                f"{tmp}/measures.txt"]
    return [cli, src, "SAI", "_", str(aw), str(ah), "1", "1", "1", "1", "row", "10", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
            f"{tmp}/denoised", f"{tmp}/diff", "8", "8", "3", "8", "3", "dct", "sadct", "haar", "0", "16", "8", "3", "8", "3",
            "dct", "sadct", "haar", "0", "opp", "0", f"{tmp}/measures.txt"]


def _clean_env(**more):
    env = {k: v for k, v in os.environ.items() if not k.startswith(("LFBM5D_VIEW_SIGMA", "LFBM5D_EQUALISE"))}
    return dict(env, LFBM5D_IO_THREADS="1", **more)


@pytest.mark.parametrize("cli", [CLI, CLI3], ids=["LFBM5Ddenoising", "LFBM3Ddenoising"])
def test_cli_parses_the_view_sigma_variables(tmp_path, cli):
    src = str(tmp_path / "nowhere")

    def run(source=src, **env):
        return subprocess.run(_args(cli, str(tmp_path), source), capture_output=True, text=True, env=_clean_env(**env))
    for bad in ("", "x", "1", "Auto", "auto ", "gain", "auto,gains"):
        r = run(LFBM5D_VIEW_SIGMA=bad)
        assert r.returncode != 0 and "LFBM5D_VIEW_SIGMA must be" in r.stdout and "Read input image" not in r.stdout, bad
    for mode in ("auto", "gains"):
        more = dict(LFBM5D_EQUALISE="auto") if mode == "gains" else {}
        for sig in ("poisson", "poisson:0.5,4", "poisson-clipped"):
            r = run(LFBM5D_VIEW_SIGMA=mode, LFBM5D_SIGMA=sig)
            assert r.returncode != 0 and "LFBM5D_VIEW_SIGMA cannot be combined with LFBM5D_SIGMA=poisson" in r.stdout and "not found" not in r.stdout
        r = run(LFBM5D_VIEW_SIGMA=mode, LFBM5D_CLIP="auto", **more)
        assert r.returncode != 0 and "cannot be combined with LFBM5D_CLIP" in r.stdout and "not found" not in r.stdout
    r = run(LFBM5D_VIEW_SIGMA="gains")
    assert r.returncode != 0 and "LFBM5D_VIEW_SIGMA=gains needs LFBM5D_EQUALISE" in r.stdout and "not found" not in r.stdout
    r = run(LFBM5D_VIEW_SIGMA="gains", LFBM5D_EQUALISE="auto", LFBM5D_SIGMA="auto")
    assert r.returncode != 0 and "needs a numeric sigma" in r.stdout and "LFBM5D_VIEW_SIGMA=auto" in r.stdout and "not found" not in r.stdout
    r = run(LFBM5D_VIEW_SIGMA="auto", LFBM5D_DETECT="auto")
    assert r.returncode != 0 and "LFBM5D_VIEW_SIGMA cannot be combined with LFBM5D_MISSING, LFBM5D_DEFECTS or LFBM5D_DETECT" in r.stdout
    for bad in ("", "x", "0", "-0.5", "1.01", " 0.5", "0.5x", "nan", "inf"):
        r = run(LFBM5D_VIEW_SIGMA_ADD=bad)
        assert r.returncode != 0 and "LFBM5D_VIEW_SIGMA_ADD must be" in r.stdout and "not found" not in r.stdout, bad
    r = run(source="none", LFBM5D_VIEW_SIGMA_ADD="0.5")
    assert r.returncode != 0 and "LFBM5D_VIEW_SIGMA_ADD needs a source light field" in r.stdout and "not found" not in r.stdout
    r = run(LFBM5D_VIEW_SIGMA_ADD="0.5", LFBM5D_SIGMA="poisson:0.5,4")
    assert r.returncode != 0 and "LFBM5D_VIEW_SIGMA_ADD cannot be combined with LFBM5D_SIGMA=poisson" in r.stdout
    for good in (dict(LFBM5D_VIEW_SIGMA="auto"), dict(LFBM5D_VIEW_SIGMA="auto", LFBM5D_SIGMA="auto"), dict(LFBM5D_VIEW_SIGMA_ADD="1"),
                 dict(LFBM5D_VIEW_SIGMA="gains", LFBM5D_EQUALISE="flat", LFBM5D_VIEW_SIGMA_ADD="0.5"),
                 dict(LFBM5D_VIEW_SIGMA="auto", LFBM5D_IMPULSE="auto", LFBM5D_EQUALISE="auto")):
        r = run(**good)                                                         # well-formed: as far as the (missing) input files
        assert r.returncode != 0 and "must" not in r.stdout and "cannot" not in r.stdout and "needs" not in r.stdout, good
        assert "SAI_01_01.png not found or not a correct png image" in r.stdout, (good, r.stdout[-300:])


def _out_dirs(tmp):
    for d in ("noisy", "basic", "denoised", "diff"):
        os.makedirs(os.path.join(tmp, d), exist_ok=True)


def _write_fixture(tmp):
    """Golden rows and columns 96..159 as 3 x 3 files of 64 x 64."""
    from PIL import Image
    lf = np.load(GOLDEN)[:, :, 96:160, 96:160].copy()
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


@pytest.mark.gpu
def test_cli_reports_the_view_sigmas_and_is_unchanged_without_them(tmp_path):
    tmp = str(tmp_path)
    src = _write_fixture(tmp)
    # every variable unset: the stored run's output
    plain = subprocess.run(_args(CLI, tmp, src), capture_output=True, text=True,
                           env={k: v for k, v in _clean_env(LFBM5D_SEED="1").items() if k != "LFBM5D_IO_THREADS"})
    assert plain.returncode == 0, plain.stdout[-2000:]
    assert "Per-view noise levels" not in plain.stdout and "vignette" not in plain.stdout
    stored = json.load(open(STORED))
    files = sorted(os.listdir(f"{tmp}/noisy"))
    assert _shape_of(plain.stdout, tmp) == stored["stdout_shape"]
    assert {f: hashlib.sha256(open(f"{tmp}/noisy/{f}", "rb").read()).hexdigest() for f in files} == stored["noisy_sha256"]
    psnr = {k: float(v) for k, v in PSNR.findall(plain.stdout)}
    for k, v in stored["psnr"].items():
        assert abs(psnr[k] - v) < 0.02, (k, psnr[k], v)
    # the noise of a devignetted capture: corner views carry sigma / 0.5, edge views sigma / 0.75
    for cli, sub in ((CLI, "a"), (CLI3, "b")):
        t = os.path.join(tmp, sub)
        _out_dirs(t)
        out = subprocess.run(_args(cli, t, src), capture_output=True, text=True,
                             env=_clean_env(LFBM5D_SEED="1", LFBM5D_VIEW_SIGMA="auto", LFBM5D_VIEW_SIGMA_ADD=str(EDGE)))
        assert out.returncode == 0, out.stdout[-2000:]
        m = LINE.search(out.stdout)
        assert m and "Add noise [sigma = 10 / vignette, corner views x 0.5]" in out.stdout, out.stdout[-2000:]
        print(os.path.basename(cli), m.group(0).strip())
        n, lo, hi, pooled, source, wlo, whi = m.groups()
        assert int(n) == 9 and source == "estimate"
        # (how close the per-SAI estimate comes on 64 x 64 views is the estimator's business, tools/views_time.py measures it: here only that
        # the centre's 10 and the corners' 20 are told apart, and the line is consistent with itself)
        assert 0.0 < float(lo) < float(hi) and float(lo) <= float(pooled) <= float(hi)
        if cli == CLI:
            assert float(wlo) == float(whi) and abs(float(wlo) - float(pooled)) < 1e-3 * float(pooled)   # one window: the root mean square
            assert out.stdout.index("Per-view noise levels:") > out.stdout.index("Steps 1 and 2 running as one job")
        else:
            assert abs(float(wlo) - float(lo)) < 1e-3 * float(lo) and abs(float(whi) - float(hi)) < 1e-3 * float(hi)   # every SAI its own
        p = {k: float(v) for k, v in PSNR.findall(out.stdout)}
        assert p["Denoised"] > p["Noisy"] + 3
    # from the gains: a planted vignette equalised away leaves sigma / g
    t = os.path.join(tmp, "c")
    _out_dirs(t)
    out = subprocess.run(_args(CLI, t, src), capture_output=True, text=True,
                         env=_clean_env(LFBM5D_SEED="1", LFBM5D_VIEW_SIGMA="gains", LFBM5D_EQUALISE="auto", LFBM5D_EQUALISE_ADD="0.6"))
    assert out.returncode == 0, out.stdout[-2000:]
    m = LINE.search(out.stdout)
    assert m and m.group(5) == "gains", out.stdout[-2000:]
    print("gains", m.group(0).strip())
    # the gains are free up to a common factor (their lower median is 1): the ratio of the extremes is the vignette's, within the 5 % of
    # tests/test_cli_equalise.py
    assert abs(float(m.group(2)) / float(m.group(3)) - 0.6) < 0.05 * 0.6
