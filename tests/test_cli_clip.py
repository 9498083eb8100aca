"""LFBM5D_CLIP / LFBM5D_CLIP_ADD of both command-line tools: the values they refuse (no GPU: the command stops before it reads a file),
and on the GPU the README command on the dark 64 x 64 tile of the golden light field, clipped: the two report lines, and files closer to
the ground truth than the same command writes without LFBM5D_CLIP."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
CLI = os.path.join(ROOT, "lfbm5d_amd", "LFBM5Ddenoising")
CLI3 = os.path.join(ROOT, "lfbm5d_amd", "LFBM3Ddenoising")


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
def test_malformed_values_and_the_poisson_mode_are_refused(tmp_path, cli):
    args = _args(cli, str(tmp_path), str(tmp_path / "missing"))
    for bad in ("", "Auto", "0", "0,", ",255", "0;255", "0,255,3", "0,255x", " 0,255", "0, 255", "255,0", "5,5", "nan,255", "0,inf"):
        r = subprocess.run(args, capture_output=True, text=True, env=_env(LFBM5D_CLIP=bad))
        assert r.returncode != 0 and "LFBM5D_CLIP must be" in r.stdout, bad
        assert "Read input image" not in r.stdout, bad
    for bad in ("0", "2", "yes", ""):
        r = subprocess.run(args, capture_output=True, text=True, env=_env(LFBM5D_CLIP="auto", LFBM5D_CLIP_ADD=bad))
        assert r.returncode != 0 and "LFBM5D_CLIP_ADD must be" in r.stdout, bad
    for mode in ("poisson", "poisson:8,0"):
        r = subprocess.run(args, capture_output=True, text=True, env=_env(LFBM5D_CLIP="auto", LFBM5D_SIGMA=mode))
        assert r.returncode != 0 and "LFBM5D_CLIP cannot be combined with LFBM5D_SIGMA=poisson" in r.stdout, mode
        assert "Read input image" not in r.stdout, mode
    for good in (dict(LFBM5D_CLIP="auto"), dict(LFBM5D_CLIP="16,235"), dict(LFBM5D_CLIP="-0.5,0.5", LFBM5D_SIGMA="auto"),
                 dict(LFBM5D_CLIP="auto", LFBM5D_CLIP_ADD="1"), dict(LFBM5D_CLIP_ADD="1")):
        r = subprocess.run(args, capture_output=True, text=True, env=_env(**good))
        assert r.returncode != 0 and "LFBM5D_CLIP" not in r.stdout, good          # as far as the (missing) input files
        assert "not found or not a correct png image" in r.stdout, good


def _write_tile(tmp):
    from PIL import Image
    lf = np.load(GOLDEN)[:, :, 192:256, 128:192]
    src = os.path.join(tmp, "sourceLF")
    os.makedirs(src)
    for s in range(3):
        for t in range(3):
            Image.fromarray(np.ascontiguousarray(lf[s * 3 + t].transpose(1, 2, 0))).save(f"{src}/SAI_{s + 1:02d}_{t + 1:02d}.png")
    for d in ("noisy", "basic", "denoised", "diff"):
        os.makedirs(os.path.join(tmp, d))
    return src, lf.astype(np.float64)


def _psnr_of_files(tmp, which, clean):
    from PIL import Image
    got = np.stack([np.asarray(Image.open(f"{tmp}/{which}/SAI_{s + 1:02d}_{t + 1:02d}.png"), np.float64).transpose(2, 0, 1)
                    for s in range(3) for t in range(3)])
    return float(10.0 * np.log10(255.0 ** 2 / ((got - clean) ** 2).mean()))


def _run(cli, tmp_path, name, **env):
    tmp = str(tmp_path / name)
    os.makedirs(tmp)
    src, clean = _write_tile(tmp)
    r = subprocess.run(_args(cli, tmp, src), capture_output=True, text=True, env=_env(LFBM5D_SEED="1", **env))
    assert r.returncode == 0, r.stdout[-2000:]
    return r.stdout, {k: _psnr_of_files(tmp, k, clean) for k in ("noisy", "basic", "denoised")}


@pytest.mark.gpu
def test_cli_declips_and_estimates_on_the_clipped_tile(tmp_path):
    """Measured on an MI355X (profiles/clip.txt): LFBM5Ddenoising with LFBM5D_CLIP sigma = 25.035, denoised 32.974 dB, without it 32.439 dB;
    LFBM3Ddenoising 31.410 against 31.083 dB."""
    out, with_clip = _run(CLI, tmp_path, "clip", LFBM5D_CLIP="auto", LFBM5D_CLIP_ADD="1", LFBM5D_SIGMA="auto")
    m = re.search(r"Estimated noise level: sigma = ([0-9.eE+-]+) \(clipping-aware: (\d+) levels, censored blocks <= ([0-9.]+) %\)", out)
    assert m, out[-3000:]
    sigma, levels, pct = float(m.group(1)), int(m.group(2)), float(m.group(3))
    assert abs(sigma / 25.0 - 1.0) < 0.06 and levels >= 4 and pct in (5.0, 10.0, 20.0, 40.0, 100.0)
    d = re.search(r"Declipping: range 0\.\.255, sigma = ([0-9.eE+-]+)", out)
    assert d and float(d.group(1)) == sigma
    assert re.search(r"Round and clip \[range 0\.\.255\]: \d+ of 110592 values at the bounds", out)
    assert out.index("Estimated noise level") < out.index("Steps 1 and 2 running as one job") < out.index("Declipping:")
    plain_out, plain = _run(CLI, tmp_path, "plain", LFBM5D_CLIP_ADD="1", LFBM5D_SIGMA="auto")
    assert "clipping-aware" not in plain_out and "Declipping" not in plain_out and "Round and clip" in plain_out
    print(f"LFBM5Ddenoising on the clipped tile: with LFBM5D_CLIP sigma = {sigma}, PSNR {with_clip}; without: PSNR {plain}")
    assert abs(with_clip["noisy"] - plain["noisy"]) < 1e-9                      # the same clipped input
    assert with_clip["denoised"] > plain["denoised"] + 0.2 and with_clip["basic"] > plain["basic"]
    # LFBM3Ddenoising: run_bm3d_LF, then the inverse on both results; a given sigma and another way to write the range
    out3, with3 = _run(CLI3, tmp_path, "clip3", LFBM5D_CLIP="0,255", LFBM5D_CLIP_ADD="1")
    d = re.search(r"Declipping: range 0\.\.255, sigma = ([0-9.eE+-]+)", out3)
    assert d and float(d.group(1)) == 25.0 and "Estimated noise level" not in out3
    _, plain3 = _run(CLI3, tmp_path, "plain3", LFBM5D_CLIP_ADD="1")
    print(f"LFBM3Ddenoising on the clipped tile: with LFBM5D_CLIP PSNR {with3}; without: PSNR {plain3}")
    assert with3["denoised"] > plain3["denoised"] + 0.2
