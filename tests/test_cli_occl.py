"""LFBM5D_OCCLUSION of both command-line tools: the values they refuse and the variable without a synthesis to apply it to (no GPU: the
command stops before it reads a file), and on the GPU LFBM5D_MISSING on the rectangular-occluder scene written as PNGs: the report line
with the variable, the line and the files as they were without it, and a missing SAI that comes back closer to the truth with it."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "lfbm5d_amd", "LFBM5Ddenoising")
CLI3 = os.path.join(ROOT, "lfbm5d_amd", "LFBM3Ddenoising")
OLD_LINE = r"View synthesis: 1 of 9 SAIs missing, 0 left; disparities -?\d+\.\.-?\d+, \d+ refinement steps"
NEW_TAIL = r", occlusion ratio ([0-9.]+): ([0-9]+\.[0-9]) % of the positions from a half-plane"


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


@pytest.mark.parametrize("cli", [CLI, CLI3], ids=["LFBM5Ddenoising", "LFBM3Ddenoising"])
def test_cli_parses_the_occlusion_variable(tmp_path, cli):
    args = _args(cli, str(tmp_path), str(tmp_path / "none"))
    for bad in ("", "Auto", "0", "0.5", "0.999", "-1", "-4", "nan", "inf", "+4", " 4", "4 ", "4x", "0x10", "0X1p4", "four", "1,2"):
        for more in (dict(LFBM5D_MISSING="1_1"), dict(LFBM5D_DETECT="auto"), {}):
            r = subprocess.run(args, capture_output=True, text=True, env=_env(LFBM5D_OCCLUSION=bad, **more))
            assert r.returncode != 0 and "Read input image" not in r.stdout, (bad, more)
            assert f'LFBM5D_OCCLUSION must be "auto" (the library\'s ratio) or a finite ratio >= 1, or unset; got "{bad}"' in r.stdout, \
                (bad, more, r.stdout[-300:])
    for good in ("auto", "1", "1.5", "4", "8.0", "1e2"):
        r = subprocess.run(args, capture_output=True, text=True, env=_env(LFBM5D_OCCLUSION=good))
        assert r.returncode != 0 and "LFBM5D_OCCLUSION needs LFBM5D_MISSING or LFBM5D_DETECT" in r.stdout, good
        assert "Read input image" not in r.stdout
        for more in (dict(LFBM5D_MISSING="1_1"), dict(LFBM5D_DETECT="auto")):   # as far as the (missing) input files
            r = subprocess.run(args, capture_output=True, text=True, env=_env(LFBM5D_IO_THREADS="1", LFBM5D_OCCLUSION=good, **more))
            assert r.returncode != 0 and "must" not in r.stdout and "needs" not in r.stdout, (good, more)
            assert ".png not found or not a correct png image" in r.stdout, (good, more, r.stdout[-300:])


def _write_scene(tmp):
    from PIL import Image
    import occl_cases as K
    lf = np.clip(np.rint(K.occluder_lf("rect", 3, 3, 64, 64, 3).reshape(9, 3, 64, 64)), 0, 255).astype(np.uint8)
    src = os.path.join(tmp, "sourceLF")
    os.makedirs(src)
    for s in range(3):
        for t in range(3):
            Image.fromarray(np.ascontiguousarray(lf[s * 3 + t].transpose(1, 2, 0))).save(f"{src}/SAI_{s + 1:02d}_{t + 1:02d}.png")
    for d in ("noisy", "basic", "denoised", "diff"):
        os.makedirs(os.path.join(tmp, d))
    return src, lf.astype(np.float64)


def _run(cli, tmp_path, name, **env):
    from PIL import Image
    tmp = str(tmp_path / name)
    os.makedirs(tmp)
    src, clean = _write_scene(tmp)
    r = subprocess.run(_args(cli, tmp, src), capture_output=True, text=True, env=_env(LFBM5D_SEED="1", LFBM5D_MISSING="2_2", **env))
    assert r.returncode == 0, r.stdout[-2000:]
    line = [l for l in r.stdout.split("\n") if l.startswith("View synthesis: 1 of")][0]
    files = {k: open(f"{tmp}/{k}/SAI_02_02.png", "rb").read() for k in ("noisy", "denoised")}
    rec = np.asarray(Image.open(f"{tmp}/denoised/SAI_02_02.png")).astype(np.float64).transpose(2, 0, 1)
    return line, files, float(10.0 * np.log10(255.0 ** 2 / ((rec - clean[4]) ** 2).mean()))


@pytest.mark.gpu
def test_cli_reports_and_reconstructs_with_the_occlusion_variable(tmp_path):
    """The centre SAI of the occluder scene (64 x 64, noise of sigma 10 added by the command, one refinement step, then the denoiser).
    The exact model's clean synthesis of the 96 x 96 scene gains 10 dB (profiles/occl.txt); here the denoised file must be closer to the
    truth with the variable than without."""
    plain, files, psnr_plain = _run(CLI, tmp_path, "plain", LFBM5D_MISSING_ITER="1")
    print(plain)
    # without the variable the line is the former text, letter for letter (as the command printed it before the variable existed)
    assert plain == "View synthesis: 1 of 9 SAIs missing, 0 left; disparities -4..4, 1 refinement steps"
    again, files2, _ = _run(CLI, tmp_path, "again", LFBM5D_MISSING_ITER="1")
    assert again == plain and files == files2                                   # and a second run writes the same files
    line, occl_files, psnr_occl = _run(CLI, tmp_path, "occl", LFBM5D_MISSING_ITER="1", LFBM5D_OCCLUSION="auto")
    m = re.fullmatch(OLD_LINE + NEW_TAIL, line)
    assert m and float(m.group(1)) == 4.0 and 0.0 < float(m.group(2)) < 100.0, line
    assert occl_files["denoised"] != files["denoised"]                          # another synthesis went into the files
    print(f"LFBM5Ddenoising, centre SAI of the occluder scene: {psnr_plain:.2f} dB without, {psnr_occl:.2f} dB with LFBM5D_OCCLUSION=auto")
    assert psnr_occl > psnr_plain
    both, _, _ = _run(CLI, tmp_path, "steps", LFBM5D_MISSING_ITER="1", LFBM5D_OCCLUSION="2.5", LFBM5D_DISPARITY_STEPS="2")
    m = re.search(r", 1 refinement steps, 2 steps per pixel" + NEW_TAIL + "$", both)
    assert m and float(m.group(1)) == 2.5, both
    line3, _, _ = _run(CLI3, tmp_path, "bm3d", LFBM5D_OCCLUSION="8")            # LFBM3Ddenoising: the synthesis alone
    m = re.fullmatch(OLD_LINE + NEW_TAIL, line3)
    assert m and float(m.group(1)) == 8.0 and float(m.group(2)) > 0.0, line3
