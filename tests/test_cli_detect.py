"""LFBM5D_DETECT of both command lines (lfbm5d_cli.cpp): malformed values and the combinations with LFBM5D_DEFECTS / LFBM5D_MISSING stop the
command before it reads a file (no GPU needed); on the GPU, a 3 x 3 x 64 x 64 light field with one dimmed SAI and a planted block gives the
report line, the bad SAI goes through the view synthesis and the flagged values through the defect inpainting, LFBM5D_DETECT_SAVE writes
maps that LFBM5D_DEFECTS reads back, and with the variable unset the command's output is the stored run's
(tests/golden/cli_detect_unset.json: the shape of stdout and the noisy files of the same command, recorded on an MI355X)."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy")
STORED = os.path.join(ROOT, "tests", "golden", "cli_detect_unset.json")
CLI = os.path.join(ROOT, "lfbm5d_amd", "LFBM5Ddenoising")
CLI3 = os.path.join(ROOT, "lfbm5d_amd", "LFBM3Ddenoising")
BLOCK = (slice(20, 26), slice(30, 36))            # rows, columns of the planted block in SAI_02_02
LINE = re.compile(r"Consistency check: (\d+) of (\d+) SAIs bad \[([0-9_ ]*)\], (\d+) of (\d+) values flagged \(([0-9.eE+-]+) %\), (\d+) SAIs untested; "
                  r"scales ([0-9.eE+-]+) ([0-9.eE+-]+) ([0-9.eE+-]+); (\d+) sweeps")


def _args(cli, tmp, src, aw=3, ah=3):
    if cli == CLI3:
        return [cli, src, "SAI", "_", str(aw), str(ah), "1", "1", "1", "1", "row", "10", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
                f"{tmp}/denoised", f"{tmp}/diff", "16", "16", "8", "3", "bior", "0", "32", "16", "8", "3", "dct", "0", "opp", "8",
                f"{tmp}/measures.txt"]
    return [cli, src, "SAI", "_", str(aw), str(ah), "1", "1", "1", "1", "row", "10", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
            f"{tmp}/denoised", f"{tmp}/diff", "8", "8", "3", "8", "3", "dct", "sadct", "haar", "0", "16", "8", "3", "8", "3",
            "dct", "sadct", "haar", "0", "opp", "0", f"{tmp}/measures.txt"]


@pytest.mark.parametrize("cli", [CLI, CLI3], ids=["LFBM5Ddenoising", "LFBM3Ddenoising"])
def test_cli_parses_the_detect_variables(tmp_path, cli):
    args = _args(cli, str(tmp_path), "none")

    def run(**env):
        return subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, LFBM5D_IO_THREADS="1", **env))
    for bad in ("", "x", "-1", " 2", "2x", "nan", "inf", "Auto"):
        r = run(LFBM5D_DETECT=bad)
        assert r.returncode != 0 and "LFBM5D_DETECT must be" in r.stdout and "Read input image" not in r.stdout, bad
    r = run(LFBM5D_DETECT="auto", LFBM5D_DEFECTS=str(tmp_path))
    assert r.returncode != 0 and "LFBM5D_DETECT cannot be combined with LFBM5D_DEFECTS" in r.stdout and "not found" not in r.stdout
    r = run(LFBM5D_DETECT="auto", LFBM5D_MISSING="1_1")
    assert r.returncode != 0 and "LFBM5D_DETECT cannot be combined with LFBM5D_MISSING" in r.stdout and "not found" not in r.stdout
    r = run(LFBM5D_DETECT_SAVE=str(tmp_path))
    assert r.returncode != 0 and "LFBM5D_DETECT_SAVE needs LFBM5D_DETECT" in r.stdout and "not found" not in r.stdout
    r = run(LFBM5D_DETECT="8", LFBM5D_DETECT_SAVE="")
    assert r.returncode != 0 and "LFBM5D_DETECT_SAVE must name a directory" in r.stdout and "not found" not in r.stdout
    for good in (dict(LFBM5D_DETECT="auto"), dict(LFBM5D_DETECT="6.5", LFBM5D_DETECT_SAVE=str(tmp_path)), dict(LFBM5D_DETECT="0")):
        r = run(**good)                                                         # well-formed: as far as the (missing) input files
        assert r.returncode != 0 and "must" not in r.stdout and "cannot" not in r.stdout, good
        assert "SAI_01_01.png not found or not a correct png image" in r.stdout, (good, r.stdout[-300:])


def _write_fixture(tmp):
    """Golden rows and columns 96..159 as 3 x 3 files of 64 x 64; SAI_01_02 at half its brightness, a 6 x 6 block of SAI_02_02 written
    as 0 or 255 (whichever is farther from the value)."""
    from PIL import Image
    lf = np.load(GOLDEN)[:, :, 96:160, 96:160].copy()
    lf[1] = lf[1] // 2
    blk = lf[4][(slice(None),) + BLOCK]
    lf[4][(slice(None),) + BLOCK] = np.where(blk > 127, 0, 255)
    src = os.path.join(tmp, "sourceLF")
    os.makedirs(src)
    for s in range(3):
        for t in range(3):
            Image.fromarray(lf[s * 3 + t].transpose(1, 2, 0)).save(f"{src}/SAI_{s + 1:02d}_{t + 1:02d}.png")
    _out_dirs(tmp)
    return src


def _out_dirs(tmp):
    for d in ("noisy", "basic", "denoised", "diff"):
        os.makedirs(os.path.join(tmp, d), exist_ok=True)


def _shape_of(stdout, tmp, drop=()):
    """stdout with the working directory's name, every number and the lines of the stages named in `drop` taken out: what stays the same
    from run to run."""
    lines = [l for l in stdout.replace(tmp, "TMP").replace("\r", "\n").split("\n") if not any(w in l for w in drop)]
    return re.sub(r"\n+", "\n", re.sub(r"[0-9.eE+-]+", "#", "\n".join(lines)))


def record_unset(tmp):
    """The command of the tests with every LFBM5D_DETECT variable unset: what tests/golden/cli_detect_unset.json stores."""
    src = _write_fixture(tmp)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LFBM5D_DETECT")}
    r = subprocess.run(_args(CLI, tmp, src), capture_output=True, text=True, env=dict(env, LFBM5D_SEED="1"))
    assert r.returncode == 0, r.stdout[-2000:]
    files = sorted(os.listdir(f"{tmp}/noisy"))
    return r, dict(stdout_shape=_shape_of(r.stdout, tmp), noisy_sha256={f: hashlib.sha256(open(f"{tmp}/noisy/{f}", "rb").read()).hexdigest() for f in files})


@pytest.mark.gpu
def test_cli_detects_synthesises_and_fills(tmp_path):
    from PIL import Image
    tmp = str(tmp_path)
    plain, rec = record_unset(tmp)
    assert "Consistency check" not in plain.stdout
    assert rec == json.load(open(STORED))                                       # unset: the stored run's stdout shape and noisy files
    src = os.path.join(tmp, "sourceLF")
    save = os.path.join(tmp, "maps")
    os.makedirs(save)
    env = dict(os.environ, LFBM5D_SEED="1")
    det = dict(env, LFBM5D_DETECT="auto", LFBM5D_DETECT_SAVE=save, LFBM5D_MISSING_ITER="1", LFBM5D_DEFECTS_ITER="1", LFBM5D_SIGMA="auto")
    out = subprocess.run(_args(CLI, tmp, src), capture_output=True, text=True, env=det)
    assert out.returncode == 0, out.stdout[-2000:]
    m = LINE.search(out.stdout)
    assert m, out.stdout[-2000:]
    print(m.group(0))
    bad, A, names, n, N, pct, untested, s0, s1, s2, sweeps = m.groups()
    assert (int(bad), int(A), names, int(N), int(sweeps)) == (1, 9, "1_2", 9 * 3 * 64 * 64, 2)
    assert 100 <= int(n) <= N_MAX and abs(float(pct) - 100.0 * int(n) / int(N)) < 1e-3 and min(float(s0), float(s1), float(s2)) > 0.0
    # the bad SAI through the view synthesis, the flagged values through the defect inpainting, each with its report line, in that order,
    # ahead of the noise estimate
    v = re.search(r"View synthesis: 1 of 9 SAIs missing, 0 left; disparities (-?\d+)\.\.(-?\d+), 1 refinement steps", out.stdout)
    f = re.search(r"Defect inpainting: (\d+) of (\d+) values flagged \(([0-9.eE+-]+) %\), 0 left; (\d+) fill passes, 1 refinement steps", out.stdout)
    assert v and f, out.stdout[-2000:]
    assert int(f.group(1)) == int(n) and int(f.group(2)) == int(N)               # exactly the detected map
    pos = [out.stdout.index(w) for w in ("Consistency check:", "View synthesis:", "Defect inpainting:", "Estimated noise level:")]
    assert pos == sorted(pos)
    assert _shape_of(out.stdout, tmp, ("Consistency check", "View synthesis", "Defect inpainting", "Estimated noise level")) == \
        _shape_of(plain.stdout, tmp, ("Estimated noise level",))                     # nothing else is printed
    for name, h in rec["noisy_sha256"].items():                                 # the noisy files are saved before anything is repaired
        assert hashlib.sha256(open(f"{tmp}/noisy/{name}", "rb").read()).hexdigest() == h, name
    # the saved maps: LFBM5D_DEFECTS' format, the list in LFBM5D_MISSING's
    assert open(f"{save}/missing.txt").read().strip() == "1_2"
    maps = {name: np.asarray(Image.open(f"{save}/{name}")) for name in sorted(os.listdir(save)) if name.endswith(".png")}
    assert sorted(maps) == sorted(rec["noisy_sha256"]) and all(a.shape == (64, 64, 3) and set(np.unique(a)) <= {0, 255} for a in maps.values())
    assert sum(int((a != 0).sum()) for a in maps.values()) == int(n)
    assert not maps["SAI_01_02.png"].any()                                      # a bad SAI carries no flags
    assert int((maps["SAI_02_02.png"][BLOCK] != 0).sum()) >= 100                # the planted block (108 values)
    # the dimmed SAI was reconstructed: closer to the undimmed view than the dimmed file is
    true = np.load(GOLDEN)[1, :, 96:160, 96:160].transpose(1, 2, 0).astype(np.float64)
    rec_sai = np.asarray(Image.open(f"{tmp}/denoised/SAI_01_02.png")).astype(np.float64)
    dim = np.asarray(Image.open(f"{src}/SAI_01_02.png")).astype(np.float64)
    psnr = lambda a: 10.0 * np.log10(255.0 ** 2 / ((a - true) ** 2).mean())
    print(f"SAI_01_02: dimmed file {psnr(dim):.2f} dB, reconstructed and denoised {psnr(rec_sai):.2f} dB")
    assert psnr(rec_sai) > psnr(dim) + 6.0
    # a camera's fixed map can be reused: the saved maps as LFBM5D_DEFECTS give the same count
    again = subprocess.run(_args(CLI, tmp, src), capture_output=True, text=True, env=dict(env, LFBM5D_DEFECTS=save, LFBM5D_DEFECTS_ITER="0"))
    assert again.returncode == 0, again.stdout[-2000:]
    g = re.search(r"Defect inpainting: (\d+) of (\d+) values flagged", again.stdout)
    assert g and int(g.group(1)) == int(n)
    # LFBM3Ddenoising: the same check, the synthesis and the fill alone
    tmp3 = os.path.join(tmp, "bm3d")
    _out_dirs(tmp3)
    out3 = subprocess.run(_args(CLI3, tmp3, src), capture_output=True, text=True, env=dict(env, LFBM5D_DETECT="auto"))
    assert out3.returncode == 0, out3.stdout[-2000:]
    m3 = LINE.search(out3.stdout)
    assert m3 and m3.groups()[:5] == m.groups()[:5]                             # the same noisy light field, the same findings
    assert "the synthesis alone" in out3.stdout and "the fill alone" in out3.stdout


N_MAX = 9 * 3 * 64 * 64 // 50                     # 2 % of the values: the block is 108, the model flags about 200 on this input
