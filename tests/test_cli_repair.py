"""LFBM5D_REPAIR of both command lines (lfbm5d_cli.cpp): malformed values and the refused combinations stop the command before it reads
a file (no GPU needed); on the GPU, the golden 3 x 3 light field as 64 x 64 files with LFBM5D_DEFECTS + LFBM5D_MISSING, and with
LFBM5D_DETECT=auto, go through one joint job: the report line and the files written; and with the variable unset a plain command's
output is the stored run's (tests/golden/cli_equalise_unset.json, read only: the same command and fixture as tests/test_cli_equalise.py)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from lfbm5d_amd import synth
import test_cli_equalise as E

CLI, CLI3 = E.CLI, E.CLI3
LINE = re.compile(r"Joint repair: (\d+) of (\d+) values flagged \(([0-9.eE+-]+) %\), (\d+) of (\d+) SAIs missing; (\d+) values from other views, "
                  r"(\d+) from the rim, (\d+) left; disparities (-?\d+)\.\.(-?\d+), (\d+) refinement steps")


def _env(**more):
    env = {k: v for k, v in os.environ.items() if not k.startswith(("LFBM5D_REPAIR", "LFBM5D_DEFECTS", "LFBM5D_MISSING", "LFBM5D_DETECT"))}
    return dict(env, LFBM5D_IO_THREADS="1", **more)


@pytest.mark.parametrize("cli", [CLI, CLI3], ids=["LFBM5Ddenoising", "LFBM3Ddenoising"])
def test_cli_parses_the_repair_variables(tmp_path, cli):
    args = E._args(cli, str(tmp_path), str(tmp_path / "nowhere"))

    def run(**env):
        return subprocess.run(args, capture_output=True, text=True, env=_env(**env))

    def refused(r, text):
        return r.returncode != 0 and text in r.stdout and "not found" not in r.stdout and "Read input image" not in r.stdout
    d = str(tmp_path)
    for bad in ("", "x", "1", "Joint", "joint ", "joint,auto"):
        assert refused(run(LFBM5D_REPAIR=bad, LFBM5D_MISSING="1_1"), "LFBM5D_REPAIR must be"), bad
    for bad in ("bogus", "", "-1", "1.5", " 2", "2x", "1001"):
        assert refused(run(LFBM5D_REPAIR="joint", LFBM5D_MISSING="1_1", LFBM5D_REPAIR_ITER=bad), "LFBM5D_REPAIR_ITER must be"), bad
    assert refused(run(LFBM5D_REPAIR_ITER="2"), "LFBM5D_REPAIR_ITER needs LFBM5D_REPAIR")
    assert refused(run(LFBM5D_REPAIR="joint"), "LFBM5D_REPAIR needs LFBM5D_DEFECTS, LFBM5D_MISSING or LFBM5D_DETECT")
    both = dict(LFBM5D_REPAIR="joint", LFBM5D_MISSING="2_2", LFBM5D_DEFECTS=d)
    for steps in ("2", "4", "x"):
        assert refused(run(LFBM5D_DISPARITY_STEPS=steps, **both), "LFBM5D_REPAIR cannot be combined with LFBM5D_DISPARITY_STEPS other than 1"), steps
    assert refused(run(LFBM5D_OCCLUSION="auto", **both), "LFBM5D_REPAIR cannot be combined with LFBM5D_OCCLUSION")
    for s in ("poisson", "poisson:0.5,4", "poisson-clipped"):
        assert refused(run(LFBM5D_SIGMA=s, **both), "LFBM5D_REPAIR cannot be combined with LFBM5D_SIGMA=poisson"), s
    assert refused(run(LFBM5D_VIEW_SIGMA="auto", **both), "LFBM5D_REPAIR cannot be combined with LFBM5D_VIEW_SIGMA")
    assert refused(run(LFBM5D_DETECT="auto", LFBM5D_REPAIR="joint", LFBM5D_DEFECTS=d), "LFBM5D_DETECT cannot be combined with LFBM5D_DEFECTS")
    # unset, the old rejection stands
    assert refused(run(LFBM5D_MISSING="2_2", LFBM5D_DEFECTS=d), "LFBM5D_MISSING cannot be combined with LFBM5D_DEFECTS")
    for good in (both, dict(both, LFBM5D_REPAIR_ITER="0", LFBM5D_DISPARITY_STEPS="1"), dict(LFBM5D_REPAIR="joint", LFBM5D_DEFECTS=d),
                 dict(LFBM5D_REPAIR="joint", LFBM5D_MISSING="1_1,3_3"), dict(LFBM5D_REPAIR="joint", LFBM5D_DETECT="auto")):
        r = run(**good)                                                         # well-formed: as far as the (missing) input files
        assert r.returncode != 0 and "must" not in r.stdout and "cannot" not in r.stdout and "needs" not in r.stdout, good
        assert "SAI_01_01.png not found or not a correct png image" in r.stdout, (good, r.stdout[-300:])


def _write_maps(tmp):
    """The defect maps of add_defects(seed=2) as 8-bit PNGs named like the SAIs; returns (directory, the boolean maps [9][64][64])."""
    from PIL import Image
    fl = synth.add_defects((9, 3, 64, 64), 2)[:, 0]
    d = os.path.join(tmp, "maps")
    os.makedirs(d)
    for s in range(3):
        for t in range(3):
            Image.fromarray((fl[s * 3 + t] * 255).astype(np.uint8)).save(f"{d}/SAI_{s + 1:02d}_{t + 1:02d}.png")
    return d, fl


def _image(path):
    from PIL import Image
    return np.asarray(Image.open(path)).astype(np.float64)


def _psnr(a, b, where=None):
    e = (a - b) ** 2
    return 10.0 * np.log10(255.0 ** 2 / (e[where] if where is not None else e).mean())


@pytest.mark.gpu
def test_cli_repairs_defects_and_a_missing_view_in_one_job(tmp_path):
    tmp = str(tmp_path)
    plain, rec = E.record_unset(tmp)
    assert "Joint repair" not in plain.stdout
    stored = json.load(open(E.STORED))
    assert rec["stdout_shape"] == stored["stdout_shape"] and rec["noisy_sha256"] == stored["noisy_sha256"]   # unset: the stored run's output
    for k, v in stored["psnr"].items():
        assert abs(rec["psnr"][k] - v) < 0.02, (k, rec["psnr"][k], v)
    src = os.path.join(tmp, "sourceLF")
    maps, fl = _write_maps(tmp)
    for cli, steps in ((CLI, "2"), (CLI3, None)):
        env = dict(LFBM5D_SEED="1", LFBM5D_REPAIR="joint", LFBM5D_DEFECTS=maps, LFBM5D_MISSING="2_2")
        if steps:
            env["LFBM5D_REPAIR_ITER"] = steps
        r = subprocess.run(E._args(cli, tmp, src), capture_output=True, text=True, env=_env(**env))
        assert r.returncode == 0, r.stdout[-2000:]
        assert "Defect inpainting" not in r.stdout and "View synthesis" not in r.stdout
        m = LINE.findall(r.stdout)
        assert len(m) == 1, r.stdout[-2000:]
        n, N, pct, b, A, v, rim, left, dmin, dmax, K = m[0]
        assert (int(n), int(N), int(b), int(A)) == (3 * int(fl.sum()), 9 * 3 * 64 * 64, 1, 9)
        assert abs(float(pct) - 100.0 * 3 * fl.sum() / (9 * 3 * 64 * 64)) < 1e-3
        unsound = 3 * int((fl | (np.arange(9) == 4)[:, None, None]).sum())
        assert int(v) + int(rim) + int(left) == unsound and int(left) == 0 and int(v) > int(rim)
        assert -4 <= int(dmin) <= int(dmax) <= 4 and int(K) == (2 if steps else 0)
        if cli == CLI3:
            assert "Joint repair: the fill alone" in r.stdout
        # the files written: the repaired SAI 2_2 is a view again, not the zeros it was dropped to
        den, ref = _image(f"{tmp}/denoised/SAI_02_02.png"), _image(f"{src}/SAI_02_02.png")
        assert _psnr(den, ref) > 25.0, _psnr(den, ref)
        for d in ("basic", "denoised", "diff"):
            assert len(os.listdir(f"{tmp}/{d}")) == 9


@pytest.mark.gpu
def test_cli_hands_what_the_check_detects_to_one_joint_job(tmp_path):
    """The fixture of tests/test_cli_detect.py: SAI_01_02 at half its brightness, a 6 x 6 block planted in SAI_02_02."""
    import test_cli_detect as T
    tmp = str(tmp_path)
    src = T._write_fixture(tmp)
    r = subprocess.run(E._args(CLI, tmp, src), capture_output=True, text=True,
                       env=_env(LFBM5D_SEED="1", LFBM5D_DETECT="auto", LFBM5D_REPAIR="joint", LFBM5D_REPAIR_ITER="1"))
    assert r.returncode == 0, r.stdout[-2000:]
    det, m = T.LINE.findall(r.stdout), LINE.findall(r.stdout)
    assert len(det) == 1 and len(m) == 1, r.stdout[-2000:]
    assert "Defect inpainting" not in r.stdout and "View synthesis" not in r.stdout          # one job in place of the two
    bad, flagged = int(det[0][0]), int(det[0][3])
    n, N, pct, b, A, v, rim, left, dmin, dmax, K = m[0]
    assert (int(b), int(A), int(K)) == (bad, 9, 1) and bad >= 1
    assert 36 <= int(n) <= 3 * 9 * 64 * 64 and flagged > 0 and int(left) == 0 and int(v) > 0
    assert len(os.listdir(f"{tmp}/denoised")) == 9
