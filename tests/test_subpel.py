"""CPU tests of the sub-pixel plane sweep (the *_steps_* forms of lfbm5d_view_* and lfbm5d_consist_*, include/lfbm5d.h): the exports, the
properties of the numpy model (tests/subpel_model.py) that pin the definition -- steps = 1 is the integer model in every bit, integer
hypotheses of a finer sweep warp as the integer sweep does, a light field that moves half a pixel per view is found at j* = 1 of
steps = 2 -- the quality figures the feature rests on, and the CLIs' parsing of LFBM5D_DISPARITY_STEPS."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core
import consist_cases as CC
import consist_model as KM
import helpers
import subpel_model as S
import view_model as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lfbm5d_consist_steps_device", "lfbm5d_consist_steps_host_sai", "lfbm5d_view_fill_steps_device", "lfbm5d_view_steps_device",
         "lfbm5d_view_steps_host_sai"]


def test_library_exports_and_binds_the_steps_entry_points():
    lib = core.lib()
    hdr = open(os.path.join(ROOT, "include", "lfbm5d.h")).read()
    assert '#include "lfbm5d_steps.h"' in hdr
    steps = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfbm5d_steps.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(lfbm5d_[a-z0-9_]+)\s*\(", steps))) == NAMES
    assert "#define LFBM5D_VIEW_STEPS_HIST 65" in steps and core.VIEW_STEPS_HIST == S.HIST == 65
    for n in NAMES:
        assert hasattr(lib, n) and getattr(lib, n).argtypes is not None, n
        sibling = getattr(lib, n.replace("_steps", ""))
        extra = 2 if "view" in n else 1                                          # steps, and the view forms' histogram
        assert len(getattr(lib, n).argtypes) == len(sibling.argtypes) + extra, n
        assert getattr(lib, n).argtypes[2] is C.c_uint                           # behind ctx and params
    # the existing structs are unchanged
    assert C.sizeof(core.ViewParamsStruct) == 7 * 4 and C.sizeof(core.ViewResultStruct) == 4 * 4 + 8 + 17 * 8
    assert L.ViewSynth._fields[:7] == ("out", "disparity", "missing", "synthesised", "left", "pixels", "disparity_hist")
    import inspect
    for f in (L.Context.view_fill, L.Context.view_synth, L.Context.consist):
        assert inspect.signature(f).parameters["disparity_steps"].default == 1


def test_split_and_weights():
    """Q y - j ds = Q (y + o) + p with 0 <= p < Q, floor division for negative numbers."""
    for Q in S.STEPS:
        for j in range(-8 * Q, 8 * Q + 1):
            for ds in (-2, -1, 0, 1, 2):
                o, p = S.split(j, ds, Q)
                assert 0 <= p < Q and Q * o + p == -j * ds
                if j % Q == 0:
                    assert p == 0 and o == -(j // Q) * ds                        # an integer hypothesis: the integer sweep's shift
    assert [int(v) for v in S.split(1, 1, 2)] == [-1, 1] and [int(v) for v in S.split(-1, 1, 2)] == [0, 1]
    assert [int(v) for v in S.split(3, 1, 4)] == [-1, 1] and [int(v) for v in S.split(-3, 2, 4)] == [1, 2]
    a, b = np.float32(-0.0), np.float32(3.0)
    assert np.signbit(S.lerp(a, b, 0, np.float32(0.0)))                          # p = 0 returns a itself, not a + 0 (b - a)
    assert S.lerp(np.float32(1.0), np.float32(3.0), 1, np.float32(0.25)) == np.float32(1.5)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_one_step_is_the_integer_model_in_every_bit():
    """Two cases: the textured 3 x 3 field with asymmetric sources (corners), and uniform values in a plane narrower than the shift."""
    rng = np.random.default_rng(11)
    cases = [(helpers.textured_lf(3, 3, 37, 70, 2).astype(np.float32).reshape(9, -1), 3, 3, 37, 70, 3, [0, 8], 3, 3, 1),
             (rng.uniform(0.0, 255.0, (3, 5 * 3)).astype(np.float32), 1, 3, 5, 3, 1, [1], 8, 7, 1)]
    for lf, ah, aw, H, W, C_, miss, D, r, R in cases:
        mask, missing = np.ones(ah * aw, np.uint32), np.zeros(ah * aw, np.uint32)
        missing[miss] = 1
        a = V.fill(lf, mask, missing, V.ROWMAJOR, aw, ah, W, H, C_, D, r, R)
        b = S.fill(lf, mask, missing, V.ROWMAJOR, aw, ah, W, H, C_, D, r, R, steps=1)
        assert np.array_equal(_bits(a["out"]), _bits(b["out"])) and np.array_equal(a["disp"], b["disp"])
        assert np.array_equal(a["flags"], b["flags"]) and (a["sais"], a["left_sais"], a["pixels"]) == (b["sais"], b["left_sais"], b["pixels"])
        assert np.array_equal(b["hist"][S.J_MAX - V.D_MAX:S.J_MAX + V.D_MAX + 1], a["hist"]) and b["hist"].sum() == a["hist"].sum()
    for name in ("textured", "1x3"):                                             # the consistency check
        c = CC.case(name)
        kw = dict(D=3, r=3, exclude=c["exclude"], **c["params"])
        a = KM.consist(c["lf"], c["mask"], c["ang_major"], c["aw"], c["ah"], c["W"], c["H"], c["C"], **kw)
        b = S.consist(c["lf"], c["mask"], c["ang_major"], c["aw"], c["ah"], c["W"], c["H"], c["C"], steps=1, **kw)
        for key in ("flags", "state", "disp", "hist", "scale_sai", "counts", "threshold", "mu"):
            assert np.array_equal(np.asarray(a[key]).view(np.uint8), np.asarray(b[key]).view(np.uint8)), (name, key)
        assert (a["bad"], a["untested"], a["tested"], a["rounds"], a["skipped"], a["scale_channel"]) == \
               (b["bad"], b["untested"], b["tested"], b["rounds"], b["skipped"], b["scale_channel"])


def test_an_integer_translation_is_found_at_a_multiple_of_the_steps():
    """The photograph moving 2 pixels per view: steps = 4 finds |j*| = 8 in the interior and returns the integer sweep's bits there
    (E = 0 cannot be beaten by a strict <)."""
    H, W, D, r = 37, 70, 3, 3
    lf = helpers.textured_lf(3, 3, H, W, 2).astype(np.float32).reshape(9, -1)
    mask, missing = np.ones(9, np.uint32), np.zeros(9, np.uint32)
    missing[[0, 4]] = 1
    a = V.fill(lf, mask, missing, V.ROWMAJOR, 3, 3, W, H, 3, D, r)
    b = S.fill(lf, mask, missing, V.ROWMAJOR, 3, 3, W, H, 3, D, r, steps=4)
    bd = D + r
    for m in (0, 4):
        j = b["disp"][m].reshape(H, W)[bd:-bd, bd:-bd]
        assert (np.abs(j) == 8).all(), np.unique(j)
        got, want = b["out"][m].reshape(3, H, W)[:, bd:-bd, bd:-bd], a["out"][m].reshape(3, H, W)[:, bd:-bd, bd:-bd]
        assert np.array_equal(_bits(got), _bits(want))
    assert b["hist"].sum() == 2 * H * W and b["hist"][S.J_MAX - 8] + b["hist"][S.J_MAX + 8] > H * W


def test_half_a_pixel_per_view_is_found_and_gains_ten_db():
    """The photograph at 1 pixel per view and double resolution, reduced by a 2 x 2 box mean to 3 x 3 views of 48 x 80: the corner SAI
    from its three (asymmetric) sources, D = 2, r = 3, 12 px off every edge.  The centre SAI's sources are symmetric, the half-pixel
    errors cancel in the mean, and nothing is gained."""
    lf = S.half_pixel_lf()
    mask = np.ones(9, np.uint32)
    got = {}
    for m in (0, 4):
        missing = np.zeros(9, np.uint32)
        missing[m] = 1
        for Q in S.STEPS:
            res = S.fill(lf, mask, missing, V.ROWMAJOR, 3, 3, 80, 48, 3, 2, 3, steps=Q)
            got[m, Q] = S.interior_psnr(res["out"][m], lf[m], 3, 48, 80, 12)
            if (m, Q) == (0, 2):
                assert (res["disp"][m].reshape(48, 80)[12:-12, 12:-12] == 1).all()
    print(", ".join(f"SAI {m} steps {Q}: {p:.4f} dB" for (m, Q), p in got.items()))
    for key, want in (((0, 1), 27.10), ((0, 2), 36.83), ((0, 4), 36.82), ((4, 1), 36.07), ((4, 2), 36.07), ((4, 4), 36.07)):
        assert abs(got[key] - want) < 0.01, (key, got[key])


def test_the_golden_crop_figures():
    """Golden rows and columns 64..191, D = 4, r = 3, disparities up to +-4 px (the integer sweep at its best): centre and corner 0."""
    clean = np.load(os.path.join(ROOT, "tests", "golden", "sourceLF_3x3_256_u8.npy"))[:, :, 64:192, 64:192].astype(np.float32).reshape(9, -1)
    mask = np.ones(9, np.uint32)
    got = {}
    for m in (4, 0):
        missing = np.zeros(9, np.uint32)
        missing[m] = 1
        for Q in S.STEPS:
            got[m, Q] = V.psnr(S.fill(clean, mask, missing, V.ROWMAJOR, 3, 3, 128, 128, 3, 4, 3, steps=Q)["out"][m], clean[m])
    print(", ".join(f"SAI {m} steps {Q}: {p:.4f} dB" for (m, Q), p in got.items()))
    for key, want in (((4, 1), 31.88), ((4, 2), 31.99), ((4, 4), 31.98), ((0, 1), 27.11), ((0, 2), 28.01), ((0, 4), 28.06)):
        assert abs(got[key] - want) < 0.01, (key, got[key])


def _readme_args(cli, tmp, src):
    if cli.endswith("LFBM3Ddenoising"):
        return [cli, src, "SAI", "_", "2", "2", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
                f"{tmp}/denoised", f"{tmp}/diff", "16", "16", "8", "3", "bior", "0", "32", "16", "8", "3", "dct", "0", "opp", "8",
                f"{tmp}/measures.txt"]
    return [cli, src, "SAI", "_", "3", "3", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
            f"{tmp}/denoised", f"{tmp}/diff", "8", "18", "6", "16", "4", "id", "sadct", "haar", "0", "16", "18", "6", "8", "4",
            "dct", "sadct", "haar", "0", "opp", "0", f"{tmp}/measures.txt"]


@pytest.mark.parametrize("cli", ["LFBM5Ddenoising", "LFBM3Ddenoising"])
def test_cli_parses_the_disparity_steps(tmp_path, cli):
    """Malformed values and the variable on its own stop the command before it reads a file; well-formed ones get as far as the
    (missing) input files."""
    args = _readme_args(os.path.join(ROOT, "lfbm5d_amd", cli), str(tmp_path), "none")
    for bad in ("", "0", "3", "8", "2.0", " 2", "2 ", "two", "-2", "4x", "1,2"):
        for more in (dict(LFBM5D_MISSING="1_1"), dict(LFBM5D_DETECT="auto"), {}):
            r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, LFBM5D_DISPARITY_STEPS=bad, **more))
            assert r.returncode != 0 and "Read input image" not in r.stdout, (bad, more)
            assert f'LFBM5D_DISPARITY_STEPS must be 1, 2 or 4, or unset; got "{bad}"' in r.stdout, (bad, more, r.stdout[-300:])
    for good in ("1", "2", "4"):
        r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, LFBM5D_DISPARITY_STEPS=good))
        assert r.returncode != 0 and "LFBM5D_DISPARITY_STEPS needs LFBM5D_MISSING or LFBM5D_DETECT" in r.stdout, good
        assert "Read input image" not in r.stdout
        for more, first in ((dict(LFBM5D_MISSING="1_1"), "SAI_01_02"), (dict(LFBM5D_DETECT="auto"), "SAI_01_01")):
            r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, LFBM5D_IO_THREADS="1", LFBM5D_DISPARITY_STEPS=good, **more))
            assert r.returncode != 0 and "must" not in r.stdout and "needs" not in r.stdout, (good, more)
            assert f"{first}.png not found or not a correct png image" in r.stdout, (good, more, r.stdout[-300:])
