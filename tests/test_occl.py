"""CPU tests of the occlusion-aware view synthesis (lfbm5d_view_*_occl_*, include/lfbm5d_occl.h): the header and the exports, the
properties of the numpy model (tests/occl_model.py) that pin the definition -- ratio 0 is the sub-pixel model in every bit, one, two
and three (corner) sources give the plain sweep, integer hypotheses of a finer sweep warp as the integer sweep, the half-planes include
the missing view's own row and column -- the quality figure the feature rests on, and the argument errors of the Python layer."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core
import helpers
import occl_cases as K
import occl_model as O
import subpel_model as S
import view_model as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lfbm5d_view_fill_occl_device", "lfbm5d_view_occl_default", "lfbm5d_view_occl_device", "lfbm5d_view_occl_host_sai"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_library_exports_and_binds_the_occlusion_entry_points():
    lib = core.lib()
    hdr = open(os.path.join(ROOT, "include", "lfbm5d.h")).read()
    assert hdr.index('#include "lfbm5d_steps.h"') < hdr.index('#include "lfbm5d_occl.h"') < hdr.rindex("#endif")
    occl = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfbm5d_occl.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(lfbm5d_[a-z0-9_]+)\s*\(", occl))) == NAMES
    assert "#define LFBM5D_VIEW_OCCL_SETS 5" in occl and O.SETS == 5
    for n in NAMES:
        assert hasattr(lib, n) and getattr(lib, n).argtypes is not None, n
    assert lib.lfbm5d_view_occl_default.restype is C.c_float and L.view_occl_default() == float(lib.lfbm5d_view_occl_default()) >= 1.0
    for n in NAMES:
        if n == "lfbm5d_view_occl_default":
            continue
        f, sibling = getattr(lib, n), getattr(lib, n.replace("_occl", "_steps"))
        assert len(f.argtypes) == len(sibling.argtypes) + 3, n                   # the ratio, the set planes, the result
        assert f.argtypes[2] is C.c_uint and f.argtypes[3] is C.c_float          # behind ctx, params and steps
        assert f.argtypes[-1]._type_ is core.ViewOcclResultStruct
    # the existing structs are unchanged, the new one holds five counters
    assert C.sizeof(core.ViewParamsStruct) == 7 * 4 and C.sizeof(core.ViewResultStruct) == 4 * 4 + 8 + 17 * 8
    assert C.sizeof(core.ViewOcclResultStruct) == 5 * 8
    assert L.ViewSynth._fields[:8] == ("out", "disparity", "missing", "synthesised", "left", "pixels", "disparity_hist", "steps_hist")
    assert L.ViewSynth._fields[8:] == ("set_hist", "sets")
    for f in (L.Context.view_fill, L.Context.view_synth):
        p = inspect.signature(f).parameters
        assert p["occlusion"].default is None and p["return_sets"].default is False and p["disparity_steps"].default == 1
    for n in ("ViewOcclResultStruct", "view_occl_default"):
        assert n in L.__all__ and hasattr(L, n)


def test_argument_errors_of_the_python_layer():
    f = L.Context._occlusion
    assert f(None) == 0.0 and f(False) == 0.0 and f(True) == L.view_occl_default() and f(8) == 8.0 and f(np.float32(1.5)) == 1.5
    assert f(0.5) == 0.5 and np.isnan(f(float("nan")))                           # the range is the library's to check
    for bad in ("auto", "4", [4.0], (1,), {}, b"4"):
        with pytest.raises(L.LfBm5dError, match="occlusion must be None, True or a ratio"):
            f(bad)
    for off in (None, False, 0, 0.0):
        with pytest.raises(L.LfBm5dError, match="need occlusion"):
            f(off, return_sets=True)
        with pytest.raises(L.LfBm5dError, match="need occlusion"):
            f(off, sets_out=np.zeros(4, np.uint8))
    assert f(True, return_sets=True) == L.view_occl_default()
    for bad in (0.5, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="occl_ratio must be 0 or a finite number of at least 1"):
            O.check_ratio(bad)


def _fields(shape, kind):
    ah, aw, H, W, C_, miss, empty, R = K.SHAPES[shape]
    lf, mask, missing = K.case(shape, kind)
    return lf, mask, missing, (K.ROWMAJOR, aw, ah, W, H, C_), R


def test_ratio_zero_is_the_sub_pixel_model_in_every_bit():
    for shape, kind, Q, D, r in (("corners", "textured", 1, 3, 3), ("centre", "textured", 2, 3, 7), ("narrow-1x3", "uniform", 4, 8, 7)):
        lf, mask, missing, dims, R = _fields(shape, kind)
        a = S.fill(lf, mask, missing, *dims, D, r, R, steps=Q)
        b = O.fill(lf, mask, missing, *dims, D, r, R, steps=Q, ratio=0.0, sets_out=np.full((len(mask), dims[3] * dims[4]), 7, np.uint8))
        assert np.array_equal(_bits(a["out"]), _bits(b["out"])) and np.array_equal(a["disp"], b["disp"]) and np.array_equal(a["hist"], b["hist"])
        assert (a["sais"], a["left_sais"], a["pixels"]) == (b["sais"], b["left_sais"], b["pixels"])
        assert (b["sets"] == 7).all() and not b["set_hist"].any()                # off: no set is written or counted


def test_one_two_and_three_sources_give_the_plain_sweep():
    """n = 1: E = 0, a copy.  n = 2: no admissible candidate, g = 1.  A corner SAI at ang_radius 1: n = 3, the candidates have 1 or 3
    members, g = 0.5 is exact.  Values and j* are the plain sweep's for every ratio."""
    for shape, kind, n in (("single-63", "uniform", 1), ("narrow-1x3", "uniform", 2), ("narrow-3x1", "textured", 2), ("corners", "textured", 3)):
        lf, mask, missing, dims, R = _fields(shape, kind)
        miss = K.SHAPES[shape][5]
        for m in miss:
            srcs = V.sources(m, mask, missing, K.ROWMAJOR, dims[1], dims[2], R)
            assert len(srcs) == n and not any(O.admissible(s, n) for s in O.sets(srcs)[1:])
        for Q, D, r in ((1, 3, 3), (2, 3, 7)):
            a = S.fill(lf, mask, missing, *dims, D, r, R, steps=Q)
            for ratio in (1.0, 4.0):
                b = O.fill(lf, mask, missing, *dims, D, r, R, steps=Q, ratio=ratio)
                assert np.array_equal(_bits(a["out"])[miss], _bits(b["out"])[miss]) and np.array_equal(a["disp"], b["disp"]), (shape, Q, ratio)
                assert b["set_hist"][0] == b["pixels"] and not b["sets"].any()
        if n == 1:
            assert np.array_equal(_bits(b["out"])[miss[0]], _bits(lf)[1 - miss[0]]) and b["hist"][S.J_MAX] == b["pixels"]


def test_the_half_planes_include_the_missing_views_own_row_and_column():
    mask, missing = np.ones(9, np.uint32), np.zeros(9, np.uint32)
    missing[4] = 1
    srcs = V.sources(4, mask, missing, V.ROWMAJOR, 3, 3, 1)
    sets = O.sets(srcs)
    assert [len(s) for s in sets] == [8, 5, 5, 5, 5]                             # strict half-planes would have 3 members
    assert [srcs[i][0] for i in sets[1]] == [0, 1, 3, 6, 7] and [srcs[i][0] for i in sets[2]] == [1, 2, 5, 7, 8]   # dt <= 0, dt >= 0
    assert [srcs[i][0] for i in sets[3]] == [0, 1, 2, 3, 5] and [srcs[i][0] for i in sets[4]] == [3, 5, 6, 7, 8]   # ds <= 0, ds >= 0
    assert all(O.admissible(s, 8) for s in sets[1:])
    missing[:] = 0
    missing[1] = 1                                                               # an edge SAI: ds >= 0 is every source
    srcs = V.sources(1, mask, missing, V.ROWMAJOR, 3, 3, 1)
    assert [len(s) for s in O.sets(srcs)] == [5, 3, 3, 2, 5] and [O.admissible(s, 5) for s in O.sets(srcs)[1:]] == [True, True, True, False]
    assert list(O.G[:4].view(np.uint32)) == list(np.array([0.0, 0.0, 1.0, 0.5], np.float32).view(np.uint32))
    assert O.G[24] == np.float32(1.0 / 23.0)


def test_integer_hypotheses_of_a_finer_sweep_warp_as_the_integer_sweep():
    lf = helpers.textured_lf(3, 3, 37, 70, 2).astype(np.float32).reshape(9, 3, 37, 70)
    mask, missing = np.ones(9, np.uint32), np.zeros(9, np.uint32)
    missing[4] = 1
    srcs = V.sources(4, mask, missing, V.ROWMAJOR, 3, 3, 1)
    for Q in (2, 4):
        for d in (-2, 0, 1):
            e1, m1 = O.set_errors(lf, srcs, d, 1)
            eq, mq = O.set_errors(lf, srcs, d * Q, Q)
            for k in range(O.SETS):
                assert np.array_equal(_bits(e1[k]), _bits(eq[k])) and np.array_equal(_bits(m1[k]), _bits(mq[k])), (Q, d, k)
    # the photograph moves 2 pixels per view: every set agrees, the full set stays, |j*| = 2 Q in the interior
    res = O.fill(lf.reshape(9, -1), mask, missing, V.ROWMAJOR, 3, 3, 70, 37, 3, 3, 3, steps=2, ratio=4.0)
    assert (np.abs(res["disp"][4].reshape(37, 70)[6:-6, 6:-6]) == 4).all() and not res["sets"][4].reshape(37, 70)[6:-6, 6:-6].any()


def test_the_choice_is_strict_and_ordered():
    e = [np.array([[8.0, 8.0, 8.0, 1.0]], np.float32), np.array([[2.0, 2.0, 1.0, 1.0]], np.float32), None,
         np.array([[2.0, 1.0, 1.0, 1.0]], np.float32), np.array([[1.0, 1.0, 1.0, 0.5]], np.float32)]
    k, v = O.choose(e, 4.0)
    assert k.tolist() == [[4, 3, 1, 0]] and v.tolist() == [[1.0, 1.0, 1.0, 1.0]]    # ties keep the earlier candidate; 0.5 * 4 < 1 is false
    k, v = O.choose(e, 1.0)
    assert k.tolist() == [[4, 3, 1, 4]]
    k, v = O.choose([e[0], None, None, None, None], 1.0)
    assert not k.any() and v is e[0]


def test_the_occluder_scene_gains_over_the_plain_sweep():
    """The rectangular-occluder scene at 96 x 96, centre missing, D = 4, r = 3, Q = 1: the exact model at the shipped ratio (4) gives
    41.32 dB on the whole SAI, the plain model (tests/view_model.py) 30.56 dB: +10.76 dB (profiles/occl.txt).  The test demands half of
    that gain: the scene is synthetic, the assertion guards the direction and the order of magnitude, not a figure."""
    lf = K.occluder_lf("rect", 3, 3, 96, 96, 3)
    mask, missing = np.ones(9, np.uint32), np.zeros(9, np.uint32)
    missing[4] = 1
    plain = V.psnr(V.fill(lf, mask, missing, V.ROWMAJOR, 3, 3, 96, 96, 3, 4, 3)["out"][4], lf[4])
    res = O.fill(lf, mask, missing, V.ROWMAJOR, 3, 3, 96, 96, 3, 4, 3, ratio=L.view_occl_default())
    occl = V.psnr(res["out"][4], lf[4])
    print(f"plain {plain:.4f} dB, occlusion-aware {occl:.4f} dB, gain {occl - plain:.4f} dB, sets {res['set_hist']}")
    assert occl - plain >= 10.76 / 2
