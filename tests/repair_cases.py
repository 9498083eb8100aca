"""The light fields the joint repair is compared on (tests/test_gpu_repair.py against the GPU, tools/repair_host_check.py against the
kernels' per-thread code compiled for the host), and the model's answer to each, computed once per process.  Parameters are spelled out
here, not taken from the library's defaults, so that a change of the defaults does not move these cases."""
import functools

import numpy as np

import consist_cases as K
import repair_model as M

ROWMAJOR, COLMAJOR = 11, 12
OUT_SENTINEL = np.float32(-777.0)
CODE_SENTINEL, DISP_SENTINEL = np.uint8(99), np.int8(-99)
DRS = ((0, 0), (3, 3))
MIN_VALIDS = (1, 3)


def scatter(shape, seed, share=0.05, per_channel=False):
    """bool [A][C][H][W]: small blobs and single values flagged, about `share` of the positions; per_channel: every channel its own."""
    A, C, H, W = shape
    rng = np.random.default_rng(seed)
    fl = np.zeros(shape, bool)
    for st in range(A):
        for c in range(C if per_channel else 1):
            m = rng.random((H, W)) < share / 3
            for _ in range(max(1, H * W // 400)):
                y, x, h, w = rng.integers(0, H), rng.integers(0, W), rng.integers(1, 5), rng.integers(1, 5)
                m[y:y + h, x:x + w] = True
            if per_channel:
                fl[st, c] = m
            else:
                fl[st, :] = m
    return fl


def _case(lf, flags, ah, aw, ang_major=ROWMAJOR, empty=(), missing=(), ang_radius=1):
    A, C, H, W = lf.shape
    mask, miss = np.ones(A, np.uint32), np.zeros(A, np.uint32)
    mask[list(empty)] = 0
    miss[list(missing)] = 1
    return dict(lf=np.ascontiguousarray(lf.reshape(A, -1)), flags=None if flags is None else np.ascontiguousarray(flags.reshape(A, -1).astype(np.uint8)),
                mask=mask, missing=miss, ang_major=ang_major, aw=aw, ah=ah, W=W, H=H, C=C, ang_radius=ang_radius)


def build(name):
    """The case `name`: a dict of lf [A][C*H*W], flags (uint8 like lf, or None), mask, missing, ang_major, aw, ah, W, H, C, ang_radius."""
    if name == "textured":                                                          # per-channel flags that differ between channels
        lf = K.data("textured", 3, 3, 37, 70, 3, 0)
        return _case(lf, scatter(lf.shape, 1, per_channel=True), 3, 3)
    if name in ("5x5-R1", "5x5-R2"):                                                # an empty SAI, a missing SAI whose neighbours carry defects
        lf = K.data("textured", 5, 5, 33, 34, 1, 0)
        return _case(lf, scatter(lf.shape, 2), 5, 5, empty=[7], missing=[12], ang_radius=1 if name == "5x5-R1" else 2)
    if name == "1x3":
        lf = K.data("uniform", 1, 3, 5, 3, 1, 53)
        fl = np.zeros(lf.shape, bool)
        fl[0, 0, 1, 1] = fl[1, 0, 2:4, 0:2] = fl[2, 0, 4, 2] = True
        return _case(lf, fl, 1, 3)
    if name == "3x1":
        lf = K.data("uniform", 3, 1, 2, 2, 1, 22)
        fl = np.zeros(lf.shape, bool)
        fl[0, 0, 0, 0] = fl[1, 0, 1, 1] = True
        return _case(lf, fl, 3, 1, missing=[2])
    if name == "tiles-65x127":
        lf = K.data("textured", 3, 3, 65, 127, 3, 0)
        fl = scatter(lf.shape, 3, share=0.03)
        fl[:, :, 30:34, 62:66] = True                                               # across the corner of four tiles, in every SAI: code 2 inside
        fl[4, :, :, 126] = fl[4, :, 64, :] = True                                   # the last column and the last row
        return _case(lf, fl, 3, 3, missing=[0])
    if name == "tiles-31x65":
        lf = K.data("textured", 3, 3, 31, 65, 1, 0)
        fl = scatter(lf.shape, 4, share=0.03)
        fl[8, :, :, 64] = True
        return _case(lf, fl, 3, 3)
    if name == "nan":                                                               # not finite among flagged and unflagged values
        lf = K.data("textured", 3, 3, 37, 70, 3, 0)
        fl = scatter(lf.shape, 5, share=0.02)
        lf[4, 1, 5:8, 60:66] = np.nan
        fl[4, :, 6, 58:63] = True
        lf[8, :, 36, 69] = np.inf
        lf[0, 0, 0, 0] = -np.inf
        lf[3, 2, 20, 30] = np.nan
        fl[3, 2, 20, 30] = True
        return _case(lf, fl, 3, 3, missing=[1])
    if name == "no-source":                                                         # one position flagged in every SAI: every source invalid, code 2
        lf = K.data("textured", 3, 3, 37, 70, 3, 0)
        fl = np.zeros(lf.shape, bool)
        fl[:, :, 8:16, 18:26] = True                                                # no warp of up to 3 reaches a sound value from its middle
        fl[2, 0, 30, 5] = True
        return _case(lf, fl, 3, 3)
    if name == "lost-plane":                                                        # a plane without one sound value and no valid source: code 3
        lf = K.data("uniform", 1, 3, 6, 7, 1, 67)
        fl = np.zeros(lf.shape, bool)
        fl[1] = True
        fl[0, 0, 2, 3] = True
        return _case(lf, fl, 1, 3, missing=[0, 2])
    if name == "quiet-tile":                                                        # 2 x 2 tiles; only the first tile of SAI 4 has unsound positions
        lf = K.data("textured", 3, 3, 40, 100, 1, 0)
        fl = np.zeros(lf.shape, bool)
        fl[4, 0, 3:9, 10:20] = True
        return _case(lf, fl, 3, 3)
    if name in ("2x3-row", "2x3-col"):                                              # both angular orders on one scene
        lf = K.data("textured", 2, 3, 21, 40, 3, 0)
        fl = scatter(lf.shape, 6)
        if name == "2x3-row":
            return _case(lf, fl, 2, 3, missing=[4])
        perm = [(st % 2) * 3 + st // 2 for st in range(6)]                          # column-major index -> row-major index
        return _case(lf[perm], fl[perm], 2, 3, ang_major=COLMAJOR, missing=[perm.index(4)])
    if name in ("clean-3x3", "clean-5x5"):                                          # property 1: no flag, missing SAIs only
        if name == "clean-3x3":
            return _case(K.data("textured", 3, 3, 37, 70, 3, 0), None, 3, 3, missing=[4, 0])
        return _case(K.data("textured", 5, 5, 33, 34, 1, 0), None, 5, 5, empty=[7], missing=[12, 24], ang_radius=2)
    raise KeyError(name)


NAMES = ("textured", "5x5-R1", "5x5-R2", "1x3", "3x1", "tiles-65x127", "tiles-31x65", "nan", "no-source", "lost-plane", "quiet-tile",
         "2x3-row", "2x3-col")
CLEAN = ("clean-3x3", "clean-5x5")


@functools.lru_cache(maxsize=None)
def case(name):
    return build(name)


@functools.lru_cache(maxsize=None)
def model(name, D, r, min_valid):
    """The model's result on the case, with a sentinel in the outputs that must not be written.  Shared: do not change it."""
    c = case(name)
    A = c["aw"] * c["ah"]
    return M.fill(c["lf"], c["flags"], c["mask"], c["missing"], c["ang_major"], c["aw"], c["ah"], c["W"], c["H"], c["C"], D, r,
                  c["ang_radius"], min_valid, out=np.full(c["lf"].shape, OUT_SENTINEL, np.float32),
                  codes=np.full(c["lf"].shape, CODE_SENTINEL, np.uint8), disp=np.full((A, c["W"] * c["H"]), DISP_SENTINEL, np.int8))


# ---- the golden crops of the quality figures (profiles/repair_defaults.txt; tests/test_repair.py asserts against them) ----

import os

import inpaint_model as IM
import view_model as VM
from lfbm5d_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sourceLF_3x3_256_u8.npy")
CROPS = ((96, 160), (64, 160))                                                     # rows and columns 96..159 and 64..159


@functools.lru_cache(maxsize=None)
def golden(lo, hi, sigma=0.0):
    """(clean [9][C*n*n], flags bool like it from add_defects(seed=2), y = clean (plus noise of `sigma`, default_rng(1)) with the flagged
    values written as 0, n)"""
    n = hi - lo
    clean = np.load(GOLDEN)[:, :, lo:hi, lo:hi].astype(np.float32).reshape(9, -1)
    fl = synth.add_defects((9, 3, n, n), 2).reshape(9, -1)
    noisy = clean if sigma == 0.0 else (clean + np.random.default_rng(1).normal(0.0, sigma, clean.shape)).astype(np.float32)
    return clean, fl, np.where(fl, np.float32(0.0), noisy).astype(np.float32), n


def mask_gain(m, D=4, r=3, min_valid=1):
    """PSNR of the synthesised SAI m of crop 96..159 over all its positions: (mask-aware sweep on the defective light field, today's
    sweep on the same data, today's sweep on the clean light field)."""
    clean, fl, y, n = golden(96, 160)
    mask, miss = np.ones(9, np.uint32), np.zeros(9, np.uint32)
    miss[m] = 1
    aware = M.fill(y, fl, mask, miss, ROWMAJOR, 3, 3, n, n, 3, D, r, 1, min_valid)["out"][m]
    unaware = VM.fill(y, mask, miss, ROWMAJOR, 3, 3, n, n, 3, D, r)["out"][m]
    ideal = VM.fill(clean, mask, miss, ROWMAJOR, 3, 3, n, n, 3, D, r)["out"][m]
    return tuple(VM.psnr(v, clean[m]) for v in (aware, unaware, ideal))


def fill_gain(lo, hi, D=4, r=3, min_valid=3, sigma=0.0):
    """PSNR over the flagged values of a golden crop, all nine SAIs: (the joint fill, the rim-inwards fill)."""
    clean, fl, y, n = golden(lo, hi, sigma)
    mask = np.ones(9, np.uint32)
    joint = M.fill(y, fl, mask, None, ROWMAJOR, 3, 3, n, n, 3, D, r, 1, min_valid)["out"]
    rim = IM.fill(y, fl, mask, n, n, 3)["out"]
    return IM.psnr_on(joint, clean, fl), IM.psnr_on(rim, clean, fl)
