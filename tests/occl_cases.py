"""The light fields the occlusion-aware plane sweep is compared on (tests/test_gpu_occl.py against the GPU, tools/occl_host_check.py
against the kernel's per-thread code compiled for the host), and the model's answer to each (tests/occl_model.py), computed once per
process.  The shapes of tests/subpel_cases.py with their sentinels, and two occluder scenes cut from the golden centre SAI: a background
at disparity -1 under a rectangular occluder at disparity +3, and diagonal occluder stripes, at sizes where the occluders' edges cross
the edges and corners of the 64 x 32 tiles."""
import functools

import numpy as np

import occl_model as O
import subpel_cases as K
import subpel_model as S
import view_model as V

ROWMAJOR = K.ROWMAJOR
OUT_SENTINEL, DISP_SENTINEL, SET_SENTINEL = K.OUT_SENTINEL, K.DISP_SENTINEL, 77
STEPS, DRS = (1, 2, 4), ((0, 0), (3, 7), (8, 0), (8, 7))
D_BG, D_FG = -1, 3

# ah, aw, H, W, C, missing, empty, ang_radius
SCENES = {}
for _scene in ("rect", "stripes"):
    for _H, _W in ((65, 127), (31, 65)):
        SCENES[f"{_scene}-{_H}x{_W}-centre"] = (3, 3, _H, _W, 3, [4], [], 1)
        SCENES[f"{_scene}-{_H}x{_W}-edge"] = (3, 3, _H, _W, 3, [1], [], 1)
        SCENES[f"{_scene}-{_H}x{_W}-two"] = (3, 3, _H, _W, 3, [0, 5], [], 1)
    SCENES[f"{_scene}-5x5"] = (5, 5, 33, 34, 1, [12], [], 2)                    # n = 24, sets of 14: the instantiation that recomputes
SHAPES = dict(K.SHAPES, **SCENES)


def default_ratio():
    from lfbm5d_amd import core
    return float(core.lib().lfbm5d_view_occl_default())


def occluder_lf(scene, ah, aw, H, W, C):
    """ah x aw views [A][C*H*W] of a background at disparity -1 (view (s, t) sees the scene at (y - s, x - t)) under an occluder at
    disparity +3 (seen at (y + 3 s, x + 3 t)): a centred rectangle of 3/8 of the plane, or diagonal stripes 24 of 48 wide.  The centre
    view is the scene's frame; both textures are the golden centre SAI."""
    src = np.load(K.GOLDEN)[4].astype(np.float32)                               # [3][256][256]
    ys, xs = np.mgrid[0:H, 0:W]
    sc, tc = ah // 2, aw // 2
    lf = np.zeros((ah * aw, C, H, W), np.float32)
    for s in range(ah):
        for t in range(aw):
            Y, X = ys + D_FG * (s - sc), xs + D_FG * (t - tc)                   # the occluder's frame
            if scene == "rect":
                h, w = 3 * H // 8, 3 * W // 8
                fg = (Y >= (H - h) // 2) & (Y < (H - h) // 2 + h) & (X >= (W - w) // 2) & (X < (W - w) // 2 + w)
            else:
                fg = ((X + Y + 480) % 48) < 24
            bg = src[:C, ys + D_BG * (s - sc) + 8, xs + D_BG * (t - tc) + 8]
            lf[s * aw + t] = np.where(fg[None], src[:C, Y + 120, X + 100], bg)
    return lf.reshape(ah * aw, -1)


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """(lf [A][C*H*W] float32 with NaN in what is never read, mask, missing) of a shape; the scenes have one kind."""
    if shape in K.SHAPES:
        return K.case(shape, kind)
    ah, aw, H, W, C, miss, empty, R = SHAPES[shape]
    lf = occluder_lf(shape.split("-")[0], ah, aw, H, W, C)
    mask, missing = np.ones(ah * aw, np.uint32), np.zeros(ah * aw, np.uint32)
    missing[miss] = 1
    lf[missing != 0] = np.nan
    return lf, mask, missing


def kinds(shape):
    return ("scene",) if shape in SCENES or shape.startswith("edges") else K.KINDS


@functools.lru_cache(maxsize=4)
def _swept(shape, kind, steps):
    """{m: the set errors of every hypothesis up to D = 8}: a sweep with a smaller D uses the first 2 D steps + 1 of them."""
    ah, aw, H, W, C, miss, empty, R = SHAPES[shape]
    lf, mask, missing = case(shape, kind)
    x = lf.reshape(ah * aw, C, H, W)
    return {m: O.sweep_errors(x, V.sources(m, mask, missing, ROWMAJOR, aw, ah, R), V.D_MAX, steps) for m in miss}


@functools.lru_cache(maxsize=None)
def model(shape, kind, steps, D, r, ratio):
    """The model's answer with sentinels in the outputs that must not be written.  Shared: do not change it."""
    ah, aw, H, W, C, miss, empty, R = SHAPES[shape]
    lf, mask, missing = case(shape, kind)
    out0 = np.full(lf.shape, OUT_SENTINEL, np.float32)
    disp0 = np.full((ah * aw, H * W), DISP_SENTINEL, np.int8)
    set0 = np.full((ah * aw, H * W), SET_SENTINEL, np.uint8)
    swept = {m: s[:2 * D * steps + 1] for m, s in _swept(shape, kind, steps).items()}
    return O.fill(lf, mask, missing, ROWMAJOR, aw, ah, W, H, C, D, r, R, out=out0, disp=disp0, steps=steps, ratio=ratio, sets_out=set0,
                  swept=swept)


def combos(shape, ratios):
    """(kind, steps, D, r, ratio) of a shape: every combination of steps, (D, r) and ratio."""
    return [(k, q, D, r, rho) for k in kinds(shape) for q in STEPS for D, r in DRS for rho in ratios]
