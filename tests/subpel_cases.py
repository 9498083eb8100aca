"""The light fields the sub-pixel plane sweep is compared on (tests/test_gpu_subpel.py against the GPU, tools/subpel_host_check.py against
the kernel's per-thread code compiled for the host), and the model's answer to each (tests/subpel_model.py), computed once per process.
The shapes are the smallest at which the kernel can go wrong: a tile is 64 x 32."""
import functools
import os

import numpy as np

import helpers
import subpel_model as S

ROWMAJOR = 11
OUT_SENTINEL, DISP_SENTINEL = -7.0, 99
TILE_W, TILE_H = 64, 32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sourceLF_3x3_256_u8.npy")
STEPS, DS, RS = (2, 4), (0, 3, 8), (0, 7)

ODD_5X5 = [s * 5 + t for s in range(5) for t in range(5) if s % 2 or t % 2]
# ah, aw, H, W, C, missing, empty, ang_radius
SHAPES = {
    "centre": (3, 3, 37, 70, 3, [4], [], 1),                                    # a tile edge in x
    "corners": (3, 3, 37, 70, 3, [0, 2, 6, 8], [], 1),                          # asymmetric sources
    "empty-source": (3, 3, 37, 70, 3, [4], [1], 1),                             # n = 7
    "upsample-R1": (5, 5, 33, 34, 1, ODD_5X5, [], 1),
    "upsample-R2": (5, 5, 33, 34, 1, ODD_5X5, [], 2),                           # n up to 6 (nine sound SAIs, at most six within two views)
    "centre-R2": (5, 5, 33, 34, 1, [12], [], 2),                                # n = 24: the instantiation that recomputes
    "narrow-1x3": (1, 3, 5, 3, 1, [1], [], 1),                                  # narrower than shift plus halo plus the +1 neighbour
    "narrow-3x1": (3, 1, 2, 2, 1, [0], [], 2),
    "single-63": (2, 1, 65, 63, 1, [1], [], 1),                                 # one source: E = 0, j* = 0, a copy
    "single-65": (2, 1, 65, 65, 1, [0], [], 1),
    "edges-65x127": (3, 3, 65, 127, 3, [4], [], 1),                             # the step-edge scene: a decision boundary across every
    "edges-31x65": (3, 3, 31, 65, 3, [0, 5], [], 1),                            # tile edge and corner
}
KINDS = ("uniform", "textured")


def step_edge_lf(H, W):
    """3 x 3 views of a scene with a background at disparity 0 and diagonal foreground stripes at disparity 2 (the scene of
    tests/test_gpu_view.py): the step edges cross every tile edge and corner of the plane."""
    src = np.load(GOLDEN)[4].astype(np.float32)                                 # [3][256][256]
    ys, xs = np.mgrid[0:H, 0:W]
    lf = np.zeros((9, 3, H, W), np.float32)
    for s in range(3):
        for t in range(3):
            Y, X = ys + 2 * s, xs + 2 * t                                       # scene coordinates of the foreground
            fg = ((X + Y) % 48) < 24
            lf[s * 3 + t] = np.where(fg[None], src[:, Y + 100, X + 20], src[:, ys, xs])
    return lf.reshape(9, -1)


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """(lf [A][C*H*W] float32 with NaN in what is never read, mask, missing) of a shape; the step-edge shapes have one kind."""
    ah, aw, H, W, C, miss, empty, R = SHAPES[shape]
    if shape.startswith("edges"):
        lf = step_edge_lf(H, W)
    elif kind == "uniform":
        lf = np.random.default_rng(H * 1000 + W).uniform(0.0, 255.0, (ah * aw, C * H * W)).astype(np.float32)
    else:
        lf = helpers.textured_lf(ah, aw, H, W, 2)[:, :C].astype(np.float32).reshape(ah * aw, -1)
    mask = np.ones(ah * aw, np.uint32)
    mask[empty] = 0
    missing = np.zeros(ah * aw, np.uint32)
    missing[miss] = 1
    lf = lf.copy()
    lf[(missing != 0) | (mask == 0)] = np.nan
    return lf, mask, missing


@functools.lru_cache(maxsize=None)
def model(shape, kind, steps, D, r):
    """The model's answer with sentinels in the outputs that must not be written.  Shared: do not change it."""
    ah, aw, H, W, C, miss, empty, R = SHAPES[shape]
    lf, mask, missing = case(shape, kind)
    out0 = np.full(lf.shape, OUT_SENTINEL, np.float32)
    disp0 = np.full((ah * aw, H * W), DISP_SENTINEL, np.int8)
    return S.fill(lf, mask, missing, ROWMAJOR, aw, ah, W, H, C, D, r, R, out=out0, disp=disp0, steps=steps)


def combos(shape):
    """(kind, steps, D, r) of a shape: every combination of the issue's grid; one kind for the step-edge scene."""
    kinds = ("scene",) if shape.startswith("edges") else KINDS
    return [(k, q, D, r) for k in kinds for q in STEPS for D in DS for r in RS]
