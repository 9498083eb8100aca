"""The light fields the consistency check is compared on (tests/test_gpu_consist.py against the GPU, tools/consist_host_check.py against
the kernels' per-thread code compiled for the host), and the model's answer to each, computed once per process.  Parameters are spelled
out here, not taken from the library's defaults, so that a change of the defaults does not move these cases."""
import functools

import numpy as np

import helpers
import consist_model as M

ROWMAJOR, COLMAJOR = 11, 12
FLAG_SENTINEL, DISP_SENTINEL = 77, 99
TILE_W, TILE_H = 64, 32                       # the sweep's tile and the new kernels'
PARAMS = dict(ang_radius=1, k=8.0, min_threshold=0.0, spread=3.0, min_sources=2, sai_factor=2.0, min_scale=0.5, max_rounds=3)
DRS = ((0, 0), (3, 3), (8, 7))


def data(kind, ah, aw, H, W, C, seed):
    """[ah*aw][C][H][W] float32: uniform random values, or the photograph moving 2 pixels per view."""
    if kind == "uniform":
        return np.random.default_rng(seed).uniform(0.0, 255.0, (ah * aw, C, H, W)).astype(np.float32)
    return helpers.textured_lf(ah, aw, H, W, 2)[:, :C].astype(np.float32)


def plant(lf, spots):
    """Blocks written as 0 or 255 (whichever is farther from the block's mean): spots = (SAI, y, x, h, w), clipped to the plane."""
    for st, y, x, h, w in spots:
        blk = lf[st, :, max(y, 0):y + h, max(x, 0):x + w]
        if blk.size:
            blk[...] = 0.0 if blk.mean() > 127.0 else 255.0
    return lf


def tile_spots(A, H, W):
    """3 x 3 blocks across every tile edge and corner of the plane, in rotating SAIs, and one in the plane's last corner."""
    spots, i = [], 0
    ys = list(range(TILE_H, H, TILE_H)) or [H // 2]
    xs = list(range(TILE_W, W, TILE_W)) or [W // 2]
    for y in ys:
        for x in xs:
            spots.append((i % A, y - 1, x - 1, 3, 3)); i += 1                    # a corner
        spots.append((i % A, y - 1, max(xs[0] // 2 - 1, 0), 3, 3)); i += 1       # a horizontal edge
    for x in xs:
        spots.append((i % A, max(ys[0] // 2 - 1, 0), x - 1, 3, 3)); i += 1       # a vertical edge
    spots.append((i % A, H - 2, W - 2, 2, 2))
    return spots


def _case(lf, ah, aw, ang_major=ROWMAJOR, empty=(), exclude=(), **params):
    A, C, H, W = lf.shape
    mask = np.ones(A, np.uint32)
    mask[list(empty)] = 0
    ex = np.zeros(A, np.uint32)
    ex[list(exclude)] = 1
    return dict(lf=np.ascontiguousarray(lf.reshape(A, -1)), mask=mask, exclude=ex if len(exclude) else None, ang_major=ang_major, aw=aw, ah=ah,
                W=W, H=H, C=C, params=dict(PARAMS, **params))


def _noise_sai(lf, st, seed):
    lf[st] = (np.random.default_rng(seed).random(lf[st].shape) * 255.0).astype(np.float32)
    return lf


def build(name):
    """The case `name`: a dict of lf [A][C*H*W], mask, exclude (or None), ang_major, aw, ah, W, H, C, params."""
    if name in ("textured", "uniform"):                                             # planted defects and one noise SAI: two rounds
        lf = plant(data(name, 3, 3, 37, 70, 3, 37070), [(4, 10, 20, 5, 5), (0, 30, 62, 3, 4), (7, 0, 0, 2, 2), (2, 15, 40, 1, 1)])
        return _case(_noise_sai(lf, 5, 1), 3, 3)
    if name in ("5x5-R1", "5x5-R2"):                                                # one empty and one excluded SAI
        lf = plant(data("textured", 5, 5, 33, 34, 1, 0), [(12, 8, 8, 5, 5), (0, 20, 3, 3, 3), (24, 30, 30, 3, 4)])
        return _case(lf, 5, 5, empty=[7], exclude=[18], ang_radius=int(name[-1]))
    if name == "1x3":                                                               # the ends have one source: untested
        return _case(plant(data("uniform", 1, 3, 5, 3, 1, 53), [(1, 2, 1, 1, 1)]), 1, 3)
    if name == "3x1":
        return _case(plant(data("uniform", 3, 1, 2, 2, 1, 22), [(1, 0, 1, 1, 1)]), 3, 1)
    if name == "tiles-65x127":
        lf = data("textured", 3, 3, 65, 127, 3, 0)
        return _case(plant(lf, tile_spots(9, 65, 127)), 3, 3)
    if name == "tiles-31x65":
        lf = data("textured", 3, 3, 31, 65, 1, 0)
        return _case(plant(lf, tile_spots(9, 31, 65)), 3, 3)
    if name == "nan":                                                               # non-finite values in tested SAIs
        lf = plant(data("textured", 3, 3, 37, 70, 3, 0), [(4, 10, 20, 5, 5)])
        lf[4, 1, 5:8, 60:66] = np.nan
        lf[8, :, 36, 69] = np.inf
        lf[0, 0, 0, 0] = -np.inf
        return _case(lf, 3, 3)
    if name in ("2x3-row", "2x3-col"):                                              # both angular orders on one scene
        lf = plant(data("textured", 2, 3, 21, 40, 3, 0), [(1, 5, 5, 4, 4), (5, 12, 30, 3, 3)])
        if name == "2x3-row":
            return _case(lf, 2, 3)
        perm = [(st % 2) * 3 + st // 2 for st in range(6)]                          # column-major index -> row-major index
        return _case(lf[perm], 2, 3, ang_major=COLMAJOR)
    raise KeyError(name)


NAMES = ("textured", "uniform", "5x5-R1", "5x5-R2", "1x3", "3x1", "tiles-65x127", "tiles-31x65", "nan", "2x3-row", "2x3-col")


@functools.lru_cache(maxsize=None)
def case(name):
    return build(name)


@functools.lru_cache(maxsize=None)
def model(name, D, r):
    """The model's result on the case, with sentinels in the outputs that must not be written.  Shared: do not change it."""
    c = case(name)
    A = c["aw"] * c["ah"]
    flags = np.full((A, c["C"] * c["H"] * c["W"]), FLAG_SENTINEL, np.uint8)
    disp = np.full((A, c["H"] * c["W"]), DISP_SENTINEL, np.int8)
    return M.consist(c["lf"], c["mask"], c["ang_major"], c["aw"], c["ah"], c["W"], c["H"], c["C"], D=D, r=r, exclude=c["exclude"], flags=flags,
                     disp=disp, **c["params"])
