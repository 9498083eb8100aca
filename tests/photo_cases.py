"""The light fields the photometric equalisation is compared on (tests/test_gpu_photo.py against the GPU, tools/photo_host_check.py
against the kernels' per-thread code compiled for the host), and the model's answer to each, computed once per process.  Parameters are
spelled out here, not taken from the library's defaults, so that a change of the defaults does not move these cases."""
import functools

import numpy as np

from lfbm5d_amd import synth
import consist_cases as K
import photo_model as M

ROWMAJOR, COLMAJOR = 11, 12
OUT_SENTINEL = np.float32(-777.0)
PARAMS = dict(ang_radius=1, steps=1, min_sources=3, max_rounds=3, tol=1.0 / 256, min_count=256, per_channel=1, anchor=None, lo=16.0, hi=200.0)
DRS = ((0, 0), (3, 3))


def planted(lf, ah, aw, edge, cast=None):
    """The light field [A][C][H][W] under vignette_gains(edge) and, with cast = (SAI, channel, factor), one channel of one view more."""
    g = np.repeat(synth.vignette_gains(aw, ah, edge)[:, None], lf.shape[1], axis=1)
    if cast:
        g[cast[0], cast[1]] *= cast[2]
    return synth.apply_gains(lf, g)


def _case(lf, ah, aw, ang_major=ROWMAJOR, empty=(), **params):
    A, C, H, W = lf.shape
    mask = np.ones(A, np.uint32)
    mask[list(empty)] = 0
    return dict(lf=np.ascontiguousarray(lf.reshape(A, -1)), mask=mask, ang_major=ang_major, aw=aw, ah=ah, W=W, H=H, C=C,
                params=dict(PARAMS, **params))


def build(name):
    """The case `name`: a dict of lf [A][C*H*W], mask, ang_major, aw, ah, W, H, C, params."""
    if name in ("textured", "uniform"):                                             # a vignette and a cast on one channel of one view
        return _case(planted(K.data(name, 3, 3, 37, 70, 3, 37070), 3, 3, 0.6, (2, 1, 1.1)), 3, 3)
    if name == "5x5-R1":                                                            # one empty SAI; the corners have 3 sources: untested
        return _case(planted(K.data("textured", 5, 5, 33, 34, 1, 0), 5, 5, 0.7), 5, 5, empty=[7], ang_radius=1, min_sources=4)
    if name == "5x5-R2":                                                            # the corners have 8
        return _case(planted(K.data("textured", 5, 5, 33, 34, 1, 0), 5, 5, 0.7), 5, 5, empty=[7], ang_radius=2, min_sources=9)
    if name == "1x3":                                                               # the ends have one source: untested
        lf = synth.apply_gains(K.data("uniform", 1, 3, 5, 3, 1, 53), [0.8, 1.3, 1.0])
        return _case(lf, 1, 3, min_sources=2, min_count=1, lo=0.0, hi=1000.0)
    if name == "3x1":
        lf = synth.apply_gains(K.data("uniform", 3, 1, 2, 2, 1, 22), [1.0, 0.7, 1.2])
        return _case(lf, 3, 1, min_sources=2, min_count=1, lo=0.0, hi=1000.0)
    if name == "tiles-65x127":
        return _case(planted(K.data("textured", 3, 3, 65, 127, 3, 0), 3, 3, 0.8, (6, 2, 0.9)), 3, 3)
    if name == "tiles-31x65":
        return _case(planted(K.data("textured", 3, 3, 31, 65, 1, 0), 3, 3, 0.8), 3, 3)
    if name == "nan":                                                               # non-finite values in tested SAIs, which are sources too
        lf = planted(K.data("textured", 3, 3, 37, 70, 3, 0), 3, 3, 0.6)
        lf[4, 1, 5:8, 60:66] = np.nan
        lf[8, :, 36, 69] = np.inf
        lf[0, 0, 0, 0] = -np.inf
        return _case(lf, 3, 3)
    if name in ("2x3-row", "2x3-col"):                                              # both angular orders on one scene
        lf = planted(K.data("textured", 2, 3, 21, 40, 3, 0), 2, 3, 0.7, (5, 0, 1.1))
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
def model(name, D, r, more=()):
    """The model's result on the case (more: a tuple of (parameter, value) pairs that replace the case's), with a sentinel in the output
    planes that must not be written.  Shared: do not change it."""
    c = case(name)
    A = c["aw"] * c["ah"]
    out = np.full((A, c["C"] * c["H"] * c["W"]), OUT_SENTINEL, np.float32)
    return M.equalise(c["lf"], c["mask"], c["ang_major"], c["aw"], c["ah"], c["W"], c["H"], c["C"], D=D, r=r, out=out,
                      **dict(c["params"], **dict(more)))
