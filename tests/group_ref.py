"""What the group kernels are held to, per case of tests/group_cases.py: the float64 model (tests/group_model.py), and the float32
round-off of the chain measured twice -- with the CPU oracle's process_group (orc_group) and with the model's own code in float32.

    E_filt = max |sample - model| / M over the filtered values (M: the largest |input| of the group and channel, pilot included)
    E_w    = max relative difference of the group weights

Both samples must agree with the model on nSx, the shape-adaptive flag and on every hard-threshold decision outside the gap
(group_model.compare); tests/test_group_model.py asserts that, tests/test_gpu_group.py bounds the kernels by 4 x the larger sample.
"""
import numpy as np

import group_cases as K
import group_model as M
from oracle import oracle as O

OPEN_CAP = 0.05      # at most this share of a case's (group, channel) pairs may have a coefficient inside the gap


def oracle_group(case):
    P = O.make_params(*K.params_tuple(case))
    if case.bm3d:      # the group loop of the oracle's bm3d_step; filt as [g][n][0][c][k2]
        pat, w, nSx = O.bm3d_group(case.step, P, case.Wb, case.Hb, case.C, case.noisy, case.basic, case.refs, case.self_idx, case.self_cnt)
        return np.ascontiguousarray(pat.transpose(0, 2, 1, 3)[:, :, None]), w, nSx, np.zeros_like(nSx)
    pat, w, nSx, sa = O.group(case.step, P, case.aw, case.aw, case.Wb, case.Hb, case.C, case.noisy, case.basic, case.mask, case.pst,
                              case.fill_quirk, case.refs, case.self_idx, case.self_cnt, case.best, case.shape)
    return np.ascontiguousarray(pat.transpose(0, 3, 1, 2, 4)), w, nSx, sa      # filt as [g][n][st][c][k2]


def reference(case):
    """model: run(case) in float64; oracle / second: group_model.compare of the two float32 samples; E_filt, E_w: the larger of each."""
    m = M.run(case)
    f, w, nSx, sa = oracle_group(case)
    ro = M.compare(case, m, f, w)
    ro["nSx"], ro["use_sadct"] = nSx, sa
    m32 = M.run(case, np.float32)
    with np.errstate(over="ignore"):
        w32 = m32["w"].astype(np.float32)
    rs = M.compare(case, m, m32["filt"], w32)
    return dict(model=m, oracle=ro, second=rs, E_filt=max(ro["E_filt"], rs["E_filt"]), E_w=max(ro["E_w"], rs["E_w"]))
