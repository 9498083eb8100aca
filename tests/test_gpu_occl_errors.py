"""What the occlusion-aware entry points refuse (lfbm5d_view_fill_occl_device, lfbm5d_view_occl_device, lfbm5d_view_occl_host_sai,
include/lfbm5d_occl.h), each returning 1 with its message and leaving the outputs untouched: a ratio between 0 and 1, negative, NaN or
infinite; d_set overlapping d_in or d_out; a context that is not a one-GPU context (the check every side stage shares refuses a
communicator and a shard alike; a shard is what one process can set up)."""
import ctypes as C

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core
import occl_cases as K
import subpel_model as S

HT = (8, 8, 3, 8, 3, "dct", "sadct", "haar")
INF, NAN = float("inf"), float("nan")
BAD_RATIOS = (0.5, 0.999, 1e-30, -1.0, -4.0, NAN, INF, -INF)
MSG = "occl_ratio must be 0 or a finite number of at least 1"
NAMES = ("lfbm5d_view_fill_occl_device", "lfbm5d_view_occl_device", "lfbm5d_view_occl_host_sai")


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


class _Case:
    """The `centre` shape on the device and on the host, outputs filled with sentinels, and the three calls on them."""

    def __init__(self):
        import torch
        self.ah, self.aw, self.H, self.W, self.C, miss, empty, self.R = K.SHAPES["centre"]
        self.lf, self.mask, self.missing = K.case("centre", "textured")
        A, HW = self.ah * self.aw, self.H * self.W
        self.d = torch.from_numpy(self.lf).cuda()
        self.out = torch.full_like(self.d, K.OUT_SENTINEL)
        self.disp = torch.full((A, HW), K.DISP_SENTINEL, dtype=torch.int8, device="cuda")
        self.sets = torch.full((A, HW), K.SET_SENTINEL, dtype=torch.uint8, device="cuda")
        self.h_in = [np.array(a) for a in self.lf]
        self.h_out = [np.full(self.lf.shape[1], K.OUT_SENTINEL, np.float32) for _ in range(A)]
        self.h_disp = [np.full(HW, K.DISP_SENTINEL, np.int8) for _ in range(A)]
        self.h_set = [np.full(HW, K.SET_SENTINEL, np.uint8) for _ in range(A)]
        self.P = core.make_params(0.0, 2.7, *HT)
        self.vp = L.view_params(3, 3, self.R, 0)
        self.res, self.occl, self.hist = core.ViewResultStruct(), core.ViewOcclResultStruct(), np.zeros(S.HIST, np.uint64)

    def call(self, h, name, ratio, d_in=None, d_out=None, d_set=None):
        lib, up = core.lib(), C.POINTER(C.c_uint)
        mp, sp = self.mask.ctypes.data_as(up), self.missing.ctypes.data_as(up)
        ptr = lambda t: C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else t)
        tail = (C.byref(self.res), self.hist.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(self.occl))
        dims = (self.W, self.H, self.C)
        d_in, d_out, d_set = (self.d if d_in is None else d_in, self.out if d_out is None else d_out, self.sets if d_set is None else d_set)
        if name == "lfbm5d_view_fill_occl_device":
            rc = lib.lfbm5d_view_fill_occl_device(h, C.byref(self.vp), 2, ratio, ptr(d_in), mp, sp, ptr(d_out), ptr(self.disp), ptr(d_set),
                                                  K.ROWMAJOR, self.aw, self.ah, *dims, *tail)
        elif name == "lfbm5d_view_occl_device":
            rc = lib.lfbm5d_view_occl_device(h, C.byref(self.vp), 2, ratio, C.byref(self.P), ptr(d_in), mp, sp, ptr(d_out), ptr(self.disp),
                                             ptr(d_set), K.ROWMAJOR, self.aw, self.ah, 1, *dims, *tail)
        else:
            rc = lib.lfbm5d_view_occl_host_sai(h, C.byref(self.vp), 2, ratio, C.byref(self.P), core._sai_ptrs(self.h_in, self.mask), mp, sp,
                                               core._sai_ptrs(self.h_out, self.mask), core._sai_ptrs(self.h_disp, self.mask, np.int8),
                                               core._sai_ptrs(self.h_set, self.mask, np.uint8), K.ROWMAJOR, self.aw, self.ah, 1, *dims, *tail)
        return rc, lib.lfbm5d_last_error(h).decode()

    def untouched(self):
        return ((self.out == K.OUT_SENTINEL).all().item() and (self.disp == K.DISP_SENTINEL).all().item()
                and (self.sets == K.SET_SENTINEL).all().item() and all((a == K.OUT_SENTINEL).all() for a in self.h_out)
                and all((a == K.DISP_SENTINEL).all() for a in self.h_disp) and all((a == K.SET_SENTINEL).all() for a in self.h_set)
                and np.array_equal(self.d.cpu().numpy().view(np.uint32), self.lf.view(np.uint32)))


@pytest.fixture(scope="module")
def case():
    return _Case()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_bad_ratios_are_refused(ctx, case, name):
    for ratio in BAD_RATIOS:
        rc, msg = case.call(ctx._h, name, ratio)
        assert rc == 1 and msg == f"{name}: {MSG}", (ratio, msg)
    assert case.untouched()
    # and through the Python layer
    with pytest.raises(L.LfBm5dError, match=MSG):
        ctx.view_fill(case.d, case.mask, case.missing, K.ROWMAJOR, case.aw, case.ah, case.W, case.H, case.C, out=case.out, occlusion=0.5)
    with pytest.raises(L.LfBm5dError, match=MSG):
        ctx.view_synth(case.lf, case.mask, case.missing, case.P, K.ROWMAJOR, case.aw, case.ah, 1, case.W, case.H, case.C, iterations=0,
                       occlusion=NAN)
    assert case.untouched()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES[:2])
def test_an_overlapping_set_plane_is_refused(ctx, case, name):
    A, HW = case.ah * case.aw, case.H * case.W
    inside_in = case.d.data_ptr() + 4 * HW                                      # a set buffer that begins inside d_in, inside d_out,
    inside_out = case.out.data_ptr() + 4 * (case.out.numel() - 1)               # on d_out's last value,
    before_in = case.d.data_ptr() - A * HW + 1                                  # and one that ends on d_in's first byte
    for d_set in (inside_in, inside_out, before_in, case.d.data_ptr(), case.out.data_ptr()):
        rc, msg = case.call(ctx._h, name, 4.0, d_set=d_set)
        assert rc == 1 and msg == f"{name}: d_set must not overlap d_in or d_out", msg
    assert case.untouched()
    rc, msg = case.call(ctx._h, name, 4.0, d_out=case.d)                        # the sibling's check stands
    assert rc == 1 and "d_out must not overlap d_in" in msg and case.untouched()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_a_context_that_is_not_one_gpu_is_refused(case, name):
    c = L.Context(0)
    try:
        c.set_shard(0, 2)
        rc, msg = case.call(c._h, name, 4.0)
        assert rc == 1 and msg == f"{name}: the view synthesis runs on one GPU (this context has a communicator or a shard)", msg
    finally:
        c.close()
    assert case.untouched()


@pytest.mark.gpu
def test_the_accepted_ratios_run(ctx):
    case = _Case()                                                              # its own outputs: this one writes them
    for ratio in (1.0, 1.0000001, 4.0, 1e30):
        rc, msg = case.call(ctx._h, "lfbm5d_view_fill_occl_device", ratio)
        assert rc == 0, msg
        assert sum(case.occl.set_hist) == case.H * case.W == case.res.pixels
    assert case.sets[4].max().item() <= 4 and (case.sets[:4] == K.SET_SENTINEL).all().item()
