"""Every message of the argument checks the side stages share (noise level, quality, super-resolution, Poisson-Gaussian, impulse repair,
inpainting, view synthesis, consistency check): each C entry is called through core.lib() with one bad argument at a time -- a NULL
required pointer, chnls 2, a width or height below the stage's minimum, a bad ang_major, awidth / aheight 0, an all-empty mask, a NULL
plane of a non-empty SAI (host forms), overlapping input and output, a context with set_shard(0, 2), the loop checks -- and the full
lfbm5d_last_error string is compared with tests/golden/side_stage_errors.json, which was recorded from the library as it stood BEFORE the
stages' host frames were merged (record(): `PYTHONPATH=. python tests/test_gpu_side_stage_errors.py` rewrites the file).  The light
field is 2 x 2 SAIs of 16 x 16 in valid, zeroed buffers: most calls return before a kernel launches, but not all.  A case its stage has
no check for is recorded as it ends: pg_forward / pg_inverse accept a width or height of 1 and run ("" in the file); a bad ang_major or
1001 iterations in superres, inpaint and denoise_pg pass the stage, whose first kernels (upsampling, fill, transform) run, and end in
the hard-thresholding step's own argument check."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from lfbm5d_amd import core

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "side_stage_errors.json")
AW, AH, W, H, CH = 2, 2, 16, 16, 3
A = AW * AH
REGION = 1 << 16          # bytes of one device region: the largest plane set of a call (super-resolution's output at scale 2) fits
HT = (8, 8, 3, 8, 3, "dct", "sadct", "haar")


class _Mem:
    """Zeroed device regions that do not overlap, and host planes that stay alive."""

    def __init__(self, L, n=12):
        self.L, self.base, self.keep = L, C.c_void_p(), []
        assert L.lfbm5d_malloc(C.byref(self.base), n * REGION) == 0
        z = np.zeros(n * REGION, np.uint8)
        assert L.lfbm5d_memcpy_h2d(self.base, z.ctypes.data, z.size) == 0
        self.n, self.used = n, 0

    def dev(self):
        assert self.used < self.n
        self.used += 1
        return self.base.value + (self.used - 1) * REGION

    def planes(self, null_at=None):
        """void*[A] over zeroed host planes; entry null_at is NULL."""
        arr = (C.c_void_p * A)()
        for i in range(A):
            if i == null_at:
                continue
            p = np.zeros(REGION // 4, np.uint8)
            self.keep.append(p)
            arr[i] = p.ctypes.data
        self.keep.append(arr)
        return arr

    def close(self):
        self.L.lfbm5d_free(self.base)


def _u(v):
    return C.c_uint(v)


def _entries(mem):
    """name -> (list of [slot, role, value], loop struct or None).  Roles: req (required pointer), opt (optional pointer or output),
    mask, hsai (required host planes), ohsai (optional host planes, given here; value: (planes, index of the SAI whose NULL plane is tried)),
    C, W, H, ang, aw, ah, in / out / fin / fout (device planes that must not overlap: also required),
    val (anything else)."""
    P, P2 = core.make_params(20.0, 2.7, *HT), core.make_params(20.0, 2.7, *HT)
    mask = np.ones(A, np.uint32)
    missing = np.array([0, 1, 0, 0], np.uint32)
    mem.keep += [P, P2, mask, missing]
    mp, up = mask.ctypes.data_as(C.POINTER(C.c_uint)), missing.ctypes.data_as(C.POINTER(C.c_uint))
    d, hp = mem.dev, mem.planes
    out = lambda T: (lambda o: (mem.keep.append(o), C.byref(o))[1])(T())
    buf = lambda n, t, ct: (lambda a: (mem.keep.append(a), a.ctypes.data_as(C.POINTER(ct)))[1])(np.zeros(n, t))
    geo4 = lambda w=W, h=H: [["asize", "val", _u(A)], ["W", "W", _u(w)], ["H", "H", _u(h)], ["C", "C", _u(CH)]]
    geo7 = lambda w=W, h=H: [["ang", "ang", _u(core.ROWMAJOR)], ["aw", "aw", _u(AW)], ["ah", "ah", _u(AH)], ["an", "val", _u(1)],
                             ["W", "W", _u(w)], ["H", "H", _u(h)], ["C", "C", _u(CH)]]
    geo6 = lambda: [s for s in geo7() if s[0] != "an"]
    geo8 = lambda: [["ang", "ang", _u(core.ROWMAJOR)], ["aw", "aw", _u(AW)], ["ah", "ah", _u(AH)], ["an1", "val", _u(1)], ["an2", "val", _u(1)],
                    ["W", "W", _u(W)], ["H", "H", _u(H)], ["C", "C", _u(CH)]]
    m = lambda: ["mask", "mask", mp]
    sr = core.sr_defaults(2, iterations=1)
    pg = core.pg_model(0.5, 4.0, CH)
    ip, inp, vw, cs = core.impulse_params(), core.inpaint_params(iterations=1), core.view_params(iterations=1), core.consist_params()
    mem.keep += [sr, pg, ip, inp, vw, cs]
    r, Pr = C.byref, lambda: ["P", "req", C.byref(P)]
    E = {}
    E["noise_level_device"] = ([["d_lf", "req", d()], m()] + geo4() + [["patch", "val", _u(8)], ["out", "req", out(core.NoiseLevelStruct)],
                               ["sig", "opt", None], ["eig", "opt", None]], None)
    E["noise_level_host_sai"] = ([["h_lf", "hsai", hp()], m()] + geo4() + [["patch", "val", _u(8)], ["out", "req", out(core.NoiseLevelStruct)],
                                 ["sig", "opt", None], ["eig", "opt", None]], None)
    qtail = lambda: [["peak", "val", C.c_double(255.0)], ["ssim", "val", C.c_int(1)], ["out", "req", out(core.QualityStruct)],
                     ["mse", "opt", None], ["ss", "opt", None]]
    E["quality_device"] = ([["d_ref", "req", d()], ["d_test", "req", d()], m()] + geo4() + qtail(), None)
    E["quality_host_sai"] = ([["h_ref", "hsai", hp()], ["h_test", "hsai", hp()], m()] + geo4() + qtail(), None)
    srp = lambda: ["sr", "req", r(sr)]
    E["sr_up_device"] = ([srp(), ["d_low", "req", d()], m(), ["d_high", "req", d()]] + geo4(), None)
    E["sr_down_device"] = ([srp(), ["d_high", "req", d()], m(), ["d_low", "req", d()]] + geo4(), None)
    E["sr_backproject_device"] = ([srp(), ["d_y", "req", d()], ["d_x", "req", d()], m(), ["d_z", "req", d()]] + geo4(), None)
    E["superres_device"] = ([srp(), Pr(), ["d_low", "req", d()], m(), ["d_high", "req", d()]] + geo7(), sr)
    E["superres_host_sai"] = ([srp(), Pr(), ["h_low", "hsai", hp()], m(), ["h_high", "hsai", hp()]] + geo7(), sr)
    ull = lambda n: buf(n, np.uint64, C.c_ulonglong)
    E["pg_histogram_device"] = ([["d_lf", "req", d()], m()] + geo4() + [["hist", "req", ull(CH * 64 * 322)], ["sum", "req", ull(CH * 64)],
                                ["blocks", "opt", None], ["skipped", "opt", None]], None)
    E["pg_estimate_device"] = ([["d_lf", "req", d()], m()] + geo4() + [["out", "req", out(core.PgEstimateStruct)], ["hist", "opt", None],
                               ["sum", "opt", None]], None)
    E["pg_estimate_host_sai"] = ([["h_lf", "hsai", hp()], m()] + geo4() + [["out", "req", out(core.PgEstimateStruct)], ["hist", "opt", None],
                                 ["sum", "opt", None]], None)
    E["pg_forward_device"] = ([["model", "req", r(pg)], ["d_in", "req", d()], m(), ["d_out", "req", d()]] + geo4(), None)
    E["pg_inverse_device"] = ([["model", "req", r(pg)], ["d_in", "req", d()], m(), ["d_out", "req", d()]] + geo4(), None)
    E["denoise_pg_device"] = ([["model", "val", r(pg)], ["used", "opt", None], ["P1", "req", r(P)], ["P2", "req", r(P2)], ["d_noisy", "req", d()],
                               m(), ["d_basic", "req", d()], ["d_den", "req", d()]] + geo8(), None)
    E["denoise_pg_host_sai"] = ([["model", "val", r(pg)], ["used", "opt", None], ["P1", "req", r(P)], ["P2", "req", r(P2)],
                                 ["h_noisy", "hsai", hp()], m(), ["h_basic", "hsai", hp()], ["h_den", "hsai", hp()]] + geo8(), None)
    E["impulse_histogram_device"] = ([["d_lf", "req", d()], m()] + geo4() + [["hist", "req", ull(CH * 386)], ["pixels", "opt", None],
                                     ["skipped", "opt", None]], None)
    itail = lambda: [["out", "opt", out(core.ImpulseResultStruct)], ["cnt", "opt", None]]
    E["impulse_repair_device"] = ([["P", "req", r(ip)], ["d_in", "in", d()], m(), ["d_out", "out", d()], ["d_flags", "opt", d()]] + geo4() + itail(),
                                  None)
    E["impulse_repair_flags_device"] = ([["d_in", "in", d()], ["d_fin", "fin", d()], m(), ["d_out", "out", d()], ["d_flags", "fout", d()]]
                                        + geo4() + itail(), None)
    E["impulse_repair_host_sai"] = ([["P", "val", r(ip)], ["h_in", "hsai", hp()], ["h_fin", "opt", None], m(), ["h_out", "hsai", hp()],
                                     ["h_flags", "ohsai", (hp(), 0)]] + geo4() + itail(), None)
    nres = lambda: ["out", "opt", out(core.InpaintResultStruct)]
    E["inpaint_fill_device"] = ([["d_in", "in", d()], ["d_fin", "fin", d()], m(), ["d_out", "out", d()], ["d_flags", "fout", d()]] + geo4()
                                + [nres()], None)
    E["inpaint_project_device"] = ([["d_flags", "req", d()], ["d_x", "req", d()], ["d_y", "req", d()], m(), ["d_out", "req", d()]] + geo4(), None)
    E["inpaint_device"] = ([["ip", "req", r(inp)], Pr(), ["d_in", "in", d()], ["d_fin", "fin", d()], m(), ["d_out", "out", d()],
                            ["d_flags", "fout", d()]] + geo7() + [nres()], inp)
    E["inpaint_host_sai"] = ([["ip", "req", r(inp)], Pr(), ["h_in", "hsai", hp()], ["h_fin", "hsai", hp()], m(), ["h_out", "hsai", hp()],
                              ["h_flags", "ohsai", (hp(), 0)]] + geo7() + [nres()], inp)
    vres = lambda: ["out", "opt", out(core.ViewResultStruct)]
    miss = lambda: ["missing", "req", up]
    E["view_fill_device"] = ([["vp", "req", r(vw)], ["d_in", "in", d()], m(), miss(), ["d_out", "out", d()], ["d_disp", "opt", d()]] + geo6()
                             + [vres()], None)
    E["view_device"] = ([["vp", "req", r(vw)], Pr(), ["d_in", "in", d()], m(), miss(), ["d_out", "out", d()], ["d_disp", "opt", d()]] + geo7()
                        + [vres()], vw)
    # SAI 0 is sound: its input plane is the one the NULL case takes away
    E["view_host_sai"] = ([["vp", "req", r(vw)], Pr(), ["h_in", "hsai", hp()], m(), miss(), ["h_out", "hsai", hp()], ["h_disp", "ohsai", (hp(), 1)]]
                          + geo7() + [vres()], vw)
    ctail = lambda: [["state", "req", buf(A, np.uint32, C.c_uint)], ["d_disp", "opt", None], ["scale", "opt", None], ["hist", "opt", None]]
    cres = lambda: ["out", "opt", out(core.ConsistResultStruct)]
    E["consist_device"] = ([["P", "req", r(cs)], ["d_in", "req", d()], m(), ["excl", "opt", None], ["d_flags", "req", d()]] + ctail() + geo6()
                           + [cres()], None)
    E["consist_host_sai"] = ([["P", "req", r(cs)], ["h_in", "hsai", hp()], m(), ["excl", "opt", None], ["h_flags", "hsai", hp()],
                              ["state", "req", buf(A, np.uint32, C.c_uint)], ["h_disp", "ohsai", (hp(), 0)], ["scale", "opt", None],
                              ["hist", "opt", None]] + geo6() + [cres()], None)
    return E


# a width or height below the stage's minimum (default: 1, below "at least 2"); quality also has 10 with SSIM on
SMALL = {"noise_level": (15,), "quality": (0, 10), "sr": (0,), "superres": (0,)}
# entries whose checks do not include "runs on one GPU": a sharded context would run their kernels
NO_ONE_GPU = ("noise_level", "quality", "sr_up", "sr_down", "sr_backproject")
LOOP = {"iterations_1001": ("iterations", 1001), "sigma_end_above_start": ("sigma_end", 1000.0), "sigma_noise_negative": ("sigma_noise", -1.0),
        "iterations_0": ("iterations", 0)}


def collect():
    """{case id: message} of every case, in a fixed order ("" where the library accepted the call)."""
    L = core.lib()
    h, hs = C.c_void_p(), C.c_void_p()
    assert L.lfbm5d_create(C.byref(h), 0) == 0 and L.lfbm5d_create(C.byref(hs), 0) == 0
    assert L.lfbm5d_set_shard(hs, 0, 2) == 0
    mem = _Mem(L, 96)
    res = {}
    try:
        E = _entries(mem)
        for name, (slots, loop) in E.items():
            fn = getattr(L, "lfbm5d_" + name)
            fn.restype = C.c_int

            def call(case, ctx=h, **repl):
                args = [repl.get(s[0], s[2][0] if s[1] == "ohsai" else s[2]) for s in slots]
                rc = fn(ctx, *args)
                res[f"{name}:{case}"] = L.lfbm5d_last_error(ctx).decode() if rc else ""

            for slot, role, val in slots:
                if role in ("req", "mask", "hsai", "in", "out", "fin"):
                    call(f"null_{slot}", **{slot: None})
                if role == "C":
                    call("chnls_2", C=_u(2))
                if role in ("W", "H"):
                    stage = next((k for k in SMALL if name.startswith(k)), None)
                    for v in SMALL.get(stage, (1,)):
                        call(f"{slot}_{v}", **{slot: _u(v)})
                if role == "ang":
                    call("ang_major_7", ang=_u(7))
                if role in ("aw", "ah"):
                    call(f"{slot}_0", **{slot: _u(0)})
                if role == "hsai":
                    call(f"null_plane_{slot}", **{slot: mem.planes(null_at=0)})
                if role == "ohsai":
                    call(f"null_plane_{slot}", **{slot: mem.planes(null_at=val[1])})
            empty = np.zeros(A, np.uint32)
            call("empty_mask", mask=empty.ctypes.data_as(C.POINTER(C.c_uint)))
            by_role = {s[1]: s for s in slots}
            if "in" in by_role and "out" in by_role:
                call("overlap_out_in", **{by_role["out"][0]: by_role["in"][2] + 4})
            if "fin" in by_role and "fout" in by_role:
                call("overlap_flags", **{by_role["fout"][0]: by_role["fin"][2] + 1})
            if not name.startswith(NO_ONE_GPU):
                call("sharded_context", ctx=hs)
            if loop is not None:
                fields = dict(type(loop)._fields_)
                for case, (field, bad) in LOOP.items():
                    if field not in fields or (case == "iterations_0" and not name.startswith("superres")):
                        continue
                    good = getattr(loop, field)
                    setattr(loop, field, bad)
                    call(case)
                    setattr(loop, field, good)
    finally:
        mem.close()
        L.lfbm5d_destroy(h)
        L.lfbm5d_destroy(hs)
    return res


def record():
    doc = {"_note": "Recorded from the library at the commit before the side stages' shared host frame (one SAI list, one set of checks, one "
                    "staging pair, one refinement loop) was introduced; the test holds the new code to these strings byte for byte.",
           "messages": collect()}
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.mark.gpu
def test_side_stage_messages_equal_the_recorded_ones():
    with open(GOLDEN) as f:
        want = json.load(f)["messages"]
    got = collect()
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


if __name__ == "__main__":
    record()
    print(GOLDEN)
