"""GPU tests of the joint repair (lfbm5d_repair_*, include/lfbm5d_repair.h): the fill equals the numpy model (tests/repair_model.py) bit for
bit -- values, codes, disparities, counts, histogram -- on the cases of tests/repair_cases.py, with sentinels in what must not be
written, and a second call returns the same bits; without defects it equals lfbm5d_view_fill_device bit for bit; the host forms return
the device form's bits; the loop equals the model's loop with the GPU's own first step as the step function."""
import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core
import repair_cases as K
import repair_model as M

HT = (8, 8, 3, 8, 3, "dct", "sadct", "haar")       # N, nSim, nDisp, k, p, tau_2D, tau_4D, tau_5D: the other loop tests' parameters


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _geo(c):
    return (c["ang_major"], c["aw"], c["ah"], c["W"], c["H"], c["C"])


def _counts(got):
    return (got.missing, got.targets, got.swept, got.passes, got.values, got.flagged, list(got.unsound), list(got.views), list(got.rim),
            list(got.left), got.positions, list(got.disparity_hist))


def _want_counts(want, C_):
    return (want["missing"], want["targets"], want["swept"], want["passes"], want["values"], want["flagged"], list(want["unsound"][:C_]),
            list(want["views"][:C_]), list(want["rim"][:C_]), list(want["left"][:C_]), want["positions"], list(want["hist"]))


def _assert_equals_model(ctx, name, D, r, mv):
    """One fill against the model with sentinels in the outputs; a second call into fresh outputs returns the same bits."""
    c, want = K.case(name), K.model(name, D, r, mv)
    A = c["aw"] * c["ah"]
    d, fl = _dev(c["lf"]), None if c["flags"] is None else _dev(c["flags"])
    out = _dev(np.full(c["lf"].shape, K.OUT_SENTINEL, np.float32))
    codes = _dev(np.full(c["lf"].shape, K.CODE_SENTINEL, np.uint8))
    disp = _dev(np.full((A, c["W"] * c["H"]), K.DISP_SENTINEL, np.int8))
    kw = dict(max_disparity=D, box_radius=r, ang_radius=c["ang_radius"], min_valid=mv)
    got = ctx.repair_fill(d, fl, c["missing"], c["mask"], *_geo(c), out=out, codes_out=codes, disparity_out=disp, **kw)
    tag = f"{name} D={D} r={r} min_valid={mv}"
    assert np.array_equal(_bits(d), c["lf"].view(np.uint32)), tag                   # the input is only read
    assert np.array_equal(disp.cpu().numpy(), want["disp"]), tag
    assert np.array_equal(codes.cpu().numpy(), want["codes"]), tag
    assert np.array_equal(_bits(out), want["out"].view(np.uint32)), tag
    assert _counts(got) == _want_counts(want, c["C"]), tag
    assert got.out is out and got.codes is codes and got.disparity is disp
    again = ctx.repair_fill(d, fl, c["missing"], c["mask"], *_geo(c), return_codes=True, return_disparity=True, **kw)
    live = c["mask"] != 0
    assert np.array_equal(_bits(again.out)[live], _bits(out)[live]) and np.array_equal(again.codes.cpu().numpy()[live], want["codes"][live]), tag
    written = want["disp"] != K.DISP_SENTINEL
    assert np.array_equal(again.disparity.cpu().numpy()[written], want["disp"][written]), tag
    assert not again.disparity.cpu().numpy()[~written].any(), tag
    assert _counts(again) == _counts(got), tag
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("name", K.NAMES)
def test_fill_equals_the_model(ctx, name):
    for D, r in K.DRS:
        for mv in K.MIN_VALIDS:
            _assert_equals_model(ctx, name, D, r, mv)


@pytest.mark.gpu
def test_the_named_cases_take_the_paths_they_are_named_for(ctx):
    got, want = _assert_equals_model(ctx, "no-source", 3, 3, 1)
    assert sum(got.rim) > 0 and sum(got.left) == 0                                  # a position where every source is invalid: code 2
    got, want = _assert_equals_model(ctx, "lost-plane", 3, 3, 1)
    assert sum(got.left) == 3 * 6 * 7 and sum(got.views) == 0 and (got.targets, got.swept) == (3, 2)   # nothing can fill it: code 3
    got, want = _assert_equals_model(ctx, "nan", 3, 3, 1)
    assert np.isfinite(got.out.cpu().numpy()).all()                                 # no NaN leaks from an invalid source
    # a tile with no unsound position: the workgroup's early exit leaves a copy of the input (the output was pre-filled with a sentinel)
    c = K.case("quiet-tile")
    got, want = _assert_equals_model(ctx, "quiet-tile", 3, 3, 1)
    o = _bits(got.out).reshape(9, 40, 100)
    assert np.array_equal(o[:, :, 64:], c["lf"].view(np.uint32).reshape(9, 40, 100)[:, :, 64:])
    assert np.array_equal(o[:, 32:, :], c["lf"].view(np.uint32).reshape(9, 40, 100)[:, 32:, :])
    assert (got.disparity.cpu().numpy().reshape(9, 40, 100)[:, :, 64:] == K.DISP_SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", K.CLEAN)
def test_without_defects_the_fill_is_the_view_synthesis(ctx, name):
    """Property 1 on the GPU: no flag, only missing SAIs: the planes and d* of lfbm5d_view_fill_device, bit for bit."""
    c = K.case(name)
    d = _dev(c["lf"])
    miss = c["missing"] != 0
    for D, r in K.DRS:
        kw = dict(max_disparity=D, box_radius=r, ang_radius=c["ang_radius"])
        view = ctx.view_fill(d, c["mask"], c["missing"], *_geo(c), return_disparity=True, **kw)
        for flags in (None, _dev(np.zeros(c["lf"].shape, np.uint8))):
            got = ctx.repair_fill(d, flags, c["missing"], c["mask"], *_geo(c), min_valid=1, return_codes=True, return_disparity=True, **kw)
            assert np.array_equal(_bits(got.out)[miss], _bits(view.out)[miss])
            assert np.array_equal(got.disparity.cpu().numpy()[miss], view.disparity.cpu().numpy()[miss])
            assert list(got.disparity_hist) == list(view.disparity_hist) and got.positions == view.pixels
            sound = (c["mask"] != 0) & ~miss
            assert np.array_equal(_bits(got.out)[sound], c["lf"].view(np.uint32)[sound])
            assert (got.codes.cpu().numpy()[miss] == 1).all() and not got.codes.cpu().numpy()[~miss].any()


@pytest.mark.gpu
def test_host_forms_return_the_device_forms_bits(ctx):
    c = K.case("nan")
    P = core.make_params(20.0, 2.7, *HT)
    kw = dict(max_disparity=3, box_radius=3, min_valid=2, iterations=0, return_codes=True, return_disparity=True)
    args = (c["mask"], P, c["ang_major"], c["aw"], c["ah"], 1, c["W"], c["H"], c["C"])
    dev = ctx.repair(_dev(c["lf"]), _dev(c["flags"]), c["missing"], *args, **kw)
    want = K.model("nan", 3, 3, 2)
    assert np.array_equal(_bits(dev.out), want["out"].view(np.uint32)) and np.array_equal(dev.codes.cpu().numpy(), want["codes"])
    forms = {"numpy": (c["lf"], c["flags"]), "list": (list(c["lf"]), list(c["flags"]))}
    for form, (lf, fl) in forms.items():
        got = ctx.repair(lf, fl, c["missing"], *args, **kw)
        assert np.array_equal(_bits(np.stack(got.out)), _bits(dev.out)), form
        assert np.array_equal(np.stack(got.codes), dev.codes.cpu().numpy()), form
        assert np.array_equal(np.stack(got.disparity), dev.disparity.cpu().numpy()), form
        assert got[3:] == dev[3:], form
    got = L.repair(_dev(c["lf"]), _dev(c["flags"]), c["missing"], *args, ctx=ctx, **kw)    # the module function, torch form
    assert np.array_equal(_bits(got.out), _bits(dev.out)) and got[3:] == dev[3:]
    got = ctx.repair(c["lf"], None, c["missing"], *args, **kw)                       # no flags: NaN, inf and the missing SAI alone
    assert got.flagged == 0 and np.isfinite(got.out).all()


@pytest.mark.gpu
def test_the_loop_equals_the_models_loop_on_the_gpus_own_step(ctx):
    """Golden crop 96..159 with add_defects(seed=2) written as 0 and SAI 4 missing, K = 2; a value nothing can fill refuses K >= 1."""
    import torch
    clean, flb, y, n = K.golden(96, 160)
    flags = flb.astype(np.uint8)
    mask, miss = np.ones(9, np.uint32), np.zeros(9, np.uint32)
    miss[4] = 1
    P = core.make_params(20.0, 2.7, *HT)
    geo = (L.ROWMAJOR, 3, 3, 1, n, n, 3)

    def step(z, sig):
        zz = _dev(z.reshape(9, -1))
        basic = torch.zeros_like(zz)
        ctx.step1(core.make_params(sig, 2.7, *HT), zz, mask, basic, *geo)
        return basic.cpu().numpy()
    x, x0, res = M.loop(y, flags, mask, miss, L.ROWMAJOR, 3, 3, n, n, 3, 3, 3, 2, 30.0, 5.0, step, min_valid=2)
    kw = dict(max_disparity=3, box_radius=3, ang_radius=1, min_valid=2, sigma_start=30.0, sigma_end=5.0, return_codes=True)
    got = ctx.repair(_dev(y), _dev(flags), miss, mask, P, *geo, iterations=2, **kw)
    assert np.array_equal(got.codes.cpu().numpy(), res["codes"])
    assert np.array_equal(_bits(got.out), x.view(np.uint32))
    assert not np.array_equal(x.view(np.uint32), x0.view(np.uint32))                # the steps did something
    zero = ctx.repair(_dev(y), _dev(flags), miss, mask, P, *geo, iterations=0, **kw)
    assert np.array_equal(_bits(zero.out), x0.view(np.uint32))                      # K = 0 is the fill alone
    c = K.case("lost-plane")
    out = _dev(np.full(c["lf"].shape, K.OUT_SENTINEL, np.float32))
    with pytest.raises(L.LfBm5dError, match="lfbm5d_repair_device: .*cannot be refined"):
        ctx.repair(_dev(c["lf"]), _dev(c["flags"]), c["missing"], c["mask"], P, c["ang_major"], c["aw"], c["ah"], 1, c["W"], c["H"], c["C"],
                   iterations=1, out=out)
    assert np.array_equal(_bits(out), K.model("lost-plane", 4, 3, 3)["out"].view(np.uint32))   # ... after the fill was written


@pytest.mark.gpu
def test_the_drop_ins_repair_lf_returns_the_device_forms_bits(ctx):
    """repair_LF of run_bm5d.h on vector<vector<float>> light fields: the fill alone, and the loop with K = 1."""
    clean, flb, y, n = K.golden(96, 160)
    flags = flb.astype(np.uint8)
    mask, miss = np.ones(9, np.uint32), np.zeros(9, np.uint32)
    miss[4] = 1
    P = core.make_params(0.0, 2.7, *HT)
    for iters in (0, 1):
        dev = ctx.repair(_dev(y), _dev(flags), miss, mask, P, L.ROWMAJOR, 3, 3, 1, n, n, 3, iterations=iters, sigma_noise=3.0)
        out, counts, dmin, dmax = core.repair_probe(y, flags, mask, miss, 3, 3, n, n, 3, 2.7, HT, iterations=iters, sigma_noise=3.0)
        assert np.array_equal(out.view(np.uint32), _bits(dev.out)), iters
        assert counts == (dev.values, dev.flagged, dev.missing, sum(dev.views), sum(dev.rim), sum(dev.left)), iters
        hist = np.flatnonzero(dev.disparity_hist) - 8
        assert (dmin, dmax) == (int(hist.min()), int(hist.max())), iters
    out, counts, dmin, dmax = core.repair_probe(y, None, mask, miss, 3, 3, n, n, 3, 2.7, HT, iterations=0)   # no flags: the missing SAI alone
    assert counts[1] == 0 and counts[2] == 1 and counts[3] == 3 * n * n
