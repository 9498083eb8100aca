"""GPU tests of the sub-pixel plane sweep (the *_steps_* forms of lfbm5d_view_* and lfbm5d_consist_*, include/lfbm5d.h): k_view_sweep_subpel
equals the numpy model (tests/subpel_model.py) bit for bit -- values, int8 j*, counts and the 65-bin histogram -- at steps 2 and 4 on
the shapes of tests/subpel_cases.py (tile edges, asymmetric sources, both instantiations, planes narrower than shift plus halo plus the
+1 neighbour, one source, a decision boundary across every tile edge and corner), with sentinels in what must not be written and a
second call returning the same bits; steps = 1 through the new entry points is the old entry points' bits; the consistency check with
the sub-pixel spread; the loop against the same calls made by hand; the host form, the C++ drop-in, rejected steps and the CLI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core
import consist_cases as CC
import subpel_cases as K
import subpel_model as S
import view_model as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "lfbm5d_amd", "LFBM5Ddenoising")
HT = (8, 8, 3, 8, 3, "dct", "sadct", "haar")


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


def _assert_equals_model(ctx, shape, kind, steps, D, r, d=None):
    """One synthesis against the model, with sentinels in what must not be written; and a second call returns the same bits."""
    ah, aw, H, W, C_, miss, empty, R = K.SHAPES[shape]
    lf, mask, missing = K.case(shape, kind)
    want = K.model(shape, kind, steps, D, r)
    d = _dev(lf) if d is None else d
    out = _dev(np.full(lf.shape, K.OUT_SENTINEL, np.float32))
    disp = _dev(np.full((ah * aw, H * W), K.DISP_SENTINEL, np.int8))
    kw = dict(max_disparity=D, box_radius=r, ang_radius=R, disparity_steps=steps)
    got = ctx.view_fill(d, mask, missing, K.ROWMAJOR, aw, ah, W, H, C_, out=out, disparity_out=disp, **kw)
    tag = f"{shape} {kind} steps={steps} D={D} r={r}"
    assert np.array_equal(disp.cpu().numpy(), want["disp"]), tag                 # j*, and the sentinel elsewhere
    assert np.array_equal(_bits(out), want["out"].view(np.uint32)), tag
    assert (got.missing, got.synthesised, got.left, got.pixels) == (want["missing"], want["synthesised"], want["left"], want["pixels"]), tag
    assert list(got.steps_hist) == list(want["hist"]) and len(got.steps_hist) == S.HIST, tag
    assert not any(got.disparity_hist), tag                                     # the 17 bins are the integer sweep's
    again = ctx.view_fill(d, mask, missing, K.ROWMAJOR, aw, ah, W, H, C_, return_disparity=True, **kw)
    s = want["sais"]
    assert np.array_equal(_bits(again.out)[s], _bits(out)[s]) and np.array_equal(again.disparity.cpu().numpy()[s], want["disp"][s]), tag
    assert again[2:] == got[2:], tag
    return got, want, d


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_synthesis_equals_the_model(ctx, shape):
    ah, aw, H, W, C_, miss, empty, R = K.SHAPES[shape]
    dev = {}
    for kind, steps, D, r in K.combos(shape):
        got, want, dev[kind] = _assert_equals_model(ctx, shape, kind, steps, D, r, dev.get(kind))
        assert (got.synthesised, got.left) == (len(miss), 0)
        assert np.isfinite(got.out.cpu().numpy()[miss]).all()
        if shape.startswith("single"):                                          # one source: E = 0 everywhere, j* = 0, a copy
            lf = K.case(shape, kind)[0]
            assert np.array_equal(_bits(got.out)[miss[0]], lf[1 - miss[0]].view(np.uint32)) and got.steps_hist[S.J_MAX] == H * W
    for kind, d in dev.items():                                                 # the input is only read
        assert np.array_equal(_bits(d), K.case(shape, kind)[0].view(np.uint32))
    if shape == "centre-R2":
        lf, mask, missing = K.case(shape, "uniform")
        assert len(V.sources(12, mask, missing, K.ROWMAJOR, aw, ah, R)) == 24   # more than 8 sources: the instantiation that recomputes ran
    if shape == "centre":                                                       # the photograph moves 2 pixels per view
        j = K.model(shape, "textured", 4, 8, 7)["disp"][4].reshape(H, W)[15:-15, 15:-15]
        assert (np.abs(j) == 8).all()
    if shape.startswith("edges"):                                               # both planes of the scene on both sides of every tile edge
        m = miss[0]
        j = K.model(shape, "scene", 2, 3, 0)["disp"][m].reshape(H, W)
        for y in range(K.TILE_H - 1, H - 1, K.TILE_H):
            assert len(np.unique(j[y])) > 1 and len(np.unique(j[y + 1])) > 1
        for x in range(K.TILE_W - 1, W - 1, K.TILE_W):
            assert len(np.unique(j[:, x])) > 1 and len(np.unique(j[:, x + 1])) > 1


@pytest.mark.gpu
def test_one_step_through_the_new_entry_points_is_the_old_entry_points_bits(ctx):
    import torch
    ah, aw, H, W, C_, miss, empty, R = K.SHAPES["centre"]
    lf, mask, missing = K.case("centre", "textured")
    d = _dev(lf)
    lib, up = core.lib(), C.POINTER(C.c_uint)
    mp, sp = mask.ctypes.data_as(up), missing.ctypes.data_as(up)
    for D, r in ((3, 3), (8, 7)):
        old = ctx.view_fill(d, mask, missing, K.ROWMAJOR, aw, ah, W, H, C_, max_disparity=D, box_radius=r, return_disparity=True)
        out = torch.full_like(d, K.OUT_SENTINEL)
        disp = torch.full((ah * aw, H * W), K.DISP_SENTINEL, dtype=torch.int8, device="cuda")
        vp, res = L.view_params(D, r, R), core.ViewResultStruct()
        hist = np.zeros(S.HIST, np.uint64)
        rc = lib.lfbm5d_view_fill_steps_device(ctx._h, C.byref(vp), 1, C.c_void_p(d.data_ptr()), mp, sp, C.c_void_p(out.data_ptr()),
                                               C.c_void_p(disp.data_ptr()), K.ROWMAJOR, aw, ah, W, H, C_, C.byref(res),
                                               hist.ctypes.data_as(C.POINTER(C.c_ulonglong)))
        assert rc == 0
        assert np.array_equal(_bits(out)[miss], _bits(old.out)[miss]) and np.array_equal(disp.cpu().numpy()[miss], old.disparity.cpu().numpy()[miss])
        assert (out[[i for i in range(9) if i not in miss]] == K.OUT_SENTINEL).all().item()
        assert tuple(res.disparity_hist) == old.disparity_hist and old.steps_hist is None
        assert list(hist[S.J_MAX - 8:S.J_MAX + 9]) == list(old.disparity_hist) and hist.sum() == sum(old.disparity_hist)
        want = V.fill(lf, mask, missing, K.ROWMAJOR, aw, ah, W, H, C_, D, r, R)  # and both are the integer model's
        assert np.array_equal(_bits(out)[miss], want["out"].view(np.uint32)[miss])
    c = CC.case("textured")                                                     # the consistency check
    a = ctx.consist(d := _dev(c["lf"]), c["mask"], c["ang_major"], 3, 3, 70, 37, 3, return_disparity=True, fill_nonfinite=False,
                    max_disparity=3, box_radius=3, **c["params"])
    P, res = L.consist_params(max_disparity=3, box_radius=3, **c["params"]), core.ConsistResultStruct()
    flags = torch.zeros(c["lf"].shape, dtype=torch.uint8, device="cuda")
    disp = torch.zeros((9, 37 * 70), dtype=torch.int8, device="cuda")
    state, ssai = np.zeros(9, np.uint32), np.zeros(9, np.float64)
    h = np.zeros((9, 3, core.IMPULSE_KEYS), np.uint64)
    rc = lib.lfbm5d_consist_steps_device(ctx._h, C.byref(P), 1, C.c_void_p(d.data_ptr()), c["mask"].ctypes.data_as(up), None,
                                         C.c_void_p(flags.data_ptr()), state.ctypes.data_as(up), C.c_void_p(disp.data_ptr()),
                                         ssai.ctypes.data_as(C.POINTER(C.c_double)), h.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                         c["ang_major"], 3, 3, 70, 37, 3, C.byref(res))
    assert rc == 0
    tested = [i for i in range(9) if state[i] == 1]
    assert np.array_equal(flags.cpu().numpy(), a.flags.cpu().numpy()) and list(state) == list(a.state)
    assert np.array_equal(disp.cpu().numpy()[tested], a.disparity.cpu().numpy()[tested])
    assert np.array_equal(h, a.hist) and np.array_equal(ssai.view(np.uint64), a.scale_sai.view(np.uint64)) and res.rounds == a.rounds


def _consist_equal(got, want, C_, tag):
    assert np.array_equal(got.flags.cpu().numpy(), want["flags"]), tag
    assert np.array_equal(got.disparity.cpu().numpy(), want["disp"]), tag
    assert list(got.state) == list(want["state"]), tag
    assert np.array_equal(got.hist, want["hist"]), tag
    assert list(got.scale_channel) == list(want["scale_channel"][:C_]), tag
    assert np.array_equal(np.array(got.threshold, np.float32).view(np.uint32), want["threshold"][:C_].view(np.uint32)), tag
    assert np.array_equal(got.scale_sai.view(np.uint64), want["scale_sai"].view(np.uint64)), tag
    assert list(got.flagged) == list(want["counts"][:C_, 0]) and list(got.nonfinite) == list(want["counts"][:C_, 1]), tag
    assert (list(got.bad), list(got.untested), got.rounds, got.pixels, got.skipped) == \
           (want["bad"], want["untested"], want["rounds"], want["pixels"], want["skipped"]), tag


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["textured", "tiles-31x65"])
def test_consist_with_two_steps_equals_the_model(ctx, name):
    """Planted defects and a noise SAI (two rounds), and defects across the tile edges, at steps = 2, (D, r) = (3, 3): flags, states, j*,
    scales, histograms and result against the model with the sub-pixel spread."""
    import torch
    c = CC.case(name)
    A, C_, H, W = c["aw"] * c["ah"], c["C"], c["H"], c["W"]
    f0 = np.full((A, C_ * H * W), CC.FLAG_SENTINEL, np.uint8)
    d0 = np.full((A, H * W), CC.DISP_SENTINEL, np.int8)
    want = S.consist(c["lf"], c["mask"], c["ang_major"], c["aw"], c["ah"], W, H, C_, steps=2, D=3, r=3, exclude=c["exclude"], flags=f0, disp=d0,
                     **c["params"])
    d = _dev(c["lf"])
    for call in ("first", "second"):
        flags, disp = _dev(f0), _dev(d0)
        got = ctx.consist(d, c["mask"], c["ang_major"], c["aw"], c["ah"], W, H, C_, exclude=c["exclude"], flags_out=flags, disparity_out=disp,
                          fill_nonfinite=False, max_disparity=3, box_radius=3, disparity_steps=2, **c["params"])
        _consist_equal(got, want, C_, f"{name} ({call} call)")
    assert np.array_equal(_bits(d), c["lf"].view(np.uint32))
    assert (np.abs(want["disp"][want["tested"]].astype(int)) % 2 == 1).any()     # fractional hypotheses were chosen
    # the host form and the C++ drop-in return the same flags and states
    h = ctx.consist(c["lf"].copy(), c["mask"], c["ang_major"], c["aw"], c["ah"], W, H, C_, exclude=c["exclude"], return_disparity=True,
                    fill_nonfinite=False, max_disparity=3, box_radius=3, disparity_steps=2, **c["params"])
    assert np.array_equal(h.flags, np.where(want["flags"] == CC.FLAG_SENTINEL, 0, want["flags"])) and list(h.state) == list(want["state"])
    assert np.array_equal(h.disparity[want["tested"]], want["disp"][want["tested"]])
    p = c["params"]
    cpp = core.consist_probe(c["lf"], c["mask"], c["aw"], c["ah"], W, H, C_, max_disparity=3, box_radius=3, ang_radius=p["ang_radius"],
                             min_sources=p["min_sources"], max_rounds=p["max_rounds"], k=p["k"], spread=p["spread"], sai_factor=p["sai_factor"],
                             ang_major=c["ang_major"], disparity_steps=2)
    assert np.array_equal(cpp[0], h.flags) and list(cpp[1]) == list(want["state"]) and cpp[6] == want["rounds"]


def _golden_crop(lo, hi):
    return np.load(K.GOLDEN)[:, :, lo:hi, lo:hi].astype(np.float32).reshape(9, -1)


@pytest.mark.gpu
def test_loop_host_form_and_drop_in(ctx):
    """lfbm5d_view_steps_device with K = 2 equals the same public calls made by hand (fill, step 1, copies) in bits; the host form equals
    the device form; the C++ drop-in runs with disparity_steps = 2."""
    import torch
    Kn, tail = 2, (L.ROWMAJOR, 3, 3, 1, 64, 64, 3)
    clean = _golden_crop(80, 144)
    mask, missing = np.ones(9, np.uint32), np.zeros(9, np.uint32)
    missing[[0, 4]] = 1
    y = clean.copy()
    y[[0, 4]] = np.nan                                                          # never read
    d_y = _dev(y)
    P = core.make_params(0.0, 2.7, *HT)
    kw = dict(max_disparity=3, box_radius=3, iterations=Kn, sigma_start=30.0, sigma_end=5.0, disparity_steps=2)
    a = ctx.view_synth(d_y, mask, missing, P, *tail, return_disparity=True, **kw)
    assert np.array_equal(_bits(d_y), y.view(np.uint32))
    x0 = ctx.view_fill(d_y, mask, missing, L.ROWMAJOR, 3, 3, 64, 64, 3, max_disparity=3, box_radius=3, return_disparity=True, disparity_steps=2)
    want = S.fill(y, mask, missing, V.ROWMAJOR, 3, 3, 64, 64, 3, 3, 3, steps=2)
    assert np.array_equal(_bits(x0.out)[[0, 4]], want["out"].view(np.uint32)[[0, 4]]) and list(x0.steps_hist) == list(want["hist"])
    assert np.array_equal(x0.disparity.cpu().numpy()[[0, 4]], a.disparity.cpu().numpy()[[0, 4]]) and a.steps_hist == x0.steps_hist
    flags = torch.zeros(y.shape, dtype=torch.uint8, device="cuda")
    flags[[0, 4]] = 1
    x = x0.out
    for sig in V.sigma_schedule(Kn, 30.0, 5.0):
        z = x.clone()
        basic = torch.zeros_like(z)
        ctx.step1(core.make_params(sig, 2.7, *HT), z, mask, basic, *tail)
        x = torch.zeros_like(z)
        ctx.inpaint_project(flags, basic, d_y, mask, x, 64, 64, 3)
    assert np.array_equal(_bits(a.out), _bits(x))
    sound = missing == 0
    assert np.array_equal(_bits(a.out)[sound], clean.view(np.uint32)[sound])
    one = ctx.view_synth(d_y, mask, missing, P, *tail, **dict(kw, disparity_steps=1))
    assert not np.array_equal(_bits(one.out), _bits(a.out)) and one.steps_hist is None
    # the host form
    h = ctx.view_synth(y.copy(), mask, missing, P, *tail, return_disparity=True, **kw)
    assert isinstance(h.out, np.ndarray) and np.array_equal(h.out.view(np.uint32), _bits(a.out))
    assert np.array_equal(h.disparity[[0, 4]], a.disparity.cpu().numpy()[[0, 4]]) and h[2:] == a[2:]
    # the C++ drop-in's view_synth_LF
    probe = {k: v for k, v in kw.items() if k != "disparity_steps"}
    cpp, done, left, jmin, jmax = core.view_synth_probe(y, mask, missing, 3, 3, 64, 64, 3, 2.7, HT, disparity_steps=2, **probe)
    assert np.array_equal(cpp.view(np.uint32), _bits(a.out))
    hist = np.array(a.steps_hist)
    assert (done, left, jmin, jmax) == (2, 0, int(np.nonzero(hist)[0][0]) - S.J_MAX, int(np.nonzero(hist)[0][-1]) - S.J_MAX)


@pytest.mark.gpu
def test_rejected_steps(ctx):
    import torch
    lf = np.random.default_rng(1).uniform(0.0, 255.0, (4, 3 * 40 * 66)).astype(np.float32)
    mask, missing = np.ones(4, np.uint32), np.array([0, 0, 0, 1], np.uint32)
    d = _dev(lf)
    out = torch.zeros_like(d)
    P = core.make_params(0.0, 2.7, *HT)
    for bad in (0, 3, 5, 8, 2 ** 31):
        with pytest.raises(L.LfBm5dError, match="steps must be 1, 2 or 4"):
            ctx.view_fill(d, mask, missing, L.ROWMAJOR, 2, 2, 66, 40, 3, out=out, disparity_steps=bad)
        with pytest.raises(L.LfBm5dError, match="steps must be 1, 2 or 4"):
            ctx.view_synth(d, mask, missing, P, L.ROWMAJOR, 2, 2, 1, 66, 40, 3, out=out, disparity_steps=bad)
        with pytest.raises(L.LfBm5dError, match="steps must be 1, 2 or 4"):
            ctx.view_synth(lf, mask, missing, P, L.ROWMAJOR, 2, 2, 1, 66, 40, 3, disparity_steps=bad)
        with pytest.raises(L.LfBm5dError, match="steps must be 1, 2 or 4"):
            ctx.consist(d, mask, L.ROWMAJOR, 2, 2, 66, 40, 3, disparity_steps=bad)
        with pytest.raises(L.LfBm5dError, match="steps must be 1, 2 or 4"):
            ctx.consist(lf, mask, L.ROWMAJOR, 2, 2, 66, 40, 3, disparity_steps=bad)
    assert not out.any().item()                                                 # nothing was written by a rejected call
    vp, res, up = L.view_params(), core.ViewResultStruct(), C.POINTER(C.c_uint)
    rc = core.lib().lfbm5d_view_fill_steps_device(ctx._h, C.byref(vp), 3, C.c_void_p(d.data_ptr()), mask.ctypes.data_as(up),
                                                  missing.ctypes.data_as(up), C.c_void_p(out.data_ptr()), None, L.ROWMAJOR, 2, 2, 66, 40, 3,
                                                  C.byref(res), None)
    assert rc == 1 and "lfbm5d_view_fill_steps_device: steps must be 1, 2 or 4" in core.lib().lfbm5d_last_error(ctx._h).decode()
    got = ctx.view_fill(d, mask, missing, L.ROWMAJOR, 2, 2, 66, 40, 3, out=out, disparity_steps=4, max_disparity=1, box_radius=1)
    assert out[3].any().item() and not out[:3].any().item() and sum(got.steps_hist) == 40 * 66


def _args(cli, tmp, src):
    return [cli, src, "SAI", "_", "3", "3", "1", "1", "1", "1", "row", "10", "2.7", f"{tmp}/noisy", f"{tmp}/basic",
            f"{tmp}/denoised", f"{tmp}/diff", "8", "8", "3", "8", "3", "dct", "sadct", "haar", "0", "16", "8", "3", "8", "3",
            "dct", "sadct", "haar", "0", "opp", "0", f"{tmp}/measures.txt"]


@pytest.mark.gpu
def test_cli_reconstructs_a_corner_sai_of_the_half_pixel_light_field(tmp_path):
    """LFBM5D_MISSING=1_1 on the half-pixel light field written as PNGs (noise of sigma 10 added by the command, one refinement step,
    then the denoiser): with LFBM5D_DISPARITY_STEPS=2 the report line says so and the missing SAI comes back better than with the
    variable unset."""
    from PIL import Image
    tmp = str(tmp_path)
    lf = np.clip(np.rint(S.half_pixel_lf().reshape(9, 3, 48, 80)), 0, 255).astype(np.uint8)
    src = os.path.join(tmp, "sourceLF")
    os.makedirs(src)
    for s in range(3):
        for t in range(3):
            Image.fromarray(lf[s * 3 + t].transpose(1, 2, 0)).save(f"{src}/SAI_{s + 1:02d}_{t + 1:02d}.png")
    for d in ("noisy", "basic", "denoised", "diff"):
        os.makedirs(os.path.join(tmp, d))
    true = lf[0].astype(np.float64)[:, 12:-12, 12:-12]
    psnr, lines = {}, {}
    for steps in (None, "2"):
        env = dict(os.environ, LFBM5D_SEED="1", LFBM5D_MISSING="1_1", LFBM5D_MISSING_ITER="1")
        env.pop("LFBM5D_DISPARITY_STEPS", None)
        if steps:
            env["LFBM5D_DISPARITY_STEPS"] = steps
        r = subprocess.run(_args(CLI, tmp, src), capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stdout[-2000:]
        lines[steps] = [l for l in r.stdout.split("\n") if l.startswith("View synthesis:")][0]
        rec = np.asarray(Image.open(f"{tmp}/denoised/SAI_01_01.png")).astype(np.float64).transpose(2, 0, 1)[:, 12:-12, 12:-12]
        psnr[steps] = 10.0 * np.log10(255.0 ** 2 / ((rec - true) ** 2).mean())
    print(lines, psnr)
    assert re.fullmatch(r"View synthesis: 1 of 9 SAIs missing, 0 left; disparities -?\d+\.\.-?\d+, 1 refinement steps", lines[None])
    m = re.fullmatch(r"View synthesis: 1 of 9 SAIs missing, 0 left; disparities (-?[\d.]+?)\.\.(-?[\d.]+), 1 refinement steps, 2 steps per pixel",
                     lines["2"])
    assert m and float(m.group(1)) <= 0.5 <= float(m.group(2)) and float(m.group(1)) * 2 == int(float(m.group(1)) * 2)
    assert psnr["2"] > psnr[None]                                               # the clean synthesis' model: 36.8 against 27.1 dB
