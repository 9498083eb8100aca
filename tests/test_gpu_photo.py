"""GPU tests of the photometric equalisation (lfbm5d_photo_*, include/lfbm5d_photo.h): histograms, counters, gains, states, rounds,
converged, residual and every output float equal the numpy model (tests/photo_model.py) bit for bit on the cases of tests/photo_cases.py
-- a planted vignette and a cast on random and textured data, an empty SAI and untested corners at both angular radii, degenerate
angular axes, planes that cross every tile edge, non-finite values, both angular orders -- at (D, r) = (0, 0) and (3, 3); with two
steps per pixel, pooled channels, an anchor, one round, a min_count that makes channels unfit; planes of empty SAIs keep a sentinel and a
second call returns the same bits; the host forms return the device form's bits; and apply_gains equals the model's multiplications,
in place too."""
import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core
import photo_cases as K
import photo_model as M


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _kw(c, D, r, more=()):
    p = dict(c["params"], **dict(more))
    return dict(p, max_disparity=D, box_radius=r)


def _run(ctx, c, D, r, more=(), lf=None):
    import torch
    A = c["aw"] * c["ah"]
    out = torch.full((A, c["C"] * c["H"] * c["W"]), float(K.OUT_SENTINEL), dtype=torch.float32, device="cuda")
    d = _dev(c["lf"]) if lf is None else lf
    got = ctx.equalise(d, c["mask"], c["ang_major"], c["aw"], c["ah"], c["W"], c["H"], c["C"], return_hist=True, out=out, **_kw(c, D, r, more))
    assert got.out is out
    return got, d


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_equal(got, want, tag):
    assert np.array_equal(got.hist, want["hist"]), tag
    assert (got.admitted, got.skipped_nonfinite, got.skipped_range) == (want["admitted"], want["nonfinite"], want["outside"]), tag
    assert (got.rounds, int(got.converged), got.fitted, got.untested, got.unfit) == \
           (want["rounds"], want["converged"], want["fitted"], want["untested"], want["unfit"]), tag
    assert list(got.state) == list(want["state"]), tag
    assert np.array_equal(_bits(got.gain), _bits(want["gain"])), tag                 # doubles, bit for bit
    assert [np.float64(v).tobytes() for v in (got.residual, got.gain_min, got.gain_max)] == \
           [np.float64(v).tobytes() for v in (want["residual"], want["gain_min"], want["gain_max"])], tag
    assert np.array_equal(_bits(got.out.cpu().numpy()), _bits(want["out"])), tag     # every output float, the sentinel planes included


@pytest.mark.gpu
@pytest.mark.parametrize("D,r", K.DRS)
@pytest.mark.parametrize("name", K.NAMES)
def test_equalise_equals_the_model(ctx, name, D, r):
    c, want = K.case(name), K.model(name, D, r)
    got, d = _run(ctx, c, D, r)
    tag = f"{name} D={D} r={r}"
    assert np.array_equal(_bits(d.cpu().numpy()), _bits(c["lf"])), tag               # the input is only read
    _assert_equal(got, want, tag)
    empty = np.nonzero(c["mask"] == 0)[0]
    assert (got.out.cpu().numpy()[empty] == K.OUT_SENTINEL).all()                    # empty SAIs keep the sentinel
    again, _ = _run(ctx, c, D, r, lf=d)
    _assert_equal(again, want, tag + " (second call)")
    # what the cases are there for
    if name in ("textured", "uniform"):
        assert want["rounds"] >= 2 and want["fitted"] == 9
        assert want["gain"][2, 1] / want["gain"][2, 0] > 1.05                        # the cast on one channel of one view is found
    if name.startswith("5x5"):
        assert want["state"][7] == M.EMPTY and [want["state"][m] for m in (0, 4, 20, 24)] == [M.UNTESTED] * 4 and want["fitted"] == 20
    if name in ("1x3", "3x1"):
        assert list(want["state"]) == [M.UNTESTED, M.FITTED, M.UNTESTED]
    if name == "nan":
        assert want["nonfinite"] > 22 and np.isnan(want["out"]).sum() == 18           # counted in sources' neighbours too; NaN stays NaN


@pytest.mark.gpu
@pytest.mark.parametrize("more", [(("steps", 2),), (("per_channel", 0),), (("anchor", 4),), (("anchor", 0), ("per_channel", 0)),
                                  (("max_rounds", 1),), (("tol", 0.0), ("max_rounds", 2)), (("tol", 10.0),), (("min_sources", 4),),
                                  (("min_sources", 9),), (("lo", 60.0), ("hi", 90.0))], ids=str)
def test_switches(ctx, more):
    name = "2x3-row" if more == (("steps", 2),) else "textured"
    c, want = K.case(name), K.model(name, 3, 3, more)
    got, _ = _run(ctx, c, 3, 3, more)
    _assert_equal(got, want, str(more))
    m = dict(more)
    if m.get("anchor") is not None:
        assert (want["gain"][m["anchor"]] == 1.0).all()
    if "per_channel" in m:
        assert (want["gain"][:, 0] == want["gain"][:, 1]).all() and (want["gain"][:, 0] == want["gain"][:, 2]).all()
    if m.get("max_rounds") == 1:
        assert (want["rounds"], want["converged"]) == (1, 0)
    if m.get("tol") == 0.0:
        assert (want["rounds"], want["converged"]) == (2, 0)
    if m.get("tol") == 10.0:                                                         # within tol at once: the output is the input
        assert (want["rounds"], want["converged"]) == (1, 1) and (want["gain"] == 1.0).all()
        assert np.array_equal(_bits(got.out.cpu().numpy()), _bits(c["lf"]))
    if m.get("min_sources") == 4:
        assert [want["state"][i] for i in (0, 2, 6, 8)] == [M.UNTESTED] * 4
    if m.get("min_sources") == 9:                                                    # nothing is tested: one sweep of nothing
        assert want["untested"] == 9 and want["admitted"] == 0 and (want["rounds"], want["converged"]) == (1, 1)


@pytest.mark.gpu
def test_a_min_count_that_makes_channels_unfit(ctx):
    """min_count between the counts the first sweep admits per (SAI, channel): about a third of the pairs are unfit, keep gain 1 and
    still count as sources."""
    c = K.case("textured")
    counts = np.sort(K.model("textured", 3, 3, (("max_rounds", 1),))["hist"].sum(axis=2).ravel())
    min_count = int(counts[len(counts) // 3]) + 1
    assert counts[0] < min_count <= counts[-1]
    more = (("min_count", min_count),)
    want = K.model("textured", 3, 3, more)
    got, _ = _run(ctx, c, 3, 3, more)
    _assert_equal(got, want, "min_count")
    assert want["unfit"] >= 1 and (want["state"] == M.UNFIT).any() and not want["fits"][0].all() and want["fits"][0].any()
    assert (want["gain"][~want["fits"][0] & ~want["fits"][-1]] == 1.0).all()


@pytest.mark.gpu
def test_both_angular_orders_agree(ctx):
    """The same scene indexed column-major: the same histograms; the sources of an SAI come in another order, so the solve's sums of
    gains may differ in their last bit, and the corrected values by one float32 rounding."""
    row, col = K.model("2x3-row", 3, 3), K.model("2x3-col", 3, 3)
    perm = [(st % 2) * 3 + st // 2 for st in range(6)]
    assert np.array_equal(col["ratios"][0], row["ratios"][0][perm]) and list(col["state"]) == list(row["state"][perm])
    assert np.abs(col["gain"] / row["gain"][perm] - 1.0).max() < 1e-12
    got, _ = _run(ctx, K.case("2x3-col"), 3, 3)
    assert np.abs(got.gain / row["gain"][perm] - 1.0).max() < 1e-12
    assert np.allclose(got.out.cpu().numpy(), row["out"][perm], rtol=2.0 ** -22, atol=0.0)


@pytest.mark.gpu
def test_host_forms_return_the_device_forms_bits(ctx):
    for name in ("textured", "5x5-R1"):
        c = K.case(name)
        A, C_, W, H = c["aw"] * c["ah"], c["C"], c["W"], c["H"]
        geo = (c["ang_major"], c["aw"], c["ah"], W, H, C_)
        kw = _kw(c, 3, 3)
        dev = ctx.equalise(_dev(c["lf"]), c["mask"], *geo, return_hist=True, **kw)
        d_out = dev.out.cpu().numpy()
        live = c["mask"] != 0
        assert np.array_equal(_bits(d_out[~live]), _bits(c["lf"][~live]))            # a fresh output is the input in empty SAIs
        h = ctx.equalise(c["lf"].copy(), c["mask"], *geo, return_hist=True, **kw)       # a flat host array
        assert isinstance(h.out, np.ndarray) and h.out.shape == c["lf"].shape and np.array_equal(_bits(h.out), _bits(d_out))
        assert np.array_equal(_bits(h.gain), _bits(dev.gain)) and list(h.state) == list(dev.state) and np.array_equal(h.hist, dev.hist)
        assert h[4:] == dev[4:]
        sais = [c["lf"][i].copy() if live[i] else None for i in range(A)]               # one array per SAI, None for empty ones
        l = L.equalise(sais, c["mask"], *geo, ctx=ctx, **kw)
        assert all(np.array_equal(_bits(l.out[i]), _bits(d_out[i])) for i in range(A) if live[i]) and l.hist is None and l[4:] == dev[4:]
        assert all(l.out[i] is None for i in range(A) if not live[i]) and np.array_equal(_bits(l.gain), _bits(dev.gain))
        t = L.equalise(_dev(c["lf"]), c["mask"], *geo, ctx=ctx, **kw)                  # the module-level torch form
        assert np.array_equal(_bits(t.out.cpu().numpy()), _bits(d_out)) and t[4:] == dev[4:]
        p = c["params"]                                                                # the C++ drop-in: equalise_LF, apply_gains_LF
        pk = dict(max_disparity=3, box_radius=3, ang_radius=p["ang_radius"], min_sources=p["min_sources"], max_rounds=p["max_rounds"],
                  per_channel=p["per_channel"], tol=p["tol"], lo=p["lo"], hi=p["hi"], ang_major=c["ang_major"])
        # equalise_LF has no min_count argument: it runs at the library's default, which these cases' parameters spell out
        assert L.photo_params().min_count == p["min_count"]
        cpp = core.equalise_probe(c["lf"], c["mask"], c["aw"], c["ah"], W, H, C_, **pk)
        assert np.array_equal(_bits(cpp[0][live]), _bits(d_out[live])) and np.array_equal(_bits(cpp[1]), _bits(dev.gain))
        assert list(cpp[2]) == list(dev.state)
        assert cpp[3:] == (dev.fitted, dev.untested, dev.unfit, dev.rounds, dev.residual, dev.gain_min, dev.gain_max)
        back = core.equalise_probe(c["lf"], c["mask"], c["aw"], c["ah"], W, H, C_, restore=True, **pk)[0]
        assert np.array_equal(_bits(back[live]), _bits(M.apply_gains(d_out, c["mask"], dev.gain, C_, invert=True)[live]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["textured", "5x5-R1", "tiles-31x65", "3x1"])
def test_apply_gains_equals_the_models_multiplications(ctx, name):
    """Planes of 37 x 70, 33 x 34, 31 x 65 and 2 x 2 floats: every alignment of a plane within 16 bytes, planes shorter than a group of
    four; a view of the tensor that starts 4 bytes off; in place; and there and back."""
    import torch
    c = K.case(name)
    A, C_ = c["aw"] * c["ah"], c["C"]
    gain = np.ones((A, 3), np.float64)
    gain[:, :C_] = np.random.default_rng(A).uniform(0.4, 1.6, (A, C_))
    mask = c["mask"]
    live = mask != 0
    d = _dev(c["lf"])
    fwd = M.apply_gains(c["lf"], mask, gain, C_)
    out = torch.full_like(d, float(K.OUT_SENTINEL))
    got = ctx.apply_gains(d, gain, chnls=C_, mask=mask, out=out)
    assert got is out and np.array_equal(_bits(got.cpu().numpy()), _bits(M.apply_gains(c["lf"], mask, gain, C_, out=np.full_like(c["lf"], K.OUT_SENTINEL))))
    assert np.array_equal(_bits(d.cpu().numpy()), _bits(c["lf"]))
    back = ctx.apply_gains(got, gain, invert=True, chnls=C_, mask=mask)               # a fresh tensor: a copy of its input in empty SAIs
    want_back = M.apply_gains(fwd, mask, gain, C_, invert=True)
    assert np.array_equal(_bits(back.cpu().numpy()[live]), _bits(want_back[live]))
    same = d.clone()
    assert ctx.apply_gains(same, gain, chnls=C_, mask=mask, out=same) is same         # in place
    assert np.array_equal(_bits(same.cpu().numpy()[live]), _bits(fwd[live])) and np.array_equal(_bits(same.cpu().numpy()[~live]), _bits(c["lf"][~live]))
    n = c["lf"].size
    pad = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
    pad[1:] = d.reshape(-1)
    off = pad[1:].view(A, -1)                                                         # 4 bytes off a 16-byte boundary
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    assert np.array_equal(_bits(ctx.apply_gains(off, gain, chnls=C_, mask=mask).cpu().numpy()[live]), _bits(fwd[live]))
    o2 = torch.zeros(n + 2, dtype=torch.float32, device="cuda")[2:].view(A, -1)       # input and output sit differently: single values
    ctx.apply_gains(off, gain, chnls=C_, mask=mask, out=o2)
    assert np.array_equal(_bits(o2.cpu().numpy()[live]), _bits(fwd[live])) and not o2.cpu().numpy()[~live].any()
    host = ctx.apply_gains(c["lf"].copy(), gain, chnls=C_, mask=mask)                  # the host form
    assert isinstance(host, np.ndarray) and np.array_equal(_bits(host[live]), _bits(fwd[live]))
    # equalise's own gains, divided out and multiplied back: the model's two multiplications
    eq = K.model(name, 3, 3)
    e = ctx.apply_gains(d, eq["gain"], chnls=C_, mask=mask)
    assert np.array_equal(_bits(e.cpu().numpy()[live]), _bits(M.apply_gains(c["lf"], mask, eq["gain"], C_)[live]))
    e2 = ctx.apply_gains(e, eq["gain"], invert=True, chnls=C_, mask=mask, out=e)
    assert np.array_equal(_bits(e2.cpu().numpy()[live]), _bits(M.apply_gains(M.apply_gains(c["lf"], mask, eq["gain"], C_), mask, eq["gain"], C_, invert=True)[live]))
