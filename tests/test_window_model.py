"""CPU tests of the model of the window-schedule kernels (tests/window_model.py) and of its cases (tests/window_cases.py): no GPU.

The model's primitives are pinned bit for bit against the CPU oracle -- colour transforms, mirror padding and cropping, the coverage
count -- and lfbm5d_sigma_table against the oracle's; every case proves that its inputs have the edges it is named for, and every
edge of the list occurs in some case; the model's fused ops equal the compositions they are defined as."""
import ctypes as C

import numpy as np
import pytest

import window_cases as K
import window_model as M
from lfbm5d_amd import core
from oracle import oracle as O

F = np.float32
CASES = K.all_cases()
bits = lambda a: np.ascontiguousarray(a, F).reshape(-1).view(np.uint32)


@pytest.mark.parametrize("cs", (O.YUV, O.YCBCR, O.OPP), ids=("yuv", "ycbcr", "opp"))
@pytest.mark.parametrize("forward", (1, 0), ids=("forward", "inverse"))
def test_colour_transforms_equal_the_oracle_bit_for_bit(cs, forward):
    rng = np.random.default_rng(7 + cs)
    W, H = 64, 67
    img = rng.uniform(-300, 600, (3, W * H)).astype(F)
    img[:, :8] = np.array([[0.0, -0.0, K.DENORMAL, -K.DENORMAL, 255.0, 600.5, -300.25, 1e30]] * 3, F)   # every channel at once
    img[0, 8:16], img[1, 16:24], img[2, 24:32] = 0.0, K.DENORMAL, -0.0                                   # ... and one at a time
    assert (img < 0).any() and (img > 255).any() and (img == 0).any() and (bits(img) == 1).any()
    want = img.copy().reshape(-1)
    assert O.lib().orc_color_transform(want, cs, W, H, 3, forward) == 0
    got = M.color(img, cs, forward)
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("W,H,Cc,N", [(64, 32, 3, 16), (67, 37, 1, 7), (9, 70, 3, 9), (130, 9, 1, 9), (65, 33, 3, 1), (5, 5, 1, 5), (20, 16, 3, 16)])
def test_padding_and_crop_equal_the_oracle(W, H, Cc, N):
    rng = np.random.default_rng(W * 1000 + H)
    img = rng.uniform(-300, 600, (Cc, H, W)).astype(F)
    want = np.full(Cc * (W + 2 * N) * (H + 2 * N), K.SENT, F)
    O.lib().orc_symetrize(img.reshape(-1), want, W, H, Cc, N)
    got = M.symetrize(img, N)
    assert got.shape == (Cc, H + 2 * N, W + 2 * N)
    assert np.array_equal(bits(got), bits(want))
    sym = rng.uniform(-300, 600, (Cc, H + 2 * N, W + 2 * N)).astype(F)
    back = np.full(Cc * W * H, K.SENT, F)
    O.lib().orc_unsymetrize(back, sym.reshape(-1), W, H, Cc, N)
    assert np.array_equal(bits(M.crop(sym, W, H, N)), bits(back))


@pytest.mark.parametrize("W,H,Cc,N,k,A", [(64, 32, 3, 16, 8, 2), (9, 70, 3, 9, 8, 3), (71, 40, 1, 7, 8, 2), (65, 33, 3, 1, 2, 2), (9, 70, 1, 2, 9, 4)])
def test_coverage_count_equals_the_oracles_percentage(W, H, Cc, N, k, A):
    """orc_denoised_percent = count * 100 / n_mask / (H-k+1) / (W-k+1) in float32: with n_mask (H-k+1) (W-k+1) <= 2^16 the counts
    are exact in float32 and neighbouring counts give percentages more than a thousand float32 steps apart, so rounding the
    percentage back is unambiguous."""
    rng = np.random.default_rng(W + H + k)
    sw, sh = W - k + 1, H - k + 1
    mask = np.ones(A, np.uint32)
    mask[-1] = 0
    n_mask = int(mask.sum())
    assert n_mask * sw * sh <= 1 << 16
    den = np.stack([K.den_values(rng, Cc * (W + 2 * N) * (H + 2 * N)) for _ in range(A)])
    pct = O.lib().orc_denoised_percent(den.reshape(-1), mask, A, W, H, Cc, N, k)
    implied = float(pct) * n_mask * sh * sw / 100.0
    assert abs(implied - round(implied)) < 1e-2
    got = sum(M.coverage(M.crop(den[st].reshape(Cc, H + 2 * N, W + 2 * N), W, H, N), k) for st in range(A) if mask[st])
    assert got == round(implied) and 0 < got < Cc * n_mask * sw * sh


def test_count_rules_on_the_special_values():
    """-0, negatives and NaN are not covered, the smallest denormal is; +0 and -0 are zeros, the denormal is not"""
    den = K.DEN_SPECIALS.reshape(1, 1, -1)
    assert M.coverage(den, 1) == 2            # the denormal and inf
    assert M.zeros(K.DEN_SPECIALS) == 2
    e = M.estimate(np.full(6, 6.0, F), K.DEN_SPECIALS, np.full(6, -1.0, F))
    assert e[0] == -1.0 and e[1] == -1.0 and np.isinf(e[2]) and e[3] == F(6.0) / F(-3.5) and e[4] == 0.0 and np.isnan(e[5])


@pytest.mark.parametrize("sigma", (1.0, 25.0, 50.5))
def test_sigma_table_equals_the_oracle(sigma):
    for Cc, spaces in ((3, (O.YUV, O.YCBCR, O.OPP, O.RGB)), (1, (O.OPP,))):
        for cs in spaces:
            want = np.zeros(3, F)
            assert O.lib().orc_sigma_table(sigma, Cc, cs, want) == 0
            got = core.sigma_table(sigma, Cc, cs)
            assert np.array_equal(bits(got), bits(want[:Cc])) and (got > 0).all()
    out = np.zeros(3, F)
    assert core.lib().lfbm5d_sigma_table(sigma, 3, 4, out.ctypes.data_as(C.POINTER(C.c_float))) != 0
    with pytest.raises(core.LfBm5dError):
        core.sigma_table(sigma, 3, 4)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_has_the_edges_it_is_named_for(case):
    assert case.edges, "a case states which edge it is there for"
    for tag in case.edges:
        assert K.EDGES[tag](case), (case.name, tag)
    for name, v in case.bufs.items():
        if v is not None:
            assert v.ndim == 1 and v.dtype in (F, np.uint32) and v.nbytes <= 5 << 20, name


def test_every_edge_occurs_in_some_case():
    used = {tag for c in CASES for tag in c.edges}
    assert used == set(K.EDGES), set(K.EDGES) - used
    # ... and where the issue asks for an edge of a particular op
    has = lambda op, *tags: any(c.op == op and set(tags) <= set(c.edges) for c in CASES)
    for op in ("window_begin", "window_end"):
        assert has(op, "direct-form") and has(op, "sums-form") and has(op, "C-1") and has(op, "C-3")
        for tag in ("slots-1", "slots-9", "slots-25", "slots-81", "empty-front", "empty-middle", "empty-end", "list-non-monotone", "list-highest-sai"):
            assert has(op, tag), (op, tag)
    for op in ("estimate_multi", "copy_rect", "count_denoised"):
        assert has(op, "slots-81", "mask-both-words"), op
    for tag in ("tile-exact", "ragged", "wide-and-low", "count-two-columns", "count-ends-on-a-block", "k-2", "k-equals-W"):
        assert has("window_end", tag), tag
    assert has("output", "in-place") and has("output", "no-pilot") and has("color_roundtrip", "in-place")
    assert has("finalize", "colour-off") and has("output", "colour-off")


@pytest.mark.parametrize("case", [c for c in CASES if c.op in ("window_begin", "window_end", "finalize", "output")], ids=lambda c: c.name)
def test_fused_ops_of_the_model_are_their_compositions(case):
    """window_begin / window_end / finalize / output of the model against the chain of plain ops on the same inputs -- the chains the
    GPU test runs through the seam as well"""
    want = K.expected(case)
    g, b = case.kw, {k: case.bufs[case.alias.get(k, k)] for k in list(case.bufs) + list(case.alias)}
    if case.op == "window_begin":
        pairs = [("noisy", "w_noisy"), ("basic", "w_basic"), ("num", "w_num"), ("den", "w_den")]
        pads = {}
        for src, dst in pairs:
            if b[src] is not None:
                pads[dst] = M.run("symetrize_multi", dict(noisy=b[src], w_noisy=K.sent(len(want["w_noisy"]))), lst=case.lst, **g)["w_noisy"]
                if dst in want:
                    assert M.same_bits(pads[dst], want[dst]).all()
        imgb, planeb = g["C"] * (g["W"] + 2 * g["N"]) * (g["H"] + 2 * g["N"]), (g["W"] + 2 * g["N"]) * (g["H"] + 2 * g["N"])
        for i, st in enumerate(case.lst):
            e = want["est"][i * planeb:(i + 1) * planeb]
            if st == K.EMPTY:
                assert np.all(e == K.SENT)
                continue
            ch0 = lambda name: pads[name][i * g["w_stride"]:i * g["w_stride"] + planeb]
            assert M.same_bits(e, M.estimate(ch0("w_num"), ch0("w_den"), ch0("w_basic" if "w_basic" in pads else "w_noisy"))).all()
        assert not want["counters"][:32].any() and np.array_equal(want["counters"][32:], b["counters"][32:])
    elif case.op == "window_end":
        src = "w_den" if b["w_den"] is not None else None
        if src:
            for name in ("num", "den"):
                back = M.run("unsymetrize_multi", dict(w_noisy=b["w_" + name], out=b[name]), lst=case.lst, **g)["out"]
                assert M.same_bits(back, want[name]).all()
            padded = b["w_den"]
            stride = g["w_stride"]
        else:
            assert set(want) == {"counters"}
            imgb = g["C"] * (g["W"] + 2 * g["N"]) * (g["H"] + 2 * g["N"])
            padded = M.run("symetrize_multi", dict(noisy=b["den"], w_noisy=K.sent(len(case.lst) * imgb)), lst=case.lst, **{**g, "w_stride": imgb})["w_noisy"]
            stride = imgb
        live = (case.lst != K.EMPTY).astype(np.uint32)
        cnt = M.run("count_denoised", dict(w_den=padded), slot_mask=live, **{**g, "w_stride": stride})["counters"]
        assert int(cnt[0]) == want["counters"] > 0
    else:
        n_sai = K._n_sai_of(case)
        dmask = np.zeros(n_sai, np.uint32)
        dmask[case.lst] = 1
        n = g["lf_stride"]
        whole = lambda v: np.concatenate([v, K.sent(n_sai * n - len(v))])   # (the last SAI's slack, so that [n_sai][n] holds)
        col = lambda v, fwd: M.run("color", dict(noisy=v, dmask=dmask), n_sai=n_sai, forward=fwd, **g)["noisy"] if g["colour"] else v
        e = M.run("estimate_lf", dict(num=whole(b["num"]), den=whole(b["den"]), sub=whole(b["sub"]), out=K.sent(n_sai * n), dmask=dmask), n=n, n_sai=n_sai)["out"]
        e = e[:len(b["num"])]
        image = (np.arange(len(e)) % n) < 3 * g["W"] * g["H"]   # (the chain also "estimates" the slack between the SAIs)
        same = lambda got, ref: (M.same_bits(got, ref) | ~image).all()
        if case.op == "finalize":
            assert same(col(col(e, 0), 1), want["basic"])
        else:
            assert same(col(e, 0), want["out"])
            noisy_name = case.alias.get("noisy_dst", "noisy_dst")
            assert same(np.where(want[noisy_name] == K.SENT, K.SENT, col(b["noisy"], 0)), want[noisy_name])   # (apart: only the listed SAIs arrive)
            if b["basic"] is not None:
                assert same(col(b["basic"], 0), want["basic"])
