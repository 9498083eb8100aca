"""Joint repair (lfbm5d_repair_*, include/lfbm5d_repair.h) without a GPU: exports, bindings and defaults; the tables; the numpy model's
two properties; what the mask is worth on the golden crops (the figures of profiles/repair_defaults.txt, written by
tools/repair_sweep.py); the loop in the CPU composition with the oracle's first step."""
import ctypes as C
import os

import numpy as np
import pytest

import lfbm5d_amd as L
from lfbm5d_amd import core
from oracle import oracle as O
import inpaint_model as IM
import repair_cases as K
import repair_model as M
import view_model as VM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HT = (8, 8, 3, 8, 3, "dct", "sadct", "haar")      # the parameters of the inpainting's and the view synthesis' loop tests
# profiles/repair_defaults.txt: the synthesised SAI of crop 96..159, mask-aware over today's sweep on the defective light field, in dB
MASK_GAIN_DB = {4: 8.3254, 1: 6.0659, 0: 4.6192}
# ... and the joint fill over the rim-inwards fill on the flagged values of both crops
FILL_GAIN_DB = {(96, 160): 2.3684, (64, 160): 3.7229}
# the loop: the joint job with K = 2 against inpaint(K = 2) followed by view_synth(K = 2), PSNR over all values of the crop 96..159 with
# SAI 4 missing, in dB; the joint job may be worse by at most the margin (profiles/repair_defaults.txt)
LOOP_JOINT_DB, LOOP_TWO_DB, LOOP_MARGIN_DB = 38.2488, 38.3607, 0.5


def test_library_exports_and_binds_the_repair_entry_points():
    lib = C.CDLL(core.library_path())
    for n in ("lfbm5d_repair_defaults", "lfbm5d_repair_fill_device", "lfbm5d_repair_device", "lfbm5d_repair_host_sai"):
        assert hasattr(lib, n), n
    assert C.sizeof(core.RepairParamsStruct) == 8 * 4
    assert C.sizeof(core.RepairResultStruct) == 4 * 4 + (2 + 4 * 3 + 1 + 17) * 8
    for n in ("repair", "repair_params", "Repair", "RepairParamsStruct", "RepairResultStruct"):
        assert n in L.__all__
    assert hasattr(L.Context, "repair_fill") and hasattr(L.Context, "repair")
    hdr = open(os.path.join(ROOT, "include", "lfbm5d.h")).read()
    assert '#include "lfbm5d_repair.h"' in hdr


def test_defaults_work_without_a_gpu_and_lie_in_the_allowed_ranges():
    P, V = L.repair_params(), L.view_params()
    assert (P.max_disparity, P.box_radius, P.ang_radius) == (4, 3, 1)
    assert (P.iterations, P.sigma_start, P.sigma_end, P.sigma_noise) == (V.iterations, V.sigma_start, V.sigma_end, V.sigma_noise)
    assert P.min_valid == 3                                                         # the sweep of profiles/repair_defaults.txt
    rec = open(os.path.join(ROOT, "profiles", "repair_defaults.txt")).read()
    assert f"-> min_valid = {P.min_valid}" in rec
    P = L.repair_params(max_disparity=2, box_radius=0, ang_radius=2, min_valid=5, iterations=0, sigma_start=12.0, sigma_end=3.0, sigma_noise=2.0)
    assert (P.max_disparity, P.box_radius, P.ang_radius, P.min_valid, P.iterations) == (2, 0, 2, 5, 0)
    assert (P.sigma_start, P.sigma_end, P.sigma_noise) == (12.0, 3.0, 2.0)


def test_the_tables_equal_their_formulas_bit_for_bit():
    f = M.f_table()
    for n in range(2, 25):
        for k in range(2, 25):
            assert f[n, k].view(np.uint32) == np.float32((n - 1) / (k - 1)).view(np.uint32)
        assert f[n, n] == np.float32(1.0)
    assert not f[:2].any() and not f[:, :2].any()
    for r in range(8):
        g = M.g_table(r)
        box = (2 * r + 1) ** 2
        assert len(g) == box + 1 and g[0] == 0 and g[box] == np.float32(1.0)
        for k in range(1, box + 1):
            assert g[k].view(np.uint32) == np.float32(box / k).view(np.uint32)
    assert np.array_equal(M.RECIP[1:], (1.0 / np.arange(1, 25)).astype(np.float32)) and M.RECIP[0] == 0


@pytest.mark.parametrize("name", K.CLEAN + ("clean-5x5-R1",))
@pytest.mark.parametrize("D, r", K.DRS)
def test_without_defects_the_model_is_the_view_synthesis(name, D, r):
    """Property 1: no flag, no value that is not finite, only missing SAIs as targets: every factor is 1.0f."""
    c = dict(K.case("clean-5x5"), ang_radius=1) if name == "clean-5x5-R1" else K.case(name)
    args = (c["ang_major"], c["aw"], c["ah"], c["W"], c["H"], c["C"], D, r, c["ang_radius"])
    got = M.fill(c["lf"], None, c["mask"], c["missing"], *args, min_valid=1)
    want = VM.fill(c["lf"], c["mask"], c["missing"], *args)
    assert want["synthesised"] == got["swept"] == got["targets"] == int(c["missing"].sum())
    assert np.array_equal(got["out"].view(np.uint32), want["out"].view(np.uint32))
    assert np.array_equal(got["disp"], want["disp"]) and np.array_equal(got["hist"], want["hist"])
    live = c["mask"] != 0
    assert np.array_equal(got["codes"][live] != 0, want["flags"][live] != 0) and (got["codes"][live] <= 1).all()
    assert int(got["rim"].sum()) == int(got["left"].sum()) == 0


def test_invalid_sources_never_leak_and_the_codes_partition_the_values():
    c, r = K.case("nan"), K.model("nan", 3, 3, 1)
    live = c["mask"] != 0
    assert np.isfinite(r["out"][live]).all()
    u = M.unsound_values(c["lf"], c["flags"], c["mask"], c["missing"], c["W"], c["H"], c["C"]).reshape(9, -1)
    assert np.array_equal(r["codes"] != 0, u)
    assert np.array_equal(r["out"][~u].view(np.uint32), c["lf"][~u].view(np.uint32))
    assert int(r["unsound"].sum()) == int(u.sum()) and r["positions"] == int(r["hist"].sum())
    # the cases the GPU tests name: a position where every source is invalid, a plane that nothing can fill
    assert int(K.model("no-source", 3, 3, 1)["rim"].sum()) > 0 and int(K.model("no-source", 0, 0, 1)["left"].sum()) == 0
    lost = K.model("lost-plane", 3, 3, 1)
    assert int(lost["left"].sum()) == 3 * 6 * 7 and int(lost["views"].sum()) == 0
    with pytest.raises(ValueError):
        M.loop(K.case("lost-plane")["lf"], K.case("lost-plane")["flags"], np.ones(3, np.uint32), np.array([1, 0, 1]), K.ROWMAJOR, 3, 1, 7, 6, 1,
               3, 3, 1, 30.0, 5.0, lambda z, s: z)


@pytest.mark.parametrize("m", [4, 1, 0])
def test_the_mask_gains_on_a_view_synthesised_from_defective_sources(m):
    """Golden crop 96..159, add_defects(seed=2) written as 0, D = 4, r = 3: the mask-aware sweep against today's (view_model.fill on the
    same data) and against today's on the clean light field.  The threshold is half of the gain recorded in
    profiles/repair_defaults.txt (centre 8.3254, edge 6.0659, corner 4.6192 dB)."""
    aware, unaware, ideal = K.mask_gain(m)
    print(f"SAI {m}: mask-aware {aware:.4f} dB, today's sweep {unaware:.4f} dB, clean sources {ideal:.4f} dB; gain {aware - unaware:.4f} dB")
    assert abs((aware - unaware) - MASK_GAIN_DB[m]) < 2e-3                         # the recorded value
    assert aware - unaware >= MASK_GAIN_DB[m] / 2
    rec = open(os.path.join(ROOT, "profiles", "repair_defaults.txt")).read()
    assert f"gain {MASK_GAIN_DB[m]:.4f}, threshold" in rec


@pytest.mark.parametrize("crop", K.CROPS)
def test_the_cross_view_fill_beats_the_rim_inwards_fill(crop):
    """Over the flagged values of both golden crops, all nine SAIs, at the default min_valid: the joint fill against inpaint_model.fill.
    The threshold is half of the gain recorded in profiles/repair_defaults.txt (2.3684 and 3.7229 dB)."""
    joint, rim = K.fill_gain(*crop, min_valid=L.repair_params().min_valid)
    print(f"crop {crop[0]}..{crop[1] - 1}: joint fill {joint:.4f} dB, rim-inwards fill {rim:.4f} dB, gain {joint - rim:.4f} dB")
    assert abs((joint - rim) - FILL_GAIN_DB[crop]) < 2e-3
    assert joint - rim >= FILL_GAIN_DB[crop] / 2


@pytest.fixture(scope="module")
def composition():
    """Crop 96..159, add_defects(seed=2) written as 0, SAI 4 missing, K = 2, sigma 30 -> 5: the joint job, and inpaint(K) followed by
    view_synth(K), both as model + the oracle's first step."""
    clean, fl, y, n = K.golden(96, 160)
    mask, miss = np.ones(9, np.uint32), np.zeros(9, np.uint32)
    miss[4] = 1

    def step(z, sig):
        _, basic, _ = O.run_step1(O.make_params(sig, 2.7, *HT), z.reshape(9, -1), mask, L.ROWMAJOR, 3, 3, 1, n, n, 3)
        return basic
    xj, x0, rj = M.loop(y, fl, mask, miss, K.ROWMAJOR, 3, 3, n, n, 3, 4, 3, 2, 30.0, 5.0, step)
    xi, _, _ = IM.loop(y, fl, mask, n, n, 3, 2, 30.0, 5.0, step)
    xv, _, _ = VM.loop(xi, mask, miss, K.ROWMAJOR, 3, 3, n, n, 3, 4, 3, 2, 30.0, 5.0, step)
    return clean, fl, y, miss, xj, x0, rj, xv


def test_the_joint_loop_is_not_worse_than_the_two_loops(composition):
    """Recorded: the PSNR over all values of the joint job (2 steps) and of the two loops one after the other (4 steps).  Asserted: the
    joint job is not worse by more than LOOP_MARGIN_DB, a margin of half a dB set ahead of the run (the two jobs differ in what the
    sweep sees -- the inpainting's result or the mask -- and in the number of steps the defects get)."""
    clean, fl, y, miss, xj, x0, rj, xv = composition
    joint, two = VM.psnr(xj, clean), VM.psnr(xv, clean)
    print(f"CPU composition: joint job, K = 2: {joint:.4f} dB (its fill {VM.psnr(x0, clean):.4f} dB); inpaint(2) then view(2): {two:.4f} dB")
    assert abs(joint - LOOP_JOINT_DB) < 2e-3 and abs(two - LOOP_TWO_DB) < 2e-3     # the recorded values
    assert joint >= two - LOOP_MARGIN_DB
    f = rj["codes"] != 0
    assert np.array_equal(xj[~f].view(np.uint32), y[~f].view(np.uint32))           # the sound values are back after every step
    assert np.isfinite(xj).all() and int(rj["left"].sum()) == 0 and f[4].all()
