"""The jobs under spatially correlated noise (lfbm5d_*_corr_*, include/lfbm5d_corr.h).  Run with -m gpu on an MI355X.

  - with the white autocorrelation the job IS the plain job under option group_generic, bit for bit: light fields and counters, the
    two-step job and the single steps, the host form and the device form;
  - the tables do not outlive their call, a failing call included;
  - the point of the feature: on a light field with correlated noise (Gaussian taps of width 0.8, sigma 25, dct in both steps) the job
    with the true autocorrelation, and the job with the blind one, reach a higher mean PSNR than the plain job at the same sigma.
    Only the sign is asserted; tools/corr_time.py records the gains in profiles/corr.txt;
  - the command-line tool: the report line with LFBM5D_NOISE_CORR=auto, the files as they were without the variable.
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import corr_model as CM
import helpers as Hh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "lfbm5d_amd", "LFBM5Ddenoising")
ENV = ("LFBM5D_EMULATE_WORLD", "LFBM5D_DATA_DRIVEN_SCHEDULE", "LFBM5D_STEP_SHARDING", "LFBM5D_LANES", "LFBM5D_MAX_WINDOWS", "LFBM5D_FUSED",
       "LFBM5D_GROUP_GENERIC")
PK1 = (4, 6, 2, 8, 4, "id", "sadct", "haar")
PK2 = (8, 6, 2, 8, 4, "dct", "sadct", "haar")
PK1_DCT = (8, 6, 2, 8, 4, "dct", "sadct", "haar")


@pytest.fixture(scope="module")
def ctx():
    import lfbm5d_amd as L
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _plain_environment(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


@functools.lru_cache(maxsize=None)
def _lf():
    clean, noisy = Hh.noisy_lf(Hh.textured_lf(3, 3, 64, 64), 25.0)
    noisy.setflags(write=False)
    return noisy


def _params(sigma, pk1=PK1, pk2=PK2):
    from lfbm5d_amd import core
    return core.make_params(sigma, 2.7, *pk1), core.make_params(sigma, 2.7, *pk2)


def _job(ctx, noisy, acf, sigma=25.0, W=64, H=64, generic=False, pk1=PK1, pk2=PK2, an=(1, 1), aw=3, ah=3):
    """(noisy, basic, denoised, stats) of the two-step job: plain (acf None; generic: under option group_generic) or with acf."""
    import lfbm5d_amd as L
    P1, P2 = _params(sigma, pk1, pk2)
    d_n = torch.from_numpy(np.array(noisy)).cuda()
    d_b, d_d = torch.zeros_like(d_n), torch.zeros_like(d_n)
    mask = np.ones(aw * ah, np.uint32)
    ctx.reset_stats()
    if generic:
        ctx.set_option("group_generic", 1)
    try:
        if acf is None:
            ctx.denoise(P1, P2, d_n, mask, d_b, d_d, L.ROWMAJOR, aw, ah, an[0], an[1], W, H, 3)
        else:
            ctx.denoise_corr(acf, P1, P2, d_n, mask, d_b, d_d, L.ROWMAJOR, aw, ah, an[0], an[1], W, H, 3)
    finally:
        if generic:
            ctx.set_option("group_generic", None)
    s = ctx.stats()
    return d_n.cpu().numpy(), d_b.cpu().numpy(), d_d.cpu().numpy(), (s.passes, s.groups, s.stack_patches, s.sadct_groups)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_white_autocorrelation_is_the_general_kernels_job(ctx):
    """3 x 3 x 64 x 64 x 3, both steps: light fields and counters bit for bit; the single steps and the host form too."""
    import lfbm5d_amd as L
    noisy = _lf()
    ref = _job(ctx, noisy, None, generic=True)
    got = _job(ctx, noisy, L.CORR_WHITE)
    assert _same(got, ref)
    # the single steps
    P1, P2 = _params(25.0)
    mask = np.ones(9, np.uint32)
    d_n = torch.from_numpy(np.array(noisy)).cuda()
    d_b, d_d = torch.zeros_like(d_n), torch.zeros_like(d_n)
    ctx.step1_corr(L.CORR_WHITE, P1, d_n, mask, d_b, L.ROWMAJOR, 3, 3, 1, 64, 64, 3)
    ctx.step2_corr(L.CORR_WHITE, P2, d_n, mask, d_b, d_d, L.ROWMAJOR, 3, 3, 1, 64, 64, 3)
    e_n = torch.from_numpy(np.array(noisy)).cuda()
    e_b, e_d = torch.zeros_like(e_n), torch.zeros_like(e_n)
    ctx.set_option("group_generic", 1)
    try:
        ctx.step1(P1, e_n, mask, e_b, L.ROWMAJOR, 3, 3, 1, 64, 64, 3)
        ctx.step2(P2, e_n, mask, e_b, e_d, L.ROWMAJOR, 3, 3, 1, 64, 64, 3)
    finally:
        ctx.set_option("group_generic", None)
    assert torch.equal(d_b, e_b) and torch.equal(d_d, e_d)
    # the host form equals the device form, with a table that matters too
    acf = L.corr_from_kernel(CM.gaussian_taps(0.8))
    for a in (L.CORR_WHITE, acf):
        dev = _job(ctx, noisy, a)
        h_n = np.array(noisy)
        h_b, h_d = np.zeros_like(h_n), np.zeros_like(h_n)
        ctx.denoise_corr(a, P1, P2, h_n, mask, h_b, h_d, L.ROWMAJOR, 3, 3, 1, 1, 64, 64, 3)
        assert np.array_equal(h_b, dev[1]) and np.array_equal(h_d, dev[2])
    assert not np.array_equal(dev[2], ref[2])                     # the table changed the result


def test_several_windows_on_lanes(ctx, monkeypatch):
    """A 5 x 5 light field runs its windows on lanes (contexts of their own): they see the job's tables."""
    import lfbm5d_amd as L
    _, noisy = Hh.noisy_lf(Hh.textured_lf(5, 5, 48, 48), 25.0)
    monkeypatch.setenv("LFBM5D_LANES", "3")
    ref = _job(ctx, noisy, None, generic=True, W=48, H=48, aw=5, ah=5)
    assert _same(_job(ctx, noisy, L.CORR_WHITE, W=48, H=48, aw=5, ah=5), ref)
    acf = L.corr_from_kernel(CM.gaussian_taps(0.8))
    a = _job(ctx, noisy, acf, W=48, H=48, aw=5, ah=5)
    monkeypatch.setenv("LFBM5D_LANES", "1")
    assert _same(_job(ctx, noisy, acf, W=48, H=48, aw=5, ah=5), a) and not np.array_equal(a[2], ref[2])


def test_tables_do_not_outlive_their_call(ctx):
    import lfbm5d_amd as L
    noisy = _lf()
    acf = L.corr_from_kernel(CM.gaussian_taps(0.8))
    fresh = L.Context(0)
    try:
        ref = _job(fresh, noisy, None)
    finally:
        fresh.close()
    with_table = _job(ctx, noisy, acf)
    assert not np.array_equal(with_table[2], ref[2])
    assert _same(_job(ctx, noisy, None), ref)
    # a call that fails on its autocorrelation, and one that fails behind a good one (an angular window larger than the light field)
    bad = np.array(acf)
    bad[3, 3] = 0.5
    with pytest.raises(L.LfBm5dError, match="1 at lag 0"):
        _job(ctx, noisy, bad)
    assert _same(_job(ctx, noisy, None), ref)
    with pytest.raises(L.LfBm5dError):
        _job(ctx, noisy, acf, an=(3, 3))
    assert _same(_job(ctx, noisy, None), ref)
    assert _same(_job(ctx, noisy, acf), with_table)
    # one GPU for now
    c2 = L.Context(0)
    try:
        c2.set_shard(0, 2)
        with pytest.raises(L.LfBm5dError, match="one GPU"):
            _job(c2, noisy, acf)
    finally:
        c2.close()


def _psnr(x, clean):
    x = np.clip(np.rint(x.astype(np.float64)), 0, 255)
    mse = ((x - clean.astype(np.float64)) ** 2).reshape(clean.shape[0], -1).mean(axis=1)
    return float(np.mean(10 * np.log10(255.0 ** 2 / mse)))


def test_the_table_beats_the_plain_job_on_correlated_noise(ctx):
    """synth.make_lf 3 x 3 x 96 x 96 x 3 with add_correlated_noise (Gaussian taps of width 0.8, sigma 25), dct in both steps: the mean
    PSNR over the SAIs with the true autocorrelation, and with the blind one measured on the noisy light field, is higher than the
    plain job's at the same sigma.  The sign only; nobody had measured these before this test (profiles/corr.txt has the figures)."""
    import lfbm5d_amd as L
    from lfbm5d_amd import synth
    taps = CM.gaussian_taps(0.8)
    clean = synth.make_lf(3, 3, 96, 96).astype(np.float32)
    noisy = synth.add_correlated_noise(clean, 25.0, taps, seed=1).reshape(9, -1)
    cl = clean.reshape(9, -1)
    kw = dict(W=96, H=96, pk1=PK1_DCT, pk2=PK2)
    plain = _psnr(_job(ctx, noisy, None, **kw)[2], cl)
    true = _psnr(_job(ctx, noisy, L.corr_from_kernel(taps), **kw)[2], cl)
    est = ctx.corr_measure(torch.from_numpy(noisy).cuda(), np.ones(9, np.uint32), 96, 96, 3)
    blind = _psnr(_job(ctx, noisy, est.acf, **kw)[2], cl)
    print("mean PSNR: noisy %.2f dB, plain job %.2f dB, true autocorrelation %.2f dB (%+.2f), blind %.2f dB (%+.2f); blind lag-1 %.3f %.3f (true %.3f), sigma %.2f"
          % (_psnr(noisy, cl), plain, true, true - plain, blind, blind - plain, est.acf[3, 4], est.acf[4, 3], L.corr_from_kernel(taps)[3, 4], est.sigma))
    assert true > plain
    assert blind > plain


def _write_scene(tmp):
    from PIL import Image
    from lfbm5d_amd import synth
    lf = synth.make_lf(3, 3, 64, 64)
    src = os.path.join(tmp, "sourceLF")
    os.makedirs(src)
    for s in range(3):
        for t in range(3):
            Image.fromarray(np.ascontiguousarray(lf[s * 3 + t].transpose(1, 2, 0))).save(f"{src}/SAI_{s + 1:02d}_{t + 1:02d}.png")
    for d in ("noisy", "basic", "denoised", "diff"):
        os.makedirs(os.path.join(tmp, d))
    return src


def _cli(tmp_path, name, **env):
    tmp = str(tmp_path / name)
    os.makedirs(tmp)
    src = _write_scene(tmp)
    args = [CLI, src, "SAI", "_", "3", "3", "1", "1", "1", "1", "row", "25", "2.7", f"{tmp}/noisy", f"{tmp}/basic", f"{tmp}/denoised", f"{tmp}/diff",
            "8", "6", "2", "8", "4", "dct", "sadct", "haar", "0", "8", "6", "2", "8", "4", "dct", "sadct", "haar", "0", "opp", "0", f"{tmp}/measures.txt"]
    e = {k: v for k, v in os.environ.items() if not k.startswith("LFBM5D_")}
    e.update(LFBM5D_SEED="1", **env)
    r = subprocess.run(args, capture_output=True, text=True, env=e)
    assert r.returncode == 0, r.stdout[-2000:]
    files = {k: open(f"{tmp}/{k}/SAI_02_02.png", "rb").read() for k in ("noisy", "basic", "denoised")}
    return r.stdout, files


def test_cli_reports_and_writes(tmp_path):
    taps = tmp_path / "taps.txt"
    taps.write_text("\n".join(" ".join("%.17g" % x for x in row) for row in CM.gaussian_taps(0.8)))
    plain, files = _cli(tmp_path, "plain", LFBM5D_ONE_JOB="1")
    again, files2 = _cli(tmp_path, "again", LFBM5D_ONE_JOB="1")
    assert "Noise correlation" not in plain and "Noise correlation" not in again and files == files2     # unset: no line, the same files run after run
    text, corr_files = _cli(tmp_path, "auto", LFBM5D_NOISE_CORR="auto", LFBM5D_NOISE_CORR_ADD=str(taps))
    line = [l for l in text.split("\n") if l.startswith("Noise correlation: ")]
    m = re.fullmatch(r"Noise correlation: lag-1 ([0-9.e+-]+) ([0-9.e+-]+), variance factors ([0-9.e+-]+)\.\.([0-9.e+-]+) \(step 1\), "
                     r"([0-9.e+-]+)\.\.([0-9.e+-]+) \(step 2\), (\d+) clamped; from estimate", line[0] if len(line) == 1 else "")
    assert m, line
    print(line[0])
    assert 0.3 < float(m.group(1)) < 0.9 and 0.3 < float(m.group(2)) < 0.9 and float(m.group(3)) < 0.5 and float(m.group(4)) > 2
    assert corr_files["noisy"] != files["noisy"] and corr_files["denoised"] != files["denoised"]
    text, _ = _cli(tmp_path, "kernel", LFBM5D_NOISE_CORR="kernel:" + str(taps), LFBM5D_NOISE_CORR_ADD=str(taps))
    assert re.search(r"Noise correlation: lag-1 0\.67\d* 0\.67\d*, variance factors 0\.015625\.\.6\.38\d* \(step 1\), 0\.015625\.\.6\.38\d* \(step 2\), 12 clamped; from kernel", text), \
        [l for l in text.split("\n") if l.startswith("Noise corr")]
