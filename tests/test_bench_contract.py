"""bench.py's one-line contract (plain and --full), its output dump, and __graft_entry__.smoke() on the GPU box (small workload:
configs[0]'s light field shape)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_names_every_baseline_configuration():
    """The workloads bench.py can time cover BASELINE.json's configurations; the default is the headline one."""
    sys.path.insert(0, ROOT)
    import bench
    names = set(bench.WORKLOADS)
    for w in ("lf3x3x256x256_sigma25", "lf3x3x256x256_sigma25_dct", "lf9x9x512x512_sigma25", "lf17x17x512x512_sigma25",
              "lf17x17x512x512_sigma10_bior", "lf15x15x625x434_sigma50_n1"):
        assert w in names
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert 'default="lf17x17x512x512_sigma25"' in src


@pytest.mark.gpu
def test_bench_line_has_the_contract_fields():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--workload", "lf3x3x256x256_sigma25", "--full"], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1                                   # ONE JSON line
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "SAI-megapixels/s" and d["dtype"] == "f32" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert d["config"]["workload"] == "lf3x3x256x256_sigma25" and "model" not in d["config"]
    # value = the units of the timed steps over the timed interval
    mp = 3 * 3 * 256 * 256 / 1e6
    assert abs(d["value"] - mp / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "per_step"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    # round 6: the distance to this design's own floor next to the (saturated) contract fraction, and the per-step fractions up front
    for k in ("frac_ht", "frac_wiener", "design_bytes", "floor_ms", "x_over_floor", "x_over_floor_by_class"):
        assert k in r, k
    assert r["design_bytes"] > 0 and r["floor_ms"] > 0 and abs(r["x_over_floor"] - r["avg_launch_ms"] / r["floor_ms"]) < 1e-6 * r["x_over_floor"]
    for step in ("ht", "wiener"):
        p = r["per_step"][step]
        assert p["launches"] >= 1 and p["avg_launch_ms"] > 0
        assert p["frac"] <= 1.0 or "flag" in p               # a fraction above 1 is never printed unflagged
        assert abs(p["design_bytes"] - sum(v["design_bytes"] for v in p["floor_by_class"].values())) < 1.0
        assert p["filt_bytes"] > 0 and p["x_over_floor"] > 0
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and d["value"] > c["value"]
    assert d["psnr"]["denoised"] > d["psnr"]["basic"] > d["psnr"]["noisy"]


def test_bench_has_the_full_and_dump_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout


def test_dump_outputs_writes_float32_whole_or_a_fixed_sample(tmp_path, monkeypatch):
    """Small arrays are written whole; larger ones as the same sorted, seeded sample on every call.  The three outputs of
    the headline workload stay within 64 MB."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    assert 3 * bench.DUMP_SAMPLE * 4 <= 64e6
    a = torch.arange(24, dtype=torch.float32).reshape(2, 12)
    bench.dump_outputs(str(tmp_path / "whole"), {"denoised": a})
    w = np.load(tmp_path / "whole" / "denoised.npy")
    assert w.dtype == np.float32 and np.array_equal(w, a.reshape(-1).numpy())
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    big = torch.arange(100000, dtype=torch.float32).reshape(10, -1) * 0.5
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), {"basic": big})
    s1, s2 = np.load(tmp_path / "s1" / "basic.npy"), np.load(tmp_path / "s2" / "basic.npy")
    assert s1.dtype == np.float32 and 90 <= s1.size <= 100 and np.array_equal(s1, s2)
    assert np.all(np.diff(s1) > 0) and np.all(np.isin(s1, big.reshape(-1).numpy()))


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """A plain run (no --full): the headline fields, none of the --full measurements, exactly --steps timed steps; two runs with
    --dump-outputs write the same outputs, and they are the denoiser's (denoised closer to the clean light field than noisy)."""
    import numpy as np
    sys.path.insert(0, ROOT)
    from lfbm5d_amd import synth
    lines = []
    for d in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                              "--workload", "lf3x3x256x256_sigma25", "--dump-outputs", str(tmp_path / d)],
                             capture_output=True, text=True, cwd=ROOT, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        js = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(js) == 1
        lines.append(json.loads(js[0]))
    d = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
        assert k in d, k
    for k in ("roofline", "kernel_ms_per_step", "psnr", "seam", "cpu_baseline"):
        assert k not in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "SAI-megapixels/s" and d["dtype"] == "f32"
    assert abs(d["value"] - 3 * 3 * 256 * 256 / 1e6 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    clean = synth.make_lf(3, 3, 256, 256).reshape(-1).astype(np.float32)
    res = {}
    for name in ("denoised", "basic", "noisy"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == clean.shape and np.array_equal(a, b), name
        res[name] = float(np.sqrt(((a - clean) ** 2).mean()))
    assert res["denoised"] < res["basic"] < res["noisy"]


@pytest.mark.gpu
def test_smoke_entry_point():
    out = subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.smoke(); print('smoke ok')"],
                         capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert out.returncode == 0 and "smoke ok" in out.stdout, out.stderr[-2000:]
