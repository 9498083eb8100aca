"""The curves and the per-value look-up of the clipped Poisson-Gaussian stage (lfbm5d_amd/csrc/lfbm5d_pgclip_values.h), compiled for the
host by tools/pgclip_host_check.cpp: on the five models of test_pgclip.py the closed-form moments and G agree with a brute-force
quadrature, the look-up the kernel runs never decreases along a ramp of step 1/64, the inverse stays inside the range and returns y from
G(y) within 1e-3."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_curves_agree_with_a_brute_force_quadrature_and_the_lookup_keeps_the_order(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "pgclip_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "tools", "pgclip_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    assert len(re.findall(r"^case ", r.stdout, re.M)) == 5
    m = re.search(r"worst: moments (\S+), G (\S+), forward table (\S+), inverse of G (\S+), bad (\d+)", r.stdout)
    assert m and float(m.group(1)) <= 1e-6 and float(m.group(2)) <= 1e-3 and float(m.group(3)) <= 2e-3 and float(m.group(4)) <= 1e-3
    assert int(m.group(5)) == 0
