"""The code the declipping kernel runs per value (declip_value, lfbm5d_amd/csrc/lfbm5d_clip_values.h), compiled for the host by
tools/clip_host_check.cpp: over sigmas from 1/100 grey level to 40 times the range the fixed number of Newton steps reaches the root
(|E(y) - d| <= 1e-9) and the float results never decrease along a ramp of step 1/64."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_newton_steps_reach_the_root_and_keep_the_order(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "clip_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "tools", "clip_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    assert len(re.findall(r"^range ", r.stdout, re.M)) == 20
    m = re.search(r"worst: \|E\(y\) - d\| = (\S+), \|y - bisection\| = (\S+), decreases (\d+)", r.stdout)
    assert m and float(m.group(1)) <= 1e-9 and float(m.group(2)) <= 1e-9 and int(m.group(3)) == 0
