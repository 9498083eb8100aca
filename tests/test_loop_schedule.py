"""The sigma sequence of the refinement loop the super-resolution, the inpainting and the view synthesis share (loop_sigma,
lfbm5d_amd/csrc/lfbm5d_side_values.h), without a GPU: the function is compiled into a stand-alone host program
(tools/loop_schedule_check.cpp) and compared, bit for bit, with the same expression in numpy float64 cast to float32:
sigma_k = max(s0 (s1 / s0)^((k-1)/(K-1)), sigma_noise), K = 1: s0."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S0, S1 = 30.0, 5.0


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    out = str(tmp_path_factory.mktemp("loop_schedule") / "loop_schedule_check")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "tools", "loop_schedule_check.cpp"), "-o", out], check=True)
    return out


def _bits(x):
    return f"{int(np.float32(x).view(np.uint32)):08x}"


def _expected(K, s0, s1, sn):
    s0, s1, sn = (np.float64(np.float32(v)) for v in (s0, s1, sn))
    out = []
    for k in range(1, K + 1):
        tau = s0 if K == 1 else s0 * np.power(s1 / s0, np.float64(k - 1) / np.float64(K - 1))
        out.append(np.float32(max(tau, sn)))
    return np.array(out, np.float32)


# sigma_noise: none, below both ends, between them, above both
@pytest.mark.parametrize("sigma_noise", [0.0, 2.0, 12.0, 40.0])
@pytest.mark.parametrize("K", [1, 2, 12])
def test_loop_sigma_equals_the_float64_expression(exe, K, sigma_noise):
    got = subprocess.run([exe, str(K), _bits(S0), _bits(S1), _bits(sigma_noise)], check=True, capture_output=True, text=True).stdout.split()
    want = _expected(K, S0, S1, sigma_noise)
    assert [int(w, 16) for w in got] == [int(v.view(np.uint32)) for v in want]
    assert want[0] == np.float32(max(S0, sigma_noise)) and (K == 1 or want[-1] == np.float32(max(S1, sigma_noise)))
    assert (np.diff(want) <= 0).all()
