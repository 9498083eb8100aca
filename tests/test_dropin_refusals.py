"""What the drop-in (run_bm5d.h, run_bm3d_lf.h) returns and prints when it is handed bad arguments: tests/dropin_refusals.cpp, a
stand-alone program over liblfbm5d_dropin.so, makes three calls per function -- (a) a mask one entry short, (b) one non-empty SAI one
float short, (c) chnls = 2 -- and its lines are compared with tests/golden/dropin_refusals.json, which was recorded from the drop-in as
it stood BEFORE its functions were given one shared frame.  The (a) cases are refused before a context exists and run without a GPU;
the (b) and (c) cases run the program once as a child process on the GPU (a few calls get as far as a kernel on 2 x 2 SAIs of 16 x 16).
Lines that the library itself writes to stdout between the program's are not part of the comparison."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "lfbm5d_amd")
with open(os.path.join(ROOT, "tests", "golden", "dropin_refusals.json")) as _f:
    GOLDEN = json.load(_f)


def _cases(tmp_path, which):
    exe = str(tmp_path / "dropin_refusals")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "dropin_refusals.cpp"), "-L" + LIBDIR,
                        "-llfbm5d_dropin", "-llfbm5d_hip", "-Wl,-rpath," + LIBDIR], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe, which], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    got = {}
    for line in r.stdout.splitlines():
        if line.startswith('{"id": '):
            rec = json.loads(line)
            got[rec["id"]] = {"rc": rec["rc"], "out": rec["out"]}
    return got


def _compare(got, letters):
    want = {k: v for k, v in GOLDEN.items() if k[-1] in letters}
    assert len(want) == 30 * len(letters)
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


def test_a_short_mask_is_refused_before_a_context(tmp_path):
    _compare(_cases(tmp_path, "a"), "a")


@pytest.mark.gpu
def test_a_short_sai_and_two_channels_are_refused(tmp_path):
    _compare(_cases(tmp_path, "bc"), "bc")
