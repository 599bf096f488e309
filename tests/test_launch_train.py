"""The launch train of generate.hip, call for call, on the CPU.  tools/launch_trace links the product's own generate.o against
recording stand-ins for every kernel launcher and HIP call it uses; each case (one entry point of the C ABI on a tiny model, one
mode: pieces, folded or unfolded norm, row count, live rows, compaction, stage caps) prints one line per call with every argument,
workspace pointers as offsets.  The traces must equal tests/golden/launch_train/<case>.txt line for line: host-side restructuring of
generate.hip cannot change what the GPU is asked to do, or how the workspace is carved, without failing here.

The goldens were recorded from commit bfc453e (the last one before each sublayer's launch sequence was written once).  When a change
alters the launch train on purpose, regenerate them and review the diff like code:

    make -C tools/launch_trace && T=gram_amd/csrc/build_trace/launch_trace
    for c in $($T --list); do $T $c > tests/golden/launch_train/$c.txt; done"""
import difflib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_train")
TOOL = os.path.join(ROOT, "gram_amd", "csrc", "build_trace", "launch_trace")
CASES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".txt"))


@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "launch_trace")], check=True, capture_output=True, text=True)
    return TOOL


def test_every_case_has_a_golden(tool):
    assert sorted(subprocess.run([tool, "--list"], check=True, capture_output=True, text=True).stdout.split()) == CASES


@pytest.mark.parametrize("case", CASES)
def test_launch_train_equals_golden(tool, case):
    got = subprocess.run([tool, case], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    with open(os.path.join(GOLDEN, case + ".txt")) as f:
        want = f.read().splitlines()
    assert got[-1] == "return 0"
    diff = "\n".join(difflib.unified_diff(want, got, "golden/" + case, "this tree", lineterm="", n=1))
    assert got == want, "the launch train changed:\n" + diff
