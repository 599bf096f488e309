"""The launch train of gram_generate_sbs / gram_generate_sbs_items on the CPU (tools/launch_trace; tests/test_launch_train.py compares
the two cases with their goldens line for line).  Here: what the train IS -- the beam search's train outside the search calls, the
stochastic beam search's init, one step per position (step 0 on one decoder row per user) and finalize in their place, and the three
per-row arrays carved behind gram_workspace_bytes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_train")
TOOL = os.path.join(ROOT, "gram_amd", "csrc", "build_trace", "launch_trace")
B, K, T = 2, 4, 4  # (the cases' shapes: tools/launch_trace/driver.cpp)


@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "launch_trace")], check=True, capture_output=True, text=True)
    return TOOL


def _trace(tool, case):
    return subprocess.run([tool, case], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()


def _golden(case):
    with open(os.path.join(GOLDEN, case + ".txt")) as f:
        return f.read().splitlines()


def test_outside_the_search_calls_it_is_the_beam_search_train(tool):
    """one piece, live rows off: every launch that is not a search call -- encoder, bank, decode steps, LSE -- equals generate's"""
    got = [ln for ln in _trace(tool, "generate_sbs_p1_items") if not ln.startswith(("gram_sbs", "gram_workspace_bytes_sbs"))]
    want = [ln for ln in _golden("generate_live_off") if not ln.startswith(("gram_beam_init", "gram_beam_step", "gram_beam_finalize"))]
    assert got == want


@pytest.mark.parametrize("case,step,pieces", [("generate_sbs_p2", "gram_sbs_step", 2), ("generate_sbs_p1_items", "gram_sbs_step_items", 1)])
def test_search_calls(tool, case, step, pieces):
    lines = _trace(tool, case)
    assert lines[-1] == "return 0"
    size = {ln.split()[0]: int(ln.split()[1]) for ln in lines if ln.startswith("gram_workspace_bytes")}
    assert size["gram_workspace_bytes_sbs"] > size["gram_workspace_bytes"]
    calls = [ln for ln in lines if ln.startswith("gram_sbs")]
    assert [c.split()[0] for c in calls] == ["gram_sbs_init"] + [step] * (T - 1) + ["gram_sbs_finalize"]
    assert lines.index(calls[0]) < min(i for i, ln in enumerate(lines) if ln.startswith("gram_dec_self_attn"))
    assert lines.index(calls[-1]) == max(i for i, ln in enumerate(lines) if ln.startswith("gram_"))

    def tail(line):  # the arguments behind the two structs
        return line.rsplit("}", 1)[1].split()
    arrays = None
    for t, c in enumerate(calls[1:-1]):
        a = tail(c) if step == "gram_sbs_step" else c.rsplit("{", 1)[0].rsplit("}", 1)[1].split()
        hidden, lm16, lm32, d, lse, V, cur_len, rpu, pc, tau, seed, phi, model, path = a[:14]
        assert (int(cur_len), int(rpu), int(pc), int(d), int(V)) == (t + 1, 1 if t == 0 else K, pieces, 128, 256)
        assert float(tau) == 0.5 and int(seed) == 0x0123456789abcdef and (lm16 == "0") == (pieces == 2)
        assert arrays in (None, (phi, model, path))
        arrays = (phi, model, path)
    offs = sorted(int(x[3:]) for x in arrays)
    assert all(x.startswith("ws+") for x in arrays) and size["gram_workspace_bytes"] <= offs[0]
    assert offs[2] + 8 * B * K <= size["gram_workspace_bytes_sbs"] and offs[1] - offs[0] >= 4 * B * K and offs[2] - offs[1] >= 4 * B * K
    init = tail(calls[0])
    assert init[0] == "0" and int(init[1]) == 0x0123456789abcdef and tuple(init[3:6]) == arrays
