"""The launch train of gram_generate_bias on the CPU (tools/launch_trace; tests/test_launch_train.py compares the cases with their
goldens line for line).  Here: what the train IS -- the beam search's train outside the search calls, and gram_beam_init, one
gram_beam_step_bias_sparse per position and gram_beam_finalize in their place, carrying the potentials' pointer and stride.

generate_bias_p1 (one piece, live rows off, one shared row of potentials) stands against the generate_live_off golden;
generate_bias_p2_items (two pieces, live rows, item filters, a row per user) against generate_p2_items, the beam search's train at
ITS settings -- a two-piece train cannot equal the one-piece golden."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_train")
TOOL = os.path.join(ROOT, "gram_amd", "csrc", "build_trace", "launch_trace")
B, K, T, N_NODES = 2, 4, 4, 40  # (the cases' shapes and Trie: tools/launch_trace/driver.cpp)
SEARCH = ("gram_beam_init", "gram_beam_step", "gram_beam_finalize")


@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "launch_trace")], check=True, capture_output=True, text=True)
    return TOOL


def _trace(tool, case):
    return subprocess.run([tool, case], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()


def _golden(case):
    with open(os.path.join(GOLDEN, case + ".txt")) as f:
        return f.read().splitlines()


@pytest.mark.parametrize("case,plain", [("generate_bias_p1", "generate_live_off"), ("generate_bias_p2_items", "generate_p2_items")])
def test_outside_the_search_calls_it_is_the_beam_search_train(tool, case, plain):
    """every launch that is not a search call -- encoder, bank, decode steps, LSE, the live-row compaction -- equals generate's,
    and the search calls sit at the same places"""
    got, want = _trace(tool, case), _golden(plain)
    assert [ln for ln in got if not ln.startswith(SEARCH)] == [ln for ln in want if not ln.startswith(SEARCH)]
    assert [i for i, ln in enumerate(got) if ln.startswith(SEARCH)] == [i for i, ln in enumerate(want) if ln.startswith(SEARCH)]
    # init and finalize are the plain search's own calls, argument for argument
    assert [ln for ln in got if ln.startswith(("gram_beam_init", "gram_beam_finalize"))] == \
           [ln for ln in want if ln.startswith(("gram_beam_init", "gram_beam_finalize"))]


@pytest.mark.parametrize("case,pieces,stride,items,live", [("generate_bias_p1", 1, 0, False, False),
                                                           ("generate_bias_p2_items", 2, N_NODES, True, True)])
def test_search_calls(tool, case, pieces, stride, items, live):
    lines = _trace(tool, case)
    assert lines[-1] == "return 0"
    calls = [ln for ln in lines if ln.startswith(SEARCH)]
    assert [c.split()[0] for c in calls] == ["gram_beam_init"] + ["gram_beam_step_bias_sparse"] * (T - 1) + ["gram_beam_finalize"]
    assert not any(ln.startswith(("gram_tail", "gram_beam_step_groups")) for ln in lines)  # no tail pass
    phis = set()
    for t, c in enumerate(calls[1:-1]):
        body = c.split("} ", 2)[2]  # behind the state and the Trie
        a = body.split("{")[0].split()
        hidden, lm16, lm32, d, lse, V, cur_len, rpu, rowpos, pc, phi, phi_stride = a[:12]
        assert (int(cur_len), int(rpu), int(pc), int(d), int(V)) == (t + 1, 1 if t == 0 else K, pieces, 128, 256)
        assert hidden.startswith("ws+") and lse.startswith("ws+") and lm16 != "0" and lm32 != "0"
        assert (rowpos != "0") == (live and t >= 1)
        assert phi.startswith("0x") and int(phi_stride) == stride  # the caller's tensor, not the workspace
        phis.add(phi)
        if items:
            assert "{" in body and body.split("{")[1].split("}")[0].split()[4:] == ["64", "0"]  # the filter's stride and mode
        else:
            assert "{" not in body and a[12] == "0"
    assert len(phis) == 1
