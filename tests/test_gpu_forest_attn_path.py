"""-m gpu: whole generate() calls through the tail pass with the forest self-attention (gram_debug_set_tail_forest_attn(1): one
gram_dec_self_attn_forest_split per layer) against the same calls with the level-by-level train of the step-wise kernel (0), in the
style of tests/test_gpu_tail_pass.py: sequences, scores and every array of the beam state behind every replayed step, raw bits.
The pass itself is forced on (these calls are small) and so is the switch either way: by default a forest this small keeps the
train, which the launch-train goldens pin; tests/test_gpu_tail_pass.py's calls of 2049 users take the forest kernel by size."""
import ctypes as C

import pytest
import torch

from tests.test_gpu_tail_pass import STATE, _inputs, _model, _run
from tests.test_tail_pass_host import BRANCHY, CHAIN, RAGGED, WIDE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    return gpu_util


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for name in ("GRAM_TAIL_PASS", "GRAM_TAIL_FOREST_ATTN", "GRAM_TOKEN_TABLES"):
        monkeypatch.delenv(name, raising=False)
    yield
    from gram_amd import _lib
    lib = _lib.load()
    lib.gram_debug_set_tail_pass(-1)
    lib.gram_debug_set_tail_forest_attn(-1)
    lib.gram_debug_set_token_tables(-1)
    lib.gram_debug_set_live_rows(-1)


def _self_attn_launches(G, fn):
    """(what fn() returns, its launches of the decoder self-attention kind)"""
    from gram_amd import _lib
    lib = G.lib()
    _lib.check(lib.gram_prof_enable(1 << _lib.K_DEC_SELF_ATTN, 4096), "prof")
    try:
        out = fn()
        ms, n, work, dropped = C.c_double(0), C.c_int64(0), C.c_double(0), C.c_int64(0)
        _lib.check(lib.gram_prof_collect(_lib.K_DEC_SELF_ATTN, C.byref(ms), C.byref(n), C.byref(work), C.byref(dropped)), "collect")
        assert dropped.value == 0
    finally:
        lib.gram_prof_enable(0, 0)
    return out, n.value


def _compare(G, m, ids, mask, cands, K, tables=-1, cuts=None):
    """forest kernel against level train at every max_length behind a replayed step, the ones that end inside the tail included"""
    from gram_amd.utils.generation_trie import FlatTrie, Trie
    lib = G.lib()
    d_tail, full = FlatTrie(Trie(cands)).tail_tables()[1], max(len(c) for c in cands)
    lib.gram_debug_set_tail_pass(1)
    lib.gram_debug_set_token_tables(tables)
    for T in cuts or range(max(d_tail, 2) + 1, full + 1):
        lib.gram_debug_set_tail_forest_attn(1)
        (seq_on, sc_on, st_on, last_on), n_on = _self_attn_launches(G, lambda: _run(G, m, ids, mask, cands, K, T))
        lib.gram_debug_set_tail_forest_attn(0)
        (seq_off, sc_off, st_off, last_off), n_off = _self_attn_launches(G, lambda: _run(G, m, ids, mask, cands, K, T))
        assert last_on[0] == 1 and last_on == last_off and last_on[1] >= 1, T  # (both took the pass, over the same forest)
        # the decode steps in front of the pass launch one self-attention per layer each; then one per layer for the whole forest,
        # where the train has one per layer, user group and level (as many for one group and a max_length that leaves one level)
        assert n_on == d_tail * m._n_dec and n_off >= n_on, (T, n_on, n_off)
        fewer = n_off > n_on
        assert torch.equal(seq_on, seq_off), T
        assert torch.equal(sc_on.view(torch.int32), sc_off.view(torch.int32)), T
        for name in STATE:
            assert torch.equal(st_on[name], st_off[name]), (name, T)
        assert int(st_on["error"].view(torch.int32)[0]) == 0
    assert fewer  # (the longest call holds more than one level)
    return last_on


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("tables", [1, 0], ids=["tables", "no-tables"])
@pytest.mark.parametrize("B,K,cands,pad", [(1, 4, CHAIN, False), (3, 20, RAGGED, True), (17, 4, BRANCHY, False), (3, 20, BRANCHY, True)],
                         ids=["B1-K4-chain", "B3-K20-ragged-padded-passage", "B17-K4-branchy", "B3-K20-branchy-padded-passage"])
def test_generate_is_bit_identical_with_the_forest_kernel_and_with_the_level_train(G, B, K, cands, pad, tables, pieces):
    """Chains, ids of l and l + 1 tokens, and the Trie with forks below d_tail; with layer 0's q|k|v from the token table and from
    the GEMM; every max_length from right behind the pass's first replayed step -- which ends inside the tail, so the deeper rows
    get no attention at all -- to the whole candidate."""
    m = _model(G, pieces)
    ids, mask = _inputs(B, 2, 64, pad, 100 * B + K)
    _compare(G, m, ids, mask, cands, K, tables=tables)


@pytest.mark.parametrize("pieces", [2, 1])
def test_a_forest_of_two_entries_per_user_and_four_levels(G, pieces):
    """WIDE: 80 to 120 rows per user, four steps below d_tail with forks at two of them"""
    m = _model(G, pieces)
    ids, mask = _inputs(3, 2, 64, False, 960)
    last = _compare(G, m, ids, mask, WIDE, 20)
    assert 65 <= last[3] <= 128


def test_the_size_rule_and_the_environment_variable(G, monkeypatch):
    """-1: GRAM_TAIL_FOREST_ATTN decides where it is set (0 / 1), the forest's size where it is not -- a forest of a few dozen rows
    keeps the level train"""
    m, lib = _model(G, 2), G.lib()
    ids, mask = _inputs(3, 2, 64, False, 5)
    from gram_amd.utils.generation_trie import FlatTrie, Trie
    full, nd, d_tail = max(len(c) for c in CHAIN), m._n_dec, FlatTrie(Trie(CHAIN)).tail_tables()[1]
    lib.gram_debug_set_tail_pass(1)
    counts = {}
    for env in (None, "1", "0"):
        if env is None:
            monkeypatch.delenv("GRAM_TAIL_FOREST_ATTN", raising=False)
        else:
            monkeypatch.setenv("GRAM_TAIL_FOREST_ATTN", env)
        (_seq, _sc, _st, last), counts[env] = _self_attn_launches(G, lambda: _run(G, m, ids, mask, CHAIN, 4, full))
        assert last[0] == 1 and 1 <= last[1] < 16384
    assert counts["1"] == d_tail * nd and counts[None] == counts["0"] > counts["1"]
