"""CPU: what the wide-Trie search tests (tests/test_gpu_wide_trie.py) stand on -- the Tries, the oracle-side helpers, and a numpy
restatement of the chunked top-P selection of beam_step_chunked_kernel (gram_amd/csrc/beam.hip): carrying the best P keys from
chunk to chunk gives the prefix of the full sort, whatever the chunk capacity, because the keys are unique and totally ordered."""
import ctypes as C
import os

import numpy as np
import torch

from oracle import gram_oracle as O

ONE_SHOT_MAX = 16384  # K * max_fanout the one-shot search step holds on chip (include/gram_hip.h, gram_trie_t)
CHUNK_KEYS = 4096     # key array of the chunked step (beam.hip, kChunkKeys)


def wide_tries():
    """name -> (candidates, B, K, V, max_length, expected max_fanout): the shapes the one-shot search step refuses"""
    root900 = [[0, a, b, 1] for a in range(2, 902) for b in (2, 3)]
    second300 = [[0, a, b, 1] for a in range(2, 8) for b in range(2, 302)] + [[0, 9, 1], [0, 10, 5, 6, 1]]
    advice = [[0, a] + [3] * 47 + [1] for a in range(2, 257)]
    vocab_root = [[0, a, 1] for a in range(2, 4000)]
    return {
        "root900": (root900, 2, 20, 1024, 4, 900),
        "second300": (second300, 2, 64, 512, 5, 300),
        "advice": (advice, 1, 64, 512, 50, 255),
        "vocab_root": (vocab_root, 1, 8, 4096, 3, 3998),
    }


def golden_cands(name):
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "tries.npz"))
    return [[int(x) for x in r if x >= 0] for r in z[f"{name}_cands"]]


def one_shot_lds_bytes(K, fan, Tmax):
    """dynamic LDS of the one-shot kernel (launch_search_step): keys + step-0 logits + new_seq/new_anc"""
    nc = 64
    while nc < K * fan:
        nc <<= 1
    return nc * 8 + (fan * 4 + 15) // 16 * 16 + 2 * K * Tmax * 4


def is_wide(K, fan, Tmax):
    return K * fan > ONE_SHOT_MAX or one_shot_lds_bytes(K, fan, Tmax) > 152 * 1024


def make_logits(kind, steps, rows, V, seed):
    """per-step logits [rows][V]: 'randn', or 'int': integers -3..3, so that dozens of candidates tie at the 2K cut and across chunk
    boundaries (the oracle's tie rule, lower flat index first, decides)"""
    g = torch.Generator().manual_seed(seed)
    if kind == "randn":
        return [torch.randn(rows, V, generator=g) * 2.0 for _ in range(steps)]
    return [torch.randint(-3, 4, (rows, V), generator=g).float() for _ in range(steps)]


def oracle_search(cands, logits, B, K, max_length, lp=1.0):
    """O.beam_search on pre-computed per-step logits (no early exit: one logits tensor per step, as the device loop consumes them)"""
    it = iter(logits)
    return O.beam_search(lambda tok: next(it), lambda idx: None, B, K, max_length, O.prefix_allowed_tokens_fn(O.Trie(cands)), lp,
                         early_exit=False)


# ------------------------------------------------------------------------------------ the selection, restated
def f2ord(x):
    """beam.hip f2ord: float32 -> uint32 whose unsigned order is the floats' order"""
    u = np.asarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def make_keys(scores, flat):
    """beam.hip cand_key: orderable score in the high word, ~flat index in the low one (ties -> the lower flat index first)"""
    return (f2ord(scores).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - flat.astype(np.uint64))


def chunked_top_p(keys, P, cap):
    """The kernel's rounds: the carried block (best P so far, zero keys while fewer were seen) and the next <= cap keys are selected
    from together; returns the carried block at the end, descending."""
    carry = np.zeros(P, dtype=np.uint64)
    for c0 in range(0, len(keys), cap):
        both = np.concatenate([carry, keys[c0:c0 + cap]])
        carry = np.sort(both)[::-1][:P]
    return carry


def test_debug_switch_signatures():
    from gram_amd import _lib
    for name in ("gram_debug_set_beam_chunked", "gram_debug_set_beam_chunk_capacity"):
        assert _lib.SIGNATURES[name] == (C.c_int, [C.c_int]), name
    lib = _lib.load()
    try:
        assert lib.gram_debug_set_beam_chunked(2) == _lib.E_ARG and lib.gram_debug_set_beam_chunked(-2) == _lib.E_ARG
        assert lib.gram_debug_set_beam_chunk_capacity(-1) == _lib.E_ARG
        for mode in (1, 0, -1):
            assert lib.gram_debug_set_beam_chunked(mode) == 0
        assert lib.gram_debug_set_beam_chunk_capacity(7) == 0
    finally:
        lib.gram_debug_set_beam_chunked(-1)
        lib.gram_debug_set_beam_chunk_capacity(0)
    assert lib.gram_abi_version() == 7


def test_wide_tries_report_their_fanout():
    from gram_amd.utils import generation_trie as gt
    for name, (cands, B, K, V, max_length, fan) in wide_tries().items():
        flat = gt.FlatTrie(gt.Trie(cands))
        assert flat.max_fanout == fan, name
        assert max(len(c) for c in cands) == max_length and max(max(c) for c in cands) < V, name
        assert is_wide(K, fan, max_length), name
    # the ADVICE shape is the one whose key count fits and whose LDS sum does not
    assert 64 * 255 <= ONE_SHOT_MAX < 64 * 263 and one_shot_lds_bytes(64, 255, 50) > 152 * 1024
    yelp = gt.FlatTrie(gt.Trie(golden_cands("Yelp")))
    assert yelp.max_fanout == 263 and is_wide(64, 263, 12) and not is_wide(20, 263, 12)
    assert not is_wide(20, gt.FlatTrie(gt.Trie(golden_cands("Beauty"))).max_fanout, 10)


def test_oracle_helper_is_the_oracle_search():
    """oracle_search / make_logits against a direct O.beam_search call on a narrow Trie, both kinds of logits"""
    cands = [[0, a, b, 1] for a in range(2, 9) for b in range(10, 14)]
    B, K, V, T = 3, 4, 128, 4
    for kind in ("randn", "int"):
        logits = make_logits(kind, T - 1, B * K, V, 5)
        step = {"t": 0}

        def step_fn(tok):
            step["t"] += 1
            return logits[step["t"] - 1]

        want = O.beam_search(step_fn, lambda idx: None, B, K, T, O.prefix_allowed_tokens_fn(O.Trie(cands)), 1.0, early_exit=False)
        got = oracle_search(cands, logits, B, K, T)
        assert got[0].tolist() == want[0].tolist() and torch.equal(got[1], want[1])
        assert torch.isfinite(got[1]).all()
    ints = make_logits("int", 1, 8, 64, 1)[0]
    assert set(ints.unique().tolist()) <= set(range(-3, 4)) and len(ints.unique()) == 7


def test_chunked_top_p_is_the_sorted_prefix():
    """1 000 random key sets with tied scores: the chunked selection = the prefix of the full descending key sort = the oracle's
    topk_candidates order (stable descending sort of the scores: ties to the lower flat index), for capacities that put the count
    on, just under, just over a chunk boundary, on 2 x + 1, and for the kernel's own capacity."""
    rng = np.random.default_rng(0)
    for trial in range(1000):
        K = int(rng.integers(1, 65))
        P = 64
        while P < 2 * K:
            P <<= 1
        n = int(rng.integers(1, 6000))
        V = int(rng.integers(n // K + 2, n // K + 2000))
        flat = np.sort(rng.choice(K * V, size=n, replace=False)).astype(np.int64)  # candidates arrive in flat-index order
        scores = rng.integers(-3, 4, n).astype(np.float32) if trial % 2 else rng.standard_normal(n).astype(np.float32)
        scores[rng.random(n) < 0.02] = -np.inf  # (legitimate: HF's -inf refills)
        keys = make_keys(scores, flat)
        assert len(np.unique(keys)) == n and keys.min() > 0
        want = np.sort(keys)[::-1][:P]
        dense = torch.full((K * V,), float("-inf"))
        dense[torch.from_numpy(flat)] = torch.from_numpy(scores)
        top = min(n, 2 * K)
        _, idx = O.topk_candidates(dense, 2 * K)
        # (-inf candidates tie with the -inf of the tokens outside the Trie: compare up to the first of them)
        fin = int(np.isfinite(ord_scores(want[:top])).sum())
        assert (np.uint64(0xFFFFFFFF) - (want[:fin] & np.uint64(0xFFFFFFFF))).astype(np.int64).tolist() == idx[:fin].tolist()
        caps = {CHUNK_KEYS - P, n + 1, n, max(1, n - 1), max(1, (n - 1) // 2), int(rng.integers(1, n + 1))}
        for cap in caps:
            got = chunked_top_p(keys, P, cap)
            assert np.array_equal(got[:min(n, P)], want), (trial, cap)
            assert (got[min(n, P):] == 0).all()


def ord_scores(keys):
    """scores back from keys (beam.hip ord2f)"""
    o = (keys >> np.uint64(32)).astype(np.uint32)
    u = np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32)
    return u.view(np.float32)
