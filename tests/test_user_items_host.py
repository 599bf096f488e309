"""CPU: the host side of the per-user item filters (include/gram_hip.h ``gram_user_items_t``): FlatTrie.leaf_ranges / item_ranks
against a brute-force walk, the argument errors of the new entry points (returned before any launch: no GPU needed), the layout
of the new struct against the header, the lists' validation in GRAM.generate and the op's fake implementation.  The launch train of
gram_generate_items is compared by tests/test_launch_train.py through its golden (generate_p2_items)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest
import torch

from gram_amd import _lib
from gram_amd.utils.generation_trie import FlatTrie, Trie

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _both(seqs):
    """The two FlatTrie constructors: straight from the sequences, and from the nested dict"""
    a = FlatTrie(Trie(seqs))
    t = Trie(seqs)
    assert t.trie_dict is not None and t.sequences() is None  # (handing the dict out makes FlatTrie walk it)
    return a, FlatTrie(t)


def _brute(flat):
    """(lo, hi) by a depth-first walk that takes children in token order, and the sequence of every leaf rank"""
    lo, hi = np.zeros(flat.n_nodes, dtype=np.int64), np.zeros(flat.n_nodes, dtype=np.int64)
    leaves = []

    def walk(node, prefix):
        lo[node] = len(leaves)
        a, b = int(flat.child_off[node]), int(flat.child_off[node + 1])
        if a == b and node != 0:
            leaves.append(tuple(prefix))
        for e in range(a, b):
            walk(int(flat.child_node[e]), prefix + [int(flat.child_tok[e])])
        hi[node] = len(leaves)

    walk(0, [])
    return lo, hi, leaves


def _random_seqs(rng, n, toks, depth):
    # an EOS (1) behind every sequence: no candidate is a proper prefix of another, so every candidate ends on a leaf
    return [[0] + [rng.randrange(2, 2 + toks) for _ in range(rng.randrange(1, depth + 1))] + [1] for _ in range(n)]


@pytest.mark.parametrize("n,toks,depth", [(1, 5, 3), (2, 2, 1), (7, 3, 2), (60, 6, 4), (300, 4, 5), (200, 90, 2)])
def test_leaf_ranges_and_item_ranks_against_a_walk(n, toks, depth):
    rng = random.Random(n * 100 + toks)
    seqs = _random_seqs(rng, n, toks, depth)
    if n >= 7:
        seqs += [list(seqs[0]), list(seqs[3]), list(seqs[0])]  # duplicate sequences share a leaf
    uniq = sorted(set(map(tuple, seqs)))
    for flat in _both(seqs):
        lo, hi = flat.leaf_ranges()
        assert lo.dtype == hi.dtype == np.int32 and lo.shape == hi.shape == (flat.n_nodes,)
        blo, bhi, leaves = _brute(flat)
        assert leaves == uniq  # the leaf rank IS the lexicographic rank of the sequence
        assert lo.tolist() == blo.tolist() and hi.tolist() == bhi.tolist()
        assert int(lo[0]) == 0 and int(hi[0]) == len(uniq)
        ranks = flat.item_ranks(seqs)
        assert ranks.dtype == np.int32 and ranks.tolist() == [uniq.index(tuple(q)) for q in seqs]
        # every leaf's own range is its rank alone
        for q, r in zip(seqs, ranks.tolist()):
            leaf = flat.leaf_of(q)
            assert (int(lo[leaf]), int(hi[leaf])) == (r, r + 1)
        assert flat.leaf_ranges()[0] is lo  # built once per Trie


def test_item_ranks_refuses_what_is_no_leaf():
    seqs = [[0, 2, 3, 1], [0, 2, 4, 1], [0, 5, 1]]
    for flat in _both(seqs):
        with pytest.raises(ValueError, match="does not end on a leaf"):
            flat.item_ranks([[0, 2, 3, 1], [0, 2]])  # an inner node
        with pytest.raises(ValueError, match="not in the Trie"):
            flat.item_ranks([[0, 2, 3, 1], [0, 7, 1]])
        with pytest.raises(ValueError, match="not in the Trie"):
            flat.item_ranks([[0, 5, 1, 1]])  # runs past a leaf
        assert flat.item_ranks([]).shape == (0,)
    # a candidate that is a proper prefix of another ends on an inner node of the Trie built from both
    for flat in _both([[0, 2], [0, 2, 3]]):
        with pytest.raises(ValueError, match="does not end on a leaf"):
            flat.item_ranks([[0, 2], [0, 2, 3]])


def test_argument_errors_without_gpu():
    """Null lists, a stride over the limit and a bad mode come back as GRAM_E_ARG before any launch"""
    lib = _lib.load()
    p = 0x1000  # (never dereferenced)
    good = dict(leaf_lo=p, leaf_hi=p, ranks=p, count=p, stride=64, mode=_lib.ITEMS_EXCLUDE)
    bad = [dict(good, **{k: None}) for k in ("leaf_lo", "leaf_hi", "ranks", "count")]
    bad += [dict(good, stride=0), dict(good, stride=_lib.GRAM_MAX_USER_ITEMS + 1), dict(good, mode=2), dict(good, mode=-1)]
    st = _lib.BeamState(B=2, K=4, Tmax=5, length_penalty=1.0, eos=1, pad=0, tokens=p, node=p, beam_scores=p, seq=p, anc=p, done=p,
                        n_hyps=p, hyp_score=p, worst=p, hyp_len=p, hyp_tok=p, error=p)
    st1 = _lib.BeamState(B=2, K=1, Tmax=5, length_penalty=1.0, eos=1, pad=0, tokens=p, node=p, beam_scores=p, seq=p, anc=p, done=p,
                         n_hyps=p, hyp_score=p, worst=p, hyp_len=p, hyp_tok=p, error=p)
    trie = _lib.Trie(p, p, p, 10, 9, 3, 2)
    width = C.c_int32(0)

    def calls(ui):
        u = C.byref(ui) if ui is not None else None
        return [
            lib.gram_generate_items(None, p, p, 2, 1, 32, 4, 4, 5, 1.0, C.byref(trie), None, u, p, 1 << 20, p, p, C.byref(width), None),
            lib.gram_beam_step_sparse_items(C.byref(st), C.byref(trie), p, p, 128, p, 256, 1, 4, None, u, None),
            lib.gram_beam_step_sparse_split_items(C.byref(st), C.byref(trie), p, p, 128, p, 256, 1, 4, None, 2, u, None),
            lib.gram_greedy_step_items(C.byref(st1), C.byref(trie), p, 256, 1, u, None),
        ]

    assert calls(None) == [_lib.E_ARG] * 4
    for kw in bad:
        assert calls(_lib.UserItems(**kw)) == [_lib.E_ARG] * 4, kw
    ok = _lib.UserItems(**good)
    # good lists, other arguments wrong: still refused before any launch
    assert lib.gram_generate_items(None, p, p, 2, 1, 32, 4, 4, 5, 1.0, C.byref(trie), None, C.byref(ok), p, 1 << 20, p, p, C.byref(width),
                                   None) == _lib.E_ARG  # (no model)
    assert lib.gram_beam_step_sparse_items(C.byref(st), C.byref(trie), p, p, 128, p, 256, 0, 4, None, C.byref(ok), None) == _lib.E_ARG
    assert lib.gram_beam_step_sparse_items(C.byref(st), C.byref(trie), p, p, 128, p, 256, 1, 1, p, C.byref(ok), None) == _lib.E_ARG  # live rows: K rows per user
    assert lib.gram_beam_step_sparse_split_items(C.byref(st), C.byref(trie), p, None, 128, p, 256, 1, 4, None, 2, C.byref(ok), None) == _lib.E_ARG
    assert lib.gram_greedy_step_items(C.byref(st), C.byref(trie), p, 256, 1, C.byref(ok), None) == _lib.E_ARG  # K != 1
    # the list preparation: null arrays, M outside 1 .. stride, stride over the limit
    prep = lib.gram_user_items_prepare
    assert prep(None, 10, p, 2, 8, p, p, 8, None) == _lib.E_ARG
    assert prep(p, 10, None, 2, 8, p, p, 8, None) == _lib.E_ARG
    assert prep(p, 10, p, 2, 8, None, p, 8, None) == _lib.E_ARG
    assert prep(p, 10, p, 2, 8, p, None, 8, None) == _lib.E_ARG
    assert prep(p, 0, p, 2, 8, p, p, 8, None) == _lib.E_ARG
    assert prep(p, 10, p, 0, 8, p, p, 8, None) == _lib.E_ARG
    assert prep(p, 10, p, 2, 0, p, p, 8, None) == _lib.E_ARG
    assert prep(p, 10, p, 2, 9, p, p, 8, None) == _lib.E_ARG
    assert prep(p, 10, p, 2, 8, p, p, _lib.GRAM_MAX_USER_ITEMS + 1, None) == _lib.E_ARG


def test_user_items_struct_matches_the_header(tmp_path):
    """gram_user_items_t against its ctypes mirror: total size and every field's offset from a C program compiled against the real
    header (gcc; no GPU), and the numbers themselves"""
    st, cname = _lib.UserItems, "gram_user_items_t"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gram_hip.h"', "int main(void) {",
             f'  printf("size %zu\\n", sizeof({cname}));', '  printf("limit %d\\n", GRAM_MAX_USER_ITEMS);',
             '  printf("modes %d\\n", GRAM_ITEMS_EXCLUDE * 10 + GRAM_ITEMS_ALLOW);', '  printf("abi %d\\n", GRAM_ABI_VERSION);']
    lines += [f'  printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in st._fields_]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    got = {k: int(v) for k, v in got.items()}
    assert got["size"] == C.sizeof(st) == 40
    want = {"leaf_lo": 0, "leaf_hi": 8, "ranks": 16, "count": 24, "stride": 32, "mode": 36}
    for f, _ in st._fields_:
        assert got[f] == getattr(st, f).offset == want[f], f
    assert got["limit"] == _lib.GRAM_MAX_USER_ITEMS == 4096
    assert got["modes"] == _lib.ITEMS_EXCLUDE * 10 + _lib.ITEMS_ALLOW == 1
    assert got["abi"] == _lib.ABI_VERSION == 7  # (new entry points only: the ABI version stays)


def test_list_validation_on_the_host():
    """GRAM._user_item_lists: what generate hands the op -- entries first, -1 behind them, M = the longest row -- and every ValueError"""
    from gram_amd.model.gram import GRAM
    cands = [[0, 2, 3, 1], [0, 2, 4, 1], [0, 5, 1], [0, 2, 3, 1]]  # (0 and 3 spell the same sequence)
    flat = FlatTrie(Trie(cands))
    f = GRAM._user_item_lists
    t = f([[1, -1, 1, 2], []], False, 2, flat, cands)
    assert t.dtype == torch.int32 and t.tolist() == [[1, 1, 2], [-1, -1, -1]]
    assert f(torch.tensor([[-1, 2, -1, 0], [-1, -1, -1, 3]], dtype=torch.int32), True, 2, flat, cands).tolist() == [[2, 0], [3, -1]]
    assert f([[], []], False, 2, flat, cands).tolist() == [[-1], [-1]]
    with pytest.raises(ValueError, match="outside"):
        f([[4]], False, 1, flat, cands)
    with pytest.raises(ValueError, match="outside"):
        f([[-2]], True, 1, flat, cands)
    with pytest.raises(ValueError, match="one list per user"):
        f([[1]], False, 2, flat, cands)
    with pytest.raises(ValueError, match="integer tensor"):
        f(torch.zeros(2, 3), False, 2, flat, cands)
    with pytest.raises(ValueError, match="integer tensor"):
        f(torch.zeros(3, 3, dtype=torch.int64), False, 2, flat, cands)
    with pytest.raises(ValueError, match="at most 4096"):
        f([[i % 4 for i in range(4097)]], True, 1, flat, cands)
    assert f([[i % 4 for i in range(4096)]], True, 1, flat, cands).shape == (1, 4096)
    # a user left with no item: nothing allowed; every LEAF excluded (candidate 3 shares candidate 0's)
    with pytest.raises(ValueError, match="user 1 without any item"):
        f([[0], [-1]], True, 2, flat, cands)
    with pytest.raises(ValueError, match="user 0 without any item"):
        f([[0, 1, 2], [1]], False, 2, flat, cands)
    assert f([[3, 1], [1]], False, 2, flat, cands).tolist() == [[3, 1], [1, -1]]  # user 0 keeps candidate 2


def test_generate_items_op_traces_with_fake_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import gram_amd.ops  # noqa: F401  (registers torch.ops.gram.*)
    with FakeTensorMode():
        ids = torch.zeros(3, 2, 32, dtype=torch.int64, device="cuda")
        t = torch.zeros(8, dtype=torch.int32, device="cuda")
        ws = torch.zeros(1024, dtype=torch.uint8, device="cuda")
        items = torch.zeros(3, 6, dtype=torch.int32, device="cuda")
        s, sc, wd = torch.ops.gram.generate_items(ids, ids.to(torch.uint8), 0, ws, t, t, t, 4, 3, 5, 5, 7, 1.0, None, None, None, None, None,
                                                  0, 0, t, t, t, items, True)
        assert s.shape == (15, 7) and s.dtype == torch.int64 and sc.shape == (15,) and sc.dtype == torch.float32 and wd.shape == (1,)
        s, sc, wd = torch.ops.gram.generate_items(ids, ids.to(torch.uint8), 0, ws, t, t, t, 4, 3, 1, 1, 7, 1.0, None, None, None, None, None,
                                                  0, 0, t, t, t, items, False)
        assert s.shape == (3, 7) and sc.shape == (0,)
