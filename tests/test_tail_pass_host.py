"""The tail tables of the tail pass (FlatTrie.tail_tables, include/gram_hip.h gram_trie_tail_t) against a plain Python walk of the
nested Trie, and the forest they promise -- the rows gram_tail_forest enumerates -- against a plain enumeration.  The launch trains of
gram_generate_tail are pinned by tests/test_launch_train.py (the generate_tail_* goldens)."""
import ctypes as C

import numpy as np
import pytest

from gram_amd import _lib
from gram_amd.utils.generation_trie import FlatTrie, Trie

CHAIN = [[0, a, a + 30, a + 60, a + 90, 1] for a in range(2, 26)]                                   # pure chains below the start token
RAGGED = CHAIN[:12] + [[0, a, a + 30, a + 60, a + 90, a + 120, 1] for a in range(14, 26)]              # ids of l and l + 1 tokens
# six bushy nodes under the start token, chains below them -- but for a fork at depth 4 and one at depth 3: d_tail = 3
BRANCHY = ([[0, a, b, 60 + 4 * (a - 2) + (b - 40), 90, 1] for a in range(2, 8) for b in range(40, 44)]
           + [[0, 2, 40, 60, 91, 1], [0, 3, 41, 84, 90, 1]])
BUSHY = [[0, a, b, c, 1] for a in range(2, 6) for b in range(2, 6) for c in range(2, 6)]              # fan-out 4 at every level


def _walk(cands):
    """{node prefix (tuple): children prefixes} of the nested Trie, and per prefix (inner, subtree rows, height)."""
    root = Trie(cands).trie_dict
    info = {}

    def rec(node, prefix):
        kids = [rec(node[t], prefix + (t,)) for t in sorted(node)]
        inner = bool(node) and len(prefix) > 0
        rows = (1 if inner else 0) + sum(k[0] for k in kids)
        height = (1 + max([k[1] for k in kids], default=0)) if inner else 0
        info[prefix] = (inner, rows if inner else 0, height)
        return rows if inner else 0, height
    rec(root, ())
    return info


def _expected(cands, factor):
    info = _walk(cands)
    inner = {p: v for p, v in info.items() if v[0]}
    deepest = max(len(p) for p in inner)
    d_tail = 0
    for d in range(deepest, 1, -1):
        at = [v for p, v in inner.items() if len(p) == d]
        if sum(v[1] for v in at) > factor * sum(v[2] for v in at):
            break
        if deepest - d + 1 >= 2:
            d_tail = d
    return info, d_tail, (deepest - d_tail + 1 if d_tail else 0)


def _node_prefixes(flat):
    """prefix (tuple) of every node of the CSR"""
    pre = {0: ()}
    for n in range(flat.n_nodes):
        for e in range(int(flat.child_off[n]), int(flat.child_off[n + 1])):
            pre[int(flat.child_node[e])] = pre[n] + (int(flat.child_tok[e]),)
    return pre


@pytest.mark.parametrize("name,cands,want_d", [("chain", CHAIN, 2), ("ragged", RAGGED, 2), ("branchy", BRANCHY, 3), ("bushy", BUSHY, 0)])
def test_tail_tables_equal_a_plain_walk(name, cands, want_d):
    flat = FlatTrie(Trie(cands))
    sub, d_tail, steps = flat.tail_tables()
    info, d_exp, steps_exp = _expected(cands, FlatTrie.TAIL_ROW_FACTOR)
    assert (d_tail, steps) == (d_exp, steps_exp)
    assert d_tail == want_d, name
    assert sub.dtype == np.int32 and sub.shape == (flat.n_nodes,)
    pre = _node_prefixes(flat)
    for n in range(flat.n_nodes):
        assert int(sub[n]) == (info[pre[n]][1] if n else sub[0]), pre[n]
    if d_tail == 0:
        assert steps == 0  # no qualifying depth: generate() decodes step by step
    else:
        assert 2 <= steps <= _lib.GRAM_TAIL_MAX_STEPS


def test_factor_moves_the_switch_depth():
    """A looser factor can only move the switch up the Trie; a factor below 1 leaves no tail (a chain's forest holds exactly the
    rows stepping does)."""
    flat = FlatTrie(Trie(BRANCHY))
    assert flat.tail_tables(0.99)[1:] == (0, 0)
    assert flat.tail_tables(1.0)[1:] == (0, 0)  # (the forks: 51 rows against 50 at depth 4)
    d = [flat.tail_tables(f)[1] for f in (1.10, 1.5, 4.0)]
    assert d == [3, 3, 2]
    assert FlatTrie(Trie(BUSHY)).tail_tables(100.0)[1] == 2
    assert flat.tail_tables()[1] == 3  # (the default is back after the sweep: the cache is per factor)


def test_both_constructors_give_the_same_tables():
    a = FlatTrie(Trie(RAGGED))
    t = Trie(RAGGED)
    _ = t.trie_dict  # (the nested-dict constructor path)
    b = FlatTrie(t)
    assert a.tail_tables()[1:] == b.tail_tables()[1:]
    assert np.array_equal(a.tail_tables()[0], b.tail_tables()[0])


@pytest.mark.parametrize("cands", [CHAIN, RAGGED, BRANCHY])
def test_forest_of_any_beam_set_has_sub_rows_rows(cands):
    """The forest gram_tail_forest builds for beams on prefixes of length d_tail: a breadth-first walk of the CSR from those nodes over
    children that have children (the device's enumeration, restated) holds exactly sum(sub_rows) rows, depth-major, every parent in
    front of its children."""
    flat = FlatTrie(Trie(cands))
    sub, d_tail, steps = flat.tail_tables()
    pre = _node_prefixes(flat)
    fan = np.diff(flat.child_off)
    beams = [n for n, p in pre.items() if len(p) == d_tail and fan[n] > 0][::2]  # every other prefix of that length
    rows = [(n, -1, d_tail - 1) for n in beams]
    head = 0
    while head < len(rows):
        n, _, pos = rows[head]
        for e in range(int(flat.child_off[n]), int(flat.child_off[n + 1])):
            c = int(flat.child_node[e])
            if fan[c] > 0:
                rows.append((c, head, pos + 1))
        head += 1
    assert len(rows) == int(sub[beams].sum())
    assert [r[2] for r in rows] == sorted(r[2] for r in rows)
    assert all(par < i for i, (_, par, _) in enumerate(rows))
    assert max(r[2] for r in rows) - (d_tail - 1) + 1 <= steps


def test_struct_sizes_and_entry_points():
    lib = _lib.load()
    assert C.sizeof(_lib.TrieTail) == 16 and C.sizeof(_lib.Forest) == 15 * 8 + 16
    assert lib.gram_abi_version() == _lib.ABI_VERSION  # (new entry points only)
    out = (C.c_int32 * 4)(7, 7, 7, 7)
    assert lib.gram_debug_tail_last(out) == 0 and lib.gram_debug_tail_last(None) == _lib.E_ARG
    assert lib.gram_workspace_bytes_tail(None, 1, 1, 32, 4, 4, 2) == _lib.E_ARG
