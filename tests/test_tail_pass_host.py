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
# forty prefixes at d_tail = 3 with four steps below them and 4 to 6 rows each: 20 beams hold more than 64 forest rows, 40 more than 128
WIDE = ([[0, a, b, 60 + (a - 2), 90, 120, 1] for a in range(2, 7) for b in range(40, 48)]
        + [[0, a, 40, 60 + (a - 2), 91, 120, 1] for a in range(2, 7)] + [[0, 2, 41, 60, 90, 121, 1]])


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


@pytest.mark.parametrize("name,cands,want_d", [("chain", CHAIN, 2), ("ragged", RAGGED, 2), ("branchy", BRANCHY, 3), ("bushy", BUSHY, 0),
                                               ("wide", WIDE, 3)])
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
    if cands is WIDE:
        at = [int(sub[n]) for n in range(flat.n_nodes) if len(pre[n]) == d_tail]
        assert steps == 4 and len(at) == 40 and set(at) == {4, 5, 6}
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


def _forest_walk(flat, beams, t):
    """(node, parent row, position) of every row of the forest below the nodes `beams`: the rows are their own queue"""
    fan = np.diff(flat.child_off)
    rows = [(n, -1, t) for n in beams]
    head = 0
    while head < len(rows):
        n, _, pos = rows[head]
        for e in range(int(flat.child_off[n]), int(flat.child_off[n + 1])):
            c = int(flat.child_node[e])
            if fan[c] > 0:
                rows.append((c, head, pos + 1))
        head += 1
    return rows


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
    rows = _forest_walk(flat, beams, d_tail - 1)
    assert len(rows) == int(sub[beams].sum())
    assert [r[2] for r in rows] == sorted(r[2] for r in rows)
    assert all(par < i for i, (_, par, _) in enumerate(rows))
    assert max(r[2] for r in rows) - (d_tail - 1) + 1 <= steps


def test_the_numpy_enumeration_of_the_gpu_tests_equals_the_plain_walk():
    """tests/tail_oracle.py is what the GPU tests compare gram_tail_forest with; here it is itself compared with the walk above, on
    BRANCHY: three users (every other prefix of length d_tail, the other ones, one finished user), a beam off the Trie and one on a
    leaf among them.  Then its comb Trie: every prefix owns the wanted number of rows by the walk, the numbers by the recursive walk
    are FlatTrie's, and a subtree table that promises more than the Trie holds gives the copies of a start row and error 3."""
    from tests import tail_oracle as T
    flat = FlatTrie(Trie(BRANCHY))
    sub, d_tail, steps = flat.tail_tables()
    assert np.array_equal(T.sub_rows_walk(flat), sub)
    pre = _node_prefixes(flat)
    fan = np.diff(flat.child_off)
    at = [n for n, p in pre.items() if len(p) == d_tail and fan[n] > 0]
    leaf = next(n for n in range(1, flat.n_nodes) if fan[n] == 0)
    beams = [at[::2] + [-1, leaf], at[1::2] + [flat.n_nodes, at[1]], at[:14]]
    B, K, t = 3, 14, d_tail - 1
    state = dict(node=np.array(beams, dtype=np.int32).reshape(-1), done=np.array([0, 0, 1], dtype=np.int32),
                 tokens=np.array([[pre[n][-1] if 0 <= n < flat.n_nodes else 0 for n in row] for row in beams], dtype=np.int32).reshape(-1))
    E = T.enumerate_forest(flat, sub, state, B, K, t, 200, 8, steps)
    assert E.fits and E.error == 0 and E.user_off[3] == E.user_off[2] == E.n  # (the finished user owns no row)
    for b in range(2):
        live = [n for n in beams[b] if 0 <= n < flat.n_nodes and fan[n] > 0]
        rows = _forest_walk(flat, live, t)
        lo, hi = int(E.user_off[b]), int(E.user_off[b + 1])
        assert hi - lo == len(rows) == int(sub[live].sum())
        assert E.node[lo:hi].tolist() == [r[0] for r in rows] and E.pos[lo:hi].tolist() == [r[2] for r in rows]
        assert E.parent[lo:hi].tolist() == [r[1] + lo if r[1] >= 0 else -1 for r in rows]
        assert E.tokens[lo:hi].tolist() == [pre[r[0]][-1] for r in rows]
        root = [b * K + k for k, n in enumerate(beams[b]) if 0 <= n < flat.n_nodes and fan[n] > 0]
        top = []  # a row's root is the beam at the top of its parent chain
        for i, r in enumerate(rows):
            top.append(root[i] if r[1] < 0 else top[r[1]])
        assert E.root[lo:hi].tolist() == top
    assert E.counts[:4].tolist() == [E.n, int(((E.per_user + 63) // 64).sum()), int(E.per_user.max()), 0]
    assert E.level_rows[0].tolist() == [int((E.pos[: E.user_off[1]] == t + l).sum()) for l in range(steps)]
    assert T.expected_rowpos(flat, E, state)[0].reshape(B, K)[0].tolist() == list(range(12)) + [-1, -1]
    over = T.enumerate_forest(flat, sub, state, B, K, t, E.n - 1, 8, steps)
    assert not over.fits and over.counts[0] == E.n and over.user_off.tolist() == E.user_off.tolist()
    # the comb
    comb = T.Comb(list(range(1, 41)) + [64, 65], 6)
    for p, r in enumerate(comb.sizes):
        rows = _forest_walk(comb.flat, [int(comb.prefix_node[p])], 2)
        assert len(rows) == r and max(q[2] for q in rows) - 2 + 1 == min(r, 6)
    assert np.array_equal(comb.flat.tail_tables()[0], comb.sub)
    chains = T.Comb([5] * 8, 5)
    assert chains.qualifies and chains.flat.tail_tables()[1:] == (3, 5)  # (Comb compared the two tables)
    more = comb.sub.copy()
    more[comb.prefix_node[3]] += 2
    st = dict(node=comb.prefix_node[[3, 0]].astype(np.int32), tokens=comb.prefix_tok[[3, 0]].astype(np.int32), done=np.zeros(1, dtype=np.int32))
    E = T.enumerate_forest(comb.flat, more, st, 1, 2, 2, 16, 2, 6)
    assert E.error == 3 and E.n == 7 and E.node.tolist()[5:] == [-1, -1] and E.root.tolist()[5:] == [0, 0] and E.pos.tolist()[5:] == [2, 2]


def _fake_forest(**kw):
    F = 0x1000  # a non-null address that is never dereferenced
    arrays = [n for n, _ in _lib.Forest._fields_[:15]]
    f = dict({n: F for n in arrays}, cap_rows=64, cap_entries=4, n_levels=4, pad_=0)
    f.update(kw)
    return _lib.Forest(**f), arrays


def test_forest_launchers_refuse_bad_arguments_without_gpu():
    """Every GRAM_E_ARG case of gram_tail_forest and gram_tail_rowpos: each call is refused before any launch, so fake pointers do and
    no GPU is needed; each differs from a legal call in the one argument its line names."""
    lib, F, E = _lib.load(), 0x1000, _lib.E_ARG

    def state(B=2, K=4, Tmax=8):
        return _lib.BeamState(B=B, K=K, Tmax=Tmax, length_penalty=1.0, eos=1, pad=0,
                              **{n: F for n, _ in _lib.BeamState._fields_[6:19]}, cand_logits_users=0, cand_logits_stride=0)
    trie = _lib.Trie(F, F, F, 10, 9, 3, 3)
    tail = _lib.TrieTail(F, 3, 4)

    def forest(st=None, tr=trie, tl=tail, t=2, null_st=False, null_f=False, **kw):
        f, _ = _fake_forest(**kw)
        return lib.gram_tail_forest(None if null_st else C.byref(st or state()), tr and C.byref(tr), tl and C.byref(tl),
                                    None if null_f else C.byref(f), t, None)

    def rowpos(st=None, tr=trie, null_st=False, null_f=False, **kw):
        f, _ = _fake_forest(**kw)
        return lib.gram_tail_rowpos(None if null_st else C.byref(st or state()), tr and C.byref(tr), None if null_f else C.byref(f), None)

    for name in _fake_forest()[1]:  # each NULL array in turn
        assert forest(**{name: None}) == E, name
        assert rowpos(**{name: None}) == E, name
    for fn in (forest, rowpos):
        assert fn(cap_rows=0) == E and fn(cap_rows=-1) == E
        assert fn(cap_entries=0) == E
        assert fn(n_levels=0) == E and fn(n_levels=_lib.GRAM_TAIL_MAX_STEPS + 1) == E
        assert fn(st=state(K=_lib.GRAM_MAX_BEAMS + 1)) == E and fn(st=state(K=0)) == E and fn(st=state(B=0)) == E
        assert fn(st=state(Tmax=1)) == E and fn(st=state(Tmax=_lib.GRAM_MAX_DEC_LEN + 1)) == E
        assert fn(null_st=True) == E and fn(tr=None) == E and fn(null_f=True) == E
    assert forest(t=-1) == E and forest(t=8) == E and forest(t=9) == E  # t >= Tmax
    assert forest(tl=None) == E and forest(tl=_lib.TrieTail(None, 3, 4)) == E  # NULL tail, NULL sub_rows


def test_scatter_rows_refuses_bad_arguments_without_gpu():
    lib, F, E = _lib.load(), 0x1000, _lib.E_ARG

    def scatter(src=F, rows=F, dst=F + 0x1000, n=4, row_bytes=256, dst_rows=8):
        return lib.gram_scatter_rows(src, rows, dst, n, row_bytes, dst_rows, None)

    assert scatter(row_bytes=8) == E and scatter(row_bytes=24) == E and scatter(row_bytes=0) == E  # whole 16-byte words, at least one
    assert scatter(n=0) == E and scatter(n=-1) == E
    assert scatter(dst_rows=0) == E
    assert scatter(src=F + 8) == E and scatter(dst=F + 0x1008) == E  # a pointer misaligned by 8
    assert scatter(src=None) == E and scatter(rows=None) == E and scatter(dst=None) == E


def test_struct_sizes_and_entry_points():
    lib = _lib.load()
    assert C.sizeof(_lib.TrieTail) == 16 and C.sizeof(_lib.Forest) == 15 * 8 + 16
    assert lib.gram_abi_version() == _lib.ABI_VERSION  # (new entry points only)
    out = (C.c_int32 * 4)(7, 7, 7, 7)
    assert lib.gram_debug_tail_last(out) == 0 and lib.gram_debug_tail_last(None) == _lib.E_ARG
    assert lib.gram_workspace_bytes_tail(None, 1, 1, 32, 4, 4, 2) == _lib.E_ARG
