"""-m gpu: the forest self-attention of the tail pass (gram_amd/csrc/forest_attn.hip, gram_dec_self_attn_forest_split) against the
launch train it replaces, bit for bit.

The reference is what tail_pass() runs with the switch off: per user group and level gram_dec_self_attn_rows_split on the level's
rows gathered by slot, with the level's ancestor table, then gram_scatter_rows -- over the tables gram_tail_forest wrote.  The forests
are gram_tail_forest's own, on hand-made beam states over the comb Tries of tests/tail_oracle.py (and checked against its
enumeration, as tests/test_gpu_tail_forest.py does); q|k|v, the cache and the search's ancestor table are random.  Compared: every
16-bit word of the output, the rows no level of the call covers and the rows behind the forest included (a sentinel), and the cache
against its image from before the launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import tail_oracle as T
from tests.test_gpu_tail_forest import Run

pytestmark = pytest.mark.gpu
SENT = 0x5A5A  # 16-bit sentinel pattern (a finite number in IEEE half and in bfloat16)
K = 4
V = 512        # rows of the layer-0 token table: above every token of a comb Trie


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    return gpu_util


def _bits(t):
    return t.view(torch.int16)


class RunAt(Run):
    """tests/test_gpu_tail_forest.py's Run with the beams' rows at position t (the comb's own depth does not bind the kernels: a
    row's position is t plus its level)"""

    def __init__(self, G, comb, state, B, Tmax, n_levels, t, sub=None, spare=37):
        self.G, self.comb, self.B, self.K, self.Tmax, self.state, self.t = G, comb, B, K, Tmax, state, t
        sub = comb.sub if sub is None else sub
        cap_rows = int(T.promised_rows(comb.flat, sub, state, B, K).sum()) + spare
        self.E = T.enumerate_forest(comb.flat, sub, state, B, K, t, cap_rows, cap_rows // T.ENTRY + B, n_levels)
        self._device(torch.device(G.DEV), sub, cap_rows, n_levels, None)

    def forest(self):
        from gram_amd import _lib
        _lib.check(self.G.lib().gram_tail_forest(C.byref(self.st), C.byref(self.ctrie), C.byref(self.tail), C.byref(self.f), self.t,
                                                 self.G.stream()), "gram_tail_forest")
        torch.cuda.synchronize()
        T.check_forest(self.E, self.whole, self.layout, self.state["anc"], self.Tmax)
        return self


def _state(comb, beams, B, Tmax, seed, done=()):
    """every user's beams on the comb's prefixes `beams` (an index per beam, -1: a beam off the Trie); users `done` are finished"""
    rng = np.random.default_rng(seed)
    p = np.array(beams, dtype=np.int64).reshape(-1, K)
    p = np.concatenate([p] * (B // len(p) + 1))[:B]
    node = np.where(p >= 0, comb.prefix_node[np.maximum(p, 0)], -1)
    tokens = np.where(p >= 0, comb.prefix_tok[np.maximum(p, 0)], 0)
    fin = np.zeros(B, dtype=np.int32)
    fin[list(done)] = 1
    return dict(node=node.reshape(-1).astype(np.int32), tokens=tokens.reshape(-1).astype(np.int32), done=fin,
                anc=rng.integers(0, B * K, size=(Tmax, B * K)).astype(np.int32))


def _compare(G, run, H, pieces, table, nlev, seed):
    """gram_dec_self_attn_forest_split over the forest of `run` against the level train, for the levels < nlev"""
    from gram_amd import _lib
    E, f, L_ = run.E, run.views, G.lib()
    n, B, Tmax, t0, inner, R = E.n, run.B, run.Tmax, run.t, H * 64, run.B * K
    assert E.fits and n >= 1 and (E.level_rows <= R).all()  # (a level's slots are cache rows: what the level train can take)
    g = torch.Generator().manual_seed(seed)
    src = G.pieces_of((torch.randn(V if table else n, 3 * inner, generator=g) * 0.7).to(G.DEV), pieces)
    bias = (torch.randn(H, 64, generator=g) * 0.5).to(G.DEV)
    kc0, vc0 = (G.pieces_of((torch.randn(Tmax, R, inner, generator=g) * 0.7).to(G.DEV), pieces) for _ in range(2))
    assert int(E.tokens.max()) < V
    guard = 3  # rows behind the forest
    out = torch.empty(2, n + guard, pieces * inner, dtype=G.DT, device=G.DEV)
    _bits(out).fill_(SENT)
    # ---- the launch under test, on the cache itself
    kc, vc = kc0.clone(), vc0.clone()
    _lib.check(L_.gram_dec_self_attn_forest_split(G.p(src), G.p(f["tokens"]) if table else None, G.p(kc), G.p(vc), G.p(run.keep["anc"]),
                                                  G.p(f["pos"]), G.p(f["parent"]), G.p(f["root"]), G.p(bias), G.p(out[0]), n, R, H, t0, Tmax,
                                                  nlev, pieces, src[0].numel(), kc[0].numel(), G.stream()), "forest")
    torch.cuda.synchronize()
    assert torch.equal(_bits(kc), _bits(kc0)) and torch.equal(_bits(vc), _bits(vc0))  # (the cache is read, never written)
    # ---- the level train of tail_pass(): two groups of users, one after the other on the same cache rows
    counts = f["counts"].cpu().tolist()
    tmp = torch.empty(R, pieces * inner, dtype=G.DT, device=G.DEV)
    for gi in range(2):
        for l in range(min(nlev, E.n_levels)):
            n_l = counts[4 + gi * T.MAX_STEPS + l]
            if not n_l:
                continue
            rows_l, toks_l, anc_l = f["lvl_rows"][gi, l], f["lvl_tokens"][gi, l], f["lvl_anc"][gi, l]
            _lib.check(L_.gram_dec_self_attn_rows_split(G.p(src), G.p(toks_l if table else rows_l), G.p(kc), G.p(vc), G.p(anc_l), G.p(bias),
                                                        G.p(tmp), R, n_l, None, H, t0 + l, Tmax, pieces, src[0].numel(), kc[0].numel(),
                                                        G.stream()), "level")
            _lib.check(L_.gram_scatter_rows(G.p(tmp), G.p(rows_l), G.p(out[1]), n_l, pieces * inner * 2, n, G.stream()), "scatter")
    torch.cuda.synchronize()
    level = torch.from_numpy(E.pos - t0)
    left = (_bits(out[1]) == SENT).all(dim=1).cpu()
    assert left[:n].tolist() == (level >= nlev).tolist() and bool(left[n:].all())  # (the reference wrote exactly the rows of its levels)
    assert torch.equal(_bits(out[0]), _bits(out[1]))
    return E


# (H, pieces, Tmax, t0): every pair of values of two of the four occurs
SHAPES = [(2, 1, 8, 1), (2, 2, 8, 4), (12, 1, 8, 4), (12, 2, 8, 1), (2, 1, 32, 4), (2, 2, 32, 1), (12, 1, 32, 1), (12, 2, 32, 4)]


@pytest.mark.parametrize("B,table", [(1, False), (3, True), (40, False)])
@pytest.mark.parametrize("H,pieces,Tmax,t0", SHAPES)
def test_pure_chains_of_every_depth_the_pass_can_hold(G, H, pieces, Tmax, t0, B, table):
    """chains of 1 to D = min(GRAM_TAIL_MAX_STEPS, Tmax - 1 - t0) rows below the beams: the beams take the depths D, D - 1, ... in
    turn (forty users: every depth; the one-row forest further down is the depth 1 alone); one, three and forty
    users: both parities"""
    D = min(T.MAX_STEPS, Tmax - 1 - t0)
    comb = T.Comb(list(range(1, D + 1)), D)
    beams = [(D - 1 - u * K - k) % D for u in range(D) for k in range(K)]
    run = RunAt(G, comb, _state(comb, beams, B, Tmax, seed=B), B, Tmax, D, t0).forest()
    E = _compare(G, run, H, pieces, table, nlev=D, seed=7 * B + H)
    assert int((E.pos - t0).max()) == D - 1 and (E.parent[E.pos > t0] >= 0).all()


@pytest.mark.parametrize("B,table,cut", [(1, True, 0), (3, False, 0), (40, True, 0), (3, True, 1)])
@pytest.mark.parametrize("H,pieces,Tmax,t0", SHAPES)
def test_forks_below_the_entry_level_two_groups_copies_of_start_rows_and_a_cut(G, H, pieces, Tmax, t0, B, table, cut):
    """Prefix 0 owns a chain of h rows with a fork on every node but the last (two rows per level below the entry level), prefix 1
    a chain of h, prefix 2 a single row.  Three and forty users: a level holds more rows than the cache has per position (B * K),
    which is what forces the two user groups of the level train; one finished user; the subtree table promises one row more than
    the Trie holds for prefix 1, so every user with such a beam gets a copy of a start row (parent -1) behind its real rows.
    cut: nlev one below the forest's depth -- the deepest rows are nobody's and keep the sentinel."""
    h = min(6, Tmax - 1 - t0)
    comb = T.Comb([2 * h - 1, h, 1], h)
    sub = comb.sub.copy()
    sub[comb.prefix_node[1]] += 1
    beams = [0, 1, -1, 2] if B == 1 else [0, 0, 1, 2]
    run = RunAt(G, comb, _state(comb, beams, B, Tmax, seed=10 + B, done=(5,) if B > 5 else ()), B, Tmax, h, t0, sub=sub).forest()
    E = _compare(G, run, H, pieces, table, nlev=h - cut, seed=11 * B + H + cut)
    assert E.error == 3 and ((E.node == -1) & (E.parent == -1) & (E.pos == t0)).sum() == (B if B <= 5 else B - 1)
    kids = np.bincount(E.parent[E.parent >= 0], minlength=E.n)
    assert (kids[E.pos > t0] > 1).any() or h < 3  # (a fork below the entry level)
    if B > 1:
        assert (E.level_rows.sum(axis=0) > B * K).any() and (E.level_rows > 0).all()


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("table", [False, True])
def test_forests_of_one_row_and_of_16_k_plus_1_rows(G, table, pieces):
    H, Tmax, t0, D = 12, 8, 1, 6
    comb = T.Comb(list(range(1, D + 1)), D)
    run = RunAt(G, comb, _state(comb, [0, -1, -1, -1], 1, Tmax, seed=1), 1, Tmax, D, t0).forest()
    assert _compare(G, run, H, pieces, table, nlev=D, seed=3).n == 1
    sizes = [1, 2, 3, 4, 5, 6, 1, 2, 3, 4, 1, 1]
    run = RunAt(G, comb, _state(comb, [s - 1 for s in sizes], 3, Tmax, seed=2), 3, Tmax, D, t0).forest()
    assert _compare(G, run, H, pieces, table, nlev=D, seed=4).n == 33


def test_the_launcher_refuses_what_it_cannot_run():
    """host-side validation, before any launch"""
    from gram_amd import _lib
    lib, p = _lib.load(), C.c_void_p(0x1000)
    ok = dict(n_rows=5, R=8, H=2, t0=1, Tmax=8, nlev=2, pieces=2, qkv_ps=4096, cache_ps=8 * 8 * 128)
    for bad in (dict(n_rows=0), dict(R=0), dict(H=17), dict(t0=8), dict(t0=-1), dict(Tmax=_lib.GRAM_MAX_DEC_LEN + 1), dict(nlev=0),
                dict(nlev=T.MAX_STEPS + 1), dict(pieces=3), dict(cache_ps=8 * 8 * 128 - 1), dict(qkv_ps=0)):
        a = dict(ok, **bad)
        assert lib.gram_dec_self_attn_forest_split(p, None, p, p, p, p, p, p, p, p, a["n_rows"], a["R"], a["H"], a["t0"], a["Tmax"], a["nlev"],
                                                   a["pieces"], a["qkv_ps"], a["cache_ps"], None) == _lib.E_ARG, bad
    assert lib.gram_dec_self_attn_forest_split(p, None, p, p, p, None, p, p, p, p, 5, 8, 2, 1, 8, 2, 2, 4096, 8192, None) == _lib.E_ARG
