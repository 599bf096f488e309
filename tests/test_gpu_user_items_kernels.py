"""The per-user item-filter kernels of gram_amd/csrc/beam.hip, driven directly through the C ABI (tests/gpu_util.py, _lib.UserItems)
at every launch form.  tests/test_gpu_user_items.py covers them through whole generate() calls on a tiny model; here the shapes
are chosen so that every instantiation runs.  launch_search_step picks the form from B and the Trie alone:

    B <= 16 and a state with cand_logits ("scratch")   sparse_logits_kernel, then beam_step_kernel<1024, gram_user_items_t> reading
                                                       its logits
    B <= 128 (17 .. 128, or <= 16 without scratch)     beam_step_kernel<1024, gram_user_items_t>, dot products in the kernel: the
                                                       dead flag parked in bit 63 of the key slot, dot(act && !dead)
    B >= 129                                           beam_step_kernel<256, gram_user_items_t>
    K * max_fanout > 16 384 or too much LDS            beam_step_chunked_kernel<1024, gram_user_items_t> (B <= 128) / <256, ...>
                                                       (B >= 129); the same two under gram_debug_set_beam_chunked(1) on any shape
                                                       ("forced")
    rowpos != NULL                                     the live-row form of whichever kernel the shape selects

Each of them runs below with exclude and with allow lists, on one-piece (gram_beam_step_sparse_items) and two-piece
(gram_beam_step_sparse_split_items) operands.  The thresholds are read once per process, so the form is chosen through B, never
through the environment.

1. gram_user_items_prepare against np.unique at every M around the kernel's 256-thread slices, outputs prefilled with -7;
2. whole filtered searches, every state array after every step bit for bit against one-user searches of the UNFILTERED kernels on
   Trie(A_b) -- the definition tests/test_gpu_user_items.py rests on; forced chunking and the live-row form against the filtered
   all-rows one-shot run;
3. filtered searches against the CPU oracle (independent of the unfiltered kernels);
4. gram_greedy_step_items against O.greedy_search with per-user callbacks;
5. the count clamp of node_alive and the argument errors with a real state behind them.

The unmarked tests check the list generators on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import gram_oracle as O
from tests.test_wide_trie_host import golden_cands, is_wide, make_logits, wide_tries

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    return gpu_util


# ------------------------------------------------------------------------------------ 1. lists for gram_user_items_prepare (numpy)
N_ITEMS = 5000
PREPARE_M = [1, 2, 255, 256, 257, 511, 512, 513, 1000, 4095, 4096]
PATTERNS = ("padding", "one_item", "ascending", "descending", "random", "straddle", "dups_and_padding", "bad_indices", "rank_zero",
            "rank_max")
BAD_INDICES = (N_ITEMS, 2 ** 31 - 1, -2)


def item_rank_table():
    """a fixed permutation of 0 .. N_ITEMS - 1 with 1 % of the entries set to -1 (never the items of rank 0 and of the largest rank)"""
    rng = np.random.default_rng(11)
    rank = rng.permutation(N_ITEMS).astype(np.int32)
    pool = np.nonzero((rank != 0) & (rank != N_ITEMS - 1))[0]
    rank[rng.choice(pool, N_ITEMS // 100, replace=False)] = -1
    return rank


def slice_len(M):
    """sorted entries per thread of user_items_prepare_kernel: npad / 256, npad the power of two >= max(M, 256)"""
    npad = 256
    while npad < M:
        npad <<= 1
    return npad // 256


def prepare_lists(M, rank, seed):
    """(items int64 [40][M], pattern name of every user): four users per pattern of PATTERNS.  'straddle' user v repeats, in SORTED
    order, the entry in front of every (v + 1)-th multiple of slice_len(M): the two copies of a rank lie in two threads' slices."""
    rng = np.random.default_rng(seed)
    valid = np.nonzero(rank >= 0)[0]
    by_rank = valid[np.argsort(rank[valid])]
    per = slice_len(M)
    rows, names = [], []
    for pat in PATTERNS:
        for v in range(4):
            row = np.full(M, -1, dtype=np.int64)
            some = valid[rng.integers(0, valid.size, M)]
            if pat == "one_item":
                row[:] = some[0]
            elif pat in ("ascending", "descending"):
                items = by_rank[np.sort(rng.choice(by_rank.size, M, replace=False))]
                row[:] = items if pat == "ascending" else items[::-1]
            elif pat == "random":
                row[:] = rng.integers(0, N_ITEMS, M)  # (about 1 % of them have no rank)
            elif pat == "straddle":
                new = np.ones(M, dtype=bool)
                new[per * (v + 1)::per * (v + 1)] = False  # sorted position i = q * per repeats position i - 1
                idx = np.cumsum(new) - 1
                items = by_rank[np.sort(rng.choice(by_rank.size, int(idx[-1]) + 1, replace=False))]
                row[:] = rng.permutation(items[idx])
            elif pat == "dups_and_padding":  # a, -1, a, b, -1, b, ...
                row[0::3] = some[: row[0::3].size]
                row[2::3] = some[: row[2::3].size]
            elif pat == "bad_indices":
                row[:] = some
                pos = np.arange(M)[np.arange(M) % 2 == v % 2]
                row[pos] = np.asarray(BAD_INDICES)[(pos // 2) % 3]
            elif pat in ("rank_zero", "rank_max"):
                item = int(np.nonzero(rank == (0 if pat == "rank_zero" else rank.max()))[0][0])
                row[:] = some
                row[rng.random(M) < 0.3] = item
                row[rng.integers(0, M)] = item
            rows.append(row)
            names.append(pat)
    return np.stack(rows), names


def prepare_reference(row, rank):
    """the entries inside [0, n_items) -> their ranks, negative ones dropped -> np.unique"""
    r = rank[row[(row >= 0) & (row < rank.size)]]
    return np.unique(r[r >= 0])


@pytest.mark.parametrize("M", PREPARE_M + [300])
def test_prepare_lists_hold_their_patterns(M):
    rank = item_rank_table()
    assert sorted(rank[rank >= 0].tolist()) == sorted(set(rank.tolist()) - {-1}) and (rank < 0).sum() == N_ITEMS // 100
    assert (rank == 0).sum() == 1 and rank.max() == N_ITEMS - 1
    rows, names = prepare_lists(M, rank, seed=M)
    assert rows.shape == (40, M) and names == [p for p in PATTERNS for _ in range(4)]
    assert rows.min() >= -(2 ** 31) and rows.max() < 2 ** 31
    per = slice_len(M)
    assert per == {1: 1, 2: 1, 255: 1, 256: 1, 257: 2, 300: 2, 511: 2, 512: 2, 513: 4, 1000: 4, 4095: 16, 4096: 16}[M]
    counts = {}
    for u, (row, pat) in enumerate(zip(rows, names)):
        ref = prepare_reference(row, rank)
        counts.setdefault(pat, []).append(ref.size)
        if pat == "straddle":  # every entry has a rank, so the sorted list is the kernel's sorted array in front of its padding
            s = np.sort(rank[row])
            assert (s >= 0).all()
            q = np.arange(per * (u % 4 + 1), M, per * (u % 4 + 1))
            assert (s[q] == s[q - 1]).all() and ref.size == M - q.size
            assert q.size > 0 or M <= per * (u % 4 + 1)
        if pat == "bad_indices" and M >= 6:
            assert set(BAD_INDICES) <= set(row.tolist()) and ref.size > 0
        if pat == "rank_zero":
            assert ref[0] == 0
        if pat == "rank_max":
            assert ref[-1] == N_ITEMS - 1
        if pat == "dups_and_padding" and M >= 3:
            assert (row[1::3] == -1).all() and (row[0::3][: row[2::3].size] == row[2::3]).all()
    assert counts["padding"] == [0] * 4 and counts["one_item"] == [1] * 4
    assert counts["ascending"] == [M] * 4 and counts["descending"] == [M] * 4


# ------------------------------------------------------------------------------------ 2. Tries and user lists of the searches
def grid(n):
    """[0, a, b, c, 1] with a, b, c in 2 .. n + 1: n^3 leaves, fan-out n on three levels"""
    r = range(2, 2 + n)
    return [[0, a, b, c, 1] for a in r for b in r for c in r]


def trie_cands(name):
    """name -> (candidates, V)"""
    if name in ("uniform", "ragged", "narrow_root"):
        from tests.test_gpu_kernels import _tries
        return _tries()[name], 256
    if name in ("grid16", "grid8"):
        return grid(int(name[4:])), 256
    if name in ("second300", "root900"):
        cands, _B, _K, V, _T, _fan = wide_tries()[name]
        return cands, V
    if name == "beauty":
        return golden_cands("Beauty"), 32128
    assert name == "rand"
    from tests.test_gpu_configs import _rand_cands
    return _rand_cands(7, 120, 2, 6), 256


def _all_but_one_leaf(cands, rng):
    """Every leaf but one under every other first token, and under every other second-level node of the remaining first tokens:
    the user's ranks inside such a node's leaf range number hi - lo - 1, one short of dead"""
    firsts = sorted({c[1] for c in cands})
    big = set(firsts[::2])
    g2, g3 = {}, {}
    for i, c in enumerate(cands):
        if c[1] in big:
            g2.setdefault(c[1], []).append(i)
        elif len(c) > 3:
            g3.setdefault((c[1], c[2]), []).append(i)
    groups = [g for _, g in sorted(g2.items())] + [g for _, g in sorted(g3.items())][::2]
    out = []
    for g in groups:
        if len(g) >= 2:
            one = g[int(rng.integers(0, len(g)))]
            out += [i for i in g if i != one]
    return out


def _trim(excl, n, min_keep):
    """drop entries from the end until at least min_keep of the n items are left (padding and repeats cost nothing)"""
    seen, out = set(), []
    for i in excl:
        if i >= 0 and i not in seen:
            if len(seen) >= n - min_keep:
                continue
            seen.add(i)
        out.append(i)
    return out


def exclude_lists(name, cands, B, top, seed, min_keep=1):
    """The exclude list of every user.  top[b]: the items of user b's unfiltered result, best first.  Users cycle through eight
    kinds by b % 8 (the random ones repeat after 32 users):
        0 nothing excluded                          4 exactly one item kept (min_keep if that is more)
        1 the top 3 of its own unfiltered result    5 a random half
        2 every item under the first token of its   6 all leaves but one under each of several inner nodes (_all_but_one_leaf)
          best item: an inner node dies             7 duplicates interleaved with -1
        3 all but 3 items (min_keep if more)
    'second300' and 'beauty' have lists of their own (see the cases of test_filtered_search_equals_per_user_tries)."""
    n = len(cands)
    lists = []
    for b in range(B):
        rng = np.random.default_rng(seed * 1000 + (b % 32))
        kind = b % 8
        if name == "second300":  # every other second token under three first tokens (and user 1's best three items)
            firsts, par = ((2, 3, 4), 0) if b % 2 == 0 else ((5, 6, 7), 1)
            r = [i for i, c in enumerate(cands) if c[1] in firsts and len(c) == 4 and c[2] % 2 == par] + (top[b][:3] if b % 2 else [])
        elif name == "beauty":  # 4 096 entries: the user's best five and 4 091 random others
            others = np.setdiff1d(np.arange(n), np.asarray(top[b][:5]))
            r = top[b][:5] + rng.choice(others, 4096 - len(top[b][:5]), replace=False).tolist()
        elif kind == 0:
            r = []
        elif kind == 1:
            r = list(top[b][:3])
        elif kind == 2:
            r = [i for i, c in enumerate(cands) if c[1] == cands[top[b][0]][1]]
        elif kind in (3, 4):
            kept = set(rng.choice(n, min(n, max(3 if kind == 3 else 1, min_keep)), replace=False).tolist())
            r = [i for i in range(n) if i not in kept]
        elif kind == 5:
            r = rng.permutation(n)[: n // 2].tolist()
        elif kind == 6:
            r = _all_but_one_leaf(cands, rng)
        else:
            x = int(rng.integers(0, n))
            r = [top[b][0], -1, top[b][0], x, -1, x, -1, top[b][min(1, len(top[b]) - 1)]]
        lists.append(_trim(r, n, min_keep))
    return lists


def keep_sets(cands, lists):
    """A_b as sorted candidate indices: what an exclude list leaves (two candidates that spell one sequence go together)"""
    seqs = [tuple(c) for c in cands]
    out = []
    for r in lists:
        gone = {seqs[i] for i in r if i >= 0}
        out.append([i for i, s in enumerate(seqs) if s not in gone])
    return out


def allow_lists(keep):
    """the complements, as allow lists; users 7, 15, ... get theirs with repeats and -1 in between when that fits"""
    out = []
    for b, kp in enumerate(keep):
        out.append([v for i in kp for v in (i, -1, i)] if b % 8 == 7 and 3 * len(kp) <= 4096 else list(kp))
        assert len(out[-1]) <= 4096
    return out


@pytest.mark.parametrize("name,B,K", [("ragged", 8, 4), ("ragged", 24, 12), ("uniform", 129, 4), ("narrow_root", 130, 20),
                                      ("grid16", 8, 64), ("grid16", 129, 20), ("second300", 2, 64), ("root900", 129, 20), ("grid8", 5, 20)])
def test_exclude_lists_hold_their_kinds(name, B, K):
    from gram_amd.utils.generation_trie import FlatTrie, Trie
    cands, V = trie_cands(name)
    n = len(cands)
    assert max(max(c) for c in cands) < V
    flat = FlatTrie(Trie(cands))
    if name == "grid16":
        assert n == 4096 and flat.max_fanout == 16
    top = [list(range(b % 5, b % 5 + 5)) for b in range(B)]  # (any items will do here)
    for min_keep in (1, K):
        lists = exclude_lists(name, cands, B, top, seed=3, min_keep=min_keep)
        keep = keep_sets(cands, lists)
        assert len(lists) == B and all(len(r) <= 4096 for r in lists) and all(len(a) <= 4096 for a in allow_lists(keep))
        assert all(len(kp) >= min(n, min_keep) for kp in keep)
        if min_keep > 1 or name == "second300":
            continue
        lo, hi = flat.leaf_ranges()
        ranks = flat.item_ranks(cands)
        for b, (r, kp) in enumerate(zip(lists, keep)):
            kind = b % 8
            if kind == 0:
                assert r == [] and len(kp) == n
            if kind == 1:
                assert r == top[b][:3]
            if kind == 2:  # the node of the first token is dead, its siblings are not
                assert {cands[i][1] for i in r} == {cands[top[b][0]][1]} and all(cands[i][1] != cands[top[b][0]][1] for i in kp)
            if kind == 3:
                assert len(kp) == 3
            if kind == 4:
                assert len(kp) == 1
            if kind == 5:
                assert len(kp) == n - n // 2
            if kind == 6:  # some inner node holds hi - lo - 1 of the user's ranks
                mine = np.sort(ranks[r])
                c = np.searchsorted(mine, hi) - np.searchsorted(mine, lo)
                assert ((c == hi - lo - 1) & (hi - lo >= 2)).any()
            if kind == 7:
                assert -1 in r and len(set(r)) < len(r)


# ------------------------------------------------------------------------------------ the search driver
STATE = ("tokens", "node", "beam_scores", "seq", "anc", "done", "n_hyps", "hyp_score", "worst", "hyp_len", "hyp_tok")
PER_ROW = ("tokens", "node", "beam_scores", "seq")


def _raw(t):
    """a state array as integers of its element size (floats compared by their bits)"""
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


def _of_user(arr, key, b, K):
    """user b's part of a batch state array"""
    if key == "anc":
        return arr[:, b * K:(b + 1) * K]
    return arr[b * K:(b + 1) * K] if key in PER_ROW else arr[b:b + 1]


class _Case:
    """One search problem: Trie, B, K, operands of one piece mode (the set-up of tests/test_gpu_wide_trie.py::_Search: E32 and
    per-step hidden states, lse from gram_gemm_bf16_lse_split + gram_lse_combine, computed once for the whole batch)."""

    def __init__(self, G, name, B, K, pieces, scratch, seed):
        from gram_amd import _lib
        from gram_amd.utils import generation_trie as gt
        self.G, self.name, self.B, self.K, self.pieces, self.scratch = G, name, B, K, pieces, scratch
        self.cands, self.V = trie_cands(name)
        self.index = {tuple(c): i for i, c in reversed(list(enumerate(self.cands)))}
        self.flat = gt.FlatTrie(gt.Trie(self.cands))
        self.ctrie, self._keep_trie = self.flat.to_device(torch.device(G.DEV))
        self.T = max(len(c) for c in self.cands)
        self.d = d = 128
        V, R, steps = self.V, B * K, self.T - 1
        g = torch.Generator().manual_seed(seed)
        self.E32 = torch.randn(V, d, generator=g).to(G.DEV)
        hidden32 = [(torch.randn(B if t == 0 else R, d, generator=g) * d ** -0.5 * 3).to(G.DEV) for t in range(steps)]
        if pieces == 2:
            self.W, self.hidden = G.inter(self.E32), [G.inter(h) for h in hidden32]
        else:
            self.W, self.hidden = G.bf(self.E32), [G.bf(h) for h in hidden32]
        sp = _lib.Split(pieces, 0, 0, 0, 1.0)
        L_ = G.lib()
        self.lse = []
        for h in self.hidden:
            rows = h.shape[0]
            part = torch.empty(rows, V // 64, 2, dtype=torch.float32, device=G.DEV)
            lse = torch.empty(rows, dtype=torch.float32, device=G.DEV)
            _lib.check(L_.gram_gemm_bf16_lse_split(G.p(h), G.p(self.W), None, G.p(part), rows, V, d, pieces * d, V, C.byref(sp), G.stream()),
                       "gemm")
            _lib.check(L_.gram_lse_combine(G.p(part), G.p(lse), rows, V // 64, G.stream()), "lse")
            self.lse.append(lse)
        self._user_tries = {}

    def step(self, st, ctrie, h, lse, t, rpu, rowpos=None, ui=None):
        """one search step: the unfiltered entry points (ui None) or the *_items ones; returns the call's code"""
        G, d, V = self.G, self.d, self.V
        L_ = G.lib()
        a = (C.byref(st), C.byref(ctrie), G.p(h))
        if self.pieces == 2:
            if ui is None:
                return L_.gram_beam_step_sparse_split(*a, G.p(self.E32), d, G.p(lse), V, t + 1, rpu, G.p(rowpos), 2, G.stream())
            return L_.gram_beam_step_sparse_split_items(*a, G.p(self.E32), d, G.p(lse), V, t + 1, rpu, G.p(rowpos), 2, C.byref(ui), G.stream())
        if ui is not None:
            return L_.gram_beam_step_sparse_items(*a, G.p(self.W), d, G.p(lse), V, t + 1, rpu, G.p(rowpos), C.byref(ui), G.stream())
        if rowpos is not None:
            return L_.gram_beam_step_sparse_live(*a, G.p(self.W), d, G.p(lse), V, t + 1, G.p(rowpos), G.stream())
        return L_.gram_beam_step_sparse(*a, G.p(self.W), d, G.p(lse), V, t + 1, rpu, G.stream())

    def finalize(self, st, B):
        from gram_amd import _lib
        G = self.G
        seqs = torch.empty(B * self.K, self.T, dtype=torch.int64, device=G.DEV)
        scores = torch.empty(B * self.K, dtype=torch.float32, device=G.DEV)
        width = torch.zeros(4, dtype=torch.int32, device=G.DEV)
        _lib.check(G.lib().gram_beam_finalize(C.byref(st), self.K, self.T, G.p(seqs), G.p(scores), G.p(width), G.stream()), "finalize")
        torch.cuda.synchronize()
        return seqs.cpu(), scores.cpu(), int(width[0])

    def search(self, B, ctrie, hidden, lse, ui=None, scratch=False):
        """A whole search of T - 1 steps, step 0 on one row per user -> dict(snaps: the state after every step, as integers on the
        host, error[0] with it; seqs, scores (their bits), width, error: what gram_beam_finalize left)."""
        from gram_amd import _lib
        G = self.G
        st, keep = G.make_beam_state(B, self.K, self.T, cand_scratch=scratch)
        _lib.check(G.lib().gram_beam_init(C.byref(st), C.byref(ctrie), 0, G.stream()), "init")
        snaps = []
        for t in range(self.T - 1):
            _lib.check(self.step(st, ctrie, hidden[t], lse[t], t, 1 if t == 0 else self.K, None, ui), "search step")
            snaps.append({k: keep[k].clone() for k in STATE + ("error",)})
        seqs, scores, width = self.finalize(st, B)
        snaps = [{k: _raw(v).cpu() for k, v in s.items()} for s in snaps]
        return dict(snaps=snaps, seqs=seqs, scores=_raw(scores), width=width, error=int(keep["error"][0]))

    def batch(self, ui=None):
        return self.search(self.B, self.ctrie, self.hidden, self.lse, ui, self.scratch)

    def user_reference(self, b, keep):
        """user b ALONE on FlatTrie(Trie(A_b)) with the unfiltered kernels, fed cloned slices of the batch's hidden and lse rows"""
        from gram_amd.utils import generation_trie as gt
        K = self.K
        key = tuple(keep)
        if key not in self._user_tries:
            self._user_tries[key] = gt.FlatTrie(gt.Trie([self.cands[i] for i in keep]))
        ctrie, _keep_alive = self._user_tries[key].to_device(torch.device(self.G.DEV))
        rows = [slice(b, b + 1) if t == 0 else slice(b * K, (b + 1) * K) for t in range(self.T - 1)]
        return self.search(1, ctrie, [h[r].clone() for h, r in zip(self.hidden, rows)], [l[r].clone() for l, r in zip(self.lse, rows)])

    def items_of(self, seqs):
        """[B][<= K] candidate indices of returned sequences, in their order (fillers and repeats left out)"""
        out = []
        for b in range(seqs.shape[0] // self.K):
            got = []
            for row in seqs[b * self.K:(b + 1) * self.K].tolist():
                while row and row[-1] == 0:
                    row.pop()
                i = self.index.get(tuple(row), -1)
                if i >= 0 and i not in got:
                    got.append(i)
            out.append(got)
        return out


def _expected(refs, t, key, K):
    """the batch's state array after step t, put together from the one-user references: rows side by side; the ancestor table
    holds row numbers, so user b's are b * K further on -- but for slot 0, which the compact step 0 fills with the USER index"""
    if key != "anc":
        return torch.cat([r["snaps"][t][key] for r in refs], 0)
    parts = []
    for b, r in enumerate(refs):
        a = r["snaps"][t]["anc"].clone()
        a[0] += b
        a[1:] += b * K
        parts.append(a)
    return torch.cat(parts, 1)


def _assert_equals_references(case, got, refs, tag):
    K, flat = case.K, case.flat
    assert got["error"] == 0 and all(r["error"] == 0 for r in refs), tag
    for t, s in enumerate(got["snaps"]):
        assert int(s["error"][0]) == 0 and all(int(r["snaps"][t]["error"][0]) == 0 for r in refs), (tag, t)
        for key in STATE:
            if key == "node":
                continue
            want = _expected(refs, t, key, K)
            if not torch.equal(s[key], want):
                bad = [b for b in range(case.B) if not torch.equal(_of_user(s[key], key, b, K), _of_user(want, key, b, K))]
                raise AssertionError((tag, "step", t, key, "users", bad[:8], _of_user(s[key], key, bad[0], K), _of_user(want, key, bad[0], K)))
        # node ids of two Tries: where the reference sits on a node, the batch sits on the shared Trie's node of the same prefix
        ref_node = _expected(refs, t, "node", K).tolist()
        seq = s["seq"].tolist()
        want = [-1 if rn < 0 else flat.leaf_of(seq[r][: t + 2]) for r, rn in enumerate(ref_node)]
        node = s["node"].tolist()
        assert node == want, (tag, "step", t, "node", [r for r in range(len(want)) if node[r] != want[r]][:8])
        assert [x == -1 for x in node] == [x < 0 for x in ref_node], (tag, t)
    assert got["width"] == max(r["width"] for r in refs), tag
    assert torch.equal(got["seqs"], torch.cat([r["seqs"] for r in refs])), tag
    assert torch.equal(got["scores"], torch.cat([r["scores"] for r in refs])), tag


def _assert_not_vacuous(case, got, plain, keep, top, tag):
    """users that filter nothing: the unfiltered shared-Trie run bit for bit, every step; users that lose an item of their
    unfiltered result: another result; nobody gets an excluded item"""
    B, K, n = case.B, case.K, len(case.cands)
    lost = 0
    for b in range(B):
        rows = slice(b * K, (b + 1) * K)
        same = torch.equal(got["seqs"][rows], plain["seqs"][rows]) and torch.equal(got["scores"][rows], plain["scores"][rows])
        if len(keep[b]) == n:
            assert same, (tag, b)
            for t, (s, p) in enumerate(zip(got["snaps"], plain["snaps"])):
                for key in STATE:
                    assert torch.equal(_of_user(s[key], key, b, K), _of_user(p[key], key, b, K)), (tag, b, t, key)
        gone = set(range(n)) - set(keep[b])
        if gone & set(top[b]):
            lost += 1
            assert not same, (tag, b)
        elif case.name not in ("second300", "beauty"):
            assert b % 8 in (0, 5, 6) or len(top[b]) < 2, (tag, b, "the list misses the user's unfiltered result")
    assert lost >= min(B, 8) // 2 or case.name in ("second300", "beauty"), tag
    assert lost >= 1, tag
    for b, items in enumerate(case.items_of(got["seqs"])):
        assert set(items) <= set(keep[b]), (tag, b)


def _world(G, name, B, K, pieces, scratch):
    """case, its unfiltered run, and the users' lists made from that run's results"""
    case = _Case(G, name, B, K, pieces, scratch, seed=1000 * B + 10 * K + pieces)
    plain = case.batch()
    assert plain["error"] == 0
    top = case.items_of(plain["seqs"])
    assert all(len(t) >= 1 for t in top)
    lists = exclude_lists(name, case.cands, B, top, seed=B + K)
    return dict(case=case, plain=plain, top=top, lists=lists, keep=keep_sets(case.cands, lists))


def _filtered(G, w, mode):
    """the batch's filtered run in one mode, its lists prepared by gram_user_items_prepare"""
    from gram_amd import _lib
    case = w["case"]
    allow = mode == "allow"
    if allow and case.name == "beauty":
        return None  # (the complement of 4 096 exclusions among 12 101 items is no list of at most 4 096)
    lists = allow_lists(w["keep"]) if allow else w["lists"]
    ui, t = G.user_items(case.flat, case.cands, lists, _lib.ITEMS_ALLOW if allow else _lib.ITEMS_EXCLUDE)
    ranks = case.flat.item_ranks(case.cands)
    assert t["count"].tolist() == [len({int(ranks[i]) for i in r if i >= 0}) for r in lists]
    return ui, t


SEARCH_CASES = [
    # Trie, B, K, pieces, scratch                what it reaches
    ("ragged", 8, 4, 1, True),                 # sparse_logits_kernel + <1024>, users finishing early
    ("ragged", 8, 4, 2, True),
    ("ragged", 8, 4, 1, False),                # <1024> with in-kernel dots
    ("ragged", 8, 4, 2, False),
    ("ragged", 24, 12, 1, False),              # B in 17 .. 128; K >= the number of items
    ("ragged", 24, 12, 2, False),
    ("uniform", 129, 4, 1, False),             # <256> one-shot
    ("uniform", 129, 4, 2, False),
    ("narrow_root", 130, 20, 2, False),        # <256>, P = 64
    ("grid16", 8, 64, 1, True),                # P = 128, lists of thousands of ranks: 12-level searches; user 3 keeps 3 of 4 096
    ("grid16", 8, 64, 2, True),
    ("grid16", 129, 20, 2, False),             # <256> with long lists
    ("second300", 2, 64, 1, False),            # chunked by its shape: beam_step_chunked_kernel<1024, gram_user_items_t>
    ("second300", 2, 64, 2, False),
    ("root900", 129, 20, 2, False),            # beam_step_chunked_kernel<256, gram_user_items_t>: step 0's shared row over several chunk rounds
    ("beauty", 2, 20, 2, True),                # real fan-out 255; 4 096 exclusions per user
]


@gpu
@pytest.mark.parametrize("name,B,K,pieces,scratch", SEARCH_CASES)
def test_filtered_search_equals_per_user_tries(G, name, B, K, pieces, scratch):
    """User b with remaining candidates A_b gets what the unfiltered kernel returns for that user alone on Trie(A_b): tokens,
    beam_scores, seq, anc, done, n_hyps, hyp_score, worst, hyp_len, hyp_tok after EVERY step and the final sequences and scores are
    compared as integers, node through the host walk of the shared Trie, error[0] == 0 on both sides.  Both modes share the
    reference (the allow lists are the complements)."""
    w = _world(G, name, B, K, pieces, scratch)
    case = w["case"]
    refs = [case.user_reference(b, w["keep"][b]) for b in range(B)]
    if name in ("second300", "root900"):
        assert is_wide(K, case.flat.max_fanout, case.T)
    else:
        assert not is_wide(K, case.flat.max_fanout, case.T)
    if name == "grid16":
        assert max(len(r) for r in w["lists"]) >= 4095 and {1, 3} <= {len(k) for k in w["keep"]}
    for mode in ("exclude", "allow"):
        prepared = _filtered(G, w, mode)
        if prepared is None:
            continue
        got = case.batch(prepared[0])
        tag = (name, B, K, pieces, scratch, mode)
        _assert_equals_references(case, got, refs, tag)
        _assert_not_vacuous(case, got, w["plain"], w["keep"], w["top"], tag)


def _candidate_counts(case, snaps):
    """candidates per user of every step of a search (tests/test_gpu_wide_trie.py::_Search.candidate_counts)"""
    fan = np.diff(case.flat.child_off)
    out = [case.K * int(fan[int(case.flat.child_node[0])])]
    for s in snaps[:-1]:
        node = s["node"].numpy().reshape(case.B, case.K)
        per = np.where(node >= 0, fan[np.maximum(node, 0)], 0).sum(1)
        out.append(int(np.where(s["done"].numpy().astype(bool), 0, per).max()))
    return out


@gpu
@pytest.mark.parametrize("name,B,K,pieces,scratch", [c for c in SEARCH_CASES if c[:3] in (("ragged", 8, 4), ("grid16", 8, 64)) and c[4]])
def test_filtered_search_forced_chunked_matches_one_shot(G, name, B, K, pieces, scratch):
    """beam_step_chunked_kernel<..., gram_user_items_t> forced onto shapes the one-shot kernel takes, at chunk capacities on and around the search's
    own candidate counts: the bits of the one-shot filtered run after every step, node and error included"""
    from tests.test_gpu_wide_trie import _boundary_caps
    w = _world(G, name, B, K, pieces, scratch)
    case = w["case"]
    L_ = G.lib()
    for mode in ("exclude", "allow"):
        ui, _keep = _filtered(G, w, mode)
        one = case.batch(ui)
        counts = _candidate_counts(case, one["snaps"])
        caps = _boundary_caps(counts)
        print(f"\n[filtered, forced chunking] {name} K={K} pieces={pieces} {mode}: candidates per step {counts}, capacities {caps}")
        assert max(counts) > 2
        for cap in caps:
            try:
                assert L_.gram_debug_set_beam_chunked(1) == 0 and L_.gram_debug_set_beam_chunk_capacity(cap) == 0
                got = case.batch(ui)
            finally:
                L_.gram_debug_set_beam_chunked(-1)
                L_.gram_debug_set_beam_chunk_capacity(0)
            for t, (a, b) in enumerate(zip(one["snaps"], got["snaps"])):
                for key in STATE + ("error",):
                    assert torch.equal(a[key], b[key]), (mode, cap, t, key)
            assert got["error"] == one["error"] == 0
            assert torch.equal(got["seqs"], one["seqs"]) and torch.equal(got["scores"], one["scores"]) and got["width"] == one["width"]


@gpu
@pytest.mark.parametrize("name,B,K,pieces", [("ragged", 8, 4, 1), ("ragged", 8, 4, 2), ("rand", 5, 20, 2)])
def test_filtered_step_live_matches_all_rows(G, name, B, K, pieces):
    """tests/test_gpu_live_rows.py::test_beam_step_live_matches_all_rows with the lists: at every step t >= 1 the state is stepped
    twice, by the filtered all-rows call and by the filtered rowpos form on hidden[rows] / lse[rows] of gram_live_rows' rows (NaN
    behind them) -- every state array bit-identical, error flag clear, and some step runs on a strict subset of the rows."""
    from gram_amd import _lib
    case = _Case(G, name, B, K, pieces, True, seed=77 + B + K + pieces)
    top = case.items_of(case.batch()["seqs"])
    lists = exclude_lists(name, case.cands, B, top, seed=5)
    L_ = G.lib()
    R = B * K
    for mode, ls in ((_lib.ITEMS_EXCLUDE, lists), (_lib.ITEMS_ALLOW, allow_lists(keep_sets(case.cands, lists)))):
        ui, _keep = G.user_items(case.flat, case.cands, ls, mode)
        st_a, a = G.make_beam_state(B, K, case.T, cand_scratch=True)
        st_b, b = G.make_beam_state(B, K, case.T, cand_scratch=True)
        _lib.check(L_.gram_beam_init(C.byref(st_a), C.byref(case.ctrie), 0, G.stream()), "init")
        n_live = []
        for t in range(case.T - 1):
            h, lse = case.hidden[t], case.lse[t]
            if t == 0:
                _lib.check(case.step(st_a, case.ctrie, h, lse, 0, 1, None, ui), "step 0")
                continue
            for k in STATE + ("error",):
                b[k].copy_(a[k])
            rows, rowpos, _users = G.device_live_rows(st_a, case.ctrie)
            n = rows.numel()
            n_live.append(n)
            _lib.check(case.step(st_a, case.ctrie, h, lse, t, K, None, ui), "all rows")
            if n == 0:  # nothing to decode: gram_generate launches nothing either
                continue
            h_live, lse_live = torch.full_like(h, float("nan")), torch.full_like(lse, float("nan"))
            h_live[:n], lse_live[:n] = h[rows.long()], lse[rows.long()]
            _lib.check(case.step(st_b, case.ctrie, h_live, lse_live, t, K, rowpos, ui), "live rows")
            torch.cuda.synchronize()
            for k in STATE:
                assert torch.equal(_raw(a[k]), _raw(b[k])), (mode, t, k)
            assert int(a["error"][0]) == 0 and int(b["error"][0]) == 0, (mode, t)
        print(f"\n[filtered live step] {name} B={B} K={K} mode {mode}: live rows per step {n_live} of {R}")
        assert any(0 < n < R for n in n_live)


# ------------------------------------------------------------------------------------ 3. against the CPU oracle
def _oracle_filtered(cands, keep, logits, B, K, T):
    fns = [O.prefix_allowed_tokens_fn(O.Trie([cands[i] for i in kp])) for kp in keep]
    it = iter(logits)
    return O.beam_search(lambda tok: next(it), lambda idx: None, B, K, T, lambda b, s: fns[b](b, s), 1.0, early_exit=False)


@gpu
@pytest.mark.parametrize("name,K", [("ragged", 4), ("ragged", 12), ("grid8", 20)])
def test_filtered_search_vs_oracle(G, name, K):
    """O.beam_search with a per-user callback over O.Trie(A_b) on logits made in fp64 from the very operands the device reads:
    equal sequences, scores within 2e-5 (the project's bound between its dense and sparse steps,
    test_beam_step_sparse_equals_dense).  Every user keeps at least K items (at 'ragged' K = 12 that is every item: the lists are
    padding and nothing else), since scores near -1e9 have a 64-wide ulp.  A seed whose oracle result rests on a near-tie -- other
    sequences once every logit is moved by up to 1e-5 -- is passed over on the CPU, before the device is asked."""
    from gram_amd import _lib
    B = 5
    for seed in (1, 2, 3, 4, 5, 6):
        case = _Case(G, name, B, K, 2, True, seed)
        E = case.E32.double().cpu()
        logits = [(G.join_inter(h).cpu() @ E.T).float() for h in case.hidden]
        logits[0] = logits[0].repeat_interleave(K, 0)
        everything = [list(range(len(case.cands)))] * B
        top = case.items_of(_oracle_filtered(case.cands, everything, logits, B, K, case.T)[0])
        lists = exclude_lists(name, case.cands, B, top, seed=seed, min_keep=K)
        keep = keep_sets(case.cands, lists)
        assert all(len(kp) >= K for kp in keep)
        seqs, scores = _oracle_filtered(case.cands, keep, logits, B, K, case.T)
        g = torch.Generator().manual_seed(100 + seed)
        noisy = [lg + (torch.rand(lg.shape, generator=g) * 2 - 1) * 1e-5 for lg in logits]
        seqs2, scores2 = _oracle_filtered(case.cands, keep, noisy, B, K, case.T)
        if seqs2.tolist() == seqs.tolist():
            break
        print(f"\n[filtered vs oracle] {name} K={K}: seed {seed} rests on a near-tie, taking the next")
    else:
        raise AssertionError("no seed without a near-tie")
    ui, _keep = G.user_items(case.flat, case.cands, lists, _lib.ITEMS_EXCLUDE)
    got = case.batch(ui)
    assert got["error"] == 0
    assert got["seqs"][:, : got["width"]].tolist() == seqs.tolist()
    dscores = got["scores"].view(torch.float32)
    worst = float((dscores - scores).abs().max())
    print(f"\n[filtered vs oracle] {name} K={K} seed {seed}: max |score - oracle score| = {worst:.3e} "
          f"(oracle under 1e-5 logit noise: {float((scores2 - scores).abs().max()):.3e})")
    assert torch.allclose(dscores, scores, atol=2e-5, rtol=0)


# ------------------------------------------------------------------------------------ 4. the greedy step
@gpu
@pytest.mark.parametrize("kind", ["randn", "int"])
@pytest.mark.parametrize("name", ["ragged", "grid16"])
def test_greedy_step_items_vs_oracle(G, name, kind):
    """gram_beam_init, gram_greedy_step_items at every step, gram_greedy_finalize on dense logits for 300 users against
    O.greedy_search with per-user callbacks over O.Trie(A_b): equal sequences and width, in both modes.  'int' logits (-3 .. 3) tie
    many children: the first maximum among the ALIVE children decides.  Users that exclude nothing get gram_greedy_step's result."""
    from gram_amd import _lib
    from gram_amd.utils import generation_trie as gt
    B = 300
    cands, V = trie_cands(name)
    index = {tuple(c): i for i, c in enumerate(cands)}
    flat = gt.FlatTrie(gt.Trie(cands))
    ctrie, _keep_trie = flat.to_device(torch.device(G.DEV))
    T = max(len(c) for c in cands)
    logits = make_logits(kind, T - 1, B, V, seed=len(name) + len(kind))
    dlogits = [lg.to(G.DEV).contiguous() for lg in logits]
    L_ = G.lib()

    def run(ui):
        st, keep = G.make_beam_state(B, 1, T)
        _lib.check(L_.gram_beam_init(C.byref(st), C.byref(ctrie), 0, G.stream()), "init")
        for t in range(T - 1):
            if ui is None:
                rc = L_.gram_greedy_step(C.byref(st), C.byref(ctrie), G.p(dlogits[t]), V, t + 1, G.stream())
            else:
                rc = L_.gram_greedy_step_items(C.byref(st), C.byref(ctrie), G.p(dlogits[t]), V, t + 1, C.byref(ui), G.stream())
            _lib.check(rc, "greedy step")
        seqs = torch.zeros(B, T, dtype=torch.int64, device=G.DEV)
        width = torch.zeros(4, dtype=torch.int32, device=G.DEV)
        _lib.check(L_.gram_greedy_finalize(C.byref(st), T, G.p(seqs), G.p(width), G.stream()), "greedy_finalize")
        torch.cuda.synchronize()
        return seqs.cpu(), int(width[0])

    def strip(row):
        while row and row[-1] == 0:
            row.pop()
        return tuple(row)

    plain, _w = run(None)
    top = [[index[strip(r)]] for r in plain.tolist()]
    lists = exclude_lists(name, cands, B, top, seed=9)
    keep = keep_sets(cands, lists)
    assert all(len(kp) >= 1 for kp in keep)
    fns = {}
    for kp in keep:
        if tuple(kp) not in fns:
            fns[tuple(kp)] = O.prefix_allowed_tokens_fn(O.Trie([cands[i] for i in kp]))
    it = iter(logits)
    ref = O.greedy_search(lambda tok: next(it), B, T, lambda b, s: fns[tuple(keep[b])](b, s))
    assert sum(strip(r) != strip(p) for r, p in zip(ref.tolist(), plain.tolist())) >= B // 4  # (the lists do change the result)
    for mode, ls in ((_lib.ITEMS_EXCLUDE, lists), (_lib.ITEMS_ALLOW, allow_lists(keep))):
        ui, _t = G.user_items(flat, cands, ls, mode)
        seqs, width = run(ui)
        assert width == ref.shape[1], mode
        assert seqs[:, :width].tolist() == ref.tolist(), mode
        assert not seqs[:, width:].any()
        for b in range(0, B, 8):
            assert seqs[b].tolist() == plain[b].tolist(), (mode, b)
        for b, row in enumerate(seqs.tolist()):
            assert index[strip(row)] in keep[b], (mode, b)


# ------------------------------------------------------------------------------------ 5. small things
def _one_step_world(G, pieces):
    """'ragged', 8 users, K = 4, lists whose stride is 8; the state after gram_beam_init"""
    from gram_amd import _lib
    case = _Case(G, "ragged", 8, 4, pieces, False, seed=31 + pieces)
    lists = [[b % 12, (b + 5) % 12, -1, (3 * b) % 12, 7, -1, 2, b % 12] for b in range(8)]
    ui, t = G.user_items(case.flat, case.cands, lists, _lib.ITEMS_EXCLUDE)
    assert ui.stride == 8
    return case, ui, t


def _two_steps(case, ui):
    """steps 0 (the shared row) and 1 from a fresh state -> the state after each, as integers"""
    from gram_amd import _lib
    G = case.G
    st, keep = G.make_beam_state(case.B, case.K, case.T)
    _lib.check(G.lib().gram_beam_init(C.byref(st), C.byref(case.ctrie), 0, G.stream()), "init")
    out = []
    for t in (0, 1):
        _lib.check(case.step(st, case.ctrie, case.hidden[t], case.lse[t], t, 1 if t == 0 else case.K, None, ui), "step")
        torch.cuda.synchronize()
        out.append({k: _raw(keep[k]).cpu() for k in STATE + ("error",)})
    return out


@gpu
@pytest.mark.parametrize("pieces", [1, 2])
def test_count_outside_its_range_is_clamped(G, pieces):
    """node_alive clamps count[b] to [0, stride]: -5 gives the bits of 0, stride + 100 those of stride (the user's whole row holds
    sorted distinct ranks, so every entry of it is a valid one), error[0] == 0"""
    case, ui, t = _one_step_world(G, pieces)
    stride = ui.stride
    t["ranks"][5] = torch.tensor([0, 2, 3, 5, 6, 8, 9, 11], dtype=torch.int32)  # 8 of the Trie's 12 leaf ranks
    count = t["count"].clone()
    count[2], count[5] = 0, stride
    t["count"].copy_(count)
    want = _two_steps(case, ui)
    assert all(int(s["error"][0]) == 0 for s in want)
    count[2], count[5] = -5, stride + 100
    t["count"].copy_(count)
    got = _two_steps(case, ui)
    for s, wnt in zip(got, want):
        for k in STATE + ("error",):
            assert torch.equal(s[k], wnt[k]), k
    # (the result does depend on these counts: 4 ranks for user 5 instead of 8 give another state)
    count[5] = 4
    t["count"].copy_(count)
    other = _two_steps(case, ui)
    assert any(not torch.equal(o[k], wnt[k]) for o, wnt in zip(other, want) for k in STATE)


@gpu
@pytest.mark.parametrize("pieces", [1, 2])
def test_argument_errors_leave_the_state_unchanged(G, pieces):
    """gram_beam_step_sparse_items / gram_beam_step_sparse_split_items: a null items, a null leaf_lo / leaf_hi / ranks / count, a
    stride of 0 or 4097, an unknown mode, rowpos with rows_per_user != K -> GRAM_E_ARG, and nothing of the state is touched"""
    from gram_amd import _lib
    case, ui, t = _one_step_world(G, pieces)
    st, keep = G.make_beam_state(case.B, case.K, case.T)
    _lib.check(G.lib().gram_beam_init(C.byref(st), C.byref(case.ctrie), 0, G.stream()), "init")
    torch.cuda.synchronize()
    before = {k: _raw(v).clone() for k, v in keep.items()}
    good = {f: getattr(ui, f) for f, _ in _lib.UserItems._fields_}
    bad = [dict(good, **{f: None}) for f in ("leaf_lo", "leaf_hi", "ranks", "count")]
    bad += [dict(good, stride=0), dict(good, stride=_lib.GRAM_MAX_USER_ITEMS + 1), dict(good, mode=2), dict(good, mode=-1)]
    rowpos = torch.arange(case.B * case.K, dtype=torch.int32, device=G.DEV)
    h, lse = case.hidden[0], case.lse[0]
    L_ = G.lib()
    a = (C.byref(st), C.byref(case.ctrie), G.p(h))

    def call(items, rpu=1, rp=None):
        if pieces == 2:
            return L_.gram_beam_step_sparse_split_items(*a, G.p(case.E32), case.d, G.p(lse), case.V, 1, rpu, G.p(rp), 2, items, G.stream())
        return L_.gram_beam_step_sparse_items(*a, G.p(case.W), case.d, G.p(lse), case.V, 1, rpu, G.p(rp), items, G.stream())

    assert call(None) == _lib.E_ARG
    for kw in bad:
        assert call(C.byref(_lib.UserItems(**kw))) == _lib.E_ARG, kw
    assert call(C.byref(ui), 1, rowpos) == _lib.E_ARG  # live rows: K rows per user
    assert call(C.byref(ui), 2, rowpos) == _lib.E_ARG
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(_raw(v), before[k]), k
    assert call(C.byref(ui)) == 0  # (and the good call is taken)
    torch.cuda.synchronize()
    assert int(keep["error"][0]) == 0 and not torch.equal(_raw(keep["tokens"]), before["tokens"])


# ------------------------------------------------------------------------------------ 1. gram_user_items_prepare on the device
@gpu
@pytest.mark.parametrize("M,stride", [(M, M) for M in PREPARE_M] + [(300, 4096)])
def test_user_items_prepare_against_numpy_unique(G, M, stride):
    """40 users of every list pattern in one launch: count[b] and ranks[b, :count[b]] are np.unique of the valid entries' ranks,
    and what lies behind a user's count still holds the -7 it was prefilled with"""
    from gram_amd import _lib
    rank = item_rank_table()
    rows, names = prepare_lists(M, rank, seed=M)
    B = rows.shape[0]
    items = torch.from_numpy(rows.astype(np.int32)).to(G.DEV)  # (built as int32 directly: ops.py would refuse the bad indices)
    rank_d = torch.from_numpy(rank).to(G.DEV)
    ranks = torch.full((B, stride), -7, dtype=torch.int32, device=G.DEV)
    count = torch.full((B,), -7, dtype=torch.int32, device=G.DEV)
    _lib.check(G.lib().gram_user_items_prepare(G.p(rank_d), N_ITEMS, G.p(items), B, M, G.p(ranks), G.p(count), stride, G.stream()), "prepare")
    torch.cuda.synchronize()
    ranks, count = ranks.cpu().numpy(), count.cpu().numpy()
    for b in range(B):
        ref = prepare_reference(rows[b], rank)
        assert count[b] == ref.size, (names[b], b, count[b], ref.size)
        assert np.array_equal(ranks[b, : ref.size], ref), (names[b], b)
        assert (ranks[b, ref.size:] == -7).all(), (names[b], b)


@gpu
def test_user_items_prepare_argument_errors(G):
    """stride < M, M < 1, stride > 4096 and n_items < 1: GRAM_E_ARG, the outputs left at -7"""
    from gram_amd import _lib
    rank_d = torch.from_numpy(item_rank_table()).to(G.DEV)
    items = torch.zeros(4, 4096, dtype=torch.int32, device=G.DEV)
    ranks = torch.full((4, 8192), -7, dtype=torch.int32, device=G.DEV)
    count = torch.full((4,), -7, dtype=torch.int32, device=G.DEV)
    prep = G.lib().gram_user_items_prepare
    for n_items, M, stride in ((N_ITEMS, 9, 8), (N_ITEMS, 0, 8), (N_ITEMS, -1, 8), (N_ITEMS, 8, 4097), (N_ITEMS, 4097, 4097), (0, 8, 8),
                               (-3, 8, 8)):
        assert prep(G.p(rank_d), n_items, G.p(items), 4, M, G.p(ranks), G.p(count), stride, G.stream()) == _lib.E_ARG, (n_items, M, stride)
    torch.cuda.synchronize()
    assert bool((ranks == -7).all()) and bool((count == -7).all())
    assert prep(G.p(rank_d), N_ITEMS, G.p(items), 4, 8, G.p(ranks), G.p(count), 8, G.stream()) == 0
    torch.cuda.synchronize()
    assert count.tolist() == [1 if item_rank_table()[0] >= 0 else 0] * 4
