"""-m gpu: the per-user item-mask kernels of gram_amd/csrc/beam.hip (gram_user_mask_t), driven directly
through the C ABI.

1. gram_user_mask_prepare against a numpy restatement of the record layout, at leaf counts around a word, around a wave's ballot and
   above what one workgroup pass covers (PASS_LEAVES), with unnamed leaves, a sliced mask and a poisoned record surplus;
2. gram_beam_step_sparse_mask: for sets a list can say (<= 4096 kept), the whole beam state after every step is ``torch.equal`` to
   the list form's in allow mode (gram_beam_step_sparse_items / _split_items) at every launch form
   tests/test_gpu_user_items_kernels.py names -- the machinery of that module drives both;
3. gram_greedy_step_mask against gram_greedy_step_items;
4. the argument errors with a real state behind them.

No tolerance anywhere: a dead candidate only removes a key from a selection of unique, totally ordered keys, and both forms call
the same candidates dead."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import test_gpu_user_items_kernels as UK
from tests.test_wide_trie_host import is_wide, make_logits

pytestmark = pytest.mark.gpu

STATE = UK.STATE
PASS_LEAVES = 1024  # kMaskPassLeaves of user_mask_prepare_kernel: leaves one workgroup pass covers (4 waves x 4 ballots of 64)
POISON = -559038737  # 0xdeadbeef


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    return gpu_util


# ------------------------------------------------------------------------------------ 1. the preparation kernel
def records_reference(mask, leaf_item, n_items):
    """mask u8 [B][n_items], leaf_item [n_leaves] -> (bits u32 [B][W], before u32 [B][W], count [B]), W = n_leaves / 32 + 1: bit j of
    word w = leaf 32 w + j is named by a candidate inside [0, n_items) whose byte is non-zero; before = the kept leaves in the
    words in front"""
    B, n_leaves = mask.shape[0], leaf_item.size
    W = n_leaves // 32 + 1
    named = (leaf_item >= 0) & (leaf_item < n_items)
    bit = np.zeros((B, W * 32), dtype=bool)
    bit[:, :n_leaves] = named[None, :] & (mask[:, np.clip(leaf_item, 0, n_items - 1)] != 0)
    bit = bit.reshape(B, W, 32)
    bits = (bit.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    pop = bit.sum(-1)
    before = (np.cumsum(pop, 1) - pop).astype(np.uint32)
    return bits, before, pop.sum(1).astype(np.int32)


def mask_rows(kind, n_items, leaf_item, rng):
    """three users' rows of one kind"""
    m = np.zeros((3, n_items), dtype=np.uint8)
    if kind == "zeros_ones_first":  # all zero, all one (any non-zero byte), only the first leaf
        m[1] = rng.integers(1, 256, n_items)
        m[2, leaf_item[0]] = 1
    elif kind == "last_half_sparse":  # only the last leaf, random at densities 0.5 and 0.01
        m[0, leaf_item[-1]] = 255
        m[1] = rng.random(n_items) < 0.5
        m[2] = (rng.random(n_items) < 0.01) * 7
    return m


@pytest.mark.parametrize("kind", ["zeros_ones_first", "last_half_sparse"])
@pytest.mark.parametrize("n_leaves", [1, 31, 32, 33, 63, 64, 65, 4097, PASS_LEAVES + 1, 3 * PASS_LEAVES])
def test_user_mask_prepare_against_numpy(G, n_leaves, kind):
    """B = 3 users in one launch.  Unnamed leaves (leaf_item = -1, and an index >= n_items) are dropped; the mask is a column slice
    of a wider tensor (row stride > n_items, rows not aligned); the record rows are 3 longer than needed and their surplus, poisoned
    beforehand, is found untouched; count = the row's kept leaves; a second run writes the same words.  PASS_LEAVES + 1 needs a
    second pass of the user's workgroup for one leaf; 3 * PASS_LEAVES one for the last record alone."""
    from gram_amd import _lib
    rng = np.random.default_rng(n_leaves * 7 + len(kind))
    n_items = n_leaves + 5
    leaf_item = rng.permutation(n_items)[:n_leaves].astype(np.int32)
    if n_leaves >= 31:  # some leaves that no candidate names (never the first and the last)
        inner = rng.choice(np.arange(1, n_leaves - 1), max(2, n_leaves // 16), replace=False)
        leaf_item[inner[0::2]] = -1
        leaf_item[inner[1::2]] = n_items + rng.integers(0, 3, inner[1::2].size)
    m = mask_rows(kind, n_items, leaf_item, rng)
    bits, before, count = records_reference(m, leaf_item, n_items)
    if kind == "zeros_ones_first":
        assert count.tolist() == [0, int(((leaf_item >= 0) & (leaf_item < n_items)).sum()), 1]
    else:
        assert count[0] == 1 and bits[0, (n_leaves - 1) // 32] == 1 << ((n_leaves - 1) % 32)
    L_ = G.lib()
    W = n_leaves // 32 + 1
    assert L_.gram_user_mask_words(n_leaves) == W
    stride = W + 3
    wide = torch.full((3, n_items + 13), 9, dtype=torch.uint8, device=G.DEV)
    dmask = wide[:, 7:7 + n_items]
    dmask.copy_(torch.from_numpy(m))
    dleaf = torch.from_numpy(leaf_item).to(G.DEV)
    runs = []
    for _ in range(2):
        words = torch.full((3, stride, 2), POISON, dtype=torch.int32, device=G.DEV)
        cnt = torch.full((3,), -7, dtype=torch.int32, device=G.DEV)
        _lib.check(L_.gram_user_mask_prepare(dmask.data_ptr(), dmask.stride(0), 3, n_items, G.p(dleaf), n_leaves, G.p(words), stride,
                                             G.p(cnt), G.stream()), "gram_user_mask_prepare")
        torch.cuda.synchronize()
        runs.append((words.cpu(), cnt.cpu()))
    words, cnt = runs[0]
    assert torch.equal(words, runs[1][0]) and torch.equal(cnt, runs[1][1])
    w = words.numpy().view(np.uint32)
    assert np.array_equal(w[:, :W, 0], bits), [b for b in range(3) if not np.array_equal(w[b, :W, 0], bits[b])]
    assert np.array_equal(w[:, :W, 1], before)
    assert (words[:, W:] == POISON).all()
    assert cnt.tolist() == count.tolist()
    assert (w[:, W - 1, 0] >> np.uint32(n_leaves % 32) == 0).all()  # ranks >= n_leaves: 0


def test_user_mask_prepare_argument_errors(G):
    """GRAM_E_ARG leaves the outputs at their prefill, and the good call is taken afterwards"""
    from gram_amd import _lib
    n = 70
    dmask = torch.ones(2, n, dtype=torch.uint8, device=G.DEV)
    dleaf = torch.arange(n, dtype=torch.int32, device=G.DEV)
    words = torch.full((2, 4, 2), POISON, dtype=torch.int32, device=G.DEV)
    cnt = torch.full((2,), -7, dtype=torch.int32, device=G.DEV)
    prep = G.lib().gram_user_mask_prepare
    for stride_m, B, n_items, n_leaves, stride in ((n - 1, 2, n, n, 3), (n, 0, n, n, 3), (n, 2, 0, n, 3), (n, 2, n, 0, 3), (n, 2, n, n, 2),
                                                   (n, 2, n, -1, 3)):
        assert prep(G.p(dmask), stride_m, B, n_items, G.p(dleaf), n_leaves, G.p(words), stride, G.p(cnt), G.stream()) == _lib.E_ARG
    torch.cuda.synchronize()
    assert bool((words == POISON).all()) and cnt.tolist() == [-7, -7]
    assert prep(G.p(dmask), n, 2, n, G.p(dleaf), n, G.p(words), 4, G.p(cnt), G.stream()) == 0
    torch.cuda.synchronize()
    assert cnt.tolist() == [n, n] and words[:, :3, 1].tolist() == [[0, 32, 64]] * 2 and bool((words[:, 3] == POISON).all())


# ------------------------------------------------------------------------------------ 2. the search step
def user_mask(G, flat, cands, keep):
    """B sets of candidate indices -> (gram_user_mask_t, keep-alive tensors): a (B, n) uint8 mask through gram_user_mask_prepare on
    the current stream.  (UK.keep_sets keeps or drops the spellings of one sequence together: no folding is needed.)"""
    from gram_amd import _lib
    dev = torch.device(G.DEV)
    B, n = len(keep), len(cands)
    m = np.zeros((B, n), dtype=np.uint8)
    for b, kp in enumerate(keep):
        m[b, list(kp)] = 1
    lo, hi = flat.leaf_ranges_on(dev)
    leaf_item = flat.leaf_items_on(dev, cands)
    n_leaves = leaf_item.numel()
    assert n_leaves == int(flat.leaf_ranges()[1][0])
    stride = int(G.lib().gram_user_mask_words(n_leaves))
    t = dict(lo=lo, hi=hi, leaf_item=leaf_item, mask=torch.from_numpy(m).to(dev),
             words=torch.full((B, stride, 2), POISON, dtype=torch.int32, device=dev), count=torch.full((B,), -7, dtype=torch.int32, device=dev))
    _lib.check(G.lib().gram_user_mask_prepare(G.p(t["mask"]), n, B, n, G.p(leaf_item), n_leaves, G.p(t["words"]), stride, G.p(t["count"]),
                                              G.stream()), "gram_user_mask_prepare")
    return _lib.UserMask(G.p(lo), G.p(hi), G.p(t["words"]), stride, n_leaves), t


class _Case(UK._Case):
    """tests/test_gpu_user_items_kernels.py's search problem with a third kind of step: ``ui`` a gram_user_mask_t"""

    def step(self, st, ctrie, h, lse, t, rpu, rowpos=None, ui=None):
        from gram_amd import _lib
        if not isinstance(ui, _lib.UserMask):
            return super().step(st, ctrie, h, lse, t, rpu, rowpos, ui)
        G = self.G
        lm16 = G.p(self.W) if self.pieces == 1 else None  # (as generate.hip's search_step: both tables of a one-piece model)
        return G.lib().gram_beam_step_sparse_mask(C.byref(st), C.byref(ctrie), G.p(h), lm16, G.p(self.E32), self.d, G.p(lse), self.V, t + 1,
                                                  rpu, G.p(rowpos), self.pieces, C.byref(ui), G.stream())


def _world(G, name, B, K, pieces, scratch):
    """case, its unfiltered run, the users' sets made from that run's results (UK.exclude_lists' eight kinds: among them a user whose
    set kills an inner node -- kind 2 -- and users that keep 3 items and 1 item, fewer than K -- kinds 3 and 4), both filters"""
    from gram_amd import _lib
    case = _Case(G, name, B, K, pieces, scratch, seed=1000 * B + 10 * K + pieces)
    plain = case.batch()
    assert plain["error"] == 0
    top = case.items_of(plain["seqs"])
    keep = UK.keep_sets(case.cands, UK.exclude_lists(name, case.cands, B, top, seed=B + K))
    assert all(1 <= len(kp) <= 4096 for kp in keep)
    ui, t_items = G.user_items(case.flat, case.cands, UK.allow_lists(keep), _lib.ITEMS_ALLOW)
    um, t_mask = user_mask(G, case.flat, case.cands, keep)
    torch.cuda.synchronize()
    ranks = case.flat.item_ranks(case.cands)
    assert t_mask["count"].tolist() == [len({int(ranks[i]) for i in kp}) for kp in keep] == t_items["count"].tolist()
    return dict(case=case, plain=plain, top=top, keep=keep, ui=ui, um=um, alive=(t_items, t_mask))


def _assert_same_run(a, b, tag):
    for t, (x, y) in enumerate(zip(a["snaps"], b["snaps"])):
        for key in STATE + ("error",):
            assert torch.equal(x[key], y[key]), (tag, "step", t, key)
    assert a["error"] == b["error"] == 0, tag
    assert torch.equal(a["seqs"], b["seqs"]) and torch.equal(a["scores"], b["scores"]) and a["width"] == b["width"], tag


MASK_CASES = [
    # Trie, B, K, pieces, scratch                what it reaches (the <..., gram_user_mask_t> instantiations)
    ("ragged", 8, 4, 1, True),                 # B <= 16 with cand_logits scratch: sparse_logits_kernel + beam_step_kernel<1024>
    ("ragged", 8, 4, 2, True),
    ("ragged", 8, 4, 2, False),                # <1024> with in-kernel dots: the dead flag parked in bit 63
    ("ragged", 24, 12, 1, False),              # B in 17 .. 128; K >= the number of items
    ("ragged", 24, 12, 2, False),
    ("uniform", 129, 4, 1, False),             # B >= 129: beam_step_kernel<256>
    ("narrow_root", 130, 20, 2, False),
    ("grid16", 8, 64, 2, True),                # 4 096 leaves: 129 records per user, sets of thousands; user 3 keeps 3, user 4 one
    ("second300", 2, 64, 1, False),            # chunked by its shape: beam_step_chunked_kernel<1024>
    ("root900", 129, 20, 2, False),            # beam_step_chunked_kernel<256>: step 0's shared row over several chunk rounds
]


@pytest.mark.parametrize("name,B,K,pieces,scratch", MASK_CASES)
def test_mask_step_equals_list_step(G, name, B, K, pieces, scratch):
    """Whole searches (step 0 on one row per user, then K rows per user), every state array after EVERY step, the error flag and
    the finalized sequences and scores: the mask form's bits are the allow-list form's.  Users that keep everything get the
    unfiltered run's rows, users that lose an item of their unfiltered result get other rows, nobody gets a dropped item."""
    w = _world(G, name, B, K, pieces, scratch)
    case = w["case"]
    assert is_wide(K, case.flat.max_fanout, case.T) == (name in ("second300", "root900"))
    want = case.batch(w["ui"])
    got = case.batch(w["um"])
    tag = (name, B, K, pieces, scratch)
    _assert_same_run(got, want, tag)
    UK._assert_not_vacuous(case, got, w["plain"], w["keep"], w["top"], tag)


@pytest.mark.parametrize("name,B,K,pieces", [("ragged", 8, 4, 1), ("ragged", 8, 4, 2), ("grid8", 5, 20, 2)])
def test_mask_step_forced_chunked_matches_list_step(G, name, B, K, pieces):
    """beam_step_chunked_kernel<..., gram_user_mask_t> forced onto shapes the one-shot kernel takes, at 7 fresh candidates per round and
    at capacities on and around the search's own candidate counts: the bits of the one-shot list run"""
    from tests.test_gpu_wide_trie import _boundary_caps
    w = _world(G, name, B, K, pieces, True)
    case = w["case"]
    one = case.batch(w["ui"])
    counts = UK._candidate_counts(case, one["snaps"])
    caps = sorted(set(_boundary_caps(counts)) | {7})
    print(f"\n[mask, forced chunking] {name} K={K} pieces={pieces}: candidates per step {counts}, capacities {caps}")
    L_ = G.lib()
    for cap in caps:
        try:
            assert L_.gram_debug_set_beam_chunked(1) == 0 and L_.gram_debug_set_beam_chunk_capacity(cap) == 0
            got = case.batch(w["um"])
        finally:
            L_.gram_debug_set_beam_chunked(-1)
            L_.gram_debug_set_beam_chunk_capacity(0)
        _assert_same_run(got, one, (name, cap))


@pytest.mark.parametrize("name,B,K,pieces", [("ragged", 8, 4, 1), ("ragged", 8, 4, 2), ("rand", 5, 20, 2)])
def test_mask_step_live_matches_list_step_on_all_rows(G, name, B, K, pieces):
    """The rowpos form: at every step t >= 1 the state is stepped twice, by the list form on all rows and by the mask form on
    hidden[rows] / lse[rows] of gram_live_rows' rows (NaN behind them) -- every state array bit-identical, the error flag clear, and
    some step runs on a strict subset of the rows"""
    from gram_amd import _lib
    case = _Case(G, name, B, K, pieces, True, seed=77 + B + K + pieces)
    top = case.items_of(case.batch()["seqs"])
    keep = UK.keep_sets(case.cands, UK.exclude_lists(name, case.cands, B, top, seed=5))
    ui, _k1 = G.user_items(case.flat, case.cands, UK.allow_lists(keep), _lib.ITEMS_ALLOW)
    um, _k2 = user_mask(G, case.flat, case.cands, keep)
    L_ = G.lib()
    R = B * K
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
        _lib.check(case.step(st_a, case.ctrie, h, lse, t, K, None, ui), "all rows, lists")
        if n == 0:
            continue
        h_live, lse_live = torch.full_like(h, float("nan")), torch.full_like(lse, float("nan"))
        h_live[:n], lse_live[:n] = h[rows.long()], lse[rows.long()]
        _lib.check(case.step(st_b, case.ctrie, h_live, lse_live, t, K, rowpos, um), "live rows, masks")
        torch.cuda.synchronize()
        for k in STATE:
            assert torch.equal(UK._raw(a[k]), UK._raw(b[k])), (t, k)
        assert int(a["error"][0]) == 0 and int(b["error"][0]) == 0, t
    assert any(0 < n < R for n in n_live), n_live


# ------------------------------------------------------------------------------------ 3. the greedy step
@pytest.mark.parametrize("name", ["ragged", "grid16"])
def test_greedy_step_mask_equals_greedy_step_items(G, name):
    """gram_beam_init, the greedy step at every step, gram_greedy_finalize on dense integer logits (-3 .. 3: many ties, the first
    maximum among the ALIVE children decides) for 300 users: the mask form's sequences and width are the allow-list form's, users
    that keep everything get gram_greedy_step's result, and the sets do change the result"""
    from gram_amd import _lib
    from gram_amd.utils import generation_trie as gt
    B = 300
    cands, V = UK.trie_cands(name)
    index = {tuple(c): i for i, c in enumerate(cands)}
    flat = gt.FlatTrie(gt.Trie(cands))
    ctrie, _keep_trie = flat.to_device(torch.device(G.DEV))
    T = max(len(c) for c in cands)
    dlogits = [lg.to(G.DEV).contiguous() for lg in make_logits("int", T - 1, B, V, seed=len(name))]
    L_ = G.lib()

    def run(f):
        st, keep = G.make_beam_state(B, 1, T)
        _lib.check(L_.gram_beam_init(C.byref(st), C.byref(ctrie), 0, G.stream()), "init")
        for t in range(T - 1):
            a = (C.byref(st), C.byref(ctrie), G.p(dlogits[t]), V, t + 1)
            if f is None:
                rc = L_.gram_greedy_step(*a, G.stream())
            elif isinstance(f, _lib.UserMask):
                rc = L_.gram_greedy_step_mask(*a, C.byref(f), G.stream())
            else:
                rc = L_.gram_greedy_step_items(*a, C.byref(f), G.stream())
            _lib.check(rc, "greedy step")
        seqs = torch.zeros(B, T, dtype=torch.int64, device=G.DEV)
        width = torch.zeros(4, dtype=torch.int32, device=G.DEV)
        _lib.check(L_.gram_greedy_finalize(C.byref(st), T, G.p(seqs), G.p(width), G.stream()), "greedy_finalize")
        torch.cuda.synchronize()
        return seqs.cpu(), int(width[0]), int(keep["error"][0])

    def strip(row):
        while row and row[-1] == 0:
            row.pop()
        return tuple(row)

    plain, _w, _e = run(None)
    top = [[index[strip(r)]] for r in plain.tolist()]
    keep = UK.keep_sets(cands, UK.exclude_lists(name, cands, B, top, seed=9))
    ui, _t1 = G.user_items(flat, cands, UK.allow_lists(keep), _lib.ITEMS_ALLOW)
    um, _t2 = user_mask(G, flat, cands, keep)
    want, got = run(ui), run(um)
    assert got[1] == want[1] and got[2] == want[2] == 0
    assert torch.equal(got[0], want[0])
    assert sum(strip(r) != strip(p) for r, p in zip(got[0].tolist(), plain.tolist())) >= B // 4
    for b, row in enumerate(got[0].tolist()):
        assert index[strip(row)] in keep[b], b
        if b % 8 == 0:
            assert torch.equal(got[0][b], plain[b]), b  # (strip shortened `row` in place)


# ------------------------------------------------------------------------------------ 4. argument errors behind a real state
@pytest.mark.parametrize("pieces", [1, 2])
def test_argument_errors_leave_the_state_unchanged(G, pieces):
    """gram_beam_step_sparse_mask: a null struct, a null leaf_lo / leaf_hi / words, n_leaves < 1, a stride below
    gram_user_mask_words(n_leaves), rowpos with rows_per_user != K -> GRAM_E_ARG and nothing of the state is touched; then the good
    call is taken.  The same for gram_greedy_step_mask on a K = 1 state."""
    from gram_amd import _lib
    case = _Case(G, "ragged", 8, 4, pieces, False, seed=31 + pieces)
    keep = [[b % 12, (b + 5) % 12, (3 * b) % 12] for b in range(8)]
    um, _t = user_mask(G, case.flat, case.cands, keep)
    L_ = G.lib()
    good = {f: getattr(um, f) for f, _ in _lib.UserMask._fields_}
    bad = [dict(good, **{f: None}) for f in ("leaf_lo", "leaf_hi", "words")]
    bad += [dict(good, n_leaves=0), dict(good, n_leaves=-3), dict(good, stride=0), dict(good, n_leaves=32 * um.stride)]
    rowpos = torch.arange(case.B * case.K, dtype=torch.int32, device=G.DEV)
    for K in (case.K, 1):
        st, keep_t = G.make_beam_state(case.B, K, case.T)
        _lib.check(L_.gram_beam_init(C.byref(st), C.byref(case.ctrie), 0, G.stream()), "init")
        torch.cuda.synchronize()
        before = {k: UK._raw(v).clone() for k, v in keep_t.items()}
        if K == 1:
            logits = torch.randn(case.B, case.V, generator=torch.Generator().manual_seed(3)).to(G.DEV)

            def call(m, rpu=1, rp=None):
                return L_.gram_greedy_step_mask(C.byref(st), C.byref(case.ctrie), G.p(logits), case.V, 1, m, G.stream())
        else:
            def call(m, rpu=1, rp=None):
                return case.step(st, case.ctrie, case.hidden[0], case.lse[0], 0, rpu, rp, m) if m is not None else \
                    L_.gram_beam_step_sparse_mask(C.byref(st), C.byref(case.ctrie), G.p(case.hidden[0]), None, G.p(case.E32), case.d,
                                                  G.p(case.lse[0]), case.V, 1, rpu, None, pieces, None, G.stream())
        assert call(None) == _lib.E_ARG
        for kw in bad:
            m = _lib.UserMask(**kw)
            assert (call(m) if K > 1 else call(C.byref(m))) == _lib.E_ARG, kw
        if K > 1:
            assert call(um, 1, rowpos) == _lib.E_ARG and call(um, 2, rowpos) == _lib.E_ARG  # live rows: K rows per user
        torch.cuda.synchronize()
        for k, v in keep_t.items():
            assert torch.equal(UK._raw(v), before[k]), (K, k)
        assert (call(um) if K > 1 else call(C.byref(um))) == 0  # (and the good call is taken)
        torch.cuda.synchronize()
        assert int(keep_t["error"][0]) == 0 and not torch.equal(UK._raw(keep_t["tokens"]), before["tokens"])
