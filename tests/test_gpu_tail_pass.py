"""-m gpu: the tail pass of generate (include/gram_hip.h, gram_generate_tail) against the same call decoded step by step.

Everything here is a comparison of raw bits (torch.equal).  Whole calls: sequences, scores and every array of the beam state after
every replayed step -- a call with max_length cut to t + 2 ends right behind the search step of position t, and the test hook
gram_debug_workspace_beam_state says where the workspace keeps the state.  The pass is forced with gram_debug_set_tail_pass(1): by
default calls this small decode step by step (gram_tail_pass_wanted) -- but for the calls of 2049 users, which the size rule itself
sends through the pass, and which reach the row counts of the persistent GEMM.  Kernels: the forest's tables against
tests/tail_oracle.py (more of that in tests/test_gpu_tail_forest.py); the entry cross-attention against
gram_cross_attn_decode_split on groups of K rows, on forests of up to 65 rows per user; the scatter of the level results.  (The
pass's self-attention is the step-wise kernel itself.)"""
import ctypes as C

import pytest
import torch

from tests.test_tail_pass_host import BRANCHY, BUSHY, CHAIN, RAGGED, WIDE

pytestmark = pytest.mark.gpu
SENT = 0x5A5A  # 16-bit sentinel pattern (a finite number in IEEE half and in bfloat16)
FEW = CHAIN[:6]  # six prefixes at d_tail: a search with 20 beams carries its -1e9 filler beams all the way


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    return gpu_util


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    monkeypatch.delenv("GRAM_TAIL_PASS", raising=False)
    yield
    from gram_amd import _lib
    lib = _lib.load()
    lib.gram_debug_set_tail_pass(-1)
    lib.gram_debug_set_tail_capacity(0)
    lib.gram_debug_set_live_rows(-1)


def _bits(t):
    return t.view(torch.int16)


def _model(G, pieces, heads=2):
    from tests.test_gpu_token_tables import _model as tiny
    return tiny(G, pieces, heads)


_FNS = {}


def _fn(cands):
    from gram_amd.utils import generation_trie as gt
    key = id(cands)
    if key not in _FNS:
        _FNS[key] = gt.prefix_allowed_tokens_fn(gt.Trie(cands))
    return _FNS[key]


STATE = ("tokens", "node", "beam_scores", "seq", "anc", "done", "n_hyps", "hyp_score", "worst", "hyp_len", "hyp_tok", "error")


def _run(G, m, ids, mask, cands, K, max_length, **kw):
    """one generate() on a zeroed workspace -> (sequences, scores, {beam-state array: raw bytes}, gram_debug_tail_last)"""
    from gram_amd import _lib
    from gram_amd.utils.generation_trie import FlatTrie, Trie
    # the larger of the two workspaces first, zeroed: both runs of a comparison then leave the same bytes in what they do not write
    B, N, L = ids.shape
    handle, steps = m._pack(), FlatTrie(Trie(cands)).tail_tables()[2]
    need = G.lib().gram_workspace_bytes(handle, B, N, L, K, max_length)
    if steps and K > 1:
        need = max(need, G.lib().gram_workspace_bytes_tail(handle, B, N, L, K, max_length, steps))
    m._ensure_workspace(need).zero_()
    out = m.generate(input_ids=ids.to(G.DEV), attention_mask=mask.to(G.DEV), max_length=max_length, prefix_allowed_tokens_fn=_fn(cands),
                     num_beams=K, num_return_sequences=K, length_penalty=1.0, **kw)
    torch.cuda.synchronize()
    last = (C.c_int32 * 4)()
    G.lib().gram_debug_tail_last(last)
    st = _lib.BeamState()
    _lib.check(G.lib().gram_debug_workspace_beam_state(handle, m._workspace.data_ptr(), B, N, L, K, max_length, C.byref(st)), "state")
    R, T, base = B * K, max_length, m._workspace.data_ptr()
    size = dict(tokens=4 * R, node=4 * R, beam_scores=4 * R, seq=4 * R * T, anc=4 * T * R, done=4 * B, n_hyps=4 * B,
                hyp_score=8 * B * (K + 1), worst=8 * B, hyp_len=4 * B * (K + 1), hyp_tok=4 * B * (K + 1) * T, error=4)
    state = {}
    for name in STATE:
        off = getattr(st, name) - base
        state[name] = m._workspace[off: off + size[name]].cpu().clone()
    sc = out["sequences_scores"]
    return out["sequences"].cpu(), None if sc is None else sc.cpu(), state, list(last)


def _inputs(B, N, L, pad_passage, seed):
    from tests.test_gpu_token_tables import _inputs as mk
    return mk(torch.Generator().manual_seed(seed), B, N, L, 256, pad_passage)


def _compare(G, m, ids, mask, cands, K, want_tail, live=-1, cuts=None, on=1, **kw):
    """tail pass on against off at every cut of max_length behind a replayed step (and the full call), or at the given cuts.
    on = None: the "on" runs come first and nobody touches the switch before them, so that the size rule decides
    (gram_tail_pass_wanted)."""
    from gram_amd.utils.generation_trie import FlatTrie, Trie
    lib = G.lib()
    d_tail = FlatTrie(Trie(cands)).tail_tables()[1]
    full = max(len(c) for c in cands)
    if cuts is None:
        cuts = range(max(d_tail, 2) + 1, full + 1) if want_tail else [full]
    ran, by_size = [], {}
    if on is None:
        lib.gram_debug_set_live_rows(live)
        by_size = {T: _run(G, m, ids, mask, cands, K, T, **kw) for T in cuts}
    for T in cuts:
        lib.gram_debug_set_live_rows(live)
        if on is not None:
            lib.gram_debug_set_tail_pass(on)
        seq_on, sc_on, st_on, last = by_size[T] if on is None else _run(G, m, ids, mask, cands, K, T, **kw)
        lib.gram_debug_set_tail_pass(0)
        seq_off, sc_off, st_off, last_off = _run(G, m, ids, mask, cands, K, T, **kw)
        ran.append(last[0])
        assert last_off[0] == 0
        assert torch.equal(seq_on, seq_off), T
        if K > 1:
            assert torch.equal(sc_on.view(torch.int32), sc_off.view(torch.int32)), T
        for name in STATE:
            assert torch.equal(st_on[name], st_off[name]), (name, T)
        assert int(st_on["error"].view(torch.int32)[0]) == 0
    if want_tail:
        assert all(r == 1 for r in ran) and last[1] >= 1 and last[2] >= 1
    else:
        assert not any(ran)
    return last


# ------------------------------------------------------------------------------------ 1. whole calls
@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("B,K,cands,pad,live", [(1, 4, CHAIN, False, -1), (3, 20, RAGGED, True, 1), (3, 20, RAGGED, False, 0),
                                               (17, 4, BRANCHY, True, -1), (3, 20, BRANCHY, False, -1), (3, 20, FEW, False, -1),
                                               (17, 20, RAGGED, False, -1)],
                         ids=["B1-K4-chain", "B3-K20-ragged-padded-passage-live", "B3-K20-ragged-live-off", "B17-K4-branchy-padded-passage",
                              "B3-K20-branchy", "B3-K20-fillers", "B17-K20-ragged"])
def test_generate_is_bit_identical_with_and_without_the_tail_pass(G, B, K, cands, pad, live, pieces):
    m = _model(G, pieces)
    ids, mask = _inputs(B, 2, 64, pad, 100 * B + K)
    last = _compare(G, m, ids, mask, cands, K, want_tail=True, live=live)
    if cands is FEW:  # six prefixes for 20 beams: the others are the -1e9 beams of HF's initial state, standing on the same six nodes
        assert last[1] == B * K * 4


@pytest.mark.parametrize("pieces", [2, 1])
def test_greedy_and_tailless_tries_decode_step_by_step(G, pieces):
    m = _model(G, pieces)
    ids, mask = _inputs(3, 2, 64, False, 7)
    _compare(G, m, ids, mask, CHAIN, 1, want_tail=False)  # K = 1: greedy search
    _compare(G, m, ids, mask, BUSHY, 4, want_tail=False)  # no depth qualifies: a Trie without a tail


@pytest.mark.parametrize("pieces", [2, 1])
def test_forest_over_capacity_goes_on_step_by_step(G, pieces):
    m = _model(G, pieces)
    ids, mask = _inputs(3, 2, 64, False, 9)
    G.lib().gram_debug_set_tail_capacity(5)
    last = _compare(G, m, ids, mask, RAGGED, 4, want_tail=False)
    assert last[1] > 5  # (the forest was counted, found too large and dropped)
    G.lib().gram_debug_set_tail_capacity(0)
    _compare(G, m, ids, mask, RAGGED, 4, want_tail=True)


@pytest.mark.parametrize("pieces", [2, 1])
def test_filtered_calls_are_routed_step_by_step(G, pieces):
    m = _model(G, pieces)
    ids, mask = _inputs(3, 2, 64, False, 11)
    lib = G.lib()
    outs = []
    for on in (1, 0):
        lib.gram_debug_set_tail_pass(on)
        o = m.generate(input_ids=ids.to(G.DEV), attention_mask=mask.to(G.DEV), max_length=max(len(c) for c in RAGGED),
                       prefix_allowed_tokens_fn=_fn(RAGGED), num_beams=4, num_return_sequences=4, length_penalty=1.0,
                       candidates=RAGGED, exclude_items=[[0, 1], [2], [5]])
        outs.append((o["sequences"].cpu(), o["sequences_scores"].cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))


@pytest.mark.parametrize("pieces", [2, 1])
def test_a_level_over_the_cache_rows_goes_on_step_by_step(G, pieces):
    """a group's level may hold as many rows as the cache has per position; the test hook lowers that so that a small forest is over it"""
    m = _model(G, pieces)
    ids, mask = _inputs(3, 2, 64, False, 13)
    G.lib().gram_debug_set_tail_level_capacity(7)  # (3 users x 4 beams: the even users' levels hold 8 rows, the forest itself fits)
    try:
        last = _compare(G, m, ids, mask, RAGGED, 4, want_tail=False)
        assert last[1] >= 8
    finally:
        G.lib().gram_debug_set_tail_level_capacity(0)
    _compare(G, m, ids, mask, RAGGED, 4, want_tail=True)


@pytest.mark.parametrize("pieces,heads", [(2, 2), (1, 4)])  # one layer's bank: 4 * B * heads * (N * L = 128) * 64 * pieces bytes
@pytest.mark.parametrize("cands,K,live", [(RAGGED, 20, 1), (BRANCHY, 4, 0)], ids=["ragged-K20-live", "branchy-K4-live-off"])
def test_the_size_rule_takes_the_pass_at_256_MB_of_bank_and_the_call_stays_bit_identical(G, cands, K, live, pieces, heads):
    """No switch and no environment variable for the "on" run: gram_tail_pass_wanted decides (generate.hip, tail_wanted).  2047 users
    hold one byte less than 256 MB of bank per layer, 2049 more.  At K = 20 the step's 40 980 rows and the forest's rows put every
    GEMM of the pass and the lm_head on the persistent ping-pong kernel, with an M tail; each level's cache rows serve both user
    groups in turn."""
    from gram_amd.utils.generation_trie import FlatTrie, Trie
    m, lib = _model(G, pieces, heads), G.lib()
    N, L, handle = 2, 64, m._pack()
    d_tail, full = FlatTrie(Trie(cands)).tail_tables()[1], max(len(c) for c in cands)
    assert lib.gram_tail_pass_wanted(handle, 2047, N, L) == 0 and lib.gram_tail_pass_wanted(handle, 2049, N, L) == 1
    ids, mask = _inputs(2049, N, L, False, 2049 + K)
    lib.gram_debug_set_live_rows(live)
    _seq, _sc, state, last = _run(G, m, ids[:2047], mask[:2047], cands, K, full)
    assert last == [0, 0, 0, 0] and int(state["error"].view(torch.int32)[0]) == 0  # (no forest was built)
    last = _compare(G, m, ids, mask, cands, K, want_tail=True, live=live, cuts=[d_tail + 2, full], on=None)
    assert last[0] == 1 and last[1] >= 2049 * K  # (every beam is live at d_tail)
    if K == 20:
        assert last[1] > 32768  # (the forest's GEMMs take the ping-pong kernel as the step's do)
    print(f"\nB=2049 K={K} pieces={pieces} heads={heads}: forest rows {last[1]}, entries {last[2]}, most rows of one user {last[3]}")


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("B,K,by_size", [(3, 20, False), (3, 40, False), (17, 20, False), (2049, 20, True)],
                         ids=["B3-K20-two-entries", "B3-K40-three-entries", "B17-K20", "B2049-K20-by-size"])
def test_a_forest_of_more_than_64_rows_per_user_is_bit_identical_to_stepping(G, B, K, by_size, pieces):
    """WIDE gives every beam four steps and 4 to 6 rows: 20 beams hold 80 to 120 forest rows -- two cross-attention entries per user,
    one full and one partial, as on the Beauty Trie -- and 40 beams three."""
    m = _model(G, pieces, 4 // pieces if by_size else 2)
    ids, mask = _inputs(B, 2, 64, False, 300 * B + K)
    if by_size:
        assert G.lib().gram_tail_pass_wanted(m._pack(), B, 2, 64) == 1
        last = _compare(G, m, ids, mask, WIDE, K, want_tail=True, cuts=[max(len(c) for c in WIDE)], on=None)
        print(f"\nB={B} K={K} pieces={pieces}: forest rows {last[1]}, entries {last[2]}, most rows of one user {last[3]}")
    else:
        last = _compare(G, m, ids, mask, WIDE, K, want_tail=True)
    if K == 20:
        assert 65 <= last[3] <= 128 and last[2] >= B + 1
    else:
        assert last[3] > 128 and last[2] >= 2 * B + 1


# ------------------------------------------------------------------------------------ 2. the forest and its self-attention
@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("table", [False, True])
def test_forest_tables_and_level_self_attention_equal_a_plain_enumeration_and_the_stepwise_kernel(G, table, pieces):
    """gram_tail_forest on a hand-made beam state over the Trie with forks below d_tail (four users: two even with live beams, one
    of them with a beam off the Trie, one odd, one finished): every table against a plain Python enumeration; then the pass's
    self-attention -- gram_dec_self_attn[_rows]_split per group and level on the rows gathered by slot, with the forest's own
    ancestor tables, the second group on the first's cache rows, gram_scatter_rows -- against the same kernel run level by level
    with a plain ancestor table in which every forest row owns a cache row (at most 64 rows), bit for bit."""
    from gram_amd import _lib
    from gram_amd.utils.generation_trie import FlatTrie, Trie
    from tests import tail_oracle
    flat = FlatTrie(Trie(BRANCHY))
    sub, d_tail, steps = flat.tail_tables()
    assert (d_tail, steps) == (3, 3)
    B, K, Tmax, H, V, cap = 4, 4, 8, 2, 256, 64
    R, t, inner = B * K, d_tail - 1, H * 64
    dev = torch.device(G.DEV)
    ctrie, _keep = flat.to_device(dev)
    sub_d = torch.from_numpy(sub).to(dev)
    tail = _lib.TrieTail(sub_d.data_ptr(), d_tail, steps)
    st, keep = G.make_beam_state(B, K, Tmax)
    g = torch.Generator().manual_seed(41 + pieces + 2 * table)
    # beams on prefixes of length 3: (0, 3, 41) forks at once, (0, 2, 40) one level down
    prefixes = [[(0, 2, 40), (0, 3, 41), None, (0, 4, 42)], [(0, 3, 41), (0, 5, 40), (0, 5, 41), (0, 7, 43)],
                [(0, 2, 40), (0, 2, 41), (0, 6, 40), (0, 3, 41)], [(0, 2, 40), (0, 2, 41), (0, 2, 42), (0, 2, 43)]]
    node = [[flat.leaf_of(p) if p else -1 for p in row] for row in prefixes]
    keep["node"].copy_(torch.tensor(node, dtype=torch.int32).flatten())
    keep["tokens"].copy_(torch.tensor([[p[-1] if p else 0 for p in row] for row in prefixes], dtype=torch.int32).flatten())
    keep["done"].copy_(torch.tensor([0, 0, 0, 1], dtype=torch.int32))  # (user 3 is finished: no rows)
    keep["anc"].copy_(torch.randint(0, R, (Tmax, R), generator=g).to(torch.int32))
    state = dict(node=keep["node"].cpu().numpy(), tokens=keep["tokens"].cpu().numpy(), done=keep["done"].cpu().numpy(),
                 anc=keep["anc"].cpu().numpy())
    f, ft, whole, layout = tail_oracle.forest_buffers(dev, B, K, Tmax, cap, steps)
    _lib.check(G.lib().gram_tail_forest(C.byref(st), C.byref(ctrie), C.byref(tail), C.byref(f), t, G.stream()), "gram_tail_forest")
    torch.cuda.synchronize()
    # ---- the plain enumeration (tests/tail_oracle.py): every cell of every table and the guard bands, then the tables one by one
    E = tail_oracle.enumerate_forest(flat, sub, state, B, K, t, cap, f.cap_entries, steps)
    tail_oracle.check_forest(E, whole, layout, state["anc"], Tmax)
    rows = list(zip(*(getattr(E, name).tolist() for name in tail_oracle.ROW_ARRAYS)))  # (token, pos, parent, root, node)
    user_off = E.user_off.tolist()
    assert user_off[4] == user_off[3] and all(r[4] >= 0 for r in rows)  # (the finished user owns no row; no row is a copy)
    n = len(rows)
    assert 20 <= n <= cap and any(r[1] > t and sum(1 for q in rows if q[2] == i) > 1 for i, r in enumerate(rows))  # (a fork below d_tail)
    counts = ft["counts"].cpu().tolist()
    assert counts[0] == n and ft["user_off"].cpu().tolist() == user_off
    for i, name in enumerate(("tokens", "pos", "parent", "root", "node")):
        assert ft[name][:n].cpu().tolist() == [r[i] for r in rows], name
    per_user = [user_off[b + 1] - user_off[b] for b in range(B)]
    assert counts[2] == max(per_user) and counts[1] == sum((c + 63) // 64 for c in per_user)
    ent_off = ft["ent_off"].cpu().tolist()
    assert ent_off == [sum((c + 63) // 64 for c in per_user[:b]) for b in range(B + 1)]
    for b in range(B):
        for e in range(ent_off[b], ent_off[b + 1]):
            assert int(ft["ent_users"][e]) == b
            want = [user_off[b] + 64 * (e - ent_off[b]) + s_ if 64 * (e - ent_off[b]) + s_ < per_user[b] else -1 for s_ in range(64)]
            assert ft["ent_rows"][e].cpu().tolist() == want
    # slots: per group and level a numbering of exactly that group's rows of the level
    slot, lvl_rows, lvl_tok, lvl_anc = (ft[k].cpu() for k in ("slot", "lvl_rows", "lvl_tokens", "lvl_anc"))
    anc0 = keep["anc"].cpu()
    grp = [(r[3] // K) & 1 for r in rows]
    lvl_n = {}
    for gi in range(2):
        for l in range(steps):
            mine = [i for i, r in enumerate(rows) if grp[i] == gi and r[1] - t == l]
            assert counts[4 + gi * _lib.GRAM_TAIL_MAX_STEPS + l] == len(mine)
            assert sorted(lvl_rows[gi, l, : len(mine)].tolist()) == mine
            assert sorted(slot[mine].tolist()) == list(range(len(mine)))
            for i in mine:
                s_ = int(slot[i])
                assert int(lvl_rows[gi, l, s_]) == i and int(lvl_tok[gi, l, s_]) == rows[i][0]
                assert lvl_anc[gi, l, :t, s_].tolist() == anc0[:t, rows[i][3]].tolist()  # below t: the beam's column
                a = rows[i][2]
                while a >= 0:  # from t on: the ancestors' slots
                    assert int(lvl_anc[gi, l, rows[a][1], s_]) == int(slot[a])
                    a = rows[a][2]
            lvl_n[gi, l] = len(mine)
    assert lvl_n[0, 0] > 0 and lvl_n[1, 0] > 0 and max(lvl_n.values()) <= R
    # ---- the self-attention of the pass against the step-wise kernel with one cache row per forest row
    i32 = dict(dtype=torch.int32, device=G.DEV)
    tokens = torch.tensor([r[0] for r in rows], **i32)
    src = G.pieces_of((torch.randn(V if table else n, 3 * inner, generator=g) * 0.7).to(G.DEV), pieces)
    bias = (torch.randn(H, 64, generator=g) * 0.5).to(G.DEV)
    kc0, vc0 = (G.pieces_of((torch.randn(Tmax, R, inner, generator=g) * 0.7).to(G.DEV), pieces) for _ in range(2))
    L_ = G.lib()
    out = torch.empty(2, n, pieces * inner, dtype=G.DT, device=G.DEV)
    _bits(out).fill_(SENT)
    kc, vc = kc0.clone(), vc0.clone()
    tmp = torch.empty(cap, pieces * inner, dtype=G.DT, device=G.DEV)
    for gi in range(2):
        for l in range(steps):
            if not lvl_n[gi, l]:
                continue
            rows_l, toks_l, anc_l = ft["lvl_rows"][gi, l], ft["lvl_tokens"][gi, l], ft["lvl_anc"][gi, l]
            _lib.check(L_.gram_dec_self_attn_rows_split(G.p(src), G.p(toks_l if table else rows_l), G.p(kc), G.p(vc), G.p(anc_l), G.p(bias),
                                                        G.p(tmp), R, lvl_n[gi, l], None, H, t + l, Tmax, pieces, src[0].numel(),
                                                        kc[0].numel(), G.stream()), "level")
            _lib.check(L_.gram_scatter_rows(G.p(tmp), G.p(rows_l), G.p(out[0]), lvl_n[gi, l], pieces * inner * 2, n, G.stream()), "scatter")
    # reference: 64 cache rows per position, forest row i owns row i; below t its beam's ancestors' k and v are copied there
    RR = 64
    kr, vr = (torch.zeros(pieces, Tmax, RR, inner, dtype=G.DT, device=G.DEV) for _ in range(2))
    ancr = torch.zeros(Tmax, RR, **i32)
    for i, r in enumerate(rows):
        for j in range(t):
            kr[:, j, i], vr[:, j, i] = kc0[:, j, int(anc0[j, r[3]])], vc0[:, j, int(anc0[j, r[3]])]
            ancr[j, i] = i
        a = r[2]
        while a >= 0:
            ancr[rows[a][1], i] = a
            a = rows[a][2]
    for pos in range(t, t + steps):
        lvl = [i for i, r in enumerate(rows) if r[1] == pos]
        if not lvl:
            continue
        o = torch.empty(len(lvl), pieces * inner, dtype=G.DT, device=G.DEV)
        idx = torch.tensor(lvl, **i32)
        if table:
            _lib.check(L_.gram_dec_self_attn_rows_split(G.p(src), G.p(tokens[lvl].contiguous()), G.p(kr), G.p(vr), G.p(ancr), G.p(bias), G.p(o),
                                                        RR, len(lvl), G.p(idx), H, pos, Tmax, pieces, src[0].numel(), kr[0].numel(),
                                                        G.stream()), "step rows")
        else:
            q = src[:, lvl].contiguous()
            _lib.check(L_.gram_dec_self_attn_split(G.p(q), G.p(kr), G.p(vr), G.p(ancr), G.p(bias), G.p(o), RR, len(lvl), G.p(idx), H, pos, Tmax,
                                                   pieces, q[0].numel(), kr[0].numel(), G.stream()), "step")
        out[1, lvl] = o
    torch.cuda.synchronize()
    assert not bool((_bits(out[1]) == SENT).all(dim=1).any())
    assert torch.equal(_bits(out[0]), _bits(out[1]))
    assert torch.equal(_bits(kc[:, :t]), _bits(kc0[:, :t]))  # (the cached positions are read, never written)


@pytest.mark.parametrize("n,row_bytes", [(1, 16), (37, 512), (64, 3072)])
def test_scatter_rows_puts_every_row_where_its_slot_says(G, n, row_bytes):
    from gram_amd import _lib
    g = torch.Generator().manual_seed(n)
    dst_rows = n + 5
    src = torch.randint(-30000, 30000, (n, row_bytes // 2), generator=g, dtype=torch.int16).to(G.DEV)
    rows = torch.randperm(dst_rows, generator=g)[:n].to(torch.int32)
    rows[n // 2] = -1 if n > 1 else rows[0]  # (a slot without a row is skipped)
    rows = rows.to(G.DEV)
    dst = torch.full((dst_rows, row_bytes // 2), SENT, dtype=torch.int16, device=G.DEV)
    _lib.check(G.lib().gram_scatter_rows(G.p(src), G.p(rows), G.p(dst), n, row_bytes, dst_rows, G.stream()), "scatter")
    torch.cuda.synchronize()
    want = torch.full_like(dst, SENT)
    for i, r in enumerate(rows.tolist()):
        if r >= 0:
            want[r] = src[i]
    assert torch.equal(dst, want)


# ------------------------------------------------------------------------------------ 3. the entry cross-attention
@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("K", [4, 20, 40])  # two waves per (user, head) up to 32 beams, one above: the split is part of a row's bits
@pytest.mark.parametrize("n0", [15, 16, 17, 63, 64, 65])
def test_cross_attn_entries_equal_the_stepwise_kernel(G, n0, K, pieces):
    from gram_amd import _lib
    B, H, S = 3, 2, 160
    inner = H * 64
    g = torch.Generator().manual_seed(100 * n0 + K + pieces)
    counts = [n0, 0, 5]  # user 1 owns no row (and no entry)
    n = sum(counts)
    q = G.pieces_of((torch.randn(n, inner, generator=g) * 0.6).to(G.DEV), pieces)
    kb = G.pieces_of((torch.randn(B, H, S, 64, generator=g) * 0.6).to(G.DEV), pieces)
    vt = G.pieces_of(G.vt_blocked((torch.randn(B, H, 64, S, generator=g) * 0.6).to(G.DEV)), pieces)
    mask = torch.ones(B, S, dtype=torch.uint8)
    mask[0, 40:64], mask[0, 150:], mask[2, :32] = 0, 0, 0  # (a fully masked 32-key step, a ragged tail)
    mask = mask.to(G.DEV)
    i32 = dict(dtype=torch.int32, device=G.DEV)
    users, rows, base = [], [], 0
    for b, c in enumerate(counts):
        for e in range((c + 63) // 64):
            users.append(b)
            rows.append([base + 64 * e + s if 64 * e + s < c else -1 for s in range(64)])
        base += c
    ent_users, ent_rows = torch.tensor(users, **i32), torch.tensor(rows, **i32).contiguous()
    out = torch.empty(2, n, pieces * inner, dtype=G.DT, device=G.DEV)
    _bits(out).fill_(SENT)
    L_ = G.lib()
    _lib.check(L_.gram_cross_attn_entries_split(G.p(q), G.p(kb), G.p(vt), G.p(mask), G.p(out[0]), len(users), K, H, S, G.p(ent_users),
                                                G.p(ent_rows), pieces, q[0].numel(), kb[0].numel(), None, G.stream()), "entries")
    # the step-wise kernel on groups of K rows per user (the last group padded with zero queries)
    base = 0
    for b, c in enumerate(counts):
        for g0 in range(0, c, K):
            k = min(K, c - g0)
            qg = torch.zeros(pieces, B * K, inner, dtype=G.DT, device=G.DEV)
            qg[:, b * K: b * K + k] = q[:, base + g0: base + g0 + k]
            og = torch.empty(B * K, pieces * inner, dtype=G.DT, device=G.DEV)
            _lib.check(L_.gram_cross_attn_decode_split(G.p(qg), G.p(kb), G.p(vt), G.p(mask), G.p(og), B, K, H, S, None, None, pieces,
                                                       qg[0].numel(), kb[0].numel(), None, G.stream()), "decode")
            out[1, base + g0: base + g0 + k] = og[b * K: b * K + k]
        base += c
    torch.cuda.synchronize()
    assert not bool((_bits(out[1]) == SENT).all(dim=1).any())
    assert torch.equal(_bits(out[0]), _bits(out[1]))
