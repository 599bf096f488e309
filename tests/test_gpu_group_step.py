"""-m gpu: the group search step (gram_beam_init_groups / gram_beam_step_groups / gram_beam_step_groups_sparse)
through the C ABI -- bit-exact against the restatement (tests/group_oracle.py) on given logits with a shared normaliser, against the
plain step at one group, sparse against dense, the streamed form against the one-shot form, per-user item filters against a Trie of
the user's own, batch invariance, and the non-finite flag."""
import ctypes as C
import math

import pytest
import torch

from gram_amd import _lib
from gram_amd.utils import generation_trie as gt
from tests import group_oracle as GO

pytestmark = pytest.mark.gpu
STATE = ("tokens", "node", "beam_scores", "seq", "anc", "done", "n_hyps", "hyp_score", "worst", "hyp_len", "hyp_tok", "error")


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    return gpu_util


def _tries():
    """the three small Tries of tests/test_gpu_kernels.py, and one with enough candidates for 64 beams"""
    uniform = [[0, a, b, 1] for a in range(2, 9) for b in range(10, 14)]
    ragged = [[0, 2, 3, 1], [0, 2, 4, 5, 1], [0, 2, 4, 6, 7, 1], [0, 3, 1], [0, 3, 8, 1], [0, 4, 9, 9, 9, 1], [0, 5, 1],
              [0, 6, 2, 1], [0, 6, 3, 1], [0, 7, 7, 1], [0, 8, 1], [0, 9, 2, 2, 1]]
    narrow_root = [[0, 2, b, c, 1] for b in range(3, 9) for c in range(3, 7)] + [[0, 9, b, c, 1] for b in range(3, 6) for c in range(3, 5)]
    wide = [[0, a, b, 1] for a in range(2, 12) for b in range(12, 20)]
    return {"uniform": uniform, "ragged": ragged, "narrow_root": narrow_root, "wide": wide}


COMBOS = [(4, 2, 1.0, 1.0), (6, 2, 1.0, 1.0), (6, 3, 0.5, 0.7), (8, 8, 2.0, 1.0), (12, 4, 1.5, 1.0), (20, 5, 0.5, 1.0), (16, 4, 1.0, 2.0),
          (64, 2, 1.0, 1.0), (64, 64, 0.5, 1.0), (4, 2, 0.0, 1.0)]
# only combinations with at least K candidates; "wide" is there for the 64-beam ones alone, which no small Trie can hold
CASES = [(n, *c) for n, cands in _tries().items() for c in COMBOS if len(cands) >= c[0] and (n != "wide" or c[0] == 64)]


def _dense_data(cands, B, K, V, seed, rows0=None):
    """randn * 2 logits per step and their fp32 normalisers, computed ONCE on the host: both sides get the same tensors"""
    g = torch.Generator().manual_seed(seed)
    T = max(len(c) for c in cands)
    logits = [torch.randn(rows0 if (t == 0 and rows0) else B * K, V, generator=g) * 2.0 for t in range(T - 1)]
    return logits, [torch.logsumexp(lg, dim=-1) for lg in logits]


def _snapshot(keep):
    return {k: keep[k].clone() for k in STATE}


def _finalize(G, st, keep, B, K, T, nret=None):
    nret = nret or K
    seqs = torch.empty(B * nret, T, dtype=torch.int64, device=G.DEV)
    scores = torch.empty(B * nret, dtype=torch.float32, device=G.DEV)
    width = torch.zeros(4, dtype=torch.int32, device=G.DEV)
    _lib.check(G.lib().gram_beam_finalize(C.byref(st), nret, T, G.p(seqs), G.p(scores), G.p(width), G.stream()), "beam_finalize")
    torch.cuda.synchronize()
    return dict(seqs=seqs[:, : int(width[0])].cpu(), scores=scores.cpu(), err=int(keep["error"][0]))


def run_dense(G, logits, lses, cands, B, K, ngroups, lam, lp=1.0, plain=False, rows0_shared=False):
    """init + one dense step per entry of logits + finalize; plain: gram_beam_init / gram_beam_step instead of the group entries"""
    L = G.lib()
    T = max(len(c) for c in cands)
    V = logits[0].shape[-1]
    st, keep = G.make_beam_state(B, K, T, lp)
    ctrie, keep2 = gt.FlatTrie(gt.Trie(cands)).to_device(torch.device(G.DEV))
    if plain:
        _lib.check(L.gram_beam_init(C.byref(st), C.byref(ctrie), 0, G.stream()), "init")
    else:
        _lib.check(L.gram_beam_init_groups(C.byref(st), C.byref(ctrie), 0, ngroups, G.stream()), "init_groups")
    trace = [_snapshot(keep)]
    for t, (lg, ls) in enumerate(zip(logits, lses)):
        lg, ls = lg.to(G.DEV).contiguous(), ls.to(G.DEV).contiguous()
        rpu = 1 if (t == 0 and rows0_shared) else K
        if plain:
            _lib.check(L.gram_beam_step(C.byref(st), C.byref(ctrie), G.p(lg), G.p(ls), V, t + 1, rpu, G.stream()), "step")
        else:
            _lib.check(L.gram_beam_step_groups(C.byref(st), C.byref(ctrie), G.p(lg), G.p(ls), V, t + 1, rpu, ngroups, lam, G.stream()),
                       "step_groups")
        trace.append(_snapshot(keep))
    out = _finalize(G, st, keep, B, K, T)
    out["trace"] = trace
    return out


def run_sparse(G, hs, lses, emb32, cands, B, K, ngroups, lam, pieces=1, live=False, lists=None, all_cands=None, lp=1.0):
    """the sparse form: hs[0] is [B][d] (the shared step-0 row), hs[t] [B * K][d], fp32 on the host; pieces: 1 = 16-bit hidden and
    lm_head, 2 = interleaved two-piece hidden and the fp32 lm_head; live: every step from 1 on runs on gram_live_rows' compact rows;
    lists: per-user allow lists (indices into all_cands) for the filtered kernels"""
    L = G.lib()
    T = max(len(c) for c in (all_cands or cands))
    V, d = emb32.shape
    st, keep = G.make_beam_state(B, K, T, lp)
    flat = gt.FlatTrie(gt.Trie(all_cands or cands))
    ctrie, keep2 = flat.to_device(torch.device(G.DEV))
    items, keep3 = (None, None) if lists is None else G.user_items(flat, all_cands, lists, _lib.ITEMS_ALLOW)
    emb16 = G.bf(emb32) if pieces == 1 else None
    e32 = emb32.to(G.DEV).contiguous() if pieces == 2 else None
    _lib.check(L.gram_beam_init_groups(C.byref(st), C.byref(ctrie), 0, ngroups, G.stream()), "init_groups")
    trace = [_snapshot(keep)]
    for t, (h, ls) in enumerate(zip(hs, lses)):
        hd = G.bf(h) if pieces == 1 else G.inter(h.to(G.DEV))
        ls = ls.to(G.DEV).contiguous()
        rowpos = None
        if live and t >= 1:
            rows, rowpos, _users = G.device_live_rows(st, ctrie)
            if rows.numel():
                hd, ls = hd[rows.long()].contiguous(), ls[rows.long()].contiguous()
        rc = L.gram_beam_step_groups_sparse(C.byref(st), C.byref(ctrie), G.p(hd), G.p(emb16), G.p(e32), d, G.p(ls), V, t + 1, 1 if t == 0 else K,
                                            G.p(rowpos), pieces, ngroups, lam, None if items is None else C.byref(items), G.stream())
        _lib.check(rc, "step_groups_sparse")
        trace.append(_snapshot(keep))
    out = _finalize(G, st, keep, B, K, T)
    out["trace"] = trace
    return out


def _sparse_data(cands, B, K, V, d, seed):
    g = torch.Generator().manual_seed(seed)
    T = max(len(c) for c in cands)
    emb = torch.randn(V, d, generator=g)
    hs = [torch.randn(B if t == 0 else B * K, d, generator=g) * d ** -0.5 * 3 for t in range(T - 1)]
    # one normaliser per row for every form of the step (any fp32 value serves: both sides of each comparison get the same tensor)
    lses = [torch.logsumexp(h @ emb.T, dim=-1) for h in hs]
    return hs, lses, emb


def _same_states(a, b, what):
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        for k in STATE:
            assert torch.equal(x[k], y[k]), (what, "step", t, k)


@pytest.mark.parametrize("name,K,ngroups,lam,lp", CASES)
def test_bit_exact_against_the_restatement(G, name, K, ngroups, lam, lp):
    """The same fp32 logits and the SAME normaliser tensor on both sides: every key is the same bits by construction, so the
    sequences, every step's tokens, beam scores and done flags are compared with ==."""
    cands = _tries()[name]
    B, V = 3, 128
    logits, lses = _dense_data(cands, B, K, V, 1000 + 10 * K + ngroups)
    ref_trace = []
    ref_seqs, ref_scores = GO.logits_search(logits, lses, cands, B, K, ngroups, lam, lp, early_exit=False, trace=ref_trace)
    got = run_dense(G, logits, lses, cands, B, K, ngroups, lam, lp)
    assert got["err"] == 0
    for t, ref in enumerate(ref_trace):
        dev = got["trace"][t + 1]
        assert dev["done"].cpu().tolist() == [int(x) for x in ref["done"]], ("done", t)
        assert dev["tokens"].cpu().view(B, K).tolist() == ref["tokens"].tolist(), ("tokens", t)
        ds, rs = dev["beam_scores"].cpu().view(B, K), ref["beam_scores"]
        assert torch.equal(ds, rs), ("beam_scores", t, (ds - rs).abs().nan_to_num(0).max())
        for b in range(B):
            if not ref["done"][b]:  # (what a finished user's rows hold is unspecified: never read)
                assert dev["seq"].cpu()[b * K:(b + 1) * K, : t + 2].tolist() == ref["input_ids"][b * K:(b + 1) * K].tolist(), ("seq", t, b)
    assert got["seqs"].tolist() == ref_seqs.tolist()
    assert torch.allclose(got["scores"], ref_scores, rtol=1e-6, atol=0)


def test_the_ragged_trie_reaches_the_corner_cases():
    """what the bit-exact test relies on the ragged Trie for: users that finish at a group in mid-step, -inf fillers and -1e9 ties"""
    cands = _tries()["ragged"]
    B, V, K, ngroups = 3, 128, 12, 4
    logits, lses = _dense_data(cands, B, K, V, 1000 + 10 * K + ngroups)
    trace = []
    GO.logits_search(logits, lses, cands, B, K, ngroups, 1.5, early_exit=False, trace=trace)
    assert any(math.isinf(x) for tr in trace for x in tr["beam_scores"].view(-1).tolist())
    assert any(any(tr["done"]) for tr in trace)


@pytest.mark.parametrize("name,K,lp", [("uniform", 4, 1.0), ("uniform", 20, 1.0), ("ragged", 5, 0.7), ("ragged", 12, 1.0),
                                        ("narrow_root", 16, 2.0)])
@pytest.mark.parametrize("shared0", [False, True])
def test_one_group_without_penalty_is_the_plain_step(G, name, K, lp, shared0):
    cands = _tries()[name]
    B, V = 3, 128
    logits, lses = _dense_data(cands, B, K, V, 77 + K, rows0=B if shared0 else None)
    plain = run_dense(G, logits, lses, cands, B, K, 1, 0.0, lp, plain=True, rows0_shared=shared0)
    group = run_dense(G, logits, lses, cands, B, K, 1, 0.0, lp, rows0_shared=shared0)
    assert plain["err"] == group["err"] == 0
    _same_states(plain["trace"], group["trace"], "plain vs one group")
    assert torch.equal(plain["seqs"], group["seqs"]) and torch.equal(plain["scores"], group["scores"])


@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("name,K,ngroups,lam", [("ragged", 6, 3, 1.0), ("narrow_root", 12, 4, 0.5)])
def test_sparse_equals_dense(G, name, K, ngroups, lam, pieces):
    """The sparse step (logits of the Trie children recomputed from hidden . lm_head) selects what the dense step selects on the
    logits of the same operands; with live rows (rowpos) it returns the bits it returns with every row in place."""
    cands = _tries()[name]
    B, V, d = 3, 128, 128
    hs, lses, emb = _sparse_data(cands, B, K, V, d, 5 + K)
    sparse = run_sparse(G, hs, lses, emb, cands, B, K, ngroups, lam, pieces)
    live = run_sparse(G, hs, lses, emb, cands, B, K, ngroups, lam, pieces, live=True)
    assert sparse["err"] == live["err"] == 0
    _same_states(sparse["trace"], live["trace"], "rowpos NULL vs live")
    assert torch.equal(sparse["seqs"], live["seqs"]) and torch.equal(sparse["scores"], live["scores"])
    # the dense step on the logits of the operands the sparse step reads (16-bit values, or the joined pieces and the fp32 lm_head)
    if pieces == 1:
        e = G.bf(emb).float()
        logits = [(G.bf(h).float() @ e.T).cpu() for h in hs]
    else:
        e = emb.to(G.DEV)
        logits = [(G.join_inter(G.inter(h.to(G.DEV))).float() @ e.T).cpu() for h in hs]
    dense = run_dense(G, logits, lses, cands, B, K, ngroups, lam, rows0_shared=True)
    assert dense["err"] == 0
    assert sparse["seqs"].tolist() == dense["seqs"].tolist()
    assert torch.allclose(sparse["scores"], dense["scores"], atol=2e-5)
    for a, b in zip(sparse["trace"], dense["trace"]):
        assert torch.equal(a["tokens"], b["tokens"]) and torch.equal(a["done"], b["done"]) and torch.equal(a["anc"], b["anc"])


@pytest.mark.parametrize("name,K,ngroups,lam,caps", [("uniform", 6, 2, 1.0, (5, 4, 12, 21)), ("ragged", 12, 4, 1.5, (1, 3, 7)),
                                                      ("narrow_root", 8, 8, 2.0, (2, 6)), ("wide", 64, 2, 1.0, (100, 256))])
def test_chunked_matches_one_shot_bit_for_bit(G, name, K, ngroups, lam, caps):
    """The streamed form at capacities that put round boundaries inside a group's candidates, between two beams of a group and at
    the group's edge (uniform, gs = 3: 12 candidates per group at the second step, 21 at the shared first one), sparse with the
    shared step-0 row and dense: every state array after every step, against the one-shot form."""
    cands = _tries()[name]
    B, V, d = 3, 128, 128
    L = G.lib()
    hs, lses, emb = _sparse_data(cands, B, K, V, d, 9 + K)
    logits, dl = _dense_data(cands, B, K, V, 19 + K)
    one_s = run_sparse(G, hs, lses, emb, cands, B, K, ngroups, lam)
    one_d = run_dense(G, logits, dl, cands, B, K, ngroups, lam)
    assert one_s["err"] == one_d["err"] == 0
    try:
        assert L.gram_debug_set_beam_chunked(1) == 0
        for cap in caps:
            assert L.gram_debug_set_beam_chunk_capacity(cap) == 0
            ch_s = run_sparse(G, hs, lses, emb, cands, B, K, ngroups, lam)
            ch_d = run_dense(G, logits, dl, cands, B, K, ngroups, lam)
            _same_states(one_s["trace"], ch_s["trace"], ("sparse", cap))
            _same_states(one_d["trace"], ch_d["trace"], ("dense", cap))
            for a, b in ((one_s, ch_s), (one_d, ch_d)):
                assert torch.equal(a["seqs"], b["seqs"]) and torch.equal(a["scores"], b["scores"])
    finally:
        L.gram_debug_set_beam_chunked(-1)
        L.gram_debug_set_beam_chunk_capacity(0)


@pytest.mark.parametrize("chunked", [False, True])
def test_item_filters_equal_the_users_own_trie(G, chunked):
    """A user with an allow list, stepped in a batch of three, equals that user stepped alone on Trie(A_b), bit for bit."""
    cands = _tries()["narrow_root"]
    B, V, d, K, ngroups, lam = 3, 128, 128, 6, 3, 1.0
    g = torch.Generator().manual_seed(4)
    lists = [sorted(torch.randperm(len(cands), generator=g)[:n].tolist()) for n in (9, 14, 30)]
    hs, lses, emb = _sparse_data(cands, B, K, V, d, 23)
    L = G.lib()
    try:
        if chunked:
            assert L.gram_debug_set_beam_chunked(1) == 0 and L.gram_debug_set_beam_chunk_capacity(5) == 0
        batch = run_sparse(G, hs, lses, emb, None, B, K, ngroups, lam, lists=lists, all_cands=cands)
        assert batch["err"] == 0
        T = max(len(c) for c in cands)
        for b in range(B):
            own = [cands[i] for i in lists[b]]
            assert max(len(c) for c in own) == T
            hb = [h[b:b + 1] if t == 0 else h[b * K:(b + 1) * K] for t, h in enumerate(hs)]
            lb = [ls[b:b + 1] if t == 0 else ls[b * K:(b + 1) * K] for t, ls in enumerate(lses)]
            alone = run_sparse(G, hb, lb, emb, own, 1, K, ngroups, lam)
            assert alone["err"] == 0
            assert torch.equal(alone["seqs"], batch["seqs"][b * K:(b + 1) * K, : alone["seqs"].shape[1]])
            assert not batch["seqs"][b * K:(b + 1) * K, alone["seqs"].shape[1]:].any()
            assert torch.equal(alone["scores"], batch["scores"][b * K:(b + 1) * K])
            for x, y in zip(alone["trace"], batch["trace"]):
                for k in ("tokens", "beam_scores"):
                    assert torch.equal(x[k], y[k][b * K:(b + 1) * K]), k
                assert int(x["done"][0]) == int(y["done"][b])
    finally:
        L.gram_debug_set_beam_chunked(-1)
        L.gram_debug_set_beam_chunk_capacity(0)


def test_batch_invariance(G):
    """User b's state is the same alone and inside a batch of three (row indices in the ancestor table shifted by the user's base)."""
    cands = _tries()["ragged"]
    B, V, K, ngroups, lam = 3, 128, 6, 3, 0.5
    logits, lses = _dense_data(cands, B, K, V, 321)
    batch = run_dense(G, logits, lses, cands, B, K, ngroups, lam)
    assert batch["err"] == 0
    for b in range(B):
        rows = slice(b * K, (b + 1) * K)
        alone = run_dense(G, [lg[rows] for lg in logits], [ls[rows] for ls in lses], cands, 1, K, ngroups, lam)
        for x, y in zip(alone["trace"], batch["trace"]):
            for k in ("tokens", "node", "beam_scores", "seq"):
                assert torch.equal(x[k], y[k][rows]), k
            assert torch.equal(x["anc"], y["anc"][:, rows] - b * K)
            for k in ("done", "n_hyps", "worst", "hyp_score", "hyp_len", "hyp_tok"):
                assert torch.equal(x[k][0], y[k][b]), k
        w = alone["seqs"].shape[1]
        assert torch.equal(alone["seqs"], batch["seqs"][rows, :w]) and torch.equal(alone["scores"], batch["scores"][rows])


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_nonfinite_logit_in_a_late_group_is_flagged(G, bad):
    cands = _tries()["uniform"]
    B, V, K, ngroups = 2, 128, 4, 2
    logits, lses = _dense_data(cands, B, K, V, 5)
    assert run_dense(G, logits, lses, cands, B, K, ngroups, 1.0)["err"] == 0
    logits[1][1 * K + 3, 11] = bad  # second step, user 1, a beam of the LAST group, a token every first piece allows
    assert run_dense(G, logits, lses, cands, B, K, ngroups, 1.0)["err"] == 4
