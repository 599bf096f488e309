"""-m gpu: the biased search step (gram_beam_step_bias / gram_beam_step_bias_sparse) through the C ABI --
bit-exact against the restatement (tests/bias_oracle.py) on given logits with a shared normaliser; a zero phi against the plain step
kernels, every state array; sparse (one piece and two) against dense; live rows against rows in place; the small-batch logits
kernel's path; the streamed form against the one-shot form, forced at small capacities and taken by shape at K = 64 over a node of
fan-out 300; one shared row of potentials and one per user; an exclude list and an allow list."""
import ctypes as C

import numpy as np
import pytest
import torch

from gram_amd import _lib
from gram_amd.utils import generation_trie as gt
from tests import bias_oracle as BO

pytestmark = pytest.mark.gpu
STATE = ("tokens", "node", "beam_scores", "seq", "anc", "done", "n_hyps", "hyp_score", "worst", "hyp_len", "hyp_tok", "error")


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    return gpu_util


def _tries():
    g = torch.Generator().manual_seed(3)
    small = BO.GO.random_cands(g, 60, 2, 4, 256)   # Tmax 6
    deep = BO.GO.random_cands(g, 150, 3, 6, 256)   # Tmax 8, enough items for 64 beams
    # a node of fan-out 300 (K * fan-out > 16 384 at K = 64: the streamed form by shape), ids of two depths, V = 512
    fan = [[0, 2, x, 1] for x in range(3, 303)] + [[0, 3, y, z, 1] for y in range(4, 12) for z in range(20, 26)]
    return {"small": small, "deep": deep, "fan": fan}


TRIES = _tries()


def _bias(cands, B, per_user, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((B, len(cands)) if per_user else (len(cands),), generator=g) * 1.5).clamp_(-4, 4).numpy()


def _dense_data(cands, B, K, V, seed, shared0=False):
    """randn * 2 logits per step and their fp32 normalisers, computed ONCE on the host: both sides get the same tensors"""
    g = torch.Generator().manual_seed(seed)
    T = max(len(c) for c in cands)
    logits = [torch.randn(B if (t == 0 and shared0) else B * K, V, generator=g) * 2.0 for t in range(T - 1)]
    return logits, [torch.logsumexp(lg, dim=-1) for lg in logits]


def _sparse_data(cands, B, K, V, d, seed):
    g = torch.Generator().manual_seed(seed)
    T = max(len(c) for c in cands)
    emb = torch.randn(V, d, generator=g)
    hs = [torch.randn(B if t == 0 else B * K, d, generator=g) * d ** -0.5 * 3 for t in range(T - 1)]
    return hs, [torch.logsumexp(h @ emb.T, dim=-1) for h in hs], emb


SPARSE_TOL = 2e-5   # |sparse logit - dense logit|: the same operands, another summation order (the bound the group step's tests use)
MIN_MARGIN = 1e-4   # a search on dense logits decides like the one on sparse logits only if no decision is closer than 2 x SPARSE_TOL


def _decidable_sparse_data(G, cands, B, K, V, d, phi, pieces, seed0, keep=None):
    """_sparse_data of the first of the seeds seed0, seed0 + 1, ... whose search has a decision margin >= MIN_MARGIN (measured by the
    restatement on the logits of the operands the sparse step reads: 16-bit values, or the joined pieces and the fp32 lm_head)
    -> (hs, lses, emb, those logits)"""
    for seed in range(seed0, seed0 + 32):
        hs, lses, emb = _sparse_data(cands, B, K, V, d, seed)
        if pieces == 1:
            e = G.bf(emb).float()
            logits = [(G.bf(h).float() @ e.T).cpu() for h in hs]
        else:
            e = emb.to(G.DEV)
            logits = [(G.join_inter(G.inter(h.to(G.DEV))).float() @ e.T).cpu() for h in hs]
        m = BO.Margin()
        full = [logits[0].repeat_interleave(K, 0)] + logits[1:]
        BO.logits_search(full, [lses[0].repeat_interleave(K, 0)] + lses[1:], cands, B, K, None, early_exit=False, margin=m, keep=keep,
                         phi=phi)
        if m.value >= MIN_MARGIN:
            return hs, lses, emb, logits
    raise AssertionError("no decidable seed")


def _snapshot(keep):
    return {k: keep[k].clone() for k in STATE}


def _finalize(G, st, keep, B, K, T):
    seqs = torch.empty(B * K, T, dtype=torch.int64, device=G.DEV)
    scores = torch.empty(B * K, dtype=torch.float32, device=G.DEV)
    width = torch.zeros(4, dtype=torch.int32, device=G.DEV)
    _lib.check(G.lib().gram_beam_finalize(C.byref(st), K, T, G.p(seqs), G.p(scores), G.p(width), G.stream()), "beam_finalize")
    torch.cuda.synchronize()
    return dict(seqs=seqs[:, : int(width[0])].cpu(), scores=scores.cpu(), err=int(keep["error"][0]))


def _phi(G, phi):
    """numpy potentials [rows][n_nodes] -> (device tensor, stride): 0 for one shared row"""
    t = torch.from_numpy(np.ascontiguousarray(phi, dtype=np.float32)).to(G.DEV)
    return t, (0 if t.shape[0] == 1 else t.shape[1])


def run_dense(G, logits, lses, cands, B, K, phi, lp=1.0, shared0=False, lists=None, mode=None):
    """init + one dense step per entry of logits + finalize.  phi None: the plain entries (gram_beam_step); lists / mode: per-user
    item lists for the filtered kernels (the biased entry only)"""
    L = G.lib()
    T = max(len(c) for c in cands)
    V = logits[0].shape[-1]
    st, keep = G.make_beam_state(B, K, T, lp)
    flat = gt.FlatTrie(gt.Trie(cands))
    ctrie, keep2 = flat.to_device(torch.device(G.DEV))
    items, keep3 = (None, None) if lists is None else G.user_items(flat, cands, lists, mode)
    if phi is not None:
        phi_t, stride = _phi(G, phi)
    _lib.check(L.gram_beam_init(C.byref(st), C.byref(ctrie), 0, G.stream()), "init")
    trace = [_snapshot(keep)]
    for t, (lg, ls) in enumerate(zip(logits, lses)):
        lg, ls = lg.to(G.DEV).contiguous(), ls.to(G.DEV).contiguous()
        rpu = 1 if (t == 0 and shared0) else K
        if phi is None:
            _lib.check(L.gram_beam_step(C.byref(st), C.byref(ctrie), G.p(lg), G.p(ls), V, t + 1, rpu, G.stream()), "step")
        else:
            _lib.check(L.gram_beam_step_bias(C.byref(st), C.byref(ctrie), G.p(lg), G.p(ls), V, t + 1, rpu, G.p(phi_t), stride,
                                             None if items is None else C.byref(items), G.stream()), "step_bias")
        trace.append(_snapshot(keep))
    out = _finalize(G, st, keep, B, K, T)
    out["trace"] = trace
    return out


def run_sparse(G, hs, lses, emb32, cands, B, K, phi, pieces=1, live=False, lists=None, mode=None, scratch=False):
    """the sparse form: hs[0] is [B][d] (the shared step-0 row), hs[t] [B * K][d], fp32 on the host; pieces: 1 = 16-bit hidden and
    lm_head, 2 = interleaved two-piece hidden and the fp32 lm_head; live: every step from 1 on runs on gram_live_rows' compact rows;
    scratch: the state carries the small-batch logits kernel's scratch (its path is taken); phi None: the plain entries"""
    L = G.lib()
    T = max(len(c) for c in cands)
    V, d = emb32.shape
    st, keep = G.make_beam_state(B, K, T, 1.0, cand_scratch=scratch)
    flat = gt.FlatTrie(gt.Trie(cands))
    ctrie, keep2 = flat.to_device(torch.device(G.DEV))
    items, keep3 = (None, None) if lists is None else G.user_items(flat, cands, lists, mode)
    emb16 = G.bf(emb32) if pieces == 1 else None
    e32 = emb32.to(G.DEV).contiguous() if pieces == 2 else None
    if phi is not None:
        phi_t, stride = _phi(G, phi)
    _lib.check(L.gram_beam_init(C.byref(st), C.byref(ctrie), 0, G.stream()), "init")
    trace = [_snapshot(keep)]
    for t, (h, ls) in enumerate(zip(hs, lses)):
        hd = G.bf(h) if pieces == 1 else G.inter(h.to(G.DEV))
        ls = ls.to(G.DEV).contiguous()
        rowpos = None
        if live and t >= 1:
            rows, rowpos, _users = G.device_live_rows(st, ctrie)
            if rows.numel():
                hd, ls = hd[rows.long()].contiguous(), ls[rows.long()].contiguous()
        rpu = 1 if t == 0 else K
        if phi is not None:
            rc = L.gram_beam_step_bias_sparse(C.byref(st), C.byref(ctrie), G.p(hd), G.p(emb16), G.p(e32), d, G.p(ls), V, t + 1, rpu,
                                              G.p(rowpos), pieces, G.p(phi_t), stride, None if items is None else C.byref(items), G.stream())
        elif pieces == 2:
            rc = L.gram_beam_step_sparse_split(C.byref(st), C.byref(ctrie), G.p(hd), G.p(e32), d, G.p(ls), V, t + 1, rpu, G.p(rowpos), pieces,
                                               G.stream())
        elif rowpos is not None:
            rc = L.gram_beam_step_sparse_live(C.byref(st), C.byref(ctrie), G.p(hd), G.p(emb16), d, G.p(ls), V, t + 1, G.p(rowpos), G.stream())
        else:
            rc = L.gram_beam_step_sparse(C.byref(st), C.byref(ctrie), G.p(hd), G.p(emb16), d, G.p(ls), V, t + 1, rpu, G.stream())
        _lib.check(rc, "step_sparse")
        trace.append(_snapshot(keep))
    out = _finalize(G, st, keep, B, K, T)
    out["trace"] = trace
    return out


def _same_states(a, b, what):
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        for k in STATE:
            assert torch.equal(x[k], y[k]), (what, "step", t, k)


def _same_result(a, b):
    assert torch.equal(a["seqs"], b["seqs"]) and torch.equal(a["scores"], b["scores"]) and a["err"] == b["err"] == 0


def _against_restatement(got, ref_trace, ref_seqs, ref_scores, B, K):
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


def _reference(logits, lses, cands, B, K, phi, lp=1.0, shared0=False, keep=None):
    """the restatement on the rows the device reads: a shared step-0 row is every beam's row"""
    if shared0:
        logits = [logits[0].repeat_interleave(K, 0)] + logits[1:]
        lses = [lses[0].repeat_interleave(K, 0)] + lses[1:]
    trace = []
    seqs, scores = BO.logits_search(logits, lses, cands, B, K, None, lp=lp, early_exit=False, trace=trace, keep=keep, phi=phi)
    return trace, seqs, scores


@pytest.mark.parametrize("name,B,K,lp", [("small", 3, 4, 1.0), ("small", 3, 20, 0.7), ("deep", 2, 64, 1.0)])
@pytest.mark.parametrize("per_user", [False, True])
@pytest.mark.parametrize("lookahead,shared0", [(True, True), (False, False)])
def test_dense_bit_exact_against_the_restatement(G, name, B, K, lp, per_user, lookahead, shared0):
    """The same fp32 logits, the SAME normaliser and the same potentials on both sides: every key is the same bits by construction"""
    cands = TRIES[name]
    phi = BO.potentials(cands, _bias(cands, B, per_user, 40 + K), lookahead)
    logits, lses = _dense_data(cands, B, K, 256, 1000 + K, shared0)
    got = run_dense(G, logits, lses, cands, B, K, phi, lp, shared0)
    _against_restatement(got, *_reference(logits, lses, cands, B, K, phi, lp, shared0), B, K)
    if lookahead:  # the bias acts: the plain search returns another list
        assert run_dense(G, logits, lses, cands, B, K, None, lp, shared0)["seqs"].tolist() != got["seqs"].tolist()


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("chunked", [False, True])
def test_zero_phi_leaves_what_the_plain_step_leaves(G, rows, chunked):
    """dense, sparse with one piece and with two (the shared step-0 row, then live rows): every state array after every step"""
    cands, B, K, V, d = TRIES["small"], 3, 6, 256, 128
    phi0 = np.zeros((rows, gt.FlatTrie(gt.Trie(cands)).n_nodes), dtype=np.float32)
    logits, dl = _dense_data(cands, B, K, V, 7)
    hs, lses, emb = _sparse_data(cands, B, K, V, d, 8)
    L = G.lib()
    try:
        if chunked:
            assert L.gram_debug_set_beam_chunked(1) == 0 and L.gram_debug_set_beam_chunk_capacity(7) == 0
        a, b = run_dense(G, logits, dl, cands, B, K, None), run_dense(G, logits, dl, cands, B, K, phi0)
        _same_states(a["trace"], b["trace"], "dense")
        _same_result(a, b)
        for pieces in (1, 2):
            for live in (False, True):
                a = run_sparse(G, hs, lses, emb, cands, B, K, None, pieces, live)
                b = run_sparse(G, hs, lses, emb, cands, B, K, phi0, pieces, live)
                _same_states(a["trace"], b["trace"], ("sparse", pieces, live))
                _same_result(a, b)
    finally:
        L.gram_debug_set_beam_chunked(-1)
        L.gram_debug_set_beam_chunk_capacity(0)


@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("name,B,K,per_user", [("small", 3, 4, True), ("small", 3, 12, False), ("deep", 2, 64, True)])
def test_sparse_equals_dense_and_live_rows_equal_rows_in_place(G, name, B, K, per_user, pieces):
    cands, V, d = TRIES[name], 256, 128
    phi = BO.potentials(cands, _bias(cands, B, per_user, 60 + K), True)
    hs, lses, emb, logits = _decidable_sparse_data(G, cands, B, K, V, d, phi, pieces, 100 * K)
    sparse = run_sparse(G, hs, lses, emb, cands, B, K, phi, pieces)
    live = run_sparse(G, hs, lses, emb, cands, B, K, phi, pieces, live=True)
    _same_states(sparse["trace"], live["trace"], "rowpos NULL vs live")
    _same_result(sparse, live)
    # the small-batch logits kernel computes the same logits: the biased step adds the same edge terms to them
    pre = run_sparse(G, hs, lses, emb, cands, B, K, phi, pieces, scratch=True)
    _same_states(sparse["trace"], pre["trace"], "own logits vs sparse_logits_kernel's")
    # the dense step on the logits of the operands the sparse step reads
    dense = run_dense(G, logits, lses, cands, B, K, phi, shared0=True)
    assert dense["err"] == 0
    assert sparse["seqs"].tolist() == dense["seqs"].tolist()
    assert torch.allclose(sparse["scores"], dense["scores"], atol=SPARSE_TOL)
    for a, b in zip(sparse["trace"], dense["trace"]):
        assert torch.equal(a["tokens"], b["tokens"]) and torch.equal(a["done"], b["done"]) and torch.equal(a["anc"], b["anc"])


@pytest.mark.parametrize("name,B,K,per_user,caps", [("small", 3, 4, True, (1, 5, 13)), ("small", 3, 20, False, (7, 100)),
                                                    ("deep", 2, 64, True, (100, 256))])
def test_chunked_matches_one_shot_bit_for_bit(G, name, B, K, per_user, caps):
    """The streamed form at capacities that put round boundaries inside a beam's children and between two beams, sparse (one piece
    and two) with the shared step-0 row and dense: every state array after every step, against the one-shot form."""
    cands, V, d = TRIES[name], 256, 128
    phi = BO.potentials(cands, _bias(cands, B, per_user, 80 + K), True)
    L = G.lib()
    hs, lses, emb = _sparse_data(cands, B, K, V, d, 9 + K)
    logits, dl = _dense_data(cands, B, K, V, 19 + K)
    one = [run_sparse(G, hs, lses, emb, cands, B, K, phi, 1), run_sparse(G, hs, lses, emb, cands, B, K, phi, 2),
           run_dense(G, logits, dl, cands, B, K, phi)]
    try:
        assert L.gram_debug_set_beam_chunked(1) == 0
        for cap in caps:
            assert L.gram_debug_set_beam_chunk_capacity(cap) == 0
            ch = [run_sparse(G, hs, lses, emb, cands, B, K, phi, 1), run_sparse(G, hs, lses, emb, cands, B, K, phi, 2),
                  run_dense(G, logits, dl, cands, B, K, phi)]
            for a, b, what in zip(one, ch, ("sparse p1", "sparse p2", "dense")):
                _same_states(a["trace"], b["trace"], (what, cap))
                _same_result(a, b)
    finally:
        L.gram_debug_set_beam_chunked(-1)
        L.gram_debug_set_beam_chunk_capacity(0)


@pytest.mark.parametrize("per_user", [False, True])
def test_fan_out_300_takes_the_streamed_form_by_shape(G, per_user):
    """B = 2, K = 64, V = 512 over a node of 300 children: K * fan-out = 19 200 > 16 384 candidates.  Dense against the restatement
    bit for bit, sparse against dense, live rows against rows in place."""
    cands, B, K, V, d = TRIES["fan"], 2, 64, 512, 128
    assert gt.FlatTrie(gt.Trie(cands)).max_fanout == 300 and K * 300 > 16384
    phi = BO.potentials(cands, _bias(cands, B, per_user, 90), True)
    logits, dl = _dense_data(cands, B, K, V, 91)
    got = run_dense(G, logits, dl, cands, B, K, phi)
    _against_restatement(got, *_reference(logits, dl, cands, B, K, phi), B, K)
    hs, lses, emb, logits2 = _decidable_sparse_data(G, cands, B, K, V, d, phi, 2, 9200)
    for pieces in (1, 2):
        sparse = run_sparse(G, hs, lses, emb, cands, B, K, phi, pieces)
        live = run_sparse(G, hs, lses, emb, cands, B, K, phi, pieces, live=True)
        _same_states(sparse["trace"], live["trace"], ("live", pieces))
        _same_result(sparse, live)
    dense = run_dense(G, logits2, lses, cands, B, K, phi, shared0=True)
    assert sparse["seqs"].tolist() == dense["seqs"].tolist() and torch.allclose(sparse["scores"], dense["scores"], atol=SPARSE_TOL)


@pytest.mark.parametrize("allow", [False, True])
@pytest.mark.parametrize("chunked", [False, True])
def test_item_filters_compose(G, allow, chunked):
    """An exclude list and an allow list per user: dense against the restatement restricted to the leaves a user keeps (the
    potentials are over the shared Trie), bit for bit; sparse (the shared step-0 row, live rows) against dense."""
    cands, B, K, V, d = TRIES["small"], 3, 6, 256, 128
    g = torch.Generator().manual_seed(4)
    lists = [sorted(torch.randperm(len(cands), generator=g)[:n].tolist()) for n in ((9, 14, 30) if allow else (3, 20, 41))]
    flat = BO.flat_trie(cands)
    keep = BO.keep_masks(flat, cands, lists, allow)
    mode = _lib.ITEMS_ALLOW if allow else _lib.ITEMS_EXCLUDE
    phi = BO.potentials(cands, _bias(cands, B, True, 70), True)
    logits, dl = _dense_data(cands, B, K, V, 71, shared0=True)
    hs, lses, emb, logits2 = _decidable_sparse_data(G, cands, B, K, V, d, phi, 2, 7200, keep=keep)
    L = G.lib()
    try:
        if chunked:
            assert L.gram_debug_set_beam_chunked(1) == 0 and L.gram_debug_set_beam_chunk_capacity(5) == 0
        got = run_dense(G, logits, dl, cands, B, K, phi, shared0=True, lists=lists, mode=mode)
        _against_restatement(got, *_reference(logits, dl, cands, B, K, phi, shared0=True, keep=keep), B, K)
        index = {tuple(c): i for i, c in enumerate(cands)}
        for b in range(B):
            mine = {index[tuple(r[: r.index(1) + 1])] for r in got["seqs"][b * K:(b + 1) * K].tolist() if 1 in r}
            assert mine and (mine <= set(lists[b]) if allow else not (mine & set(lists[b])))
        sparse = run_sparse(G, hs, lses, emb, cands, B, K, phi, 2, lists=lists, mode=mode)
        live = run_sparse(G, hs, lses, emb, cands, B, K, phi, 2, live=True, lists=lists, mode=mode)
        _same_states(sparse["trace"], live["trace"], "live")
        dense = run_dense(G, logits2, lses, cands, B, K, phi, shared0=True, lists=lists, mode=mode)
        assert sparse["err"] == dense["err"] == 0 and sparse["seqs"].tolist() == dense["seqs"].tolist()
        assert torch.allclose(sparse["scores"], dense["scores"], atol=SPARSE_TOL)
    finally:
        L.gram_debug_set_beam_chunked(-1)
        L.gram_debug_set_beam_chunk_capacity(0)
