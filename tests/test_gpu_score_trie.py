"""-m gpu: every catalogue item scored in one decoder pass over the Trie (gram_score_trie, GRAM.score_all_items).

The two new kernels through the C ABI against fp64 restatements and, bit for bit, against the teacher-forced kernels on the Trie
unrolled into explicit sequences; the whole path against the CPU oracle (tests/tf_oracle.py), against GRAM.score_sequences
(torch.equal), against generate's sequences_scores; batch / chunk / passage-cache / compaction invariance.  Tolerances are those of
tests/test_gpu_teacher_forced.py (imported, not restated).  Neither new kernel has a workgroup barrier or LDS, so there is no
chaos-build case.  Observed values are printed."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from gram_amd import _lib
from gram_amd.utils import generation_trie as gt
from oracle import gram_oracle as O
from tests import gpu_util as U
from tests import test_gpu_teacher_forced as TFT
from tests import tf_oracle as TF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gram_amd
    return gram_amd


@pytest.fixture(scope="module")
def small(gpu):
    """(state dict, model) of the T5-small oracle config, shared by the whole-path tests"""
    oc = O.OracleConfig.named("t5-small", max_item_num=4)
    sd, m = TFT._model(gpu, oc, 21)
    return oc, sd, m


# ---------------------------------------------------------------------------------------------------------- Tries
def _chain63():
    rng = random.Random(63)
    return [[0] + [rng.randint(2, 199) for _ in range(62)] + [1]]  # 63 labels: rows at positions 0..62, fan-out 1 everywhere


def _single():
    return [[0, 1]]  # Q = 1


def _bushy():
    """fan-out 40 below the start token, 1 to a few below that, candidates of 3..9 tokens; tokens < 200"""
    rng = random.Random(4)
    cands = set()
    for a in rng.sample(range(2, 200), 40):
        for _ in range(rng.randint(1, 2)):
            ln = rng.randint(3, 9)
            cands.add(tuple([0, a] + [rng.randint(2, 6) for _ in range(ln - 3)] + [1]))
    return [list(c) for c in sorted(cands)]


TRIES = {"chain63": _chain63, "single": _single, "bushy": _bushy}


def _random_cands(seed, n, lo, hi, toks):
    rng = random.Random(seed)
    cands = set()
    while len(cands) < n:
        cands.add(tuple([0] + [rng.randint(2, 1 + toks) for _ in range(rng.randint(lo, hi) - 2)] + [1]))
    out = [list(c) for c in cands]
    rng.shuffle(out)
    return out


def _tables(cands):
    flat = gt.FlatTrie(gt.Trie(cands))
    r = flat.decoder_rows()
    t = {f: torch.from_numpy(np.ascontiguousarray(getattr(r, f))).to(DEV) for f in gt.DecoderRows.ARRAYS}
    c = _lib.TrieRows(*[t[f].data_ptr() for f in gt.DecoderRows.ARRAYS], r.Q, r.Tq, r.n_nodes, r.n_leaves)
    return flat, r, t, c


def _labels_of(cands, T=None):
    T = T or max(len(c) for c in cands) - 1
    lab = torch.full((len(cands), T), -100, dtype=torch.long)
    for i, c in enumerate(cands):
        lab[i, : len(c) - 1] = torch.tensor(c[1:])
    return lab


def test_the_bushy_trie_is_what_the_kernel_tests_need(gpu):
    _, r, _, _ = _tables(_bushy())
    fan = np.bincount(r.node_row[r.node_row >= 0])
    print(f"bushy: Q={r.Q} Tq={r.Tq} leaves={r.n_leaves} fan-outs {fan.min()}..{fan.max()}")
    assert 150 <= r.Q <= 260 and r.Q % 16 and r.Tq == 8 and fan.min() == 1 and fan.max() == 40


# ---------------------------------------------------------------------------------------------------------- 1. kernel 2a
@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("trie", ["chain63", "single", "bushy"])
def test_tree_self_attn_vs_fp64_and_bitwise_vs_the_sequence_kernel(gpu, trie, pieces):
    flat, r, t, _ = _tables(TRIES[trie]())
    torch.manual_seed(r.Q + pieces)
    B, H, Q, Tq = 2, 3, r.Q, r.Tq  # two users: a user's rows cannot reach the other's
    inner, R = H * 64, B * r.Q
    qkv = U.pieces_of(torch.randn(R, 3 * inner, device=DEV) * 0.5, pieces)  # planar [pieces][R][3 inner]
    bias = torch.randn(H, _lib.GRAM_MAX_DEC_LEN, device=DEV)
    out = torch.full((R, pieces * inner), 7.0, dtype=U.DT, device=DEV)
    L = U.lib()
    _lib.check(L.gram_dec_self_attn_tree_split(qkv.data_ptr(), t["pos"].data_ptr(), t["anc"].data_ptr(), bias.data_ptr(), out.data_ptr(), B,
                                               Q, Tq, H, pieces, R * 3 * inner, U.stream()), "gram_dec_self_attn_tree_split")
    torch.cuda.synchronize()
    anc, pos = t["anc"].long(), t["pos"].long()
    dist = pos[:, None] - torch.arange(Tq, device=DEV)[None, :]  # (Q, Tq): >= 0 on the row's own path
    # fp64: row i over the rows anc[i][0..pos[i]] of its user.  Bounds: test_dec_self_attn_tf_kernel_vs_fp64's, the same expression
    v = U.join(qkv).view(B, Q, 3, H, 64)
    q, k, vv = v[:, :, 0], v[:, :, 1][:, anc], v[:, :, 2][:, anc]  # (B, Q, H, 64), (B, Q, Tq, H, 64) x 2
    s = torch.einsum("bqhd,bqjhd->bhqj", q, k) + bias.double()[:, dist.clamp(min=0)][None]
    s = s.masked_fill((dist < 0)[None, None], float("-inf"))
    ref = torch.einsum("bhqj,bqjhd->bqhd", torch.softmax(s, -1), vv).reshape(R, inner)
    got = U.join_inter(out) if pieces == 2 else out.double()
    err = float((got - ref).abs().max())
    print(f"tree self-attn {trie} pieces={pieces} Q={Q} Tq={Tq}: vs fp64 {err:.2e}")
    # (one piece: the output's rounding to 16 bits dominates -- |out| <= max |v| ~ 2.5, half-ulp 2^-11 relative on IEEE half; bfloat16
    # in the PIECE=bf16 A/B build carries three mantissa bits fewer, hence x 8 there.  Two pieces: 2e-5 holds in both builds)
    assert err < (2e-5 if pieces == 2 else 3e-3 * (1 if U.F16 else 8))
    # the Trie unrolled: sequence (b, i) holds the q|k|v rows of row i's path; gram_dec_self_attn_tf_split's position j of it and the
    # tree kernel's row anc[i][j] are the same prefix -- the same bits, for every row of every path
    un = qkv.view(pieces, B, Q, 3 * inner)[:, :, anc].contiguous()  # (pieces, B, Q, Tq, 3 inner)
    n_seq = B * Q
    out_tf = torch.full((n_seq * Tq, pieces * inner), 9.0, dtype=U.DT, device=DEV)
    _lib.check(L.gram_dec_self_attn_tf_split(un.data_ptr(), bias.data_ptr(), out_tf.data_ptr(), n_seq, Tq, H, pieces, n_seq * Tq * 3 * inner,
                                             U.stream()), "gram_dec_self_attn_tf_split")
    torch.cuda.synchronize()
    on = dist >= 0
    assert torch.equal(out.view(B, Q, -1)[:, anc][:, on], out_tf.view(B, Q, Tq, -1)[:, on])


# ---------------------------------------------------------------------------------------------------------- 2. kernel 2b
@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("trie", ["chain63", "single", "bushy"])
def test_leaf_logprob_vs_fp64_and_bitwise_vs_label_logprob(gpu, trie, pieces):
    flat, r, t, crows = _tables(TRIES[trie]())
    torch.manual_seed(r.Q + 10 * pieces)
    B, d, V, Q, Tq, nn, nl = 2, 256, 512, r.Q, r.Tq, r.n_nodes, r.n_leaves
    R = B * Q
    h = torch.randn(R, d, device=DEV)
    E = torch.randn(V, d, device=DEV) * 0.05
    hd, Wd = (U.inter(h), U.inter(E)) if pieces == 2 else (U.bf(h), U.bf(E))
    E32 = E.contiguous()
    logits = torch.empty(R, V, device=DEV)
    part = torch.empty(R, V // 64, 2, device=DEV)
    lse = torch.empty(R, device=DEV)
    sp = _lib.Split(pieces, 0, 0, 0, 1.0)
    L = U.lib()
    _lib.check(L.gram_gemm_bf16_lse_split(hd.data_ptr(), Wd.data_ptr(), logits.data_ptr(), part.data_ptr(), R, V, d, pieces * d, V,
                                          C.byref(sp), U.stream()), "lse gemm")
    _lib.check(L.gram_lse_combine(part.data_ptr(), lse.data_ptr(), R, V // 64, U.stream()), "lse combine")
    edge = torch.full((R,), 7.0, device=DEV)
    leaf = torch.full((B, nl), 7.0, device=DEV)
    node = torch.full((B, nn), 7.0, device=DEV)
    _lib.check(L.gram_trie_leaf_logprob_split(hd.data_ptr(), Wd.data_ptr(), E32.data_ptr() if pieces == 2 else None, d, lse.data_ptr(),
                                              C.byref(crows), B, V, pieces, edge.data_ptr(), leaf.data_ptr(), node.data_ptr(), U.stream()),
               "gram_trie_leaf_logprob_split")
    torch.cuda.synchronize()
    # fp64 on the kernel's own operands (the hidden pieces, the lm_head rows it reads, the same lse).  Bound per edge term: the fp32
    # dot product of d terms ((d + 8) * 2^-24 * sum |h_k e_k|: accumulation, the piece sum of h, the lane sums) and the rounding
    # of the subtraction (2^-23 * (|dot| + |lse|)); per leaf the bounds of its path plus Tq fp32 additions of the partial sums
    h64 = U.join_inter(hd) if pieces == 2 else hd.double()
    E64 = E32.double() if pieces == 2 else Wd.double()
    node_row, node_tok = t["node_row"].long(), t["node_tok"].long()
    has = node_row >= 0
    hr = h64.view(B, Q, d)[:, node_row.clamp(min=0)]  # (B, n_nodes, d)
    er = E64[node_tok.clamp(min=0)][None]
    ls = lse.double().view(B, Q)[:, node_row.clamp(min=0)]
    dot = (hr * er).sum(-1)
    term = torch.where(has[None], dot - ls, torch.zeros((), dtype=torch.float64, device=DEV))
    tb = torch.where(has[None], (d + 8) * 2.0 ** -24 * (hr.abs() * er.abs()).sum(-1) + 2.0 ** -23 * (dot.abs() + ls.abs()),
                     torch.zeros((), dtype=torch.float64, device=DEV))
    assert bool(((node.double() - term).abs() <= tb).all()), float(((node.double() - term).abs() - tb).max())
    parent = t["row_node"].long()[node_row.clamp(min=0)]  # node of the parent row (breadth-first numbering: parents come first)
    total, bound, mag = term.clone(), tb.clone(), term.abs()
    for n in range(2, nn):
        p = int(parent[n])
        total[:, n] += total[:, p]
        bound[:, n] += bound[:, p]
        mag[:, n] += mag[:, p]
    is_leaf = t["node_leaf"] >= 0
    rank = t["node_leaf"].long()[is_leaf]
    ref = torch.empty(B, nl, dtype=torch.float64, device=DEV)
    lim = torch.empty(B, nl, dtype=torch.float64, device=DEV)
    ref[:, rank] = total[:, is_leaf]
    lim[:, rank] = bound[:, is_leaf] + Tq * 2.0 ** -24 * mag[:, is_leaf]
    err = (leaf.double() - ref).abs()
    print(f"leaf logprob {trie} pieces={pieces}: max |leaf - fp64| {float(err.max()):.2e} (bound {float(lim.max()):.2e}), "
          f"max |term - fp64| {float((node.double() - term).abs().max()):.2e}")
    assert bool((err <= lim).all())
    assert torch.equal(node[:, ~has], torch.zeros(B, int((~has).sum()), device=DEV))  # the root and the start token's node
    # the Trie unrolled into one explicit sequence per leaf: gram_label_logprob_split's tokens and sums, bit for bit
    leaves = torch.nonzero(is_leaf)[:, 0]
    leaves = leaves[torch.argsort(t["node_leaf"].long()[leaves])]  # by rank
    i = node_row[leaves]
    tl = t["pos"].long()[i]
    anc = t["anc"].long()[i]  # (n_leaves, Tq) rows of the path
    j = torch.arange(Tq, device=DEV)[None, :]
    nxt = torch.cat([anc[:, 1:], anc[:, :1]], 1)  # the row at position j + 1
    lab = torch.where(j < tl[:, None], t["tokens"].long()[nxt], node_tok[leaves][:, None])
    lab = torch.where(j <= tl[:, None], lab, torch.full_like(lab, -100))
    path_node = torch.where(j < tl[:, None], t["row_node"].long()[nxt], leaves[:, None])
    hid_un = hd.view(B, Q, -1)[:, anc].contiguous()  # (B, n_leaves, Tq, pieces * d)
    lse_un = lse.view(B, Q)[:, anc].contiguous()
    lab_un = lab[None].expand(B, nl, Tq).to(torch.int32).contiguous()
    tok = torch.full((B * nl * Tq,), 7.0, device=DEV)
    seq = torch.full((B * nl,), 7.0, device=DEV)
    _lib.check(L.gram_label_logprob_split(hid_un.data_ptr(), Wd.data_ptr(), E32.data_ptr() if pieces == 2 else None, d, lse_un.data_ptr(),
                                          lab_un.data_ptr(), B * nl, Tq, V, pieces, tok.data_ptr(), seq.data_ptr(), U.stream()),
               "gram_label_logprob_split")
    torch.cuda.synchronize()
    assert torch.equal(seq.view(B, nl), leaf)
    on = j <= tl[:, None]
    assert torch.equal(tok.view(B, nl, Tq)[:, on], node[:, path_node[on]])


# ---------------------------------------------------------------------------------------------------------- 3. the CPU oracle
def _score_trie_with_nodes(m, ids, mask, fn):
    """torch.ops.gram.score_trie as score_all_items calls it, with the per-edge terms: (leaf (B, n_leaves), node (B, n_nodes))"""
    flat = m._flat_trie(fn)
    rows, tables = flat.decoder_rows_on(torch.device(DEV))
    _c, (t_off, t_tok, t_node) = flat.to_device(torch.device(DEV))
    outs, _ = m._tf_chunks(ids, mask, None, None,
                           lambda cid, cmask, handle, ws, _d, _l, *comp: torch.ops.gram.score_trie(
                               cid, cmask, handle, ws, t_off, t_tok, t_node, int(flat.max_fanout), int(flat.min_seq_len), *tables,
                               int(rows.n_leaves), int(m.config.vocab_size), True, *comp),
                           trie_rows=(int(rows.Q), int(rows.n_leaves + rows.n_nodes)))
    assert len(outs) == 1
    return outs[0]


def test_score_all_items_matches_the_oracle(gpu, small):
    oc, sd, m = small
    g = torch.Generator().manual_seed(31)
    B, N, Lx = 3, 3, 32
    ids, mask = TFT._ragged(g, B, N, Lx, oc.vocab_size)
    cands = _random_cands(31, 36, 3, 7, 5)
    flat = gt.FlatTrie(gt.Trie(cands))
    assert flat.decoder_rows().Q > 64  # the grouped cross-attention
    lab = _labels_of(cands)
    Cn, T = lab.shape
    ref_logits = TF.teacher_forced_logits(sd, oc, ids, mask, TF.shift_right(lab).repeat(B, 1))
    _, ref_tok = TF.loss_and_token_logp(ref_logits, lab.repeat(B, 1))
    ref = ref_tok.sum(-1).view(B, Cn)
    n_lab = torch.tensor([len(c) - 1 for c in cands], dtype=torch.float64)
    fn = gt.prefix_allowed_tokens_fn(gt.Trie(cands))
    for mode in TFT._modes():
        m.set_precision(mode)
        got = m.score_all_items(ids.to(DEV), mask.to(DEV), fn, cands).cpu()
        assert got.shape == (B, Cn) and got.dtype == torch.float32
        dev = (got.double() - ref).abs()
        print(f"score_all_items vs oracle [{mode}] Q={flat.decoder_rows().Q}: max |d| {float(dev.max()):.2e}, "
              f"max |d| / labels {float((dev / n_lab).max()):.2e}")
        assert bool((dev < TFT._tol(mode)["logp"] * n_lab[None]).all())
        # the per-edge terms of the op (want_nodes) are the oracle's per-token log-probs, at the per-token bound
        leaf, node = _score_trie_with_nodes(m, ids.to(DEV), mask.to(DEV), fn)
        assert torch.equal(leaf[:, torch.from_numpy(flat.item_ranks(cands)).long().to(DEV)].cpu(), got)
        worst = 0.0
        for ci, c in enumerate(cands):
            path = torch.tensor([flat.leaf_of(c[:k]) for k in range(2, len(c) + 1)])
            d = (node[:, path].cpu().double() - ref_tok.view(B, Cn, T)[:, ci, : len(c) - 1]).abs()
            worst = max(worst, float(d.max()))
        print(f"  per-edge terms vs oracle tokens [{mode}]: max |d| {worst:.2e}")
        assert worst < TFT._tol(mode)["logp"]


# ---------------------------------------------------------------------------------------------------------- 4. score_sequences
def test_score_all_items_equals_score_sequences_bit_for_bit(gpu, small):
    oc, sd, m = small
    g = torch.Generator().manual_seed(41)
    B = 3
    ids, mask = TFT._ragged(g, B, 3, 32, oc.vocab_size)
    cands = _random_cands(41, 300, 3, 8, 6)
    rows = gt.FlatTrie(gt.Trie(cands)).decoder_rows()
    lab = _labels_of(cands)[None].expand(B, -1, -1).contiguous()
    fn = gt.prefix_allowed_tokens_fn(gt.Trie(cands))
    idd, mk = ids.to(DEV), mask.to(DEV)
    for mode in TFT._modes():
        m.set_precision(mode)
        one = m.score_all_items(idd, mk, fn, cands)
        ref = m.score_sequences(idd, mk, lab.to(DEV))
        d = float((one.double() - ref.double()).abs().max())
        print(f"score_all_items vs score_sequences [{mode}]: {rows.Q} rows against {lab.shape[1] * lab.shape[2]} per user, "
              f"max |d| {d:.2e}, bit-equal: {torch.equal(one, ref)}")
        assert torch.equal(one, ref)


# ---------------------------------------------------------------------------------------------------------- 5. generate
def test_generate_scores_match_score_all_items(gpu, small):
    oc, sd, m = small
    g = torch.Generator().manual_seed(12)
    B, N, Lx, K = 3, 3, 32, 10
    ids, mask = TFT._ragged(g, B, N, Lx, oc.vocab_size, pad_last=False)
    cands = [[0, a, b, c, 1] for a in (5, 6, 7, 8) for b in (9, 10, 11) for c in (12, 13)] + [[0, 20, 21, 1], [0, 22, 1]]
    lp = 0.7
    fn = gt.prefix_allowed_tokens_fn(gt.Trie(cands))
    for mode in TFT._modes():
        m.set_precision(mode)
        out = m.generate(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), max_length=5, prefix_allowed_tokens_fn=fn, num_beams=K,
                         num_return_sequences=K, output_scores=True, return_dict_in_generate=True, length_penalty=lp)
        scores = out["sequences_scores"]
        assert torch.isfinite(scores).all()
        item = m.sequence_items(out["sequences"], fn, cands).long()
        assert bool((item >= 0).all())
        every = m.score_all_items(ids.to(DEV), mask.to(DEV), fn, cands, length_penalty=lp)
        at = every[torch.arange(B, device=DEV).repeat_interleave(K), item]
        dev = float((at.double() - scores.double()).abs().max())
        print(f"generate vs score_all_items [{mode}]: max |score diff| {dev:.2e}")
        assert dev < TFT._tol(mode)["logp"]


# ---------------------------------------------------------------------------------------------------------- 6. invariance
def test_invariance_to_batch_chunk_cache_compaction_and_candidate_order(gpu, small):
    oc, sd, m = small
    g = torch.Generator().manual_seed(61)
    B, N, Lx = 64, 3, 32
    ids, mask = TFT._ragged(g, B, N, Lx, oc.vocab_size)
    ids[:, 1:] = ids[0, 1:]  # item passages shared across users: the cache has something to find
    mask[:, 1:] = mask[0, 1:]
    mask[-1, -1] = False
    ids[-1, -1] = 0
    cands = _random_cands(61, 40, 3, 7, 5)
    cands = cands + [list(cands[3]), list(cands[17])]  # two candidates that spell an earlier one's sequence
    fn = gt.prefix_allowed_tokens_fn(gt.Trie(cands))
    idd, mk = ids.to(DEV), mask.to(DEV)
    perm = torch.randperm(len(cands), generator=g).tolist()
    shuffled = [cands[i] for i in perm]
    fn_shuffled = gt.prefix_allowed_tokens_fn(gt.Trie(shuffled))
    lens = torch.tensor([len(c) - 1 for c in cands], dtype=torch.float64, device=DEV)
    for mode in TFT._modes():
        m.set_precision(mode)
        m.clear_passage_cache()
        full = m.score_all_items(idd, mk, fn, cands)
        assert full.shape == (B, len(cands))
        assert torch.equal(full[:, 40], full[:, 3]) and torch.equal(full[:, 41], full[:, 17]), mode
        for b in range(B):  # every user alone
            assert torch.equal(m.score_all_items(idd[b:b + 1], mk[b:b + 1], fn, cands)[0], full[b]), (mode, b)
        assert torch.equal(m.score_all_items(idd, mk, fn, cands, users_per_call=5), full), mode
        m.cache_passages(idd[:, 1:], mk[:, 1:])
        try:
            cached = m.score_all_items(idd, mk, fn, cands)
        finally:
            m.clear_passage_cache()
        os.environ["GRAM_COMPACT"] = "0"
        try:
            plain = m.score_all_items(idd, mk, fn, cands)
        finally:
            del os.environ["GRAM_COMPACT"]
        assert torch.equal(cached, full) and torch.equal(plain, full), mode
        again = m.score_all_items(idd[:4], mk[:4], fn_shuffled, shuffled)
        assert torch.equal(again, full[:4][:, torch.tensor(perm, device=DEV)]), mode  # the columns follow `candidates`
        # length_penalty: the sums over len ** penalty, the power in float64
        assert torch.equal(m.score_all_items(idd[:4], mk[:4], fn, cands, length_penalty=0.7), (full[:4].double() / lens ** 0.7).float()), mode
        print(f"invariance [{mode}]: B = {B} against every single user, users_per_call=5, warm cache, GRAM_COMPACT=0, duplicates, "
              f"column order, length_penalty: torch.equal")
    with pytest.raises(ValueError, match="closure"):
        m.score_all_items(idd[:1], mk[:1], lambda b, s: [1], cands)
    with pytest.raises(ValueError, match="start token"):
        bad = [[5, 6, 1]]
        m.score_all_items(idd[:1], mk[:1], gt.prefix_allowed_tokens_fn(gt.Trie(bad)), bad)
