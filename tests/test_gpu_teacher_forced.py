"""-m gpu: the teacher-forced decoder pass (gram_teacher_forced, GRAM.forward(labels=...), GRAM.score_sequences).

Against the reference's own forward (tests/golden/ref_forward.npz), the CPU restatement (tests/tf_oracle.py), fp64 restatements of
the three new kernels, the stepped decoder (gram_decode_step) and the beam search's own sequences_scores; plus batch invariance,
passage-cache / compaction neutrality, the autograd guard and a race screen against the chaos build.  Tolerances: f16x3 (two IEEE-half
pieces per value) per-token |d logp| <= 1e-4 and loss relative <= 1e-5; one piece (f16) 2e-2.  Observed values are printed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gram_amd import _lib
from oracle import gram_oracle as O
from tests import gpu_util as U
from tests import tf_oracle as TF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = 1.0 if U.F16 else 16.0  # the PIECE=bf16 A/B build carries 2^-18 per product
TOL = {"f16x3": dict(logp=1e-4 * X, loss=1e-5 * X, logit=1e-4 * X), "f16": dict(logp=2e-2, loss=2e-2, logit=3e-2)}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gram_amd
    return gram_amd


def _modes():
    return ("f16x3", "f16") if U.F16 else ("bf16x3", "bf16")


def _tol(mode):
    return TOL["f16x3" if mode.endswith("x3") else "f16"]


def _model(gpu, oc, seed):
    sd = O.init_state_dict(oc, seed)
    cfg = gpu.T5Config(vocab_size=oc.vocab_size, d_model=oc.d_model, d_ff=oc.d_ff, num_layers=oc.num_layers,
                       num_decoder_layers=oc.num_decoder_layers, num_heads=oc.num_heads, max_item_num=oc.max_item_num)
    m = gpu.create_model("gram", cfg)
    m.load_state_dict(sd)
    return sd, m.to(DEV).eval()


def _tiny():
    return O.OracleConfig(vocab_size=256, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2, max_item_num=5)


def _ragged(g, B, N, L, V, pad_last=True):
    ids = torch.randint(2, V, (B, N, L), generator=g)
    mask = torch.zeros(B, N, L, dtype=torch.bool)
    for b in range(B):
        for n in range(N):
            ln = 0 if (pad_last and b == B - 1 and n == N - 1 and N > 1) else int(torch.randint(max(2, L // 3), L + 1, (1,), generator=g))
            mask[b, n, :ln] = True
            ids[b, n, ln:] = 0
    return ids, mask


def _labels(g, shape, V, min_len=1):
    lab = torch.randint(2, V, shape, generator=g)
    T = shape[-1]
    lens = torch.randint(min_len, T + 1, shape[:-1], generator=g)
    pos = torch.arange(T)
    lab = torch.where(pos == (lens[..., None] - 1), torch.ones((), dtype=lab.dtype), lab)
    return lab.masked_fill(pos >= lens[..., None], -100)


# ---------------------------------------------------------------------------------------------------------- 1. the reference itself
@pytest.mark.parametrize("case", ["tiny", "base"])
def test_forward_matches_the_reference_golden(gpu, case):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_forward.npz"))
    if case == "tiny":
        oc, seed, pre = _tiny(), int(z["seed"]), "tiny_"
    else:
        oc, seed, pre = O.OracleConfig.named("t5-base"), int(z["base_seed"]), "base_"
    sd, m = _model(gpu, oc, seed)
    ids, mask, lab = (torch.from_numpy(z[pre + k]).to(DEV) for k in ("ids", "mask", "labels"))
    for mode in _modes():
        m.set_precision(mode)
        tol = _tol(mode)
        with torch.no_grad():
            out = m(input_ids=ids, attention_mask=mask, labels=lab, return_dict=False)  # the reference runners' call
        assert isinstance(out, tuple) and len(out) == 2
        loss, logits = out[0].cpu(), out[1].cpu()
        ref_loss = float(z[pre + "loss"])
        if case == "tiny":
            dl = float((logits - torch.from_numpy(z["tiny_logits"])).abs().max())
        else:
            cols = torch.from_numpy(z["base_cols"])
            dl = float((logits[..., cols] - torch.from_numpy(z["base_logits_cols"])).abs().max())
            _, tok = TF.loss_and_token_logp(logits, lab.cpu())
            dt = float((tok - torch.from_numpy(z["base_token_logp"]).double()).abs().max())
            print(f"  token logp {dt:.2e}")
            assert dt < tol["logp"]
        rel = abs(float(loss) - ref_loss) / abs(ref_loss)
        print(f"{case} [{mode}]: max |logit diff| {dl:.2e}, loss rel {rel:.2e}")
        assert dl < tol["logit"] and rel < tol["loss"]


# ---------------------------------------------------------------------------------------------------------- 2. the oracle
@pytest.mark.parametrize("name,T,B", [("t5-small", 1, 3), ("t5-small", 10, 3), ("t5-small", 64, 2), ("t5-base", 10, 2)])
def test_forward_matches_the_oracle(gpu, name, T, B):
    oc = O.OracleConfig.named(name, max_item_num=4)
    sd, m = _model(gpu, oc, 5)
    g = torch.Generator().manual_seed(100 + T)
    ids, mask = _ragged(g, B, 3, 32, oc.vocab_size)
    lab = _labels(g, (B, T), oc.vocab_size)
    ref_logits = TF.teacher_forced_logits(sd, oc, ids, mask, TF.shift_right(lab))
    ref_loss, ref_tok = TF.loss_and_token_logp(ref_logits, lab)
    for mode in _modes():
        m.set_precision(mode)
        tol = _tol(mode)
        with torch.no_grad():
            out = m(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), labels=lab.to(DEV))
        _, tok = TF.loss_and_token_logp(out.logits.cpu(), lab)
        dt = float((tok - ref_tok).abs().max())
        rel = abs(float(out.loss) - float(ref_loss)) / abs(float(ref_loss))
        seq = m.score_sequences(ids.to(DEV), mask.to(DEV), lab[:, None].to(DEV)).cpu()
        ds = float((seq[:, 0].double() - ref_tok.sum(-1)).abs().max())
        print(f"{name} T={T} [{mode}]: token logp {dt:.2e}, loss rel {rel:.2e}, sequence sum {ds:.2e}")
        assert dt < tol["logp"] and rel < tol["loss"] and ds < tol["logp"] * T


def test_score_sequences_many_rows_per_user(gpu):
    """C = 20 candidates of T = 10: 200 query rows per user, above the cross-attention's 64 -- the grouped path."""
    oc = O.OracleConfig.named("t5-small", max_item_num=4)
    sd, m = _model(gpu, oc, 6)
    g = torch.Generator().manual_seed(7)
    B, Cn, T = 2, 20, 10
    ids, mask = _ragged(g, B, 3, 32, oc.vocab_size)
    lab = _labels(g, (B, Cn, T), oc.vocab_size, min_len=3)
    ref_logits = TF.teacher_forced_logits(sd, oc, ids, mask, TF.shift_right(lab.view(B * Cn, T)))
    _, ref_tok = TF.loss_and_token_logp(ref_logits, lab.view(B * Cn, T))
    for mode in _modes():
        m.set_precision(mode)
        seq, tok = m.score_sequences(ids.to(DEV), mask.to(DEV), lab.to(DEV), return_tokens=True)
        dt = float((tok.cpu().view(B * Cn, T).double() - ref_tok).abs().max())
        ds = float((seq.cpu().view(-1).double() - ref_tok.sum(-1)).abs().max())
        print(f"C=20 T=10 [{mode}]: token logp {dt:.2e}, sequence sums {ds:.2e}")
        assert dt < _tol(mode)["logp"] and ds < _tol(mode)["logp"] * T
        assert torch.equal(tok.cpu()[lab < 0], torch.zeros(int((lab < 0).sum())))


# ---------------------------------------------------------------------------------------------------------- 3. the kernels
@pytest.mark.parametrize("pieces,T", [(1, 10), (2, 10), (2, 64), (1, 1), (1, 64), (2, 33)])
def test_dec_self_attn_tf_kernel_vs_fp64(gpu, pieces, T):
    torch.manual_seed(T)
    n_seq, H = 5, 4
    inner = H * 64
    R = n_seq * T
    x = torch.randn(R, 3 * inner, device=DEV) * 0.5
    qkv = U.pieces_of(x, pieces)  # planar [pieces][R][3 inner]
    bias = torch.randn(H, _lib.GRAM_MAX_DEC_LEN, device=DEV)
    out = torch.zeros(R, pieces * inner, dtype=U.DT, device=DEV)
    _lib.check(U.lib().gram_dec_self_attn_tf_split(qkv.data_ptr(), bias.data_ptr(), out.data_ptr(), n_seq, T, H, pieces, R * 3 * inner,
                                                   U.stream()), "gram_dec_self_attn_tf_split")
    torch.cuda.synchronize()
    got = U.join_inter(out) if pieces == 2 else out.double()
    v = U.join(qkv).view(n_seq, T, 3, H, 64)
    q, k, vv = (v[:, :, i].permute(0, 2, 1, 3) for i in range(3))  # (n, H, T, 64)
    s = q @ k.transpose(-1, -2)
    dist = torch.arange(T)[:, None] - torch.arange(T)[None, :]
    s = s + bias.double()[:, dist.clamp(min=0).to(DEV)][None]
    s = s.masked_fill((dist < 0).to(DEV), float("-inf"))
    ref = (torch.softmax(s, -1) @ vv).permute(0, 2, 1, 3).reshape(R, inner)
    err = float((got - ref).abs().max())
    print(f"self-attn tf pieces={pieces} T={T}: {err:.2e}")
    assert err < (2e-5 if pieces == 2 else 3e-3)


@pytest.mark.parametrize("pieces,Q", [pytest.param(1, 10, id="10"), pytest.param(1, 64, id="64"), pytest.param(1, 200, id="200"),
                                       (1, 65), (1, 128), (2, 10), (2, 65), (2, 128), (2, 200)])
def test_cross_attn_rows_vs_decode_kernel_and_fp64(gpu, pieces, Q):
    """Q = 65: a 1-row tail group; Q = 128: two full groups, no tail.  Two pieces: planar q / bank pieces and the interleaved output, as
    gram_teacher_forced passes them (set up as tests/test_gpu_split.py test_split_cross_attn)."""
    torch.manual_seed(Q)
    B, H, S = 3, 2, 96
    inner = H * 64
    if pieces == 1:
        q = (torch.randn(B * Q, inner, device=DEV) * 0.3).to(U.DT).contiguous()
        kb = (torch.randn(B, H, S, 64, device=DEV) * 0.3).to(U.DT).contiguous()
        vb = torch.randn(B, H, S, 64, device=DEV).to(U.DT)
        vt = vb.view(B, H, S // 32, 32, 64).transpose(-1, -2).contiguous()  # (B, H, S/32, 64, 32)
        q_ps = bank_ps = 0
    else:
        q32, k32 = torch.randn(B * Q, inner, device=DEV) * 0.3, torch.randn(B, H, S, 64, device=DEV) * 0.3
        v32 = torch.randn(B, H, S, 64, device=DEV)
        q, kb, vt = U.pieces_of(q32), U.pieces_of(k32), U.pieces_of(U.vt_blocked(v32.transpose(2, 3).contiguous()))  # planar [2][...]
        q_ps, bank_ps = q[0].numel(), kb[0].numel()
    mask = torch.ones(B, S, dtype=torch.uint8, device=DEV)
    mask[1, 70:] = 0
    mask[2, 10:40] = 0
    rowmap = torch.empty(B * (1 + 2 * _lib.GRAM_MAX_BEAMS), dtype=torch.int32, device=DEV)
    out = torch.zeros(B * Q, pieces * inner, dtype=U.DT, device=DEV)  # (two pieces: interleaved)
    _lib.check(U.lib().gram_cross_attn_rows_split(q.data_ptr(), kb.data_ptr(), vt.data_ptr(), mask.data_ptr(), out.data_ptr(), B, Q, H, S,
                                                  pieces, q_ps, bank_ps, None, rowmap.data_ptr(), U.stream()), "gram_cross_attn_rows_split")
    torch.cuda.synchronize()
    if pieces == 1:
        qd, kd, vd, got = q.double(), kb.double(), vb.double(), out.double()
    else:
        qd, kd, vd, got = U.join(q), U.join(kb), U.vt_unblocked(U.join(vt)).transpose(2, 3), U.join_inter(out)
    s = torch.einsum("bqhd,bhsd->bhqs", qd.view(B, Q, H, 64), kd)
    s = s.masked_fill(mask.bool().logical_not()[:, None, None, :], float("-inf"))
    ref = torch.einsum("bhqs,bhsd->bqhd", torch.softmax(s, -1), vd).reshape(B * Q, inner)
    err = float((got - ref).abs().max())
    print(f"cross rows pieces={pieces} Q={Q}: vs fp64 {err:.2e}")
    assert err < (2e-5 * X if pieces == 2 else 3e-3)
    if Q > 64:  # each group of <= 64 rows against the decode kernel on that group alone: the same bits
        for r0 in range(0, Q, 64):
            kc = min(64, Q - r0)
            if pieces == 1:
                qg = q.view(B, Q, inner)[:, r0:r0 + kc].contiguous().view(B * kc, inner)
                og = torch.zeros_like(qg)
                _lib.check(U.lib().gram_cross_attn_decode(qg.data_ptr(), kb.data_ptr(), vt.data_ptr(), mask.data_ptr(), og.data_ptr(), B,
                                                          kc, H, S, U.stream()), "gram_cross_attn_decode")
            else:
                qg = q.view(2, B, Q, inner)[:, :, r0:r0 + kc].contiguous()
                og = torch.zeros(B * kc, 2 * inner, dtype=U.DT, device=DEV)
                _lib.check(U.lib().gram_cross_attn_decode_split(qg.data_ptr(), kb.data_ptr(), vt.data_ptr(), mask.data_ptr(),
                                                                og.data_ptr(), B, kc, H, S, None, None, 2, qg[0].numel(), bank_ps, None,
                                                                U.stream()), "gram_cross_attn_decode_split")
            torch.cuda.synchronize()
            assert torch.equal(og.view(B, kc, -1), out.view(B, Q, -1)[:, r0:r0 + kc])


@pytest.mark.parametrize("pieces,T", [pytest.param(1, 12, id="1"), pytest.param(2, 12, id="2"), (1, 40), (2, 40)])
def test_label_logprob_vs_log_softmax_of_gemm_logits(gpu, pieces, T):
    """T = 40: the kernel's second trip of 32 positions, with a sequence whose only label sits in it"""
    torch.manual_seed(pieces)
    n_seq, d, V = 6, 256, 512
    cut = 9 if T == 12 else 37  # labels from position `cut` on are ignored
    R = n_seq * T
    h = torch.randn(R, d, device=DEV)
    E = torch.randn(V, d, device=DEV) * 0.05
    if pieces == 2:
        hd, Wd = U.inter(h), U.inter(E)
    else:
        hd, Wd = U.bf(h), U.bf(E)
    logits = torch.empty(R, V, device=DEV)
    part = torch.empty(R, V // 64, 2, device=DEV)
    lse = torch.empty(R, device=DEV)
    sp = _lib.Split(pieces, 0, 0, 0, 1.0)
    L = U.lib()
    _lib.check(L.gram_gemm_bf16_lse_split(hd.data_ptr(), Wd.data_ptr(), logits.data_ptr(), part.data_ptr(), R, V, d, pieces * d, V,
                                          C.byref(sp), U.stream()), "lse gemm")
    _lib.check(L.gram_lse_combine(part.data_ptr(), lse.data_ptr(), R, V // 64, U.stream()), "lse combine")
    g = torch.Generator().manual_seed(3)
    lab = torch.randint(0, V, (n_seq, T), generator=g)
    lab[:, cut:] = -100
    lab[0, :] = -100
    if T > 32:
        lab[1, :] = -100
        lab[1, 34] = 5
    lab = lab.to(DEV, torch.int32).contiguous()
    tok = torch.full((R,), 7.0, device=DEV)
    seq = torch.full((n_seq,), 7.0, device=DEV)
    E32 = E.contiguous()
    _lib.check(L.gram_label_logprob_split(hd.data_ptr(), Wd.data_ptr(), E32.data_ptr() if pieces == 2 else None, d, lse.data_ptr(),
                                          lab.data_ptr(), n_seq, T, V, pieces, tok.data_ptr(), seq.data_ptr(), U.stream()), "label logprob")
    torch.cuda.synchronize()
    lf = lab.view(-1).long()
    ref = torch.log_softmax(logits.double(), -1).gather(1, lf.clamp(min=0)[:, None])[:, 0]
    ref = torch.where(lf >= 0, ref, torch.zeros((), dtype=ref.dtype, device=DEV))
    err = float((tok.double() - ref).abs().max())
    serr = float((seq.double() - ref.view(n_seq, T).sum(1)).abs().max())
    print(f"label logprob pieces={pieces} T={T}: token {err:.2e}, sequence {serr:.2e}")
    assert err < 1e-3 and serr < 1e-2
    assert float(seq[0]) == 0.0 and torch.equal(tok.view(n_seq, T)[:, cut:], torch.zeros(n_seq, T - cut, device=DEV))
    if T > 32:
        assert float(tok[T + 34]) != 0.0 and float(seq[1]) == float(tok[T + 34])


# ---------------------------------------------------------------------------------------------------------- 4. teacher forced vs stepped
def test_teacher_forced_logits_vs_stepped_decode(gpu):
    oc = O.OracleConfig.named("t5-small", max_item_num=4)
    sd, m = _model(gpu, oc, 9)
    g = torch.Generator().manual_seed(9)
    B, N, L, Cn, T = 2, 3, 32, 4, 6
    ids, mask = _ragged(g, B, N, L, oc.vocab_size, pad_last=False)
    lab = _labels(g, (B, Cn, T), oc.vocab_size, min_len=T)
    dec = TF.shift_right(lab).to(DEV, torch.int32).contiguous()
    lib = _lib.load()
    for mode in _modes():
        m.set_precision(mode)
        h = m._pack()
        idd, mk = ids.to(DEV).contiguous(), mask.to(DEV).view(torch.uint8).contiguous()
        with torch.no_grad():
            logits_tf, _, _ = m._teacher_forced(idd, mk.bool(), dec, lab.to(DEV), want_logits=True)
        Tmax = T + 1
        need = lib.gram_workspace_bytes(h, B, N, L, Cn, Tmax)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        _lib.check(lib.gram_encode_fused(h, idd.data_ptr(), mk.data_ptr(), B, N, L, ws.data_ptr(), need, Cn, Tmax, None, U.stream()), "enc")
        anc = torch.arange(B * Cn, dtype=torch.int32, device=DEV).repeat(Tmax, 1).contiguous()
        worst, equal = 0.0, True
        for t in range(T):
            tokens = dec[:, :, t].reshape(-1).contiguous()
            lg = torch.empty(B * Cn, oc.vocab_size, device=DEV)
            _lib.check(lib.gram_decode_step(h, tokens.data_ptr(), anc.data_ptr(), mk.data_ptr(), B, N, L, Cn, Tmax, t, ws.data_ptr(), need,
                                            lg.data_ptr(), U.stream()), "decode step")
            torch.cuda.synchronize()
            ref = lg.view(B, Cn, -1)
            got = logits_tf[:, :, t]
            worst = max(worst, float((got - ref).abs().max()))
            equal &= torch.equal(got, ref)
        print(f"teacher forced vs stepped [{mode}]: max |logit diff| {worst:.2e}, bit-equal: {equal}")
        assert worst < _tol(mode)["logit"]


# ---------------------------------------------------------------------------------------------------------- 5. beam-score audit
def test_sequences_scores_equal_scored_sequences(gpu):
    from gram_amd.utils import generation_trie as gt
    oc = O.OracleConfig.named("t5-small", max_item_num=4)
    sd, m = _model(gpu, oc, 12)
    g = torch.Generator().manual_seed(12)
    B, N, L, K = 3, 3, 32, 10
    ids, mask = _ragged(g, B, N, L, oc.vocab_size, pad_last=False)
    cands = [[0, a, b, c, 1] for a in (5, 6, 7, 8) for b in (9, 10, 11) for c in (12, 13)] + [[0, 20, 21, 1], [0, 22, 1]]
    lp = 0.7  # (not 1: the normaliser's exponent is exercised)
    for mode in _modes():
        m.set_precision(mode)
        out = m.generate(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), max_length=5,
                         prefix_allowed_tokens_fn=gt.prefix_allowed_tokens_fn(gt.Trie(cands)), num_beams=K, num_return_sequences=K,
                         output_scores=True, return_dict_in_generate=True, length_penalty=lp)
        assert torch.isfinite(out["sequences_scores"]).all()  # (26 candidates: no -inf filler rows at K = 10)
        seqs, scores = out["sequences"].cpu(), out["sequences_scores"].cpu()
        lab = seqs[:, 1:].clone()
        T = lab.shape[1]
        # BeamHypotheses.add divides by the length of the hypothesis BEFORE its EOS is appended: the start token plus the tokens
        # ahead of EOS = the label count including EOS; a hypothesis finalised at max_length without EOS counts all max_length tokens
        hyp_len = torch.empty(lab.shape[0], dtype=torch.long)
        for r in range(lab.shape[0]):
            eos = (lab[r] == 1).nonzero()
            n = int(eos[0]) + 1 if eos.numel() else T
            hyp_len[r] = n if eos.numel() else T + 1
            lab[r, n:] = -100
        seq = m.score_sequences(ids.to(DEV), mask.to(DEV), lab.view(B, K, T).to(DEV)).cpu().view(-1)
        norm = seq.double() / hyp_len.double() ** lp
        dev = float((norm - scores.double()).abs().max())
        print(f"beam audit [{mode}]: max |score diff| {dev:.2e}, bit-equal: {torch.equal(norm.float(), scores)}")
        assert dev < _tol(mode)["logp"]


# ---------------------------------------------------------------------------------------------------------- 6. invariance / neutrality
def test_batch_invariance_and_cache_neutrality(gpu):
    oc = O.OracleConfig.named("t5-small", max_item_num=4)
    sd, m = _model(gpu, oc, 13)
    g = torch.Generator().manual_seed(13)
    B, N, L, Cn, T = 64, 3, 32, 3, 8
    ids, mask = _ragged(g, B, N, L, oc.vocab_size)
    ids[:, 1:] = ids[0, 1:]  # item passages shared across users: the cache has something to find
    mask[:, 1:] = mask[0, 1:]
    mask[-1, -1] = False
    ids[-1, -1] = 0
    lab = _labels(g, (B, Cn, T), oc.vocab_size)
    idd, mk, lb = ids.to(DEV), mask.to(DEV), lab.to(DEV)
    full, tok = m.score_sequences(idd, mk, lb, return_tokens=True)
    for b in (0, 17, 63):
        one, tok1 = m.score_sequences(idd[b:b + 1], mk[b:b + 1], lb[b:b + 1], return_tokens=True)
        assert torch.equal(one[0], full[b]) and torch.equal(tok1[0], tok[b]), b
    chunked = m.score_sequences(idd, mk, lb, users_per_call=5)
    assert torch.equal(chunked, full)
    m.cache_passages(idd[:, 1:], mk[:, 1:])
    cached = m.score_sequences(idd, mk, lb)
    m.clear_passage_cache()
    os.environ["GRAM_COMPACT"] = "0"
    try:
        plain = m.score_sequences(idd, mk, lb)
    finally:
        del os.environ["GRAM_COMPACT"]
    assert torch.equal(cached, full) and torch.equal(plain, full)


# ---------------------------------------------------------------------------------------------------------- 7. autograd
def test_backward_raises_and_no_grad_loss_is_plain(gpu):
    oc = _tiny()
    sd, m = _model(gpu, oc, 14)
    g = torch.Generator().manual_seed(14)
    ids, mask = _ragged(g, 2, 2, 32, oc.vocab_size)
    lab = _labels(g, (2, 5), oc.vocab_size).to(DEV)
    m.train()
    loss = m(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), labels=lab, return_dict=False)[0]
    assert loss.requires_grad
    with pytest.raises(NotImplementedError, match="backward"):
        loss.backward()
    m.eval()
    with torch.no_grad():
        out = m(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), labels=lab)
    assert not out.loss.requires_grad and out.loss.grad_fn is None
    assert torch.equal(out[0], out.loss)
    with pytest.raises(ValueError):
        m(input_ids=ids.to(DEV), attention_mask=mask.to(DEV))
    with pytest.raises(NotImplementedError):
        m(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), labels=lab, output_attentions=True)
    with pytest.raises(NotImplementedError):
        m(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), labels=lab, decoder_attention_mask=torch.zeros_like(lab))
    logits_only = m(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), decoder_input_ids=TF.shift_right(lab), return_dict=False)
    assert len(logits_only) == 1 and logits_only[0].shape == (2, 5, oc.vocab_size)


# ---------------------------------------------------------------------------------------------------------- 8. race screen
def test_race_screen_against_the_chaos_build(gpu, tmp_path):
    lib = os.path.join(ROOT, "gram_amd", "csrc", "libgram_hip_chaos.so")
    if not os.path.exists(lib):
        pytest.skip("libgram_hip_chaos.so not built (make -C gram_amd/csrc CHAOS=1)")
    res = {}
    for name, path in (("product", None), ("chaos", lib)):
        env = dict(os.environ)
        env.pop("GRAM_LIB", None)
        if path:
            env["GRAM_LIB"] = path
        out = str(tmp_path / f"{name}.pt")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tf_oracle.py"), "--child", out], env=env, timeout=600,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        res[name] = torch.load(out)
    assert torch.equal(res["product"]["seq"], res["chaos"]["seq"])
    assert torch.equal(res["product"]["tok"], res["chaos"]["tok"])
