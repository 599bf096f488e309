"""-m gpu: the whole path at the model shapes the library accepts beside the four named backbones.

gram_model_create takes any (d_model, n_heads, d_ff) with d_model and d_ff multiples of 128, d_model <= 1024 and an even n_heads <= 16;
inner = 64 * n_heads is independent of d_model.  The rest of the suite holds the path against the fp32 oracle at shapes with
inner == d_model and d_ff = 2 or 4 d_model only.  Here: six shapes, the smallest that flip each decision --

    (128,  4, 384)  inner = 256 > d; K = d = 128 (the ping-pong GEMM declines, the ring runs shorter than its stages); nblk = 2
    (384,  2, 640)  inner = 128 < d (wo GEMM K = 128); nblk = 6; no GEMM N a multiple of 256; inner % 256 != 0 in the bank epilogue
    (256,  6, 128)  inner = 384; d_ff < d, the smallest d_ff (wi is one 128-column tile, wo2 has K = 128)
    (128, 16, 256)  the largest inner (1024, QKV N = 3072) on the smallest d; H = 16
    (1024, 2, 128)  the largest d (a row kernel's v[4] full, nblk = 16) with the smallest inner and d_ff
    (640, 14, 896)  all three odd multiples of 128; inner > d; H = 14; nblk = 10

-- each with vocab 384 (an odd multiple of 128, as 32 128), 2 + 2 layers, max_item_num 5, weights from O.init_state_dict.  Per shape,
against the oracle on the same weights and inputs (ragged masks, one fully padded passage): the fused encoder, five decode steps with
beam reorders, generate (two pieces: the oracle's top-K; one piece: Trie membership and the teacher-forced decoder's score of every
returned row) and the teacher-forced pass (token log-probs, sequence sums, loss; both modes).  Bit for bit: token tables on / off, live
rows on / off, a user alone against the same user in batches on either side of both stacks' streaming / tiled GEMM boundary.  Two
shapes at 32 768 encoder and decoder rows, where 1/rms comes from gram_row_rscale_xs and the GEMMs the ping-pong kernel declines fall
back to the tiled kernels.  Two shapes with every gram_model_desc_t.w_scales slot at a power of its own.  The refused side of the
boundary: tests/test_model_shapes_host.py, and one GRAM with d_model = 1152 here.

Every tolerance is the suite's own (tests/test_gpu_path.py, tests/test_gpu_teacher_forced.py), unchanged.  Observed maxima on an MI355X
(f16 pieces), printed by the tests:

                    encoder          decode steps  generate              teacher forced: token logp / sequence sums / loss rel
    shape           rel / max abs    logit, logp   two pieces  one piece  two pieces                    one piece
    (128,  4, 384)  4.1e-7 / 2.2e-6  3.8e-6        1.4e-6      1.9e-7     2.2e-6 / 4.3e-6 / 4.0e-8      1.8e-3 / 2.8e-3 / 5.2e-5
    (384,  2, 640)  4.7e-7 / 2.5e-6  8.6e-6        2.9e-6      3.8e-7     4.5e-6 / 1.2e-5 / 3.0e-8      1.9e-3 / 3.7e-3 / 1.8e-5
    (256,  6, 128)  3.9e-7 / 1.9e-6  4.8e-6        2.9e-6      1.4e-4     3.0e-6 / 3.3e-6 / 7.3e-9      2.0e-3 / 4.8e-3 / 3.9e-5
    (128, 16, 256)  4.2e-7 / 1.7e-6  2.9e-6        1.4e-6      1.6e-7     1.6e-6 / 2.8e-6 / 2.2e-9      1.3e-3 / 2.5e-3 / 8.7e-6
    (1024, 2, 128)  5.2e-7 / 2.6e-6  1.1e-5        4.8e-6      3.8e-7     8.8e-6 / 8.5e-6 / 8.3e-8      1.8e-3 / 2.6e-3 / 1.1e-5
    (640, 14, 896)  5.4e-7 / 2.6e-6  1.1e-5        4.8e-6      2.7e-4     8.4e-6 / 2.0e-5 / 2.6e-7      1.6e-3 / 2.2e-3 / 9.7e-6
    tolerance       1e-5 / 5e-5      5e-5          2e-5        2e-2       1e-4 / 6e-4 / 1e-5            2e-2 / 1.2e-1 / 2e-2
  (generate, two pieces: |score - the oracle's score of the same sequence|; one piece: |score - the teacher-forced decoder's score of
  the same row|, held to the one-piece log-prob tolerance 2e-2.)
    32 768 rows, two pieces, users 0 and 511 against the oracle: (384, 2, 640) 3.8e-6, (128, 4, 384) 1.4e-6
    weight-scale slots (untied lm_head, |logit| up to 27): generate P / Q; token logp two pieces P / Q; one piece P / Q
    (384,  2, 640)  3.8e-6 / 5.7e-6;  6.5e-6 / 6.9e-6;  1.0e-2 / 7.2e-3
    (640, 14, 896)  7.6e-6 / 1.9e-5;  2.2e-5 / 2.0e-5;  1.6e-2 / 1.8e-2
  The last two rows sit close to SCORE_TOL and to the one-piece 2e-2 because an untied lm_head has no d^-0.5 rescale: the logits
  reach 25-27 where the tied models' are O(1), and the deviations grow with them.  The fp32 oracle against itself in fp64 on these
  four models differs by 6.3e-6 - 8.3e-6 (d = 384) and 1.4e-5 - 1.8e-5 (d = 640) in token log-prob, and its sequence scores (-8 to -13
  here) move by up to 3.8e-6 (d = 384) and 9.5e-6 (d = 640) between 8 and 16 CPU threads: the two-piece figures are the oracle's own
  rounding, spread over every token, not one operator's.  With two w_scales entries of GRAM._pack exchanged (enc_wqkv of layers 0
  and 1) the same test fails by 0.22 and 0.92 in the first score it compares.
"""
import functools
import math
import types

import pytest
import torch

from gram_amd import _lib
from oracle import gram_oracle as O
from tests import test_gpu_path as P
from tests import tf_oracle as TF
from tests.test_gpu_configs import ONE, TWO
from tests.test_gpu_path import DEV, SCORE_TOL, _check_generate, _inputs, _random_items
from tests.test_gpu_scale import THRESHOLD, _released, _rescored, _same_rows
from tests.test_gpu_teacher_forced import _labels, _tol

pytestmark = pytest.mark.gpu

V = 384
SHAPES = [(128, 4, 384), (384, 2, 640), (256, 6, 128), (128, 16, 256), (1024, 2, 128), (640, 14, 896)]
BIG_SHAPES = [(384, 2, 640), (128, 4, 384)]
SCALE_SHAPES = [(384, 2, 640), (640, 14, 896)]
MODES = [TWO, ONE]
_id = lambda s: "-".join(str(v) for v in s) if isinstance(s, tuple) else str(s)  # noqa: E731
shapes = pytest.mark.parametrize("shape", SHAPES, ids=_id)
modes = pytest.mark.parametrize("mode", MODES)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gram_amd
    return gram_amd


def _oc(shape, **kw):
    d, h, f = shape
    return O.OracleConfig(vocab_size=V, d_model=d, d_kv=64, d_ff=f, num_layers=2, num_decoder_layers=2, num_heads=h, max_item_num=5, **kw)


def _gen(m, ids, mask, cands, K):
    return P._gen(m, ids, mask, max(len(c) for c in cands), _fn(cands), K)


def _fn(cands, _cache={}):
    from gram_amd.utils import generation_trie as gt
    if id(cands) not in _cache:
        _cache[id(cands)] = (cands, gt.prefix_allowed_tokens_fn(gt.Trie(cands)))  # (cands kept: its id stays its own)
    return _cache[id(cands)][1]


def _tf_refs(sd, oc, ids, mask, lab):
    """oracle token log-probs (B * C, T), and the loss of every user's first sequence"""
    B, C, T = lab.shape
    logits = TF.teacher_forced_logits(sd, oc, ids, mask, TF.shift_right(lab.view(B * C, T)))
    _, tok = TF.loss_and_token_logp(logits, lab.view(B * C, T))
    loss, _ = TF.loss_and_token_logp(logits.view(B, C, T, -1)[:, 0], lab[:, 0])
    return tok, float(loss)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """One shape's weights, inputs and oracle results, computed once and shared (read only) by the tests of that shape."""
    oc = _oc(shape)
    sd = O.init_state_dict(oc, 11)
    g = torch.Generator().manual_seed(1000 + shape[0] + shape[1])
    B, N, L, K, C, T = 3, 2, 32, 6, 2, 6
    ids, mask = _inputs(g, B, N, L, V)
    cands = _random_items(g, 60, 2, 4, 60)
    lab = _labels(g, (B, C, T), V)
    ref = O.generate(sd, oc, ids, mask, max(len(c) for c in cands), O.prefix_allowed_tokens_fn(O.Trie(cands)), K, K, 1.0)
    ref_tok, ref_loss = _tf_refs(sd, oc, ids, mask, lab)
    return types.SimpleNamespace(oc=oc, sd=sd, ids=ids, mask=mask, cands=cands, K=K, lab=lab, ref=ref, ref_tok=ref_tok, ref_loss=ref_loss,
                                 enc_ref=O.encode_fused(sd, oc, ids, mask))


_MODELS = {}


def _model(gpu, shape, mode):
    """the shape's model in one precision mode (one instance per mode: no repacking between the tests)"""
    if (shape, mode) not in _MODELS:
        c = _case(shape)
        m = P._model(gpu, c.oc, 11, sd=c.sd)[2]
        m.set_precision(mode)
        _MODELS[shape, mode] = m
    return _MODELS[shape, mode]


def _tf(m, ids, mask, lab):
    """(token log-probs (B, C, T), sequence sums (B, C)) of one score_sequences call on the whole batch, on the host"""
    seq, tok = m.score_sequences(ids.to(DEV), mask.to(DEV), lab.to(DEV), return_tokens=True, users_per_call=ids.shape[0])
    return tok.cpu(), seq.cpu()


def _check_tf(m, mode, sd, oc, ids, mask, lab, ref_tok, ref_loss, tag):
    """token log-probs, sequence sums and the loss against the oracle's, at the teacher-forced tolerances of the mode"""
    B, C, T = lab.shape
    tol = _tol(mode)
    tok, seq = _tf(m, ids, mask, lab)
    with torch.no_grad():
        loss = float(m(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), labels=lab[:, 0].to(DEV)).loss)
    dt = float((tok.view(B * C, T).double() - ref_tok).abs().max())
    ds = float((seq.view(-1).double() - ref_tok.sum(-1)).abs().max())
    rel = abs(loss - ref_loss) / abs(ref_loss)
    print(f"[teacher forced {tag} {mode}] token logp {dt:.2e}, sequence sums {ds:.2e}, loss rel {rel:.2e}")
    assert dt < tol["logp"] and ds < tol["logp"] * T and rel < tol["loss"], (dt, ds, rel)


# ---------------------------------------------------------------------------------------------------------- 1. against the oracle
@shapes
def test_encoder_vs_oracle(gpu, shape):
    c = _case(shape)
    P._check_encoder(_model(gpu, shape, TWO), c.ids, c.mask, c.enc_ref, _id(shape))


@shapes
def test_decode_steps_vs_oracle(gpu, shape):
    c = _case(shape)
    worst = P._check_decode_steps(c.oc, c.sd, _model(gpu, shape, TWO), torch.Generator().manual_seed(8), 2, 2, 32, 3, 5)
    print(f"[decode steps {_id(shape)}] max |logit / log-prob err| over 5 steps {worst:.2e}")


@modes
@shapes
def test_generate_vs_oracle(gpu, shape, mode):
    """Two pieces: the oracle's top-K at SCORE_TOL.  One piece: every returned row is a Trie member whose score is the teacher-forced
    decoder's score of that row (generate and the teacher-forced pass are two independent decoders)."""
    c = _case(shape)
    m = _model(gpu, shape, mode)
    out = _gen(m, c.ids, c.mask, c.cands, c.K)
    seqs, scores = out["sequences"].cpu(), out["sequences_scores"].cpu()
    assert seqs.shape[0] == c.ids.shape[0] * c.K and bool(torch.isfinite(scores).all())
    if mode == TWO:
        assert seqs.shape[1] == c.ref["sequences"].shape[1]
        _check_generate(c.oc, c.sd, out, c.ref, c.ids, c.mask, c.cands, c.K, tol=SCORE_TOL)
    else:
        cand_set = {tuple(x) for x in c.cands}
        for r in seqs.tolist():
            while r and r[-1] == 0:
                r.pop()
            assert tuple(r) in cand_set, r
        audit = float((_rescored(m, c.ids, c.mask, seqs, c.K) - scores.double()).abs().max())
        print(f"[generate {_id(shape)} {mode}] beam audit: max |score - teacher-forced score of the same row| {audit:.2e}")
        assert audit < _tol(mode)["logp"], audit


@modes
@shapes
def test_teacher_forced_vs_oracle(gpu, shape, mode):
    c = _case(shape)
    _check_tf(_model(gpu, shape, mode), mode, c.sd, c.oc, c.ids, c.mask, c.lab, c.ref_tok, c.ref_loss, _id(shape))


# ---------------------------------------------------------------------------------------------------------- 2. bit for bit
def _on_off(gpu, shape, mode, hook):
    c = _case(shape)
    m = _model(gpu, shape, mode)
    got = []
    try:
        for on in (1, 0):
            hook(on)
            out = _gen(m, c.ids, c.mask, c.cands, c.K)
            got.append((out["sequences"].cpu(), out["sequences_scores"].cpu(), _tf(m, c.ids, c.mask, c.lab)[0]))
    finally:
        hook(-1)
    (s1, v1, t1), (s0, v0, t0) = got
    assert bool(torch.isfinite(v1).all())
    assert torch.equal(s1, s0) and torch.equal(v1, v0) and torch.equal(t1, t0)


@modes
@shapes
def test_token_tables_on_and_off(gpu, shape, mode):
    assert _model(gpu, shape, mode)._pack() and _model(gpu, shape, mode)._token_tables is not None
    _on_off(gpu, shape, mode, _lib.load().gram_debug_set_token_tables)


@modes
@shapes
def test_live_rows_on_and_off(gpu, shape, mode):
    _on_off(gpu, shape, mode, _lib.load().gram_debug_set_live_rows)


@modes
@shapes
def test_a_user_alone_and_inside_larger_batches(gpu, shape, mode):
    """K = 8, N = 1, L = 32 (one 32-row passage and 8 decoder rows per user).  B = 1: 8 / 32 rows, the streaming GEMM with quarter
    partials; B = 64: 512 decoder rows, its last size; B = 65: the first tiled decoder size; B = 17: 544 encoder rows, the first
    tiled encoder size.  User 0 and the last user of each call get the bits they get alone (the promise of max_users_per_call)."""
    stream_max = _lib.load().gram_gemm_stream_max_m()
    K, N, L, C, T = 8, 1, 32, 2, 6
    assert 64 * K == stream_max and 16 * N * L == stream_max, stream_max  # (the sizes below sit on the boundary)
    c = _case(shape)
    m = _model(gpu, shape, mode)
    g = torch.Generator().manual_seed(65)
    ids, mask = _inputs(g, 65, N, L, V)
    lab = _labels(g, (65, C, T), V)
    solo = {}
    for u in (0, 16, 63, 64):
        out = _gen(m, ids[u:u + 1], mask[u:u + 1], c.cands, K)
        solo[u] = (out["sequences"].cpu(), out["sequences_scores"].cpu(), _tf(m, ids[u:u + 1], mask[u:u + 1], lab[u:u + 1])[0])
        assert bool(torch.isfinite(solo[u][1]).all())
    for B in (64, 65, 17):
        out = _gen(m, ids[:B], mask[:B], c.cands, K)
        seqs, scores = out["sequences"].cpu(), out["sequences_scores"].cpu()
        tok = _tf(m, ids[:B], mask[:B], lab[:B])[0]
        for u in (0, B - 1):
            s1, v1, t1 = solo[u]
            assert _same_rows(s1, seqs[u * K:(u + 1) * K]), (B, u)
            assert torch.equal(v1, scores[u * K:(u + 1) * K]), (B, u)
            assert torch.equal(t1[0], tok[u]), (B, u)


# ---------------------------------------------------------------------------------------------------------- 3. 32 768 rows
@modes
@pytest.mark.parametrize("shape", BIG_SHAPES, ids=_id)
def test_generate_at_32768_rows(gpu, shape, mode):
    """B = 512, N = 2, L = 32, K = 64: 32 768 encoder rows and 32 768 decoder rows.  NormChain::pre_rs hands 1/rms from
    gram_row_rscale_xs to GEMMs the ping-pong kernel declines (N % 256 != 0, K / 64 < 4, inner % 256 != 0 in the bank epilogue), which
    run on the tiled kernels.  Users 0, 255 and 511 get the bits they get alone and in a call of the three; two pieces: users 0 and 511
    against the oracle."""
    c = _case(shape)
    m = _model(gpu, shape, mode)
    B, N, L, K = 512, 2, 32, _lib.GRAM_MAX_BEAMS
    assert B * K >= THRESHOLD and B * N * L >= THRESHOLD
    g = torch.Generator().manual_seed(512 + shape[0])
    ids, mask = _inputs(g, B, N, L, V)
    cands = _random_items(g, 240, 2, 4, 60)
    assert len(cands) >= 200
    users = [0, 255, 511]
    try:
        big = _gen(m, ids, mask, cands, K)
        seqs, scores = big["sequences"].cpu(), big["sequences_scores"].cpu()
        assert bool(torch.isfinite(scores).all())  # (no user ran short of hypotheses)
        three = _gen(m, ids[users], mask[users], cands, K)
        for j, u in enumerate(users):
            alone = _gen(m, ids[u:u + 1], mask[u:u + 1], cands, K)
            for o, rows in ((alone, slice(0, K)), (three, slice(j * K, (j + 1) * K))):
                assert _same_rows(o["sequences"][rows], seqs[u * K:(u + 1) * K]), u
                assert torch.equal(o["sequences_scores"][rows].cpu(), scores[u * K:(u + 1) * K]), u
    finally:
        _released(m)
    if mode == TWO:
        ends = [0, 511]
        ref = O.generate(c.sd, c.oc, ids[ends], mask[ends], max(len(x) for x in cands), O.prefix_allowed_tokens_fn(O.Trie(cands)), K, K, 1.0)
        rows = torch.cat([torch.arange(u * K, (u + 1) * K) for u in ends])
        _check_generate(c.oc, c.sd, dict(sequences=seqs[rows], sequences_scores=scores[rows]), ref, ids[ends], mask[ends], cands, K,
                        tol=SCORE_TOL)


# ---------------------------------------------------------------------------------------------------------- 4. the weight-scale slots
def _scale_slots(n_enc, n_dec):
    """gram_model_desc_t.w_scales, slot by slot in the header's order: (the state dict's matrices that share the slot, the norm gain
    GRAM._pack folds into them or None)"""
    e, d = "encoder.encoder.block.{}.module.layer", "decoder.block.{}.layer"
    qkv = lambda p: [p + ".q.weight", p + ".k.weight", p + ".v.weight"]  # noqa: E731
    enc, dec = [e.format(i) for i in range(n_enc)], [d.format(i) for i in range(n_dec)]
    slots = [(qkv(p + ".0.SelfAttention"), p + ".0.layer_norm.weight") for p in enc]
    slots += [([p + ".0.SelfAttention.o.weight"], None) for p in enc]
    slots += [([p + ".1.DenseReluDense.wi.weight"], p + ".1.layer_norm.weight") for p in enc]
    slots += [([p + ".1.DenseReluDense.wo.weight"], None) for p in enc]
    slots += [(qkv(p + ".0.SelfAttention"), p + ".0.layer_norm.weight") for p in dec]
    slots += [([p + ".0.SelfAttention.o.weight"], None) for p in dec]
    slots += [([p + ".1.EncDecAttention.q.weight"], p + ".1.layer_norm.weight") for p in dec]
    slots += [([p + ".1.EncDecAttention.o.weight"], None) for p in dec]
    slots += [([p + ".2.DenseReluDense.wi.weight"], p + ".2.layer_norm.weight") for p in dec]
    slots += [([p + ".2.DenseReluDense.wo.weight"], None) for p in dec]
    slots += [([p + ".1.EncDecAttention." + kv + ".weight" for p in dec for kv in "kv"], None)]
    slots += [(["lm_head.weight"], None)]
    assert len(slots) == 4 * n_enc + 6 * n_dec + 2
    return slots


def _slot_power(sd, slot):
    """floor(log2 amax) of the matrix a slot's scale is computed from (GRAM._pack: the gain folded in, q|k|v and all k|v as one matrix)"""
    names, gain = slot
    amax = max(float((sd[n] * (sd[gain][None, :] if gain else 1.0)).abs().max()) for n in names)
    return math.floor(math.log2(amax))


def _scaled_pair(oc):
    """Two state dicts whose matrices are multiplied, slot by slot, by 2^e, e in [-2, 2], chosen so that the pair of powers
    (floor(log2 amax) in P, in Q) differs between any two slots.  lm_head takes the smallest pair (logits stay small); the other slots
    take, in order, the pair of smallest exponents that is still free."""
    P_, Q_ = dict(O.init_state_dict(oc, 21)), dict(O.init_state_dict(oc, 22))
    slots = _scale_slots(oc.num_layers, oc.num_decoder_layers)
    grid = [(a, b) for a in range(-2, 3) for b in range(-2, 3)]
    taken, exps = set(), {}
    for s in [len(slots) - 1] + list(range(len(slots) - 1)):
        base = (_slot_power(P_, slots[s]), _slot_power(Q_, slots[s]))
        smallest = lambda e: (e[0] + e[1], e)  # noqa: E731
        nearest_zero = lambda e: (max(abs(e[0]), abs(e[1])), abs(e[0]) + abs(e[1]), e)  # noqa: E731
        order = sorted(grid, key=smallest if s == len(slots) - 1 else nearest_zero)
        e = next(e for e in order if (base[0] + e[0], base[1] + e[1]) not in taken)  # (25 candidates, at most 21 taken)
        taken.add((base[0] + e[0], base[1] + e[1]))
        exps[s] = e
    for s, (names, _) in enumerate(slots):
        for n in names:
            P_[n] = P_[n] * 2.0 ** exps[s][0]
            Q_[n] = Q_[n] * 2.0 ** exps[s][1]
    return P_, Q_, slots


@pytest.mark.parametrize("shape", SCALE_SHAPES, ids=_id)
def test_every_weight_scale_slot_at_a_power_of_its_own(gpu, shape):
    """GRAM._pack collects one power of two per weight matrix in call order and rotates the list into the order of
    gram_model_desc_t.w_scales; at random init nearly every matrix gets the same power, and two slots exchanged change nothing.  Here
    two models, P and Q (untied lm_head), whose 22 slots carry 22 different pairs of powers: any assignment of scales to slots but the
    right one puts at least one GEMM off by a factor of 2 or more in at least one of them.  Generate (two pieces) and the teacher-forced
    token log-probs (both modes) against the oracle at the ordinary tolerances.  The PIECE=bf16 build scales nothing -- every
    w_scales entry is 1 -- so there the slot order is trivially right and the test has nothing of its own to catch.  (Run against
    that build, the generate and two-piece comparisons pass; the one-piece token log-probs of the P models come out at 6.2e-2
    (384, 2, 640) and 1.4e-1 (640, 14, 896) against the 2e-2 the one-piece modes share, and the test fails there: |logit| ~ 25 of the
    untied head times bfloat16's 2^-9.  The default f16 build, which the suite runs, observes 1.0e-2 and 1.6e-2.)"""
    oc = _oc(shape, tie_word_embeddings=False)
    sd_p, sd_q, slots = _scaled_pair(oc)
    pairs = [(_slot_power(sd_p, s), _slot_power(sd_q, s)) for s in slots]
    assert len(pairs) == 22 and len(set(pairs)) == 22, pairs
    g = torch.Generator().manual_seed(2200 + shape[0])
    B, N, L, K, C, T = 3, 2, 32, 6, 2, 6
    ids, mask = _inputs(g, B, N, L, V)
    cands = _random_items(g, 60, 2, 4, 60)
    lab = _labels(g, (B, C, T), V)
    for name, sd in (("P", sd_p), ("Q", sd_q)):
        ref = O.generate(sd, oc, ids, mask, max(len(c) for c in cands), O.prefix_allowed_tokens_fn(O.Trie(cands)), K, K, 1.0)
        assert bool(torch.isfinite(ref["sequences_scores"]).all())
        ref_tok, ref_loss = _tf_refs(sd, oc, ids, mask, lab)
        m = P._model(gpu, oc, 0, sd=sd)[2]
        for mode in MODES:
            m.set_precision(mode)
            if mode == TWO:
                _check_generate(oc, sd, _gen(m, ids, mask, cands, K), ref, ids, mask, cands, K, tol=SCORE_TOL)
            _check_tf(m, mode, sd, oc, ids, mask, lab, ref_tok, ref_loss, f"{_id(shape)} scales {name}")


# ---------------------------------------------------------------------------------------------------------- 5. the refused side
def test_a_model_wider_than_1024_is_refused_before_any_launch(gpu):
    cfg = gpu.T5Config(vocab_size=V, d_model=1152, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2, max_item_num=5)
    torch.manual_seed(0)
    m = gpu.create_model("gram", cfg).to(DEV).eval()
    c = _case(SHAPES[0])
    with pytest.raises(_lib.GramHipError, match="gram_model_create rejected"):
        _gen(m, c.ids, c.mask, c.cands, c.K)
    assert m._packed is None and m._workspace is None  # (no handle, no workspace: nothing was launched)
