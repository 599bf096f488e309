"""-m gpu: the whole scoring path (gram_amd.GRAM.generate -> gram_generate in libgram_hip.so) against
the oracle on the same weights and inputs, plus the golden vectors made from the reference.

The HIP path computes in the model's default arithmetic -- the two-piece mode "f16x3": every operand as two IEEE-half
pieces, three MFMA products per product (~2^-22), fp32 accumulation -- and the reference in fp32, so floating-point
results are compared within stated tolerances (each <= 10x the deviation observed in this mode, printed by the tests)
and the *integer* results (which items, in which order) through tolerance-aware checks: a returned sequence must be a
Trie member, its score must match the oracle's score of that same sequence, and any disagreement in membership/order
must be between candidates whose oracle scores are closer than the tolerance."""
import os

import numpy as np
import pytest
import torch

from oracle import gram_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
from gram_amd import _lib as _L

F16 = _L.piece_dtype() == torch.float16
# default (two-piece) mode, every tolerance <= 10x the deviation observed with f16 pieces (gpurun r03b: logits 5.0e-6, log-probs
# 5.7e-6, fused encoder states 9.3e-7 relative / 4.8e-6 abs at T5-base, sequence scores 1.9e-6 -- fp32's own rounding: the oracle's
# summation order differs).  The PIECE=bf16 build carries 2^-18 per product: 16x these.
X = 1.0 if F16 else 16.0
LOGIT_TOL = 5e-5 * X
ENC_REL_TOL = 1e-5 * X
ENC_ABS_TOL = 5e-5 * X
SCORE_TOL = 2e-5 * X


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gram_amd
    return gram_amd


def _cfgs(name):
    """(OracleConfig, T5Config) of a named backbone, or of an OracleConfig as given"""
    if isinstance(name, O.OracleConfig):
        oc = name
    elif name == "tiny":
        oc = O.OracleConfig(vocab_size=256, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2,
                            max_item_num=5)
    elif name == "small":
        oc = O.OracleConfig.named("t5-small", max_item_num=4)
    else:
        oc = O.OracleConfig.named(name)
    from gram_amd import T5Config
    gc = T5Config(vocab_size=oc.vocab_size, d_model=oc.d_model, d_ff=oc.d_ff, num_layers=oc.num_layers,
                  num_decoder_layers=oc.num_decoder_layers, num_heads=oc.num_heads, max_item_num=oc.max_item_num,
                  tie_word_embeddings=oc.tie_word_embeddings)
    return oc, gc


def _model(gpu, name, seed, sd=None):
    """name: a backbone name or an OracleConfig; sd: the weights to load instead of init_state_dict(oc, seed)"""
    oc, gc = _cfgs(name)
    if sd is None:
        sd = O.init_state_dict(oc, seed)
    m = gpu.create_model("gram", gc)
    m.load_state_dict(sd)
    return oc, sd, m.to(DEV).eval()


def _inputs(g, B, N, L, V, ragged=True):
    ids = torch.randint(2, V, (B, N, L), generator=g)
    mask = torch.ones(B, N, L, dtype=torch.bool)
    if ragged:
        for b in range(B):
            for n in range(N):
                ln = int(torch.randint(max(2, L // 3), L + 1, (1,), generator=g))
                mask[b, n, ln:] = False
                ids[b, n, ln - 1] = 1
                ids[b, n, ln:] = 0
        if N > 1:
            mask[B - 1, N - 1] = False  # one fully padded passage
            ids[B - 1, N - 1] = 0
    return ids, mask


def _encode_device(m, ids, mask, K=2, max_length=6):
    from gram_amd import _lib
    lib = _lib.load()
    handle = m._pack()
    B, N, L = ids.shape
    ws = m._get_workspace(handle, B, N, L, K, max_length)
    d = m.config.d_model
    pieces = m._PIECES[m.precision]  # two-piece mode: the fused encoder states come back interleaved, [B*N*L][2 d]
    assert pieces == 2
    enc = torch.empty(B * N * L, 2 * d, dtype=_L.piece_dtype(), device=DEV)
    idd = ids.to(DEV).contiguous()
    mk = mask.to(DEV).view(torch.uint8).contiguous()
    rc = lib.gram_encode_fused(handle, idd.data_ptr(), mk.data_ptr(), B, N, L, ws.data_ptr(), ws.numel(), K, max_length,
                               enc.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "gram_encode_fused")
    return _L.deinterleave(enc).double().sum(0).float().cpu().view(B, N * L, d), ws, mk, handle


def _check_encoder(m, ids, mask, ref, tag):
    """gram_encode_fused (two-piece mode) against the oracle's fused encoder states `ref`, over the valid positions;
    returns (relative, max abs) deviation"""
    B = ids.shape[0]
    enc, *_ = _encode_device(m, ids, mask)
    valid = mask.reshape(B, -1)
    err = (enc - ref)[valid]
    rel = err.norm() / ref[valid].norm()
    # hidden states are O(1) after the final RMSNorm
    print(f"[encoder {tag}] rel {float(rel):.2e} max abs {float(err.abs().max()):.2e}")
    assert rel < ENC_REL_TOL, float(rel)
    assert err.abs().max() < ENC_ABS_TOL, float(err.abs().max())
    return float(rel), float(err.abs().max())


@pytest.mark.parametrize("name,B,N,L", [("tiny", 2, 3, 32), ("tiny", 3, 2, 64), ("small", 2, 2, 128), ("t5-base", 1, 3, 32)])
def test_encoder_fused_vs_oracle(gpu, name, B, N, L):
    oc, sd, m = _model(gpu, name, 11)
    g = torch.Generator().manual_seed(3)
    ids, mask = _inputs(g, B, N, L, min(oc.vocab_size, 32100))
    _check_encoder(m, ids, mask, O.encode_fused(sd, oc, ids, mask), name)


def test_encoder_matches_reference_golden(gpu, golden_dir):
    """Directly against the reference's own output (tests/golden/ref_tiny.npz)."""
    z = np.load(os.path.join(golden_dir, "ref_tiny.npz"))
    oc, sd, m = _model(gpu, "tiny", int(z["seed"]))
    ids, mask = torch.from_numpy(z["input_ids"]), torch.from_numpy(z["attention_mask"])
    enc, *_ = _encode_device(m, ids, mask)
    ref = torch.from_numpy(z["enc_fused"])
    valid = mask.reshape(mask.shape[0], -1)
    rel = (enc - ref)[valid].norm() / ref[valid].norm()
    print(f"[encoder golden] rel {float(rel):.2e}")
    assert rel < ENC_REL_TOL, float(rel)


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_decode_steps_vs_oracle(gpu, name):
    """gram_decode_step logits for a fixed token stream with beam reorders, vs the oracle's cached
    decoder (= the reference's tuple cache + _reorder_cache, pinned by tests/golden)."""
    oc, sd, m = _model(gpu, name, 11)
    _check_decode_steps(oc, sd, m, torch.Generator().manual_seed(8), 2, 2, 32, 3, 5)


def _check_decode_steps(oc, sd, m, g, B, N, L, K, T):
    """T steps of gram_decode_step on random tokens, the beams reordered after each, against O.decoder_step; returns the largest
    deviation of the logits and of the log-probs"""
    from gram_amd import _lib
    V = oc.vocab_size
    worst = 0.0
    ids, mask = _inputs(g, B, N, L, min(V, 32100))
    _, ws, mk, handle = _encode_device(m, ids, mask, K=K, max_length=T + 1)
    enc_ref = O.encode_fused(sd, oc, ids, mask)
    ext = ((1.0 - mask.reshape(B, -1).float().repeat_interleave(K, 0)) * O.FMIN)[:, None, None, :]
    st = O.DecodeState(O.cross_kv(sd, oc, enc_ref), ext, K)
    R = B * K
    anc = torch.arange(R, dtype=torch.int32).repeat(T + 1, 1).to(DEV)
    logits = torch.empty(R, V, dtype=torch.float32, device=DEV)
    lib = _lib.load()
    for t in range(T):
        toks = torch.randint(2, min(V, 32100), (R,), generator=g)
        if t == 0:
            toks[:] = 0
        ref = O.decoder_step(sd, oc, toks, st)
        rc = lib.gram_decode_step(handle, toks.int().to(DEV).data_ptr(), anc.data_ptr(), mk.data_ptr(), B, N, L, K, T + 1, t,
                                  ws.data_ptr(), ws.numel(), logits.data_ptr(), torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "gram_decode_step")
        got = logits.cpu()
        # logits are O(1) (tied head, d^-0.5 rescale); bf16 operand error accumulates over the decoder layers
        lp_err = (torch.log_softmax(got, -1) - torch.log_softmax(ref, -1)).abs().max()
        print(f"[decode step {t}] max |logit err| {float((got - ref).abs().max()):.2e}  max |log-prob err| {float(lp_err):.2e}")
        assert (got - ref).abs().max() < LOGIT_TOL, (t, float((got - ref).abs().max()))
        assert lp_err < LOGIT_TOL, (t, float(lp_err))
        worst = max(worst, float((got - ref).abs().max()), float(lp_err))
        parent = torch.cat([torch.randperm(K, generator=g) + b * K for b in range(B)])
        st.reorder(parent)
        a = anc.cpu()
        new = a.clone()
        new[:t, :] = a[:t, parent]
        new[t, :] = parent.int()
        anc.copy_(new)
    return worst


def _random_items(g, n_items, depth_lo, depth_hi, tok_hi):
    items = set()
    while len(items) < n_items:
        d = int(torch.randint(depth_lo, depth_hi + 1, (1,), generator=g))
        items.add(tuple(int(x) for x in torch.randint(2, tok_hi, (d,), generator=g)))
    return [[0] + list(it) + [1] for it in sorted(items)]


def _check_generate(oc, sd, out, ref, ids, mask, cands, K, tol, lp=1.0):
    """Tolerance-aware comparison of device vs oracle top-K lists (see module docstring)."""
    cand_set = {tuple(c) for c in cands}
    B = ids.shape[0]
    seqs, scores = out["sequences"].cpu(), out["sequences_scores"].cpu()
    rseqs, rscores = ref["sequences"], ref["sequences_scores"]

    def strip(row):
        row = [int(x) for x in row]
        while row and row[-1] == 0:
            row.pop()
        return tuple(row)

    n_order_diff = 0
    max_dev = 0.0
    for b in range(B):
        dev = [strip(r) for r in seqs[b * K:(b + 1) * K]]
        orc = [strip(r) for r in rseqs[b * K:(b + 1) * K]]
        osc = {s: float(v) for s, v in zip(orc, rscores[b * K:(b + 1) * K])}
        assert len(set(dev)) == K, "duplicate hypotheses"
        kth = float(rscores[(b + 1) * K - 1])
        dsc = scores[b * K:(b + 1) * K]
        assert all(dsc[i] >= dsc[i + 1] for i in range(K - 1)), "scores not descending"
        for i, s in enumerate(dev):
            assert s in cand_set, f"user {b}: {s} is not a Trie member"
            if s in osc:
                exact = osc[s]
            else:  # not in the oracle's top-K: must be a near-miss of the K-th score
                exact = O.sequence_logprob(sd, oc, ids[b:b + 1], mask[b:b + 1], list(s)) / (len(s) - 1) ** lp
                assert exact > kth - 2 * tol, (b, s, exact, kth)
            assert abs(float(dsc[i]) - exact) < tol, (b, s, float(dsc[i]), exact)
            max_dev = max(max_dev, abs(float(dsc[i]) - exact))
        # order: any inversion w.r.t. oracle scores must be within tolerance
        ex = [osc.get(s) for s in dev]
        for i in range(K - 1):
            if ex[i] is not None and ex[i + 1] is not None and ex[i] < ex[i + 1]:
                assert ex[i + 1] - ex[i] < 2 * tol
                n_order_diff += 1
    print(f"[generate parity] max |score - oracle score of the same sequence| = {max_dev:.2e} (tol {tol}); tolerated order inversions {n_order_diff}")
    return n_order_diff


@pytest.mark.parametrize("name,B,N,L,K,n_items,depth", [
    ("tiny", 4, 3, 32, 4, 40, (3, 3)), ("tiny", 3, 2, 48, 6, 60, (2, 4)), ("tiny", 2, 1, 32, 20, 200, (3, 4)),
    ("small", 2, 2, 64, 8, 100, (3, 4)),
])
def test_generate_vs_oracle(gpu, name, B, N, L, K, n_items, depth):
    from gram_amd.utils import generation_trie as gt
    oc, sd, m = _model(gpu, name, 11)
    g = torch.Generator().manual_seed(B * 100 + K)
    ids, mask = _inputs(g, B, N, L, min(oc.vocab_size, 32100))
    cands = _random_items(g, n_items, depth[0], depth[1], 60)
    max_length = max(len(c) for c in cands)
    ref = O.generate(sd, oc, ids, mask, max_length, O.prefix_allowed_tokens_fn(O.Trie(cands)), K, K, 1.0)
    fn = gt.prefix_allowed_tokens_fn(gt.Trie(cands))
    out = m.generate(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), max_length=max_length, prefix_allowed_tokens_fn=fn,
                     num_beams=K, num_return_sequences=K, output_scores=True, return_dict_in_generate=True, length_penalty=1.0)
    assert out["sequences"].shape[0] == B * K and out["sequences"].dtype == torch.int64
    assert out["sequences"].shape[1] == ref["sequences"].shape[1]
    assert bool((out["sequences"][:, 0] == 0).all())
    _check_generate(oc, sd, out, ref, ids, mask, cands, K, tol=SCORE_TOL)


def _gen(m, ids, mask, max_length, fn, K):
    return m.generate(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), max_length=max_length, prefix_allowed_tokens_fn=fn,
                      num_beams=K, num_return_sequences=K, output_scores=True, return_dict_in_generate=True, length_penalty=1.0)


def test_long_ids_decode_to_48_tokens(gpu):
    """max_length past round 3's 32-step limit (GRAM_MAX_DEC_LEN = 64: the reference's "term" id type decodes with max_length = 50,
    single_runner_gram.py:637): candidates of 40-46 tokens, every step through the self-attention cache, the ancestor table and
    T5's log-spaced distance buckets, against the oracle."""
    from gram_amd.utils import generation_trie as gt
    oc, sd, m = _model(gpu, "tiny", 13)
    g = torch.Generator().manual_seed(77)
    B, N, L, K = 2, 2, 32, 4
    ids, mask = _inputs(g, B, N, L, min(oc.vocab_size, 32100))
    cands = _random_items(g, 24, 40, 46, 12)  # (12 token values: shared prefixes, so beams branch all the way down)
    max_length = max(len(c) for c in cands)
    assert 32 < max_length <= 50
    ref = O.generate(sd, oc, ids, mask, max_length, O.prefix_allowed_tokens_fn(O.Trie(cands)), K, K, 1.0)
    out = _gen(m, ids, mask, max_length, gt.prefix_allowed_tokens_fn(gt.Trie(cands)), K)
    assert out["sequences"].shape == ref["sequences"].shape
    _check_generate(oc, sd, out, ref, ids, mask, cands, K, tol=SCORE_TOL)


@pytest.mark.parametrize("kind", ["trie_shallower_than_50", "candidates_longer_than_50"])
def test_max_length_50(gpu, kind):
    """What the "term" id type asks of generate() (max_length = 50 whatever the candidates are, single_runner_gram.py:637).
    (a) A Trie 4-6 tokens deep: the result equals the oracle's at 50 AND the device's own result at the Trie's depth, bit for bit --
    the runner decodes to the depth (gram_amd/runner/base.py: past it every candidate is -inf and every user already holds K finite
    hypotheses).  (b) Some candidates longer than 50 tokens: they never finish, BeamSearchScorer.finalize adds the running beams cut
    at 50 tokens where they beat a finished hypothesis -- same rows, same order, same scores as the oracle."""
    from gram_amd.utils import generation_trie as gt
    oc, sd, m = _model(gpu, "tiny", 17)
    g = torch.Generator().manual_seed(31)
    B, N, L, K = 3, 2, 32, 4
    ids, mask = _inputs(g, B, N, L, min(oc.vocab_size, 32100))
    cands = _random_items(g, 40, 2, 4, 60)
    if kind == "candidates_longer_than_50":
        cands = cands[:6] + _random_items(g, 12, 52, 56, 8)
    depth = max(len(c) for c in cands)
    fn = gt.prefix_allowed_tokens_fn(gt.Trie(cands))
    ref = O.generate(sd, oc, ids, mask, 50, O.prefix_allowed_tokens_fn(O.Trie(cands)), K, K, 1.0)
    out = _gen(m, ids, mask, 50, fn, K)
    sc, rsc = out["sequences_scores"].cpu(), ref["sequences_scores"]
    assert bool(torch.isfinite(rsc).all()) and bool(torch.isfinite(sc).all())
    assert out["sequences"].shape == ref["sequences"].shape
    if kind == "trie_shallower_than_50":
        _check_generate(oc, sd, out, ref, ids, mask, cands, K, tol=SCORE_TOL)
        short = _gen(m, ids, mask, depth, fn, K)
        assert torch.equal(out["sequences"], short["sequences"]) and torch.equal(out["sequences_scores"], short["sequences_scores"])
    else:
        assert out["sequences"].shape[1] == 50
        cut = (ref["sequences"][:, -1] != 0) & (ref["sequences"][:, -1] != 1)
        assert bool(cut.any()), "no running beam made it into the oracle's top-K: the case does not test the truncation"
        assert torch.equal(out["sequences"].cpu(), ref["sequences"])
        assert float((sc - rsc).abs().max()) < SCORE_TOL


@pytest.mark.parametrize("kind", ["whole_table_3e5", "outlier_features"])
def test_large_residual_stream_matches_the_oracle(gpu, kind):
    """T5's residual stream leaves the IEEE-half range in trained checkpoints (the reference's own T5 carries the fp16 clamp for it:
    gram_t5_modeling.py:773-776,803-808,824-827).  The 16-bit copy of the stream carries a power-of-two factor per row
    (gram_norm_fusion_t.xs_in / xs_out), so a model whose embedding table puts the stream at ~3e5 -- or whose rows carry outlier features
    1e4 times the ordinary ones -- is scored like any other: same top-K as the fp32 oracle at the ordinary score tolerance."""
    from gram_amd import T5Config
    from gram_amd.utils import generation_trie as gt
    oc = O.OracleConfig(vocab_size=256, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2, max_item_num=5,
                        tie_word_embeddings=False)  # (an untied lm_head: the logits keep their ordinary scale)
    gc = T5Config(vocab_size=256, d_model=128, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2, max_item_num=5,
                  tie_word_embeddings=False)
    sd = O.init_state_dict(oc, 3)
    emb = sd["shared.weight"].clone()
    if kind == "whole_table_3e5":
        emb *= 3.0e5
    else:
        emb[:, [7, 70, 101]] *= 1.0e4
    for k in ("shared.weight", "encoder.encoder.embed_tokens.weight", "decoder.embed_tokens.weight"):
        sd[k] = emb
    m = gpu.create_model("gram", gc)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    B, N, L, K = 4, 3, 32, 6
    ids, mask = _inputs(g, B, N, L, min(oc.vocab_size, 32100))
    cands = _random_items(g, 40, 3, 4, 60)
    max_length = max(len(c) for c in cands)
    ref = O.generate(sd, oc, ids, mask, max_length, O.prefix_allowed_tokens_fn(O.Trie(cands)), K, K, 1.0)
    out = m.generate(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), max_length=max_length,
                     prefix_allowed_tokens_fn=gt.prefix_allowed_tokens_fn(gt.Trie(cands)), num_beams=K, num_return_sequences=K,
                     length_penalty=1.0)
    _check_generate(oc, sd, out, ref, ids, mask, cands, K, tol=SCORE_TOL)
    # one user at a time: the row factors are a function of the row alone (batch invariance, bit for bit)
    one = m.generate(input_ids=ids[1:2].to(DEV), attention_mask=mask[1:2].to(DEV), max_length=max_length,
                     prefix_allowed_tokens_fn=gt.prefix_allowed_tokens_fn(gt.Trie(cands)), num_beams=K, num_return_sequences=K,
                     length_penalty=1.0)
    w = min(one["sequences"].shape[1], out["sequences"].shape[1])
    assert torch.equal(one["sequences"][:, :w], out["sequences"][K:2 * K, :w])
    assert torch.equal(one["sequences_scores"], out["sequences_scores"][K:2 * K])


def test_activation_overflow_of_the_half_pieces_is_an_error(gpu):
    """Non-finite arithmetic must not return a garbage ranking: generate() raises GRAM_E_NONFINITE.  (The half range of the pieces
    alone no longer gets there -- test_large_residual_stream_matches_the_oracle -- so the stream here leaves fp32 itself.)"""
    from gram_amd import _lib
    from gram_amd.utils import generation_trie as gt
    if _lib.piece_dtype() != torch.float16:
        pytest.skip("bfloat16 build: the pieces have fp32's exponent range")
    oc, gc = _cfgs("tiny")
    sd = O.init_state_dict(oc, 3)
    big = sd["shared.weight"] * 1.0e30  # embeddings whose squares leave fp32 itself: no row factor can help (the sums of squares are inf)
    for k in ("shared.weight", "encoder.encoder.embed_tokens.weight", "decoder.embed_tokens.weight", "lm_head.weight"):  # (one tied table)
        sd[k] = big
    m = gpu.create_model("gram", gc)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    ids, mask = _inputs(g, 2, 2, 32, min(oc.vocab_size, 32100), ragged=False)
    cands = _random_items(g, 30, 3, 3, 60)
    fn = gt.prefix_allowed_tokens_fn(gt.Trie(cands))
    with pytest.raises(_lib.GramHipError, match="GRAM_E_NONFINITE"):
        m.generate(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), max_length=max(len(c) for c in cands), prefix_allowed_tokens_fn=fn,
                   num_beams=4, num_return_sequences=4, length_penalty=1.0)


def test_generate_matches_reference_golden(gpu, golden_dir):
    """Whole path vs the golden produced by reference forward + reference Trie + HF beam search."""
    from gram_amd.utils import generation_trie as gt
    z = np.load(os.path.join(golden_dir, "ref_generate.npz"))
    oc, sd, m = _model(gpu, "tiny", int(z["seed"]))
    for ci in range(int(z["n_cases"])):
        ids, mask = torch.from_numpy(z[f"c{ci}_ids"]), torch.from_numpy(z[f"c{ci}_mask"])
        cands = z[f"c{ci}_cands"].tolist()
        K = int(z[f"c{ci}_K"])
        fn = gt.prefix_allowed_tokens_fn(gt.Trie(cands))
        out = m.generate(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), max_length=len(cands[0]), prefix_allowed_tokens_fn=fn,
                         num_beams=K, num_return_sequences=K, length_penalty=1.0)
        ref = {"sequences": torch.from_numpy(z[f"c{ci}_sequences"]), "sequences_scores": torch.from_numpy(z[f"c{ci}_scores"])}
        _check_generate(oc, sd, out, ref, ids, mask, cands, K, tol=SCORE_TOL)


def test_metric_parity_population(gpu):
    """Recall@5 / NDCG@5 of device vs the CPU oracle over a small user population whose gold items sit at known
    oracle ranks (so the metric is sensitive to every rank flip), in the model's default arithmetic (two pieces) and with
    one piece.  The north-star bound itself (1e-4 on 16 384 T5-base users against the fp32 reference, two populations) is
    asserted in tests/test_gpu_precision.py; here: at most one near-tie flip in the default mode, the round-1 bounds for one piece."""
    from gram_amd.utils import evaluate as ev, generation_trie as gt
    oc, sd, m = _model(gpu, "tiny", 11)
    results = {}
    two, one = m.default_precision(), m.default_precision()[:-2]
    for mode in (two, one):
        m.set_precision(mode)
        g = torch.Generator().manual_seed(77)
        cands = _random_items(g, 300, 3, 4, 40)
        max_length = max(len(c) for c in cands)
        K, B, nb = 10, 16, 8
        ofn = O.prefix_allowed_tokens_fn(O.Trie(cands))
        dfn = gt.prefix_allowed_tokens_fn(gt.Trie(cands))
        metrics = ["hit@5", "hit@10", "ndcg@5", "ndcg@10"]
        o_sum, d_sum, total, flips = np.zeros(4), np.zeros(4), 0, 0
        strip = lambda s: tuple(int(t) for t in s if int(t) not in (0, 1))
        for it in range(nb):
            ids, mask = _inputs(g, B, 3, 32, 256)
            ref = O.generate(sd, oc, ids, mask, max_length, ofn, K, K, 1.0)
            out = m.generate(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), max_length=max_length, prefix_allowed_tokens_fn=dfn,
                             num_beams=K, num_return_sequences=K)
            opred = [strip(s) for s in ref["sequences"]]
            dpred = [strip(s) for s in out["sequences"].cpu()]
            gold = [opred[b * K + (b + it) % K] for b in range(B)]  # gold = oracle's rank-((b+it)%K) item
            orel = ev.rel_results(opred, gold, ref["sequences_scores"].tolist(), K)
            drel = ev.rel_results(dpred, gold, out["sequences_scores"].cpu().tolist(), K)
            flips += int((ev.hit_ranks(orel) != ev.hit_ranks(drel)).sum())
            o_sum += ev.get_metrics_results(orel, metrics)
            d_sum += ev.get_metrics_results(drel, metrics)
            total += B
        delta = np.abs(o_sum - d_sum) / total
        print(f"\n[metric parity, {mode}] users={total} rank flips={flips} |delta| hit@5/hit@10/ndcg@5/ndcg@10 = {delta}")
        results[mode] = (flips, delta, total)
    flips, delta, total = results[two]
    assert flips <= 1 and (delta < 0.01).all(), (flips, delta)
    flips, delta, total = results[one]
    assert flips <= 0.15 * total and (delta < 0.05).all(), (flips, delta)


def test_greedy_matches_oracle(gpu):
    """BASELINE configs[0] shape (single granularity, num_beams = 1 -> HF greedy_search): device vs oracle.
    Token sequences must be identical unless the oracle's own top-2 allowed logits at the first differing step
    are closer than the logit tolerance (a near-tie)."""
    from gram_amd.utils import generation_trie as gt
    oc, sd, m = _model(gpu, "small", 11)
    g = torch.Generator().manual_seed(101)
    B, N, L = 24, 1, 128
    ids, mask = _inputs(g, B, N, L, 32100)
    cands = _random_items(g, 400, 2, 5, 300)
    max_length = max(len(c) for c in cands)
    ref = O.generate(sd, oc, ids, mask, max_length, O.prefix_allowed_tokens_fn(O.Trie(cands)), 1, 1)
    out = m.generate(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), max_length=max_length,
                     prefix_allowed_tokens_fn=gt.prefix_allowed_tokens_fn(gt.Trie(cands)), num_beams=1, num_return_sequences=1)
    assert out["sequences_scores"] is None
    dseq, rseq = out["sequences"].cpu(), ref["sequences"]
    cand_set = {tuple(c) for c in cands}
    same = 0
    for b in range(B):
        d = [int(x) for x in dseq[b]]
        while d and d[-1] == 0:
            d.pop()
        assert tuple(d) in cand_set
        r = [int(x) for x in rseq[b]]
        while r and r[-1] == 0:
            r.pop()
        if d == r:
            same += 1
            continue
        t = next(i for i in range(min(len(d), len(r))) if d[i] != r[i])
        # near-tie check with the oracle's logits at step t-1 for this user
        ext = ((1.0 - mask[b:b + 1].reshape(1, -1).float()) * O.FMIN)[:, None, None, :]
        st = O.DecodeState(O.cross_kv(sd, oc, O.encode_fused(sd, oc, ids[b:b + 1], mask[b:b + 1])), ext, 1)
        for i in range(t):
            lg = O.decoder_step(sd, oc, torch.tensor([r[i]]), st)
        assert abs(float(lg[0, d[t]] - lg[0, r[t]])) < LOGIT_TOL, (b, t, d, r)
    print(f"\n[greedy] identical sequences {same}/{B}; width {tuple(dseq.shape)} vs oracle {tuple(rseq.shape)}")
    assert same >= B - 2
    if same == B:
        assert dseq.shape == rseq.shape and torch.equal(dseq, rseq)


def test_generic_callback_matches_trie_fast_path(gpu):
    """An arbitrary prefix_allowed_tokens_fn (no Trie in its closure) goes through the step-wise fallback; with a
    callback that answers from the same candidate set it must reproduce the fast path's sequences and scores."""
    from gram_amd.utils import generation_trie as gt
    oc, sd, m = _model(gpu, "tiny", 11)
    g = torch.Generator().manual_seed(77)
    B, N, L, K = 3, 2, 32, 5
    ids, mask = _inputs(g, B, N, L, 256)
    cands = _random_items(g, 60, 2, 4, 40)
    max_length = max(len(c) for c in cands)
    trie = gt.Trie(cands)
    fast = m.generate(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), max_length=max_length,
                      prefix_allowed_tokens_fn=gt.prefix_allowed_tokens_fn(trie), num_beams=K, num_return_sequences=K)
    table = {}
    for c in cands:
        for i in range(1, len(c)):
            table.setdefault(tuple(c[:i]), set()).add(c[i])
    calls = []

    def generic(batch_id, sent):  # plain function: nothing Trie-like in its closure cells
        calls.append(batch_id)
        return sorted(table.get(tuple(int(x) for x in sent), ()))

    slow = m.generate(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), max_length=max_length, prefix_allowed_tokens_fn=generic,
                      num_beams=K, num_return_sequences=K)
    assert len(calls) == B * K * (max_length - 1) and set(calls) == set(range(B))
    assert torch.equal(slow["sequences"].cpu(), fast["sequences"].cpu())
    # dense logits + row LSE vs sparse logits + fused LSE partials: same values up to fp32 summation order
    assert torch.allclose(slow["sequences_scores"].cpu(), fast["sequences_scores"].cpu(), atol=2e-5)


def test_unfolded_norm_path_vs_oracle_and_the_folded_path(gpu, monkeypatch):
    """GRAM_FOLD_NORM=0 at one piece per value: separate norm kernels in front of every consumer GEMM instead of the norm folded into
    the GEMMs (generate.hip NormChain; INTEGRATION.md's A/B and debugging path).  The smoke shape, generate / forward(labels) /
    score_sequences, against the oracle within the one-piece tolerances the folded path is held to (sequence scores 0.01 as smoke();
    token log-probs, the loss and sequence sums as tests/test_gpu_teacher_forced.py), and against the folded path within the same."""
    from gram_amd.utils import generation_trie as gt
    from tests import tf_oracle as TF
    LOGP_TOL = LOSS_TOL = 2e-2
    B, N, L, K, C, T = 2, 3, 32, 4, 3, 4
    oc, _ = _cfgs("tiny")
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(2, 256, (B, N, L), generator=g)
    mask = torch.ones(B, N, L, dtype=torch.bool)
    mask[:, :, 20:] = False
    ids[:, :, 20:] = 0
    cands = [[0, a, b, c, 1] for a in (2, 3, 4) for b in (5, 6, 7) for c in (8, 9)]
    lab = torch.randint(2, 256, (B, C, T), generator=g)
    lab[:, 1, 3:] = -100
    got = {}
    for fold in ("0", "1"):
        monkeypatch.setenv("GRAM_FOLD_NORM", fold)  # read when the model packs its weights
        _, sd, m = _model(gpu, "tiny", 11)
        m.set_precision("f16" if F16 else "bf16")
        if not got:
            ref = O.generate(sd, oc, ids, mask, 5, O.prefix_allowed_tokens_fn(O.Trie(cands)), K, K, 1.0)
            ref_logits = TF.teacher_forced_logits(sd, oc, ids, mask, TF.shift_right(lab.view(B * C, T)))
            _, ref_tok = TF.loss_and_token_logp(ref_logits, lab.view(B * C, T))
            ref_loss, _ = TF.loss_and_token_logp(ref_logits.view(B, C, T, -1)[:, 0], lab[:, 0])
        out = _gen(m, ids, mask, 5, gt.prefix_allowed_tokens_fn(gt.Trie(cands)), K)
        _check_generate(oc, sd, out, ref, ids, mask, cands, K, tol=0.01)
        with torch.no_grad():
            loss = float(m(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), labels=lab[:, 0].to(DEV)).loss)
        seq, tok = m.score_sequences(ids.to(DEV), mask.to(DEV), lab.to(DEV), return_tokens=True)
        seq, tok = seq.cpu().view(-1).double(), tok.cpu().view(B * C, T).double()
        dt, ds = float((tok - ref_tok).abs().max()), float((seq - ref_tok.sum(-1)).abs().max())
        rel = abs(loss - float(ref_loss)) / abs(float(ref_loss))
        print(f"fold_norm={fold}: token logp {dt:.2e}, sequence sums {ds:.2e}, loss rel {rel:.2e}")
        assert dt < LOGP_TOL and ds < LOGP_TOL * T and rel < LOSS_TOL
        scores = {(i // K, tuple(s.tolist())): float(v) for i, (s, v) in enumerate(zip(out["sequences"].cpu(), out["sequences_scores"].cpu()))}
        got[fold] = (scores, tok, seq, loss)
    (s0, tok0, seq0, loss0), (s1, tok1, seq1, loss1) = got["0"], got["1"]
    shared = set(s0) & set(s1)
    d_score = max(abs(s0[k] - s1[k]) for k in shared)
    dt, ds, rel = float((tok0 - tok1).abs().max()), float((seq0 - seq1).abs().max()), abs(loss0 - loss1) / abs(loss1)
    print(f"unfolded vs folded: {len(shared)}/{B * K} shared sequences, scores {d_score:.2e}, token logp {dt:.2e}, sums {ds:.2e}, loss rel {rel:.2e}")
    assert len(shared) >= B and d_score < 0.01 and dt < LOGP_TOL and ds < LOGP_TOL * T and rel < LOSS_TOL
