"""-m gpu: generate() and score_sequences() where the decoders change how they compute -- at 32 768 decoder rows and above.

From R >= 32 768 rows (kPrecomputedRsRows, generate.hip; pp_min_m(), gemm.hip) decode_step and decoder_tf take 1/rms and the row
factors of the 16-bit copy from gram_row_rscale_xs at every norm point instead of the GEMM epilogues' partials, and their residual-add,
wide and lm_head LSE-partials GEMMs run on the persistent ping-pong kernel.  The headline workloads live there (bench.py: 4 096 users x
20 beams = 81 920 rows; tests/bench_teacher_forced.py: 737 280 rows per call); the rest of the suite stays below it.

Checked here: a user scored inside a >= 32 768-row batch gets the bits it gets alone or in a batch below the threshold (the promise of
GRAM.max_users_per_call and score_sequences), that the threshold really was crossed (the ping-pong kernel's clock counters), and a few
users against the fp32 oracle at the suite's tolerances.  Both arithmetic modes; the generate oracle comparisons in the two-piece mode
(as test_config5_full_shape_properties), the teacher-forced ones in both (the TF tolerance table).  Observed deviations are printed."""
import ctypes as C

import pytest
import torch

from gram_amd import _lib
from oracle import gram_oracle as O
from tests import tf_oracle as TF
from tests.test_gpu_configs import ONE, TWO, _generate, _realistic_inputs, _strip, _trie_cands
from tests.test_gpu_path import DEV, SCORE_TOL, _check_generate, _model
from tests.test_gpu_teacher_forced import _labels, _tol

pytestmark = pytest.mark.gpu
THRESHOLD = 32768  # decoder rows from which pre_rs and the ping-pong GEMMs are on (generate.hip kPrecomputedRsRows = gemm.hip pp_min_m())


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gram_amd
    return gram_amd


def _t5_base_2023(gpu, q_sharpen):
    """bench.py main()'s model (q_sharpen 4, its --q-sharpen default) and tests/bench_teacher_forced.py's (q_sharpen 1), restated"""
    torch.manual_seed(2023)
    m = gpu.create_model("gram", gpu.T5Config.named("t5-base"))
    if q_sharpen != 1.0:
        with torch.no_grad():
            for name, p_ in m.named_parameters():
                if name.endswith(".q.weight"):
                    p_.mul_(q_sharpen)
    return m.to(DEV).eval()


def _released(m):
    """teardown: the model's workspace (up to ~3/4 of the HBM here) goes back to the device, not to the caching allocator"""
    m._workspace = None
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def bench_model(gpu):
    torch.cuda.empty_cache()
    m = _t5_base_2023(gpu, 4.0)
    yield m
    _released(m)


@pytest.fixture(scope="module")
def tf_bench_model(gpu):
    m = _t5_base_2023(gpu, 1.0)
    yield m
    _released(m)


def _with_pp_clock(fn):
    """(fn(), the time-weighted clock gram_prof_pp_clock reports for the ping-pong GEMM launches inside fn): 0 unless one ran"""
    lib = _lib.load()
    lib.gram_prof_pp_clock_enable(1)
    try:
        _lib.check(lib.gram_prof_pp_clock(None, 1), "pp_clock reset")
        out = fn()
        ghz = C.c_double(-1.0)
        _lib.check(lib.gram_prof_pp_clock(C.byref(ghz), 1), "pp_clock")
    finally:
        lib.gram_prof_pp_clock_enable(0)
    return out, ghz.value


def _same_rows(a, b):
    """sequences of two generate() calls (0-padded to their own widths): the same tokens, bit for bit"""
    w = max(a.shape[1], b.shape[1])
    pad = lambda x: torch.nn.functional.pad(x.cpu(), (0, w - x.shape[1]))
    return torch.equal(pad(a), pad(b))


def _rescored(m, ids, mask, seqs, K):
    """The (B * K, width) rows a generate() returned, scored again by the teacher-forced decoder in one score_sequences call: the
    f64 sums of their token log-probs over the hypothesis length (length_penalty 1), what their sequences_scores must equal."""
    B = ids.shape[0]
    lab = seqs[:, 1:].clone()
    T = lab.shape[1]
    eos = lab == 1
    has_eos = eos.any(1)
    n = torch.where(has_eos, eos.int().argmax(1) + 1, torch.full((B * K,), T))  # labels up to and including EOS
    hyp_len = torch.where(has_eos, n, torch.full((B * K,), T + 1))  # (as test_sequences_scores_equal_scored_sequences)
    lab[torch.arange(T)[None, :] >= n[:, None]] = -100
    seq = m.score_sequences(ids.to(DEV), mask.to(DEV), lab.view(B, K, T).to(DEV)).cpu().view(-1)
    return seq.double() / hyp_len.double()  # length_penalty 1


# ---------------------------------------------------------------------------------------------------------- 1. bench.py's workload
@pytest.mark.parametrize("mode", [TWO, ONE])  # (the larger, two-piece workspace first)
def test_generate_at_the_bench_workload(gpu, bench_model, mode):
    """bench.py's default step (T5-base, Beauty Trie, N = 3 x L = 128, beam 20, B = 4 096 users: 81 920 rows per full-width decode step):
    users scored alone and in a 16-user batch get the bits they get in it (user 12's rows 240-259 straddle a 256-row tile, user 4 095
    is the M tail), three users against the fp32 oracle on the GPU, and every returned sequence re-scored by the teacher-forced decoder
    in one >= 32 768-row score_sequences call equals its beam score."""
    m = bench_model
    # the two-piece workspace of this call is ~3/4 of the HBM: the previous call's goes back to the device before the mode switch
    # re-packs the weights, so that they are not placed inside its freed (cached) segment and keep it from being released
    _released(m)
    m.set_precision(mode)
    cands = _trie_cands("Beauty")
    B, N, L, K = 4096, 3, 128, 20
    g = torch.Generator().manual_seed(1000)
    ids = torch.randint(2, 32100, (B, N, L), generator=g)
    ids[:, :, -1] = 1
    mask = torch.ones(B, N, L, dtype=torch.bool)
    assert B * K >= THRESHOLD
    out = _generate(m, ids, mask, cands, K)
    seqs, scores = out["sequences"].cpu(), out["sequences_scores"].cpu()
    assert seqs.shape[0] == B * K and torch.isfinite(scores).all()
    sel = [0, 12, 2047, 4095]
    for sub in [[u] for u in sel] + [sel + list(range(100, 112))]:
        o = _generate(m, ids[sub], mask[sub], cands, K)
        assert len(sub) * K < THRESHOLD
        for j, u in enumerate(sub):
            assert _same_rows(o["sequences"][j * K:(j + 1) * K], seqs[u * K:(u + 1) * K]), (sub, u)
            assert torch.equal(o["sequences_scores"][j * K:(j + 1) * K].cpu(), scores[u * K:(u + 1) * K]), (sub, u)
    # beam audit: generate and the teacher-forced pass are two independent decoders
    assert B * K * (seqs.shape[1] - 1) >= THRESHOLD
    norm = _rescored(m, ids, mask, seqs, K)
    audit = float((norm - scores.double()).abs().max())
    print(f"\n[bench workload {mode}] beam audit over {B * K} sequences: max |score diff| {audit:.2e}, "
          f"bit-equal {int((norm.float() == scores).sum())}/{B * K}")
    assert audit < _tol(mode)["logp"]
    if mode == TWO:
        oc = O.OracleConfig.named("t5-base")
        seen, sd_dev = {}, {}
        for k_, v_ in m.state_dict().items():  # (aliases stay aliased)
            sd_dev[k_] = seen.setdefault(v_.data_ptr(), v_.detach().to(DEV, torch.float32))
        users = [12, 2047, 4095]
        ref = O.generate(sd_dev, oc, ids[users].to(DEV), mask[users].to(DEV), max(len(c) for c in cands),
                         O.prefix_allowed_tokens_fn(O.Trie(cands)), K, K, 1.0)
        rs, rq = ref["sequences_scores"].cpu(), ref["sequences"].cpu()
        for j, u in enumerate(users):
            want = {_strip(r): float(v) for r, v in zip(rq[j * K:(j + 1) * K].tolist(), rs[j * K:(j + 1) * K])}
            mine = [(_strip(r), float(v)) for r, v in zip(seqs[u * K:(u + 1) * K].tolist(), scores[u * K:(u + 1) * K])]
            shared = [abs(want[r] - v) for r, v in mine if r in want]
            print(f"[bench workload {mode}] user {u} vs the on-GPU fp32 oracle: shared {len(shared)}/{K}, "
                  f"max |score diff| {max(shared):.2e}")
            assert len(shared) >= K - 2 and max(shared) < 1.5 * SCORE_TOL, (u, len(shared), max(shared))


# ---------------------------------------------------------------------------------------------------------- 2. generate, decoder only
@pytest.mark.parametrize("mode", [ONE, TWO])
def test_generate_across_the_decoder_threshold(gpu, mode):
    """t5-small, N = 1 x L = 32, K = 64 (GRAM_MAX_BEAMS), Beauty Trie: B = 512 users are 32 768 rows at the full-width decode steps,
    B = 511 are 32 704; the encoder and the bank GEMM see 16 384 rows at most, so whatever runs on the ping-pong kernel is the decoder's."""
    oc, sd, m = _model(gpu, "small", 21)
    m.set_precision(mode)
    cands = _trie_cands("Beauty")
    N, L, K = 1, 32, _lib.GRAM_MAX_BEAMS
    g = torch.Generator().manual_seed(21)
    ids, mask = _realistic_inputs(g, 512, N, L, lo=8)
    assert 512 * K >= THRESHOLD > 511 * K and 512 * N * L < THRESHOLD
    big, ghz_big = _with_pp_clock(lambda: _generate(m, ids, mask, cands, K))
    small, ghz_small = _with_pp_clock(lambda: _generate(m, ids[:511], mask[:511], cands, K))
    print(f"\n[generate threshold {mode}] ping-pong clock: B=512 {ghz_big:.3f} GHz, B=511 {ghz_small:.3f} GHz")
    assert ghz_big > 0 and ghz_small == 0
    seqs, scores = big["sequences"].cpu(), big["sequences_scores"].cpu()
    assert torch.isfinite(scores).all()
    assert _same_rows(small["sequences"], seqs[:511 * K])
    assert torch.equal(small["sequences_scores"].cpu(), scores[:511 * K])
    if mode == TWO:
        users = [0, 511]
        ref = O.generate(sd, oc, ids[users], mask[users], max(len(c) for c in cands), O.prefix_allowed_tokens_fn(O.Trie(cands)), K, K, 1.0)
        rows = torch.cat([torch.arange(u * K, (u + 1) * K) for u in users])
        _check_generate(oc, sd, dict(sequences=seqs[rows], sequences_scores=scores[rows]), ref, ids[users], mask[users], cands, K,
                        tol=SCORE_TOL)


# ---------------------------------------------------------------------------------------------------------- 3. teacher forced, threshold
@pytest.mark.parametrize("mode", [ONE, TWO])
def test_teacher_forced_across_the_threshold(gpu, mode):
    """t5-small, N = 1 x L = 32, C = 16 candidates of T = 8 (ragged -100 tails): 128 rows per user, B = 256 is R = 32 768, B = 255 is
    32 640.  Same bits for users 0..254 in both calls and for three users scored alone; three users against the CPU oracle."""
    oc, sd, m = _model(gpu, "small", 31)
    m.set_precision(mode)
    tol = _tol(mode)
    N, L, Cn, T = 1, 32, 16, 8
    g = torch.Generator().manual_seed(31)
    ids, mask = _realistic_inputs(g, 256, N, L, lo=8)
    lab = _labels(g, (256, Cn, T), oc.vocab_size, min_len=1)
    assert 256 * Cn * T >= THRESHOLD > 255 * Cn * T
    idd, mk, lb = ids.to(DEV), mask.to(DEV), lab.to(DEV)
    (seq, tok), ghz_big = _with_pp_clock(lambda: m.score_sequences(idd, mk, lb, return_tokens=True, users_per_call=256))
    (seq1, tok1), ghz_small = _with_pp_clock(lambda: m.score_sequences(idd[:255], mk[:255], lb[:255], return_tokens=True,
                                                                       users_per_call=255))
    print(f"\n[teacher forced threshold {mode}] ping-pong clock: B=256 {ghz_big:.3f} GHz, B=255 {ghz_small:.3f} GHz")
    assert ghz_big > 0 and ghz_small == 0
    assert torch.equal(seq1, seq[:255]) and torch.equal(tok1, tok[:255])
    users = [0, 77, 255]
    alone, tok_alone = m.score_sequences(idd[users], mk[users], lb[users], return_tokens=True, users_per_call=1)
    assert torch.equal(alone, seq[users]) and torch.equal(tok_alone, tok[users])
    ref_logits = TF.teacher_forced_logits(sd, oc, ids[users], mask[users], TF.shift_right(lab[users]).view(-1, T))
    _, ref_tok = TF.loss_and_token_logp(ref_logits, lab[users].view(-1, T))
    dt = float((tok[users].cpu().view(-1, T).double() - ref_tok).abs().max())
    ds = float((seq[users].cpu().view(-1).double() - ref_tok.sum(-1)).abs().max())
    print(f"[teacher forced threshold {mode}] users {users} vs the oracle: token logp {dt:.2e}, sequence sums {ds:.2e}")
    assert dt < tol["logp"] and ds < tol["logp"] * T


# ---------------------------------------------------------------------------------------------------------- 4. bench_teacher_forced
@pytest.mark.parametrize("mode", [ONE, TWO])
def test_teacher_forced_at_the_bench_teacher_forced_shape(gpu, tf_bench_model, mode):
    """tests/bench_teacher_forced.py's shape: T5-base, N = 3 x L = 128, C = 20 Beauty items in label form, T = 9; B = 512 users is
    R = 92 160 rows, Q = 180 query rows per user (cross-attention groups of 64, 64 and 52).  Chunks of 37 users (6 660 rows, a partial
    last chunk) and users alone give the single call's bits; two users against the CPU oracle."""
    m = tf_bench_model
    m.set_precision(mode)
    tol = _tol(mode)
    cands = _trie_cands("Beauty")
    B, N, L, Cn = 512, 3, 128, 20
    T = max(len(c) for c in cands) - 1
    assert T == 9 and Cn * T == 180
    g = torch.Generator().manual_seed(99)
    ids, mask = _realistic_inputs(g, B, N, L)
    pick = torch.randint(0, len(cands), (B, Cn), generator=g)
    lab = torch.full((B, Cn, T), -100, dtype=torch.long)
    for b in range(B):
        for c in range(Cn):
            s = cands[int(pick[b, c])][1:]
            lab[b, c, :len(s)] = torch.tensor(s)
    assert B * Cn * T >= THRESHOLD > 37 * Cn * T and B % 37
    idd, mk, lb = ids.to(DEV), mask.to(DEV), lab.to(DEV)
    seq, tok = m.score_sequences(idd, mk, lb, return_tokens=True, users_per_call=B)
    assert torch.isfinite(seq).all()
    seq37, tok37 = m.score_sequences(idd, mk, lb, return_tokens=True, users_per_call=37)
    assert torch.equal(seq37, seq) and torch.equal(tok37, tok)
    for u in (0, 255, 511):
        s1, t1 = m.score_sequences(idd[u:u + 1], mk[u:u + 1], lb[u:u + 1], return_tokens=True)
        assert torch.equal(s1[0], seq[u]) and torch.equal(t1[0], tok[u]), u
    users = [0, 300]
    sd = {k_: v_.detach().cpu() for k_, v_ in m.state_dict().items()}
    oc = O.OracleConfig.named("t5-base")
    ref_logits = TF.teacher_forced_logits(sd, oc, ids[users], mask[users], TF.shift_right(lab[users]).view(-1, T))
    _, ref_tok = TF.loss_and_token_logp(ref_logits, lab[users].view(-1, T))
    dt = float((tok[users].cpu().view(-1, T).double() - ref_tok).abs().max())
    ds = float((seq[users].cpu().view(-1).double() - ref_tok.sum(-1)).abs().max())
    print(f"\n[bench_teacher_forced shape {mode}] users {users} vs the oracle: token logp {dt:.2e}, sequence sums {ds:.2e}")
    assert dt < tol["logp"] and ds < tol["logp"] * T
