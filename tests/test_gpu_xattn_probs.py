"""-m gpu: the cross-attention probabilities (gram_cross_attn_probs_split, xattn_probs.hip), their reducers (gram_xattn_head_sum,
gram_xattn_passage_scores) and the whole path over them (GRAM.cross_attentions, GRAM.passage_attention, get_crossattention_scores).

1. the probes of tests/test_gpu_attn_probes.py: every (head, row, key) weight against fp64 under that file's comparator and bounds
   (derived for a 16-bit output; this kernel's is fp32, so they hold with room), exact zeros, the uniform user;
2. a row's bits depend on nothing but that row and its user;
3. sum_s probs . V = what the shipped cross-attention kernel returns, within tests/test_gpu_split.py's bound;
4. the reducers against fp64 numpy, the NaN of an empty passage;
5. the whole path against tests/xattn_oracle.py in fp64 at the tiny config and T5-small.
Observed values are printed."""
import numpy as np
import pytest
import torch

from gram_amd import _lib
from oracle import gram_oracle as O
from tests import test_gpu_attn_probes as P
from tests import xattn_oracle as XO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    return gpu_util


def _key_bits(G, m8, S):
    bits = torch.full((m8.shape[0], 128), -1, dtype=torch.int32, device=G.DEV)
    _lib.check(G.lib().gram_mask_key_bits(G.p(m8), G.p(bits), m8.shape[0], S, G.stream()), "bits")
    return bits


def _probs(G, q, kb, m8, B, Q, H, S, pieces, key_bits=None):
    """q [pieces][B*Q][inner] planar, kb [pieces][B][H][S][64] -> probs f32 [B][H][Q][S], pre-filled with NaN"""
    out = torch.full((B, H, Q, S), float("nan"), dtype=torch.float32, device=G.DEV)
    _lib.check(G.lib().gram_cross_attn_probs_split(G.p(q), G.p(kb), G.p(m8), G.p(out), B, Q, H, S, pieces, q[0].numel(), kb[0].numel(),
                                                   G.p(key_bits), G.stream()), "gram_cross_attn_probs_split")
    return out


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1. probes
@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("S", [32, 96, 2080, 4096])  # one step, an odd number of steps, the second ballot word, the maximum
@pytest.mark.parametrize("Q", [1, 16, 17, 64, 65, 130])  # one row, a full MFMA tile, one over, two workgroups' worth, one over, five tiles
def test_probe_cross_attn_probs(G, Q, S, pieces):
    """Users 0 and 2 carry the probe of tests/test_gpu_attn_probes.py (exact scores, a mask with skipped, single-key and sparse steps),
    user 1 has no valid key: every (head, row, key) of the NaN-pre-filled output against the fp64 weights, expected zeros exactly 0.0,
    user 1 uniform 1 / S; key_bits NULL and precomputed give the same bits."""
    rtol = P._rtol(G, pieces)
    p = P.xattn_probe(Q, S)
    wmin = P.precondition(p["ref"], pieces)
    H, B, inner = p["H"], 3, p["H"] * 64
    q = torch.zeros(B, Q, H, 64, device=G.DEV)
    q[..., 0] = P._dev(G, p["qf"])[None]
    kb = torch.zeros(pieces, B, H, S, 64, dtype=G.DT, device=G.DEV)
    kb[0, :, :, :, 0] = P._dev(G, p["kv"]).to(G.DT)[None]
    assert torch.equal(kb[0, 0, :, :, 0].double().cpu(), torch.from_numpy(p["kv"]))
    mask = np.tile(p["mask"], (B, 1))
    mask[1] = 0
    m8 = P._dev(G, mask, torch.uint8)
    qp = P._pieces(G, q.view(B * Q, inner), pieces)
    out = _probs(G, qp, kb, m8, B, Q, H, S, pieces)
    bits = _key_bits(G, m8, S)
    assert not bool(bits[1, : S // 32].any())
    assert _same_bits(out, _probs(G, qp, kb, m8, B, Q, H, S, pieces, key_bits=bits))
    W = out.double().cpu().numpy()
    worst = 0.0
    for b in (0, 2):
        ok, e = P.compare(W[b], p["ref"], rtol)
        assert ok, (b, e, rtol)
        worst = max(worst, e)
    uniform = np.full_like(p["ref"], 1.0 / S)
    P.precondition(uniform, 1)
    ok, e1 = P.compare(W[1], uniform, rtol)
    P._report("cross probs", f"Q={Q} S={S} valid keys={int((p['mask'] != 0).sum())} (uniform user: {e1:.2e})", pieces, ok, max(worst, e1),
              rtol, wmin)


# ------------------------------------------------------------------------------------------------ 2. row independence
def _random_case(G, B, Q, H, S, pieces, seed):
    g = torch.Generator().manual_seed(seed)
    q32 = (torch.randn(B * Q, H * 64, generator=g) * 0.3).to(G.DEV)
    k32 = torch.randn(B, H, S, 64, generator=g).to(G.DEV)
    mask = torch.rand(B, S, generator=g) > 0.3
    mask[1, : S // 2] = False
    if S >= 64 and B > 2:
        mask[2, 32:] = False
    return q32, k32, mask, G.pieces_of(q32, pieces), G.pieces_of(k32, pieces), mask.to(G.DEV).view(torch.uint8).contiguous()


@pytest.mark.parametrize("pieces", [1, 2])
def test_probs_rows_are_independent(G, pieces):
    """Bit for bit: user 0's rows in a B = 1 call and in the B = 3 call; rows 0..4 of a Q = 130 call and a Q = 5 call on those rows."""
    B, Q, H, S = 3, 130, 2, 160
    inner = H * 64
    _q32, _k32, _mask, q, kb, m8 = _random_case(G, B, Q, H, S, pieces, 77)
    full = _probs(G, q, kb, m8, B, Q, H, S, pieces)
    one = _probs(G, q[:, :Q].contiguous(), kb[:, :1].contiguous(), m8[:1].contiguous(), 1, Q, H, S, pieces)
    assert _same_bits(one[0], full[0])
    q5 = q.view(pieces, B, Q, inner)[:, :, :5].reshape(pieces, B * 5, inner).contiguous()
    few = _probs(G, q5, kb, m8, B, 5, H, S, pieces)
    assert _same_bits(few, full[:, :, :5].contiguous())
    assert bool(torch.isfinite(full).all())


# ------------------------------------------------------------------------------------------------ 3. the shipped kernel
@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("S", [96, 384])
@pytest.mark.parametrize("K", [4, 40])
def test_probs_times_v_is_the_cross_attention(G, K, S, pieces):
    """sum over s of probs . V (fp64, V as the bank holds it) against gram_cross_attn_decode_split on the same random operands
    (tests/test_gpu_split.py::test_split_cross_attn's), within that test's bound: 10 * tol(G) relative to rms for two pieces,
    tests/test_gpu_kernels.py::test_cross_attn_decode's 1e-2 for one."""
    from tests.test_gpu_split import relerr, tol
    B, H = 3, 2
    inner = H * 64
    g = torch.Generator().manual_seed(K * 1000 + S)
    q32 = (torch.randn(B * K, inner, generator=g) * 0.3).to(G.DEV)
    k32 = torch.randn(B, H, S, 64, generator=g).to(G.DEV)
    v32 = torch.randn(B, H, S, 64, generator=g).to(G.DEV)
    q, kb, vt = G.pieces_of(q32, pieces), G.pieces_of(k32, pieces), G.pieces_of(G.vt_blocked(v32.transpose(2, 3).contiguous()), pieces)
    mask = torch.rand(B, S, generator=g) > 0.3
    mask[1, : S // 2] = False
    mask[2, 32:] = False
    m8 = mask.to(G.DEV).view(torch.uint8).contiguous()
    out = torch.empty(B * K, pieces * inner, dtype=G.DT, device=G.DEV)
    _lib.check(G.lib().gram_cross_attn_decode_split(G.p(q), G.p(kb), G.p(vt), G.p(m8), G.p(out), B, K, H, S, None, None, pieces,
                                                    q[0].numel(), kb[0].numel(), None, G.stream()), "xattn")
    probs = _probs(G, q, kb, m8, B, K, H, S, pieces)
    v = G.vt_unblocked(G.join(vt)).transpose(2, 3)  # (B, H, S, 64) fp64
    mine = torch.matmul(probs.double(), v).transpose(1, 2).reshape(B * K, inner).cpu()
    got = (G.join_inter(out) if pieces == 2 else out.double()).cpu()
    masked = ~mask[:, None, None, :].expand(B, H, K, S)
    assert bool((probs.cpu()[masked] == 0).all())
    e = relerr(got, mine)
    print(f"\n[probs . V vs cross attn] K={K} S={S} pieces={pieces}: {e:.2e} of rms")
    if pieces == 2:
        assert e < 10 * tol(G)
    else:
        assert torch.allclose(got, mine, atol=1e-2, rtol=1e-2)


# ------------------------------------------------------------------------------------------------ 4. reducers
@pytest.mark.parametrize("N,L", [(3, 32), (21, 128)])
def test_reducers_vs_fp64(G, N, L):
    """gram_xattn_head_sum first, then accumulating; gram_xattn_passage_scores on a ragged mask with an empty passage (NaN)."""
    B, Q, H, S = 2, 5, 3, N * L
    rng = np.random.default_rng(N * 1000 + L)
    pr = [rng.random((B, H, Q, S), dtype=np.float32) / S for _ in range(2)]
    acc = torch.full((B, Q, S), float("nan"), dtype=torch.float32, device=G.DEV)
    for i, p in enumerate(pr):
        d = P._dev(G, p)
        _lib.check(G.lib().gram_xattn_head_sum(G.p(d), G.p(acc), B, Q, H, S, int(i == 0), G.stream()), "gram_xattn_head_sum")
        if i == 0:
            first = acc.cpu().numpy().copy()
    # head order, fp32, one add at a time: the same bits as numpy's sequential fp32 sum
    want32 = np.zeros((B, Q, S), dtype=np.float32)
    for h in range(H):
        want32 = want32 + pr[0][:, h]
    assert np.array_equal(first, want32)
    want = sum(p.astype(np.float64).sum(1) for p in pr)
    got = acc.cpu().numpy()
    e = float(np.abs(got - want).max() / want.max())
    assert e < 2 * H * 2.0 ** -24, e  # 2 H fp32 additions
    lens = rng.integers(1, L + 1, (B, N))
    lens[0, 0], lens[B - 1, N - 1] = L, 0
    valid = np.arange(L)[None, None, :] < lens[..., None]
    mask = P.mask_bytes(rng, valid)
    sc = torch.full((B, Q, N), -1.0, dtype=torch.float32, device=G.DEV)
    denom = float(2 * H)
    _lib.check(G.lib().gram_xattn_passage_scores(G.p(acc), G.p(P._dev(G, mask, torch.uint8)), G.p(sc), B, Q, N, L, denom, G.stream()),
               "gram_xattn_passage_scores")
    s = sc.cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = (got.astype(np.float64).reshape(B, Q, N, L) * valid[:, None]).sum(-1) / (lens[:, None, :] * denom)
    assert np.array_equal(np.isnan(s), np.isnan(ref)) and np.isnan(s[B - 1, :, N - 1]).all() and int(np.isnan(s).sum()) == Q
    ok = ~np.isnan(ref)
    e2 = float((np.abs(s[ok] - ref[ok]) / ref[ok]).max())
    print(f"\n[reducers] N={N} L={L}: head sum {e:.2e}, passage scores {e2:.2e} relative")
    assert e2 < (np.log2(L) + 4) * 2.0 ** -24  # <= L/64 sequential + 6 butterfly additions, one division


# ------------------------------------------------------------------------------------------------ 5. whole path
def _model(oc, seed):
    import gram_amd
    sd = O.init_state_dict(oc, seed)
    cfg = gram_amd.T5Config(vocab_size=oc.vocab_size, d_model=oc.d_model, d_ff=oc.d_ff, num_layers=oc.num_layers,
                            num_decoder_layers=oc.num_decoder_layers, num_heads=oc.num_heads, max_item_num=oc.max_item_num)
    m = gram_amd.create_model("gram", cfg)
    m.load_state_dict(sd)
    return sd, m.to("cuda:0").eval()


def _ragged(g, B, N, L, V):
    """ragged masks; the last user's last passage fully padded"""
    ids = torch.randint(2, V, (B, N, L), generator=g)
    mask = torch.zeros(B, N, L, dtype=torch.bool)
    for b in range(B):
        for n in range(N):
            ln = 0 if (b == B - 1 and n == N - 1) else int(torch.randint(max(2, L // 3), L + 1, (1,), generator=g))
            mask[b, n, :ln] = True
            ids[b, n, ln:] = 0
    return ids, mask


@pytest.fixture(scope="module", params=["tiny", "t5-small"])
def whole(request, G):
    """model, inputs, the fp64 oracle's cross_attentions (computed once) -- L = 40: not a multiple of 32"""
    if request.param == "tiny":
        oc = O.OracleConfig(vocab_size=256, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2, max_item_num=5)
        B, N, L, Cn, T = 3, 3, 40, 2, 4
    else:
        oc = O.OracleConfig.named("t5-small", max_item_num=4)
        B, N, L, Cn, T = 2, 3, 40, 2, 3
    sd, m = _model(oc, 11)
    g = torch.Generator().manual_seed(29)
    ids, mask = _ragged(g, B, N, L, oc.vocab_size)
    lab = torch.randint(2, oc.vocab_size, (B, Cn, T), generator=g)
    lab[0, 0, T - 1] = -100
    from tests.tf_oracle import shift_right
    ref = XO.cross_attentions(sd, oc, ids, mask, shift_right(lab).view(B * Cn, T), fp64=True)  # nl x (B*C, H, T, N*L)
    return dict(name=request.param, oc=oc, m=m, ids=ids, mask=mask, lab=lab, ref=ref, dims=(B, N, L, Cn, T))


def test_whole_path_vs_oracle(whole):
    """cross_attentions and passage_attention at the default precision against the fp64 oracle: probabilities within 2e-5 absolute
    (the project's two-piece whole-path tolerance, tests/test_gpu_path.py::test_split_generate_vs_oracle), rows sum to 1 within 1e-6,
    masked keys exactly 0; the reduced scores within the same per-weight error."""
    m, ids, mask, lab, ref = (whole[k] for k in ("m", "ids", "mask", "lab", "ref"))
    B, N, L, Cn, T = whole["dims"]
    oc = whole["oc"]
    nl, H = oc.num_decoder_layers, oc.num_heads
    idd, mk = ids.cuda(), mask.cuda()
    worst, worst_sum = 0.0, 0.0
    for c in range(Cn):
        ca = m.cross_attentions(idd, mk, labels=lab[:, c].cuda())
        assert isinstance(ca, tuple) and len(ca) == nl
        for i in range(nl):
            got = ca[i].cpu()
            assert got.dtype == torch.float32 and got.shape == (B, H, T, N * L)
            want = ref[i].view(B, Cn, H, T, N * L)[:, c]
            worst = max(worst, float((got.double() - want).abs().max()))
            worst_sum = max(worst_sum, float((got.double().sum(-1) - 1).abs().max()))
            assert bool((got[~mask.reshape(B, 1, 1, N * L).expand_as(got)] == 0).all())
    tok, sc = m.passage_attention(idd, mk, lab.cuda())
    assert tok.shape == (B, Cn, T, N, L) and sc.shape == (B, Cn, T, N)
    ref_tok, ref_sc = XO.passage_scores([r.view(B, Cn, H, T, N * L).transpose(1, 2).reshape(B, H, Cn * T, N * L) for r in ref], mask)
    dt = float((tok.cpu().double().reshape(B, Cn * T, N, L) - ref_tok).abs().max())
    got_sc = sc.cpu().double().reshape(B, Cn * T, N)
    assert torch.equal(got_sc.isnan(), ref_sc.isnan()) and bool(got_sc[B - 1, :, N - 1].isnan().all()) and int(got_sc.isnan().sum()) == Cn * T
    ds = float((got_sc - ref_sc).nan_to_num().abs().max())
    print(f"\n[whole path {whole['name']}] precision {m.precision}: max |p - oracle| {worst:.2e}, max |row sum - 1| {worst_sum:.2e}, "
          f"token scores {dt:.2e} (sum of {nl * H} weights), passage scores {ds:.2e}")
    assert worst <= 2e-5 and worst_sum <= 1e-6
    assert dt <= 2e-5 * nl * H and ds <= 2e-5


def test_first_token_scores_equal_passage_attention(whole):
    """get_crossattention_scores([cross_attentions(decoder_input_ids = zeros(B, 1))], mask[b:b+1], b) = passage_attention's first
    position, per user: passage scores within 1e-6 relative (fp32 sums in another order), the NaN pattern equal."""
    m, ids, mask, lab = (whole[k] for k in ("m", "ids", "mask", "lab"))
    B, N, L, Cn, T = whole["dims"]
    idd, mk = ids.cuda(), mask.cuda()
    ca = m.cross_attentions(idd, mk, decoder_input_ids=torch.zeros(B, 1, dtype=torch.long, device="cuda"))
    assert ca[0].shape == (B, whole["oc"].num_heads, 1, N * L)
    tok, sc = m.passage_attention(idd, mk, lab.cuda())
    worst = 0.0
    for b in range(B):
        t1, s1 = m.get_crossattention_scores([ca], mk[b:b + 1], b)
        s1, want = s1.cpu()[0], sc[b, 0, 0].cpu()
        assert torch.equal(s1.isnan(), want.isnan())
        ok = ~want.isnan()
        worst = max(worst, float(((s1[ok] - want[ok]).abs() / want[ok]).max()))
        t1 = torch.tensor(t1)
        assert t1.shape == (N, L)
        torch.testing.assert_close(t1, tok[b, 0, 0].cpu(), rtol=1e-6, atol=1e-9)
    print(f"\n[first token {whole['name']}] passage scores: {worst:.2e} relative")
    assert worst <= 1e-6


def test_whole_path_bits_do_not_depend_on_the_call(whole):
    """The same bits with users_per_call = 1 and in one call, with a warmed passage cache; score_sequences returns the same bits before
    and after an attention call (the extra launches only read)."""
    m, ids, mask, lab = (whole[k] for k in ("m", "ids", "mask", "lab"))
    idd, mk, lb = ids.cuda(), mask.cuda(), lab.cuda()
    before = m.score_sequences(idd, mk, lb, return_tokens=True)
    ca = m.cross_attentions(idd, mk, labels=lb[:, 0])
    tok, sc = m.passage_attention(idd, mk, lb)
    after = m.score_sequences(idd, mk, lb, return_tokens=True)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    ca1 = m.cross_attentions(idd, mk, labels=lb[:, 0], users_per_call=1)
    tok1, sc1 = m.passage_attention(idd, mk, lb, users_per_call=1)
    assert all(_same_bits(a.contiguous(), b.contiguous()) for a, b in zip(ca, ca1))
    assert _same_bits(tok.contiguous(), tok1.contiguous()) and _same_bits(sc, sc1)
    m.cache_passages(idd[:, 1:], mk[:, 1:])
    try:
        ca2 = m.cross_attentions(idd, mk, labels=lb[:, 0])
        tok2, sc2 = m.passage_attention(idd, mk, lb)
    finally:
        m.clear_passage_cache()
    assert all(_same_bits(a.contiguous(), b.contiguous()) for a, b in zip(ca, ca2))
    assert _same_bits(tok.contiguous(), tok2.contiguous()) and _same_bits(sc, sc2)
    with pytest.raises(NotImplementedError):  # the refusal of forward(output_attentions=True) stays
        m(input_ids=idd, attention_mask=mk, labels=lb[:, 0], output_attentions=True)
