"""-m gpu: the head-summed token scores over fused contexts of up to 16 384 keys (gram_cross_attn_token_scores_split,
xattn_scores.hip), the whole path over them (gram_teacher_forced_scores, torch.ops.gram.teacher_forced_scores) and
``GRAM.passage_attention(fused=...)``.

1. The probes of tests/test_gpu_attn_probes.py at every key-bit word: the sum over heads of the fp64 weights under that file's
   comparator and bounds (a sum of weights each within rtol is within rtol), expected zeros exactly 0.0, the user without a valid
   key H / S.
2. Dense masks across many steps (tests/test_gpu_fused_len.py's six users) against fp64 softmax on the kernel's own rounded
   operands: per valid key within the probes' bound, masked keys exactly 0.0, rows sum to H.
3. Accumulation over two launches (first = 1, then 0); a fully masked step's keys stay 0.0.
4. Bit equalities: a user alone and among five; rows 0..4 of a Q = 65 and a Q = 5 call; the same valid keys at three paddings; NaN in
   every masked position of the K bank.
5. The whole path on a raised tiny model against tests/xattn_oracle.py in fp64, above 4096 fused keys.
6. fused=True against fused=False below 4096 keys; users_per_call; score_sequences untouched; cross_attentions keeps its limit.
7. The custom op against the C ABI call.

Every acc is pre-filled with NaN before a first = 1 launch.  Observed values are printed."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gram_amd import _lib
from tests import test_gpu_attn_probes as P
from tests import test_gpu_path as TP
from tests import xattn_oracle as XO
from tests.test_gpu_fused_len import _bank, _bits, _masks, _model, _oc, _place, _queries, _users  # noqa: F401
from tests.test_gpu_xattn_probs import _ragged
from tests.tf_oracle import shift_right

pytestmark = pytest.mark.gpu

H_ = 3


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    return gpu_util


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gram_amd
    return gram_amd


def _scores(G, q, kb, bits, B, Q, H, S, pieces, first=1, acc=None):
    """q [pieces][B*Q][inner] planar, kb [pieces][B][H][S][64], bits from gram_mask_key_bits_long -> acc f32 [B][Q][S] (NaN-pre-filled
    when not given)"""
    if acc is None:
        acc = torch.full((B, Q, S), float("nan"), dtype=torch.float32, device=G.DEV)
    _lib.check(G.lib().gram_cross_attn_token_scores_split(G.p(q), G.p(kb), G.p(acc), B, Q, H, S, pieces, q[0].numel(), kb[0].numel(),
                                                          G.p(bits), int(first), G.stream()), "gram_cross_attn_token_scores_split")
    torch.cuda.synchronize()
    return acc


def _m8(G, mask):
    return mask.to(G.DEV).view(torch.uint8).contiguous()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1. probes
@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("S", [32, 96, 4096, 4128, 8224, 12320, 16384])
@pytest.mark.parametrize("Q", [1, 17, 33, 65])
def test_probe_token_scores(G, Q, S, pieces):
    """Users 0 and 2 carry the probe, user 1 has no valid key (as tests/test_gpu_xattn_probs.py::test_probe_cross_attn_probs)."""
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
    bits = _bits(G, m8, B, S)
    assert not bool(bits[1, : S // 32].any())
    qp = P._pieces(G, q.view(B * Q, inner), pieces)
    W = _scores(G, qp, kb, bits, B, Q, H, S, pieces).double().cpu().numpy()
    want = p["ref"].sum(0)  # (Q, S): heads summed in fp64
    worst = 0.0
    for b in (0, 2):
        ok, e = P.compare(W[b], want, rtol)
        assert ok, (b, e, rtol)
        worst = max(worst, e)
    ok, e1 = P.compare(W[1], np.full_like(want, H / S), rtol)
    steps = np.nonzero((p["mask"] != 0).reshape(-1, 32).any(1))[0]
    P._report("token scores", f"Q={Q} S={S} valid steps={steps.size} in [{steps.min()}, {steps.max()}] (uniform user: {e1:.2e})", pieces, ok,
              max(worst, e1), rtol, wmin)


# ------------------------------------------------------------------------------------------------ 2. dense masks
def _reference(G, q, bank, mask, Q):
    """fp64 softmax of the rounded operands, summed over heads -> (B, Q, S); a masked key scores finfo.min exactly"""
    B, H = bank.B, bank.H
    qh = G.join(q).view(B, Q, H, 64).permute(0, 2, 1, 3)
    sc = torch.matmul(qh, bank.k64.transpose(3, 2))
    sc = torch.where(mask.to(sc.device)[:, None, None, :], sc, torch.full((), float(P.FMIN), dtype=torch.float64, device=sc.device))
    return torch.softmax(sc, -1).sum(1)


def _check_dense(got, ref, mask, H, rtol, what):
    """per valid key the relative error (every key of a user without a valid one), masked keys exactly 0.0, rows sum to H"""
    md = mask.to(ref.device)
    none = ~md.any(1)
    counted = (md | none[:, None])[:, None, :].expand_as(ref)
    assert float(ref[counted].min()) >= 1e-20  # (on the reference alone: queries scaled by 0.3 keep every weight far above this)
    g64 = got.double()
    assert bool(torch.isfinite(got).all())
    rel = float(((g64 - ref).abs() / ref)[counted].max())
    assert bool((got[~counted] == 0).all()), "a masked key is not exactly 0.0"
    rows = float((g64.sum(-1) - H).abs().max())
    print(f"\n[token scores {what}] max relative error on a valid key {rel:.2e} (bound {rtol:.2e}), max |row sum - H| {rows:.2e}")
    assert rows <= H * 1e-6, rows
    return rel


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("Q", [5, 40])
@pytest.mark.parametrize("S", [4128, 8224, 16384])
def test_dense_masks_against_fp64_on_the_kernels_own_operands(G, S, Q, pieces):
    rtol = P._rtol(G, pieces)
    mask = _masks(S, torch.Generator().manual_seed(S))
    bank = _bank(G, 6, S, pieces, seed=S + pieces)
    q = _queries(G, 6 * Q, pieces, seed=Q)
    got = _scores(G, q, bank.kb, _bits(G, _m8(G, mask), 6, S), 6, Q, H_, S, pieces)
    rel = _check_dense(got, _reference(G, q, bank, mask, Q), mask, H_, rtol, f"S={S} Q={Q} pieces={pieces}")
    assert rel <= rtol, rel


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("H", [1, 8, 9, 12, 16])
def test_every_head_count_path(G, H, pieces):
    """One wave; eight waves, one round; two rounds with one, four and eight waves owning a second head (T5-base: 12 heads)."""
    S, Q, B = 4128, 37, 6
    rtol = P._rtol(G, pieces)
    mask = _masks(S, torch.Generator().manual_seed(H))
    bank = _bank(G, B, S, pieces, seed=70 + H, H=H)
    q = _queries(G, B * Q, pieces, seed=7, H=H)
    got = _scores(G, q, bank.kb, _bits(G, _m8(G, mask), B, S), B, Q, H, S, pieces)
    rel = _check_dense(got, _reference(G, q, bank, mask, Q), mask, H, rtol, f"H={H} S={S} Q={Q} pieces={pieces}")
    assert rel <= rtol, rel


# ------------------------------------------------------------------------------------------------ 3. accumulation
@pytest.mark.parametrize("pieces", [2, 1])
def test_two_launches_accumulate(G, pieces):
    """first = 1 on one K bank, first = 0 on another: the sum of both against fp64 within twice the bound of one launch; the keys of
    fully masked steps are written as 0.0 by the first launch and left alone by the second."""
    S, Q, B = 8224, 37, 6
    rtol = P._rtol(G, pieces)
    mask = _masks(S, torch.Generator().manual_seed(5))
    banks = [_bank(G, B, S, pieces, seed=81 + i) for i in range(2)]
    q = _queries(G, B * Q, pieces, seed=83)
    bits = _bits(G, _m8(G, mask), B, S)
    acc = _scores(G, q, banks[0].kb, bits, B, Q, H_, S, pieces)
    one = acc.clone()
    _scores(G, q, banks[1].kb, bits, B, Q, H_, S, pieces, first=0, acc=acc)
    ref = _reference(G, q, banks[0], mask, Q) + _reference(G, q, banks[1], mask, Q)
    md = mask.to(G.DEV)
    counted = (md | ~md.any(1)[:, None])[:, None, :].expand_as(ref)
    rel = float(((acc.double() - ref).abs() / ref)[counted].max())
    print(f"\n[token scores, two launches] pieces={pieces}: max relative error {rel:.2e} (bound {2 * rtol:.2e})")
    assert rel <= 2 * rtol, rel
    assert bool((acc[~counted] == 0).all()) and bool((one[~counted] == 0).all())
    dead = ~md.view(B, S // 32, 32).any(-1) & md.any(1)[:, None]  # fully masked steps of users that have valid keys
    assert bool(dead[4].any()) and bool((acc.view(B, Q, S // 32, 32)[dead[:, None].expand(B, Q, -1)] == 0).all())
    assert bool((acc[counted] >= one[counted]).all()) and float((acc - one).sum()) > 0.5 * B * Q * H_  # (the second launch came on top)


# ------------------------------------------------------------------------------------------------ 4. bit equalities
@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("S", [4128, 12320])
def test_a_user_alone_and_among_five(G, S, pieces):
    B, Q = 5, 40
    mask = _masks(S, torch.Generator().manual_seed(3))[[0, 1, 3, 4, 2]]
    bank = _bank(G, B, S, pieces, seed=11)
    q = _queries(G, B * Q, pieces, seed=12)
    out = _scores(G, q, bank.kb, _bits(G, _m8(G, mask), B, S), B, Q, H_, S, pieces)
    assert bool(torch.isfinite(out).all())
    for u in range(B):
        got = _scores(G, q[:, u * Q:(u + 1) * Q].contiguous(), bank.kb[:, u:u + 1].contiguous(), _bits(G, _m8(G, mask[u:u + 1]), 1, S), 1, Q,
                      H_, S, pieces)
        assert _same_bits(got[0], out[u]), u


@pytest.mark.parametrize("pieces", [2, 1])
def test_rows_do_not_depend_on_the_number_of_rows(G, pieces):
    B, S, inner = 3, 8224, H_ * 64
    mask = _masks(S, torch.Generator().manual_seed(6))[[1, 3, 5]]
    bank = _bank(G, B, S, pieces, seed=31)
    q = _queries(G, B * 65, pieces, seed=32)
    bits = _bits(G, _m8(G, mask), B, S)
    full = _scores(G, q, bank.kb, bits, B, 65, H_, S, pieces)
    q5 = q.view(pieces, B, 65, inner)[:, :, :5].reshape(pieces, B * 5, inner).contiguous()
    few = _scores(G, q5, bank.kb, bits, B, 5, H_, S, pieces)
    assert bool(torch.isfinite(full).all()) and _same_bits(few, full[:, :5])


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("N0", [24, 60])
def test_the_same_valid_keys_at_three_paddings(G, N0, pieces):
    """L = 96 | the same passages padded to 256 (N0 = 24: 2304 -> 6144 keys; N0 = 60: 5760 -> 15360: keys move across 4096 and 8192) |
    N padded with fully masked passages: the same bits on the valid keys, 0.0 everywhere else."""
    Q, L0 = 37, 96
    lens = torch.randint(65, L0 + 1, (N0,), generator=torch.Generator().manual_seed(N0))
    base = _bank(G, 1, N0 * L0, pieces, seed=41)
    q = _queries(G, Q, pieces, seed=42)
    outs = []
    for L, N in ((L0, N0), (256, N0), (L0, N0 + 8)):
        bank, mask = _place(G, base, lens, L0, L, N, pieces, seed=43 + L + N)
        acc = _scores(G, q, bank.kb, _bits(G, _m8(G, mask), 1, N * L), 1, Q, H_, N * L, pieces)
        md = mask[0].to(G.DEV)
        assert bool((acc[0][:, ~md] == 0).all())
        outs.append(acc[0][:, md])
    assert outs[0].shape == (Q, int(lens.sum())) and bool((outs[0] > 0).all())
    assert _same_bits(outs[0], outs[1]) and _same_bits(outs[0], outs[2])


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("S", [4128, 12320])
def test_masked_keys_contribute_nothing(G, S, pieces):
    """NaN in every masked position of the K bank (every piece): the same bits.  (The user without a valid key is left out: all its
    keys count.)"""
    B, Q = 5, 40
    mask = _masks(S, torch.Generator().manual_seed(8))[:5]
    assert bool(mask.any(1).all())
    bank = _bank(G, B, S, pieces, seed=61)
    q = _queries(G, B * Q, pieces, seed=62)
    bits = _bits(G, _m8(G, mask), B, S)
    clean = _scores(G, q, bank.kb, bits, B, Q, H_, S, pieces)
    nan = torch.full((), float("nan"), dtype=G.DT, device=G.DEV)
    dirty_k = torch.where(mask.to(G.DEV)[None, :, None, :, None], bank.kb, nan).contiguous()
    assert bool(torch.isnan(dirty_k.float()).any())
    dirty = _scores(G, q, dirty_k, bits, B, Q, H_, S, pieces)
    assert bool(torch.isfinite(dirty).all()) and _same_bits(clean, dirty)


# ------------------------------------------------------------------------------------------------ 5. - 7. the whole path
@functools.lru_cache(maxsize=None)
def _raised(gpu):
    """the tiny backbone at the default precision, raised to 512-token passages and 16 384 fused tokens"""
    oc, sd, m = TP._model(gpu, _oc("tiny"), 11)
    m.set_max_passage_len(512)
    m.set_max_fused_tokens(16384)
    return oc, sd, m


def _oracle(sd, oc, ids, mask, lab):
    B, Cn, T = lab.shape
    N, L = ids.shape[1:]
    H = oc.num_heads
    ref = XO.cross_attentions(sd, oc, ids, mask, shift_right(lab).view(B * Cn, T), fp64=True)  # nl x (B*C, H, T, N*L)
    return XO.passage_scores([r.view(B, Cn, H, T, N * L).transpose(1, 2).reshape(B, H, Cn * T, N * L) for r in ref], mask)


def _against_oracle(tok, sc, ref_tok, ref_sc, dims, nl, H, what):
    B, N, L, Cn, T = dims
    assert tok.shape == (B, Cn, T, N, L) and sc.shape == (B, Cn, T, N) and tok.dtype == sc.dtype == torch.float32
    dt = float((tok.cpu().double().reshape(B, Cn * T, N, L) - ref_tok).abs().max())
    got_sc = sc.cpu().double().reshape(B, Cn * T, N)
    assert torch.equal(got_sc.isnan(), ref_sc.isnan()) and bool(got_sc[B - 1, :, N - 1].isnan().all()) and int(got_sc.isnan().sum()) == Cn * T
    ds = float((got_sc - ref_sc).nan_to_num().abs().max())
    print(f"\n[passage_attention {what}] token scores {dt:.2e} (sum of {nl * H} weights; bound {2e-5 * nl * H:.1e}), passage scores {ds:.2e} "
          f"(bound 2e-5)")
    assert dt <= 2e-5 * nl * H and ds <= 2e-5
    return dt, ds


@pytest.mark.parametrize("B,N,L", [(2, 21, 224), (1, 32, 512)])
def test_whole_path_above_4096_keys_vs_oracle(gpu, B, N, L):
    """4704 and 16 384 fused keys, ragged masks with one empty passage, against the fp64 oracle: token scores within 2e-5 * layers *
    heads, passage scores within 2e-5 (tests/test_gpu_xattn_probs.py::test_whole_path_vs_oracle's bounds), the NaN pattern equal."""
    oc, sd, m = _raised(gpu)
    Cn, T = 2, 3
    g = torch.Generator().manual_seed(N * L + B)
    ids, mask = _ragged(g, B, N, L, oc.vocab_size)
    lab = torch.randint(2, oc.vocab_size, (B, Cn, T), generator=g)
    lab[0, 0, T - 1] = -100
    ref_tok, ref_sc = _oracle(sd, oc, ids, mask, lab)
    tok, sc = m.passage_attention(ids.cuda(), mask.cuda(), lab.cuda())
    _against_oracle(tok, sc, ref_tok, ref_sc, (B, N, L, Cn, T), oc.num_decoder_layers, oc.num_heads, f"{B}x{N}x{L}")
    assert bool((tok.cpu()[~mask[:, None, None].expand(B, Cn, T, N, L)] == 0).all())


def test_fused_against_unfused_below_4096_keys(gpu):
    oc, sd, m = _raised(gpu)
    B, N, L, Cn, T = 3, 3, 40, 2, 4
    nl, H = oc.num_decoder_layers, oc.num_heads
    g = torch.Generator().manual_seed(29)
    ids, mask = _ragged(g, B, N, L, oc.vocab_size)
    lab = torch.randint(2, oc.vocab_size, (B, Cn, T), generator=g)
    lab[0, 0, T - 1] = -100
    idd, mk, lb = ids.cuda(), mask.cuda(), lab.cuda()
    ref_tok, ref_sc = _oracle(sd, oc, ids, mask, lab)
    before = m.score_sequences(idd, mk, lb, return_tokens=True)
    tok0, sc0 = m.passage_attention(idd, mk, lb, fused=False)
    tok1, sc1 = m.passage_attention(idd, mk, lb, fused=True)
    after = m.score_sequences(idd, mk, lb, return_tokens=True)
    assert all(torch.equal(a, b) for a, b in zip(before, after))  # (the extra launches only read)
    _against_oracle(tok0, sc0, ref_tok, ref_sc, (B, N, L, Cn, T), nl, H, "fused=False")
    _against_oracle(tok1, sc1, ref_tok, ref_sc, (B, N, L, Cn, T), nl, H, "fused=True")
    d_tok = float((tok0.double() - tok1.double()).abs().max())
    d_sc = float((sc0.double() - sc1.double()).nan_to_num().abs().max())
    print(f"[fused vs unfused] token scores {d_tok:.2e}, passage scores {d_sc:.2e}")
    assert d_tok <= 2 * 2e-5 * nl * H and d_sc <= 2 * 2e-5 and torch.equal(sc0.isnan(), sc1.isnan())
    tokd, scd = m.passage_attention(idd, mk, lb)  # the default below 4096 keys: today's path
    assert _same_bits(tokd, tok0) and _same_bits(scd, sc0)
    tok2, sc2 = m.passage_attention(idd, mk, lb, fused=True, users_per_call=1)
    assert _same_bits(tok1, tok2) and _same_bits(sc1, sc2)
    ids5, mask5, _c, _l = _users(2, 21, 224)
    with pytest.raises(ValueError, match="limited to 4096 fused tokens"):
        m.cross_attentions(ids5.cuda(), mask5.cuda(), decoder_input_ids=torch.zeros(2, 1, dtype=torch.long))
    with pytest.raises(ValueError, match="limited to 4096 fused tokens"):
        m.passage_attention(ids5.cuda(), mask5.cuda(), torch.ones(2, 1, 2, dtype=torch.long), fused=False)


def test_the_custom_op_equals_the_c_abi_call(gpu):
    import gram_amd.ops  # noqa: F401
    oc, sd, m = _raised(gpu)
    B, N, L, Cn, T = 2, 21, 224, 2, 3
    g = torch.Generator().manual_seed(77)
    ids, mask = _ragged(g, B, N, L, oc.vocab_size)
    lab = torch.randint(2, oc.vocab_size, (B, Cn, T), generator=g)
    dev = torch.device("cuda:0")
    idd = ids.to(dev, torch.int64).contiguous()
    m8 = mask.to(dev).view(torch.uint8).contiguous()
    dec, lb = shift_right(lab).to(dev, torch.int32).contiguous(), lab.to(dev, torch.int32).contiguous()
    lib = _lib.load()
    handle = m._pack()
    need = lib.gram_workspace_bytes_tf(handle, B, N, L, Cn, T)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    tok, sc = torch.ops.gram.teacher_forced_scores(idd, m8, int(handle), ws, dec, lb, int(oc.vocab_size), None, None, None, None, None, 0, 0)
    assert tok.shape == (B, Cn * T, N * L) and sc.shape == (B, Cn * T, N)
    f = dict(dtype=torch.float32, device=dev)
    tok2, sc2 = torch.full((B, Cn * T, N * L), float("nan"), **f), torch.full((B, Cn * T, N), -1.0, **f)
    tlp, slp = torch.empty(B, Cn, T, **f), torch.empty(B, Cn, **f)
    out = _lib.XattnScores(tok2.data_ptr(), sc2.data_ptr())
    with torch.cuda.device(dev):
        rc = lib.gram_teacher_forced_scores(handle, idd.data_ptr(), m8.data_ptr(), B, N, L, None, dec.data_ptr(), lb.data_ptr(), Cn, T,
                                            ws.data_ptr(), ws.numel(), None, tlp.data_ptr(), slp.data_ptr(), C.byref(out),
                                            torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "gram_teacher_forced_scores")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tok2).all()) and _same_bits(tok, tok2) and _same_bits(sc, sc2)
    seq = m.score_sequences(idd, mask.to(dev), lab.to(dev))
    assert torch.equal(seq.view(B, Cn), slp)  # the pass's own outputs are gram_teacher_forced's
    default = TP._model(gpu, _oc("tiny"), 11)[2]
    with pytest.raises(ValueError, match="set_max_fused_tokens"):
        default.passage_attention(idd[:, :3, :32], mask[:, :3, :32].to(dev), lab.to(dev), fused=True)
