"""-m gpu: fused contexts of up to 16 384 tokens -- the segmented cross-attention (gram_mask_key_bits_long,
gram_cross_attn_long_split, gram_cross_attn_rows_long_split), the KV-bank GEMM epilogue at S > 4096 and the whole path on a model
raised by ``GRAM.set_max_fused_tokens``.

1. The kernel through the C ABI against an fp64 restatement on its own rounded operands, both piece modes, K = 4, 20, 40, 64, H = 3,
   at S = 32 (one step), 4096 (exactly one segment), 4128 (one step into the second), 8192 (exactly two), 8224, 12320, 16384.  One
   user per mask: all valid | a valid prefix ending inside the second segment | valid keys in the first 4096 only | valid keys in the
   last 32 positions plus scattered holes | every other passage of 128 fully masked | nothing valid (the mean of V over exactly S
   keys).  Tolerances are the project's own for the same roundings: tests/test_gpu_split.py::test_split_cross_attn at two pieces
   (imported), tests/test_gpu_kernels.py::test_cross_attn_decode at one (its allclose bounds, which that test states inline).  Every
   output row carries a NaN sentinel before the launch: every live row is written and no other.
2. Bit equalities of the long form: a user alone and among five; the live-row form and the all-rows form; the same query rows at
   K = 4, 20, 40, 64; the same valid keys at three paddings (L = 96, the same padded to 256 -- keys move across 4096 and 8192 -- and
   N padded with masked passages), for a user of one segment and a user of two; the rows form at Q = 70 and 130 against the all-rows
   form on the gathered rows.
3. Masked keys contribute nothing: NaN in every masked position of the K and V^T banks, same bits.
4. gram_mask_key_bits_long against a Python packing.
5. The KV-bank GEMM epilogue at S = 4128 and 16384 (identity) and at (N, L) = (33, 128), (21, 512) (compaction), through the
   128-row kernel and the ping-pong kernel, both piece modes: both kernels the same bits, every row where its passage belongs, nothing
   else written in the bank or behind it.  (Reduction length 128 at two pieces; 256 at one piece, where the ping-pong kernel declines
   128: it wants four 64-column steps.)  The guard of the ping-pong kernel: S = 16416 and M = 2^28 refused.
6. The whole path against the oracle on a raised model (fused encoder, generate, score_sequences, score_all_items == score_sequences,
   generate with exclude_items), and its bit equalities: a batch against each user alone, (N, L) = (9, 480) against the same users
   padded to (21, 512), cold against warm passage cache, token tables on and off, live rows on and off.  A default model names
   set_max_fused_tokens(4704) and computes what it computed; attention probabilities on a raised model below 4096 keys.

Observed values are printed."""
import ctypes as C
import functools
import types

import pytest
import torch

from gram_amd import _lib
from oracle import gram_oracle as O
from tests import test_gpu_path as TP
from tests.test_gpu_configs import ONE, TWO
from tests.test_gpu_long_passages import _fn, _gen, _run, _same
from tests.test_gpu_path import DEV, SCORE_TOL, _check_generate, _inputs, _random_items
from tests.test_gpu_scale import _rescored
from tests.test_gpu_split import relerr, tol
from tests.test_gpu_teacher_forced import _labels, _tol

pytestmark = pytest.mark.gpu

H_ = 3
SENTINEL = 0x7D7D  # an IEEE-half NaN (and a bfloat16 one): no attention output
STRIDE, WORDS = _lib.GRAM_KEY_BITS_LONG_STRIDE, _lib.GRAM_KEY_BITS_LONG_WORDS
S_ALL = [32, 4096, 4128, 8192, 8224, 12320, 16384]
K_ALL = [4, 20, 40, 64]


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


# ------------------------------------------------------------------------------------------------------------ the kernel alone
def _masks(S, g):
    """(6, S) bool, one user per row: see the module docstring"""
    m = torch.zeros(6, S, dtype=torch.bool)
    m[0] = True
    lo, hi = (4097, min(S, 8192)) if S > 4097 else (1, S)
    m[1, : int(torch.randint(lo, hi + 1, (1,), generator=g))] = True
    n = min(4096, S)
    m[2, :n] = torch.rand(n, generator=g) > 0.4
    m[2, 5] = True
    m[3, : S - 32] = torch.rand(S - 32, generator=g) > 0.5
    m[3, S - 32 + int(torch.randint(0, 32, (1,), generator=g))] = True
    m[4] = (torch.arange(S) // 128) % 2 == 0
    return m


def _bank(G, B, S, pieces, seed, H=H_):
    """random K / V^T banks as planar pieces [pieces][B][H][S][64] / [pieces][B][H][S/32][64][32], with their fp64 values (device)"""
    g = torch.Generator(device=G.DEV).manual_seed(seed)
    k32 = torch.randn(B, H, S, 64, generator=g, device=G.DEV)
    v32 = torch.randn(B, H, S, 64, generator=g, device=G.DEV)
    kb = G.pieces_of(k32, pieces)
    vt = G.pieces_of(G.vt_blocked(v32.transpose(2, 3).contiguous()), pieces)
    return types.SimpleNamespace(kb=kb, vt=vt, k64=G.join(kb), v64=G.vt_unblocked(G.join(vt)).transpose(2, 3), B=B, S=S, H=H, pieces=pieces)


def _queries(G, rows, pieces, seed, H=H_):
    g = torch.Generator(device=G.DEV).manual_seed(seed)
    return G.pieces_of(torch.randn(rows, H * 64, generator=g, device=G.DEV) * 0.3, pieces)


def _bits(G, mask8, B, S):
    bits = torch.full((B, STRIDE), -1, dtype=torch.int32, device=G.DEV)
    _lib.check(G.lib().gram_mask_key_bits_long(G.p(mask8), G.p(bits), B, S, G.stream()), "gram_mask_key_bits_long")
    return bits


def _scratch(G, rows, H, S):
    n = G.lib().gram_cross_attn_long_scratch_bytes(rows, H, S)
    assert n >= 0
    return torch.full((max(n // 4, 4),), float("nan"), dtype=torch.float32, device=G.DEV)


def _launch(G, q, bank, mask, K, users=None, rowpos=None, n_rows=None):
    """gram_cross_attn_long_split on planar pieces -> the raw output ([rows][pieces * inner]) pre-filled with the sentinel"""
    B, S, H, pieces = bank.B, bank.S, bank.H, bank.pieces
    m8 = mask.to(G.DEV).view(torch.uint8).contiguous()
    bits = _bits(G, m8, B, S)
    nu = B if users is None else int(users.numel())
    out = torch.full((q.shape[1] if n_rows is None else n_rows, pieces * H * 64), SENTINEL, dtype=torch.int16, device=G.DEV).view(G.DT)
    rc = G.lib().gram_cross_attn_long_split(G.p(q), G.p(bank.kb), G.p(bank.vt), G.p(m8), G.p(out), nu, K, H, S, G.p(users), G.p(rowpos), pieces,
                                            q[0].numel(), bank.kb[0].numel(), G.p(bits), G.p(_scratch(G, nu * K, H, S)), G.stream())
    _lib.check(rc, "gram_cross_attn_long_split")
    torch.cuda.synchronize()
    return out


def _written(out):
    """bool per row: no element of the row is the sentinel any more"""
    return (out.view(torch.int16) != SENTINEL).all(1)


def _value(G, out, pieces):
    return G.join_inter(out) if pieces == 2 else out.double()


def _reference(q64, bank, mask, K):
    """fp64 softmax attention of the rounded operands; a masked key scores finfo.min exactly, so a user without a valid key gets the
    uniform row over all S keys"""
    B, H = bank.B, bank.H
    qh = q64.view(B, K, H, 64).permute(0, 2, 1, 3)
    sc = torch.matmul(qh, bank.k64.transpose(3, 2))
    sc = torch.where(mask.to(sc.device)[:, None, None, :], sc, torch.full((), float(O.FMIN), dtype=torch.float64, device=sc.device))
    return torch.matmul(torch.softmax(sc, -1), bank.v64).transpose(1, 2).reshape(B * K, H * 64)


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("S", S_ALL)
def test_kernel_against_fp64_on_its_own_operands(G, S, pieces):
    """Observed on MI355X (printed per case): max error / rms of the reference 1.2e-6 .. 1.7e-5 at two pieces (bound
    2e-4), max abs 1.06e-3 at one piece (bound 1e-2) -- no larger above 4096 keys than below, so the shipped kernel's bounds hold at
    every S and none was derived for the longer sums."""
    g = torch.Generator().manual_seed(S)
    mask = _masks(S, g)
    bank = _bank(G, 6, S, pieces, seed=S + pieces)
    for K in K_ALL:
        q = _queries(G, 6 * K, pieces, seed=K)
        out = _launch(G, q, bank, mask, K)
        assert bool(_written(out).all()), "rows left unwritten"
        got, ref = _value(G, out, pieces), _reference(G.join(q), bank, mask, K)
        e, a = relerr(got, ref), float((got - ref).abs().max())
        print(f"\n[long cross attn S={S} K={K}] pieces={pieces}: max err / rms {e:.2e}, max abs {a:.2e}")
        if pieces == 2:
            assert e < 10 * tol(G), e  # tests/test_gpu_split.py::test_split_cross_attn
        else:
            assert torch.allclose(got, ref, atol=1e-2, rtol=1e-2), a  # tests/test_gpu_kernels.py::test_cross_attn_decode
        # nothing valid: the mean of V over exactly S keys
        mean_v = bank.v64[5].mean(1)  # (H, 64)
        d = float((got[5 * K:].view(K, bank.H, 64) - mean_v[None]).abs().max())
        assert d < (1e-5 if pieces == 2 else 2e-3), d


# ---- bit equalities
def _user_masks(S, B, seed):
    g = torch.Generator().manual_seed(seed)
    m = _masks(S, g)
    return m[[0, 1, 3, 4, 2, 5][:B]]


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("S", [4128, 12320])
def test_a_user_alone_and_among_five(G, S, pieces):
    B, K = 5, 20
    mask = _user_masks(S, B, 3)
    bank = _bank(G, B, S, pieces, seed=11)
    q = _queries(G, B * K, pieces, seed=12)
    out = _launch(G, q, bank, mask, K)
    for u in range(B):
        one = types.SimpleNamespace(kb=bank.kb[:, u:u + 1].contiguous(), vt=bank.vt[:, u:u + 1].contiguous(), B=1, S=S, H=bank.H, pieces=pieces)
        got = _launch(G, q[:, u * K:(u + 1) * K].contiguous(), one, mask[u:u + 1], K)
        assert bool(_written(got).all()) and torch.equal(got.view(torch.int16), out[u * K:(u + 1) * K].view(torch.int16)), u


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("S", [4096, 8224])
def test_the_live_row_form_equals_the_all_rows_form(G, S, pieces):
    """some beams dead, one user dropped: the compact rows hold what the all-rows form put at b * K + beam, and nothing else is written"""
    B, K = 4, 20
    mask = _user_masks(S, B, 4)
    bank = _bank(G, B, S, pieces, seed=21)
    q = _queries(G, B * K, pieces, seed=22)
    full = _launch(G, q, bank, mask, K)
    g = torch.Generator().manual_seed(5)
    live = torch.rand(B * K, generator=g) > 0.3
    live[2 * K:3 * K] = False  # user 2 is gone
    live[0] = True
    rows = torch.nonzero(live).flatten()
    rowpos = torch.full((B * K,), -1, dtype=torch.int32)
    rowpos[rows] = torch.arange(rows.numel(), dtype=torch.int32)
    users = torch.tensor([0, 1, 3], dtype=torch.int32, device=G.DEV)
    qc = q[:, rows.to(G.DEV)].contiguous()
    n = int(rows.numel())
    out = _launch(G, qc, bank, mask, K, users=users, rowpos=rowpos.to(G.DEV), n_rows=n + 3)
    w = _written(out)
    assert bool(w[:n].all()) and not bool(w[n:].any())
    assert torch.equal(out[:n].view(torch.int16), full[rows.to(G.DEV)].view(torch.int16))


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("S", [4096, 8224])
def test_the_same_query_rows_at_every_beam_tile_count(G, S, pieces):
    B = 3
    mask = _user_masks(S, B, 6)
    bank = _bank(G, B, S, pieces, seed=31)
    q64 = _queries(G, B * 64, pieces, seed=32)
    ref = _launch(G, q64, bank, mask, 64).view(B, 64, -1)
    for K in (4, 20, 40):
        q = q64.view(pieces, B, 64, -1)[:, :, :K].reshape(pieces, B * K, -1).contiguous()
        out = _launch(G, q, bank, mask, K).view(B, K, -1)
        assert torch.equal(out.view(torch.int16), ref[:, :K].contiguous().view(torch.int16)), K


def _place(G, base, lens, L0, L, N, pieces, seed):
    """One user: the valid keys of `base` (a bank at N0 passages of L0, lens valid each) in a bank of N passages of L; the rest of the new
    bank is other random data, masked."""
    N0 = lens.numel()
    new = _bank(G, 1, N * L, pieces, seed=seed, H=base.H)
    mask = torch.zeros(1, N * L, dtype=torch.bool)
    kb = new.kb.view(pieces, 1, base.H, N, L, 64)
    vt = G.vt_unblocked(new.vt).view(pieces, 1, base.H, 64, N, L)
    kb[:, :, :, :N0, :L0] = base.kb.view(pieces, 1, base.H, N0, L0, 64)
    vt[:, :, :, :, :N0, :L0] = G.vt_unblocked(base.vt).view(pieces, 1, base.H, 64, N0, L0)
    for n in range(N0):
        mask[0, n * L: n * L + int(lens[n])] = True
    new.kb = kb.view(pieces, 1, base.H, N * L, 64).contiguous()
    new.vt = G.vt_blocked(vt.reshape(pieces, 1, base.H, 64, N * L)).contiguous()
    return new, mask


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("N0", [24, 60])  # <= 72 valid steps: one segment; 180: two
def test_the_same_valid_keys_at_three_paddings(G, N0, pieces):
    """L = 96 | the same passages padded to 256 (N0 = 24: 2304 -> 6144 keys, passages 16.. move past 4096; N0 = 60: 5760 -> 15360) | N
    padded with fully masked passages.  The collator trims L and N per batch: a user's bits must not follow."""
    K, L0 = 20, 96
    g = torch.Generator().manual_seed(N0)
    lens = torch.randint(65, L0 + 1, (N0,), generator=g)  # three steps per passage
    base = _bank(G, 1, N0 * L0, pieces, seed=41)
    q = _queries(G, K, pieces, seed=42)
    outs = []
    for L, N in ((L0, N0), (256, N0), (L0, N0 + 8)):
        bank, mask = _place(G, base, lens, L0, L, N, pieces, seed=43 + L + N)
        out = _launch(G, q, bank, mask, K)
        assert bool(_written(out).all())
        outs.append(out.view(torch.int16))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("Q", [70, 130])
def test_the_rows_form_equals_the_all_rows_form_on_gathered_rows(G, Q, pieces):
    B, S = 2, 8224
    mask = _user_masks(S, B, 7)
    bank = _bank(G, B, S, pieces, seed=51)
    q = _queries(G, B * Q, pieces, seed=52)
    m8 = mask.to(G.DEV).view(torch.uint8).contiguous()
    bits = _bits(G, m8, B, S)
    inner = bank.H * 64
    out = torch.full((B * Q, pieces * inner), SENTINEL, dtype=torch.int16, device=G.DEV).view(G.DT)
    rowmap = torch.zeros(B * (1 + 2 * _lib.GRAM_MAX_BEAMS), dtype=torch.int32, device=G.DEV)
    rc = G.lib().gram_cross_attn_rows_long_split(G.p(q), G.p(bank.kb), G.p(bank.vt), G.p(m8), G.p(out), B, Q, bank.H, S, pieces, q[0].numel(),
                                                 bank.kb[0].numel(), G.p(bits), G.p(_scratch(G, B * 64, bank.H, S)), G.p(rowmap), G.stream())
    _lib.check(rc, "gram_cross_attn_rows_long_split")
    torch.cuda.synchronize()
    assert bool(_written(out).all())
    out = out.view(B, Q, -1)
    for r0 in range(0, Q, 64):
        kc = min(64, Q - r0)
        qg = q.view(pieces, B, Q, inner)[:, :, r0:r0 + kc].reshape(pieces, B * kc, inner).contiguous()
        grp = _launch(G, qg, bank, mask, kc).view(B, kc, -1)
        assert torch.equal(grp.view(torch.int16), out[:, r0:r0 + kc].contiguous().view(torch.int16)), r0


# ---- masked keys
@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("S", [4128, 12320])
def test_masked_keys_contribute_nothing(G, S, pieces):
    """NaN in every masked position of both banks (every piece): the same bits.  (The user without a valid key is left out: all its
    keys count.)"""
    B, K = 5, 20
    mask = _user_masks(S, B, 8)
    assert bool(mask.any(1).all())
    bank = _bank(G, B, S, pieces, seed=61)
    q = _queries(G, B * K, pieces, seed=62)
    clean = _launch(G, q, bank, mask, K)
    md = mask.to(G.DEV)
    nan = torch.full((), float("nan"), dtype=G.DT, device=G.DEV)
    bank.kb = torch.where(md[None, :, None, :, None], bank.kb, nan).contiguous()
    vt = G.vt_unblocked(bank.vt)  # [pieces][B][H][64][S]
    bank.vt = G.vt_blocked(torch.where(md[None, :, None, None, :], vt, nan)).contiguous()
    assert bool(torch.isnan(bank.kb.float()).any()) and bool(torch.isnan(bank.vt.float()).any())
    dirty = _launch(G, q, bank, mask, K)
    assert torch.equal(clean.view(torch.int16), dirty.view(torch.int16))
    assert not bool(torch.isnan(_value(G, dirty, pieces)).any())


# ---- the key bits
@pytest.mark.parametrize("S", [32, 4128, 16384])
def test_long_key_bits_against_a_python_packing(G, S):
    B = 6
    mask = _masks(S, torch.Generator().manual_seed(S + 1))
    mask[4] = False
    mask[4, 33 if S > 64 else 1] = True  # one bit in one word
    m8 = mask.to(G.DEV).view(torch.uint8).contiguous()
    bits = _bits(G, m8, B, S).cpu()
    w = (mask.view(B, S // 32, 32).long() << torch.arange(32)).sum(-1)  # bit j of word st = mask[32 st + j]
    w = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
    assert torch.equal(bits[:, : S // 32], w)
    assert not bool(bits[:, S // 32: WORDS].any()) and not bool(bits[:, WORDS + 1:].any())
    assert torch.equal(bits[:, WORDS].long(), (w != 0).sum(1))
    assert int(bits[5, WORDS]) == 0 and int(bits[0, WORDS]) == S // 32 and int(bits[4, WORDS]) == 1


# ------------------------------------------------------------------------------------------------------------ the KV-bank GEMM
@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("B,N,L,compact", [(3, 1, 16384, False), (2, 1, 4128, False), (12, 33, 128, True), (5, 21, 512, True)])
def test_kv_bank_epilogue_above_4096_keys(G, B, N, L, compact, pieces):
    L_ = G.lib()
    H, S = 4, N * L
    inner, d = H * 64, (128 if pieces == 2 else 256)
    g = torch.Generator().manual_seed(S + pieces)
    if compact:
        keep = torch.rand(B * N, generator=g) < 0.8
        keep[0] = keep[B * N - 1] = True
        pmap = torch.nonzero(keep).flatten().to(torch.int32)
        P = int(pmap.numel())
        if (P * L) % 256 == 0:  # an M tail
            pmap, P = pmap[:-1], P - 1
        M = P * L
    else:
        pmap, M = None, B * S
    a32 = torch.randn(M, d, generator=g).to(G.DEV)
    w32 = (torch.randn(2 * inner, d, generator=g) * d ** -0.5).to(G.DEV)
    A, W = (G.inter(a32), G.inter(w32)) if pieces == 2 else (G.bf(a32), G.bf(w32))
    a64, w64 = (a32.double(), w32.double()) if pieces == 2 else (A.double(), W.double())
    ref = (a64 @ w64.T).view(M, 2, H, 64)
    # where row m of A lives in the bank (the existing bank-epilogue tests' restatement)
    rows = torch.arange(M, device=G.DEV)
    if compact:
        flat = pmap.to(G.DEV).long()[rows // L]
        b_of, s_of = flat // N, (flat % N) * L + rows % L
    else:
        b_of, s_of = rows // S, rows % S
    n_bank, guard = B * H * S * 64, 4096
    res = {}
    sp = _lib.Split(pieces, 0, 0, n_bank + guard, 1.0)
    try:
        for v in (3, 22):
            L_.gram_debug_set_gemm_variant(v)
            k = torch.full((pieces, n_bank + guard), SENTINEL, dtype=torch.int16, device=G.DEV).view(G.DT)
            vt = torch.full((pieces, n_bank + guard), SENTINEL, dtype=torch.int16, device=G.DEV).view(G.DT)
            pm = pmap.to(G.DEV) if compact else None
            bank = _lib.KVBank(k.data_ptr(), vt.data_ptr(), 1, B, H, S, G.p(pm), N if compact else 0, L if compact else 0)
            _lib.check(L_.gram_gemm_bf16_split(G.p(A), G.p(W), None, M, 2 * inner, d, pieces * d, 2 * inner, _lib.EPI_KV_BANK, C.byref(bank), None,
                                               C.byref(sp), G.stream()), f"kv bank, variant {v}")
            torch.cuda.synchronize()
            res[v] = (k, vt)
    finally:
        L_.gram_debug_set_gemm_variant(-1)
    assert torch.equal(res[3][0].view(torch.int16), res[22][0].view(torch.int16)) and torch.equal(res[3][1].view(torch.int16), res[22][1].view(torch.int16))
    k, vt = res[22]
    assert bool((k[:, n_bank:].view(torch.int16) == SENTINEL).all()) and bool((vt[:, n_bank:].view(torch.int16) == SENTINEL).all())  # behind the bank
    kb = k[:, :n_bank].view(pieces, B, H, S, 64)
    vb = G.vt_unblocked(vt[:, :n_bank].view(pieces, B, H, S // 32, 64, 32))  # [pieces][B][H][64][S]
    # every position a row maps to is written, in every piece, and no other position is
    want = torch.zeros(B, S, dtype=torch.bool, device=G.DEV)
    want[b_of, s_of] = True
    assert int(want.sum()) == M  # (one row per position)
    assert torch.equal((kb.view(torch.int16) != SENTINEL).all(-1).all(0).all(1), want) and torch.equal((kb.view(torch.int16) != SENTINEL).any(-1).any(0).any(1), want)
    assert torch.equal((vb.view(torch.int16) != SENTINEL).all(0).all(1).all(1), want) and torch.equal((vb.view(torch.int16) != SENTINEL).any(0).any(1).any(1), want)
    got_k = kb.double().sum(0)[b_of, :, s_of]  # (M, H, 64)
    got_v = vb.double().sum(0).permute(0, 3, 1, 2)[b_of, s_of]  # (M, H, 64)
    if pieces == 2:
        ek, ev = relerr(got_k, ref[:, 0]), relerr(got_v, ref[:, 1])
        print(f"\n[kv bank B={B} N={N} L={L}] two pieces: K {ek:.2e}, V^T {ev:.2e} of rms")
        assert ek < tol(G) and ev < tol(G)  # tests/test_gpu_split.py::test_split_gemm_kv_bank_persistent
    else:  # tests/test_gpu_kernels.py::test_gemm_kv_bank
        assert torch.allclose(got_k, ref[:, 0], atol=2e-2, rtol=1e-2) and torch.allclose(got_v, ref[:, 1], atol=2e-2, rtol=1e-2)


def test_the_ping_pong_guard_on_a_device(G):
    """what tests/test_fused_len_host.py cannot tell apart without a device: with the ping-pong kernel forced, S = 16416 and M = 2^28
    come back GRAM_E_ARG (the pointers are never touched) -- and S = 16384 is taken (the test above)"""
    L_ = G.lib()
    FAKE = 0x1000
    try:
        L_.gram_debug_set_gemm_variant(22)
        for B, S in ((2, 16416), (1 << 14, 16384)):
            bank = _lib.KVBank(FAKE, FAKE, 1, B, 4, S, None, 0, 0)
            sp = _lib.Split(2, 0, 0, B * 4 * S * 64, 1.0)
            assert L_.gram_gemm_bf16_split(FAKE, FAKE, None, B * S, 512, 128, 256, 512, _lib.EPI_KV_BANK, C.byref(bank), None, C.byref(sp),
                                           G.stream()) == _lib.E_ARG
    finally:
        L_.gram_debug_set_gemm_variant(-1)


# ------------------------------------------------------------------------------------------------------------ the whole path
_MODELS = {}


def _oc(name):
    if name == "tiny":
        return O.OracleConfig(vocab_size=256, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2, max_item_num=31)
    return O.OracleConfig.named("t5-small", max_item_num=16)


def _model(gpu, name, mode):
    """a backbone with room for 32 (tiny) / 17 (small) passages, raised to 512-token passages and 16 384 fused tokens"""
    if (name, mode) not in _MODELS:
        oc, sd, m = TP._model(gpu, _oc(name), 11)
        m.set_precision(mode)
        m.set_max_passage_len(512)
        m.set_max_fused_tokens(16384)
        _MODELS[name, mode] = (oc, sd, m)
    return _MODELS[name, mode]


@functools.lru_cache(maxsize=None)
def _case(name, B, N, L):
    """inputs and oracle results of one (backbone, shape), computed once and shared (read only)"""
    oc = _oc(name)
    sd = O.init_state_dict(oc, 11)
    g = torch.Generator().manual_seed(B * 1000 + N * L)
    ids, mask = _inputs(g, B, N, L, min(oc.vocab_size, 32100))
    cands = _random_items(g, 30, 2, 3, 60)
    K = 4
    ref = O.generate(sd, oc, ids, mask, max(len(c) for c in cands), O.prefix_allowed_tokens_fn(O.Trie(cands)), K, K, 1.0)
    return types.SimpleNamespace(ids=ids, mask=mask, cands=cands, K=K, ref=ref, enc_ref=O.encode_fused(sd, oc, ids, mask), sd=sd)


WHOLE = [("tiny", 2, 21, 224), ("tiny", 2, 21, 512), ("tiny", 1, 32, 512), ("small", 2, 17, 256)]


@pytest.mark.parametrize("name,B,N,L", WHOLE)
def test_fused_encoder_vs_oracle(gpu, name, B, N, L):
    oc, sd, m = _model(gpu, name, TWO)
    c = _case(name, B, N, L)
    TP._check_encoder(m, c.ids, c.mask, c.enc_ref, f"{name} {B}x{N}x{L}")


@pytest.mark.parametrize("mode", [TWO, ONE])
@pytest.mark.parametrize("name,B,N,L", WHOLE)
def test_generate_vs_oracle(gpu, name, B, N, L, mode):
    """tests/test_gpu_long_passages.py's checks.  Two pieces: the oracle's top-K at SCORE_TOL with the near-tie rule.  One piece: Trie
    members whose scores are the teacher-forced decoder's scores of the same rows."""
    oc, sd, m = _model(gpu, name, mode)
    c = _case(name, B, N, L)
    out = _gen(m, c.ids, c.mask, c.cands, c.K)
    seqs, scores = out["sequences"].cpu(), out["sequences_scores"].cpu()
    assert seqs.shape[0] == B * c.K and bool(torch.isfinite(scores).all())
    if mode == TWO:
        assert seqs.shape[1] == c.ref["sequences"].shape[1]
        _check_generate(oc, sd, out, c.ref, c.ids, c.mask, c.cands, c.K, tol=SCORE_TOL)
    else:
        cand_set = {tuple(x) for x in c.cands}
        for r in seqs.tolist():
            while r and r[-1] == 0:
                r.pop()
            assert tuple(r) in cand_set, r
        audit = float((_rescored(m, c.ids, c.mask, seqs, c.K) - scores.double()).abs().max())
        print(f"[fused generate {name} {B}x{N}x{L} {mode}] max |score - teacher-forced score of the same row| {audit:.2e}")
        assert audit < _tol(mode)["logp"], audit


@pytest.mark.parametrize("mode", [TWO, ONE])
@pytest.mark.parametrize("name,B,N,L", WHOLE)
def test_score_sequences_vs_oracle_and_score_all_items(gpu, name, B, N, L, mode):
    from tests import tf_oracle as TF
    from tests.test_gpu_score_trie import _labels_of
    oc, sd, m = _model(gpu, name, mode)
    c = _case(name, B, N, L)
    lab1 = _labels_of(c.cands)  # every candidate as a label row: (C, T)
    Cn, T = lab1.shape
    lab = lab1[None].expand(B, -1, -1).contiguous()
    idd, mk = c.ids.to(DEV), c.mask.to(DEV)
    seq, tok = m.score_sequences(idd, mk, lab.to(DEV), return_tokens=True)
    few = 4  # (the oracle on four of the candidates)
    logits = TF.teacher_forced_logits(sd, oc, c.ids, c.mask, TF.shift_right(lab1[:few]).repeat(B, 1))
    _, ref_tok = TF.loss_and_token_logp(logits, lab1[:few].repeat(B, 1))
    dt = float((tok.cpu().view(B, Cn, T)[:, :few].double() - ref_tok.view(B, few, T)).abs().max())
    print(f"[fused score_sequences {name} {B}x{N}x{L} {mode}] token logp {dt:.2e}")
    assert dt < _tol(mode)["logp"], dt
    one = m.score_all_items(idd, mk, _fn(c.cands), c.cands)
    assert torch.equal(one, seq.view(B, Cn))


def test_generate_with_exclude_items_vs_oracle(gpu):
    oc, sd, m = _model(gpu, "tiny", TWO)
    c = _case("tiny", 2, 21, 224)
    n = len(c.cands)
    g = torch.Generator().manual_seed(3)
    lists = [torch.randperm(n, generator=g)[:k].tolist() for k in (10, n - 2 * c.K)]
    keep = [sorted(set(range(n)) - set(r)) for r in lists]
    fns = [O.prefix_allowed_tokens_fn(O.Trie([c.cands[i] for i in kp])) for kp in keep]
    max_length = max(len(x) for x in c.cands)
    ref = O.generate(sd, oc, c.ids, c.mask, max_length, lambda b, sent: fns[b](b, sent), c.K, c.K, 1.0)
    out = m.generate(input_ids=c.ids.to(DEV), attention_mask=c.mask.to(DEV), max_length=max_length, prefix_allowed_tokens_fn=_fn(c.cands),
                     num_beams=c.K, num_return_sequences=c.K, output_scores=True, return_dict_in_generate=True, length_penalty=1.0,
                     exclude_items=lists, candidates=c.cands)
    _check_generate(oc, sd, out, ref, c.ids, c.mask, c.cands, c.K, tol=SCORE_TOL)


# ---- bit for bit on the raised model
@functools.lru_cache(maxsize=None)
def _users(B, N, L, seed=21):
    g = torch.Generator().manual_seed(seed)
    ids, mask = _inputs(g, B, N, L, 250)
    return ids, mask, _random_items(g, 30, 2, 3, 60), _labels(g, (B, 2, 5), 250)


@pytest.mark.parametrize("mode", [TWO, ONE])
def test_a_batch_of_four_and_each_user_alone(gpu, mode):
    m = _model(gpu, "tiny", mode)[2]
    ids, mask, cands, lab = _users(4, 21, 224)
    seqs, scores, tok = _run(m, ids, mask, cands, lab)
    for u in range(4):
        s1, v1, t1 = _run(m, ids[u:u + 1], mask[u:u + 1], cands, lab[u:u + 1])
        w = min(s1.shape[1], seqs.shape[1])  # (a user alone may return fewer columns: the batch's width is its longest hypothesis)
        assert torch.equal(s1[:, :w], seqs[u * 4:(u + 1) * 4, :w]) and not bool(s1[:, w:].any()) and not bool(seqs[u * 4:(u + 1) * 4, w:].any())
        assert torch.equal(v1, scores[u * 4:(u + 1) * 4]) and torch.equal(t1[0], tok[u]), u


@pytest.mark.parametrize("mode", [TWO, ONE])
def test_a_batch_at_9_by_480_and_the_same_users_padded_to_21_by_512(gpu, mode):
    """4320 fused tokens against 10 752: the keys move across 4096 and 8192, twelve masked passages follow"""
    m = _model(gpu, "tiny", mode)[2]
    ids, mask, cands, lab = _users(3, 9, 480)
    a = _run(m, ids, mask, cands, lab)
    pad = (0, 32, 0, 12)
    b = _run(m, torch.nn.functional.pad(ids, pad), torch.nn.functional.pad(mask, pad), cands, lab)
    assert _same(a, b)


@pytest.mark.parametrize("mode", [TWO, ONE])
def test_cold_model_and_warm_passage_cache(gpu, mode):
    m = _model(gpu, "tiny", mode)[2]
    ids, mask, cands, lab = _users(2, 21, 224)
    m.clear_passage_cache()
    cold = _run(m, ids, mask, cands, lab)
    try:
        m.set_passage_harvest(True)
        first = _run(m, ids, mask, cands, lab)
        assert m._pcache is not None and m._pcache["n"] > 0
        warm = _run(m, ids, mask, cands, lab)
    finally:
        m.set_passage_harvest(False)
        m.clear_passage_cache()
    assert _same(cold, first) and _same(cold, warm)


@pytest.mark.parametrize("mode", [TWO, ONE])
@pytest.mark.parametrize("hook", ["gram_debug_set_token_tables", "gram_debug_set_live_rows"])
def test_token_tables_and_live_rows_on_and_off(gpu, mode, hook):
    m = _model(gpu, "tiny", mode)[2]
    ids, mask, cands, lab = _users(2, 21, 224)
    fn = getattr(_lib.load(), hook)
    try:
        fn(1)
        on = _run(m, ids, mask, cands, lab)
        fn(0)
        off = _run(m, ids, mask, cands, lab)
    finally:
        fn(-1)
    assert _same(on, off)


# ---- a default model
def test_a_default_model_names_the_way_out_and_computes_what_it_did(gpu):
    oc, sd, m = TP._model(gpu, _oc("tiny"), 11)
    m.set_max_passage_len(256)
    ids, mask, cands, lab = _users(2, 21, 224)
    for call in (lambda: _gen(m, ids, mask, cands, 4), lambda: m.score_sequences(ids.to(DEV), mask.to(DEV), lab.to(DEV)),
                 lambda: m.score_all_items(ids.to(DEV), mask.to(DEV), _fn(cands), cands)):
        with pytest.raises(ValueError, match=r"set_max_fused_tokens\(4704\) first"):
            call()
    handle = m._pack()
    assert _lib.load().gram_workspace_bytes(handle, 2, 21, 224, 4, 6) == _lib.E_ARG
    # (2, 3, 128): what tests/test_gpu_path.py checks of a default model -- and the raised model's own bits differ only by rounding
    oc5, sd5, m5 = TP._model(gpu, "tiny", 11)
    g = torch.Generator().manual_seed(2128)
    ids3, mask3 = _inputs(g, 2, 3, 128, 250)
    cands3 = _random_items(g, 30, 2, 3, 60)
    ref = O.generate(sd5, oc5, ids3, mask3, max(len(x) for x in cands3), O.prefix_allowed_tokens_fn(O.Trie(cands3)), 4, 4, 1.0)
    out = _gen(m5, ids3, mask3, cands3, 4)
    _check_generate(oc5, sd5, out, ref, ids3, mask3, cands3, 4, tol=SCORE_TOL)
    m.set_max_fused_tokens(4704)
    assert _lib.load().gram_workspace_bytes(handle, 2, 21, 224, 4, 6) > 0  # (forwarded to the live handle)
    assert bool(torch.isfinite(_gen(m, ids, mask, cands, 4)["sequences_scores"]).all())
    with pytest.raises(ValueError, match="limited to 4096 fused tokens"):
        m.cross_attentions(ids.to(DEV), mask.to(DEV), decoder_input_ids=torch.zeros(2, 1, dtype=torch.long))


def test_attention_probabilities_below_4096_keys_on_a_raised_model(gpu):
    """A raised handle carves the long form's key bits, so the probabilities kernel packs its own from the mask: layer 0's are the
    default model's bit for bit (the same queries and bank), the later layers' differ by the cross-attention's rounding only."""
    ids, mask, _c, _l = _users(2, 3, 128, seed=23)
    dec = torch.zeros(2, 1, dtype=torch.long)
    res = []
    for raise_it in (False, True):
        _oc_, _sd, m = TP._model(gpu, _oc("tiny"), 11)
        m.set_precision(TWO)
        if raise_it:
            m.set_max_fused_tokens(8192)
        res.append(m.cross_attentions(ids.to(DEV), mask.to(DEV), decoder_input_ids=dec.to(DEV)))
    assert len(res[0]) == len(res[1]) == 2 and torch.equal(res[0][0], res[1][0])
    d = float((res[0][1].double() - res[1][1].double()).abs().max())
    print(f"[probabilities, raised vs default] layer 1: max |d| {d:.2e}")
    # (two models that differ by two-piece rounding: the whole path's own two-piece tolerance, on values <= 1)
    assert 0 < float(res[1][1].max()) <= 1 + 1e-6 and d < SCORE_TOL


def test_the_custom_op_and_its_validation(G):
    import gram_amd.ops  # noqa: F401
    B, K, S = 2, 20, 8224
    mask = _user_masks(S, B, 9)
    bank = _bank(G, B, S, 1, seed=71)
    q = _queries(G, B * K, 1, seed=72)
    m8 = mask.to(G.DEV).view(torch.uint8).contiguous()
    out = torch.ops.gram.cross_attn_long(q[0], bank.kb[0], bank.vt[0], m8, K)
    assert torch.equal(out.view(torch.int16), _launch(G, q, bank, mask, K).view(torch.int16))
    for args in ((q[0], bank.kb[0], bank.vt[0], m8, 65), (q[0], bank.kb[0], bank.vt[0], m8[:, :S - 32].contiguous(), K),
                 (q[0].float(), bank.kb[0], bank.vt[0], m8, K), (q[0][:-1], bank.kb[0], bank.vt[0], m8, K)):
        with pytest.raises((ValueError, RuntimeError)):
            torch.ops.gram.cross_attn_long(*args)
