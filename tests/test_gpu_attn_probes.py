"""Probes of the four attention kernels (enc_attn.hip, dec_attn.hip, tf_attn.hip): every (query, key) softmax weight, every slot of
the relative bias table and every mask bit is observed on its own.

The other kernel tests feed `randn` operands and T5's bucketed bias table.  A softmax over scores of std ~8 is carried by a few keys
and neighbouring slots of a bucketed table hold the same value beyond distance ~16, so an error that touches ONE key, ONE bias slot
or ONE mask bit stays under their tolerances.  A probe is built so that the kernel's output IS the weight matrix:

  * q is one-hot in dimension 0 of a head times a per-row factor (a multiple of 1/8; zero for the heads h % 3 == 0 of the
    self-attention kernels, where the bias alone decides), K holds a distinct multiple of 2^-7 in [-2, 2) per key in dimension 0 and
    zeros elsewhere: every product is exact in either 16-bit format and in either piece mode;
  * the bias table is raw: a seeded permutation of linspace(-2, 2, n) per head, all slots distinct;
  * v[key] = e_(key mod 64): output dimension d of the instance that serves keys 64 g .. 64 g + 63 (a passage of the encoder, a user of
    the cross-attention -- all instances in ONE launch) is the weight of key 64 g + d.

The reference is softmax(score + bias + (1 - m) * finfo(float32).min) in fp64.  Masked keys of a row that has a valid key, and the
causally excluded positions, must come back as exactly 0.0; every other weight within a relative bound that follows from the format:

  * one piece: P = exp(s - max) is rounded once and the output once, each to 2^-11 relative on IEEE half (normal numbers: every
    expected weight is asserted >= 2^-13 on the reference alone, and P >= the weight) -> rtol = 4 * 2^-11, twice the two roundings.
    Only in the IEEE-half build: bfloat16's 2^-8 cannot resolve bias values 4/254 apart with margin.
  * two pieces: the design error of tests/test_gpu_split.py, 10 * tol(G).  On IEEE half the low piece of a value below 2^-3 is
    subnormal (quantum 2^-24), an absolute error of up to 2^-25 per output; the probes keep every expected weight >= 3 * 2^-25 / 2e-4
    = 4.5e-4 (asserted on the reference), so that this floor is at most a third of the bound.  (The uniform 2^-12 of a bank of 4096
    masked keys is below that, but a 16-bit number itself: its low piece is zero.)

The unmarked test at the end needs no GPU: it applies one index error at a time to the fp64 weights and asserts that the comparator
used above rejects each of them."""
import numpy as np
import pytest
import torch

from gram_amd import _lib

FMIN = float(torch.finfo(torch.float32).min)
EPS16 = 2.0 ** -11            # unit roundoff of IEEE half
FLOOR = 2.0 ** -13            # every expected non-zero weight is at least this: a normal number in IEEE half
FLOOR2 = 3 * 2.0 ** -25 / 2e-4  # ... and this in a two-piece probe (see above)
RTOL1 = 4 * EPS16
DEC_LEN = _lib.GRAM_MAX_DEC_LEN
MASK_BYTES = np.array([1, 2, 255], dtype=np.uint8)  # "valid" is != 0, not == 1


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    return gpu_util


# ------------------------------------------------------------------------------------------------ host side: inputs and references
def softmax_ref(score, valid):
    """softmax over the last axis of score + (1 - valid) * finfo(float32).min in fp64: exact zeros for the masked keys of a row that
    has a valid key, the uniform row for one that has none (the scores drown in finfo.min, as they do in the fp32 reference)"""
    s = score + (1.0 - np.asarray(valid, dtype=np.float64)) * FMIN
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def compare(W, ref, rtol):
    """The probes' comparator -> (accepted, largest relative error of an expected non-zero weight).  Expected zeros must be 0.0."""
    W, ref = np.asarray(W, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert W.shape == ref.shape, (W.shape, ref.shape)
    nz = ref != 0
    rel = np.abs(W[nz] - ref[nz]) / ref[nz]
    worst = float(rel.max()) if rel.size else 0.0
    return bool((W[~nz] == 0).all() and np.isfinite(W).all() and worst <= rtol), worst


def precondition(ref, pieces=2):
    """A condition on the inputs, not a measurement: checked on the fp64 reference alone."""
    wmin = float(ref[ref != 0].min())
    assert wmin >= FLOOR, wmin
    if pieces == 2:
        assert wmin >= FLOOR2, wmin
    return wmin


def grid_values(rng, n):
    """n distinct multiples of 2^-7 in [-2, 2), in a seeded random order (n <= 512)"""
    return (rng.permutation(512)[:n] - 256) / 128.0


def raw_bias(rng, H, n):
    """[H][n] fp32: per head a permutation of linspace(-2, 2, n) -- no two slots of a head alike"""
    return np.stack([rng.permutation(np.linspace(-2.0, 2.0, n)) for _ in range(H)]).astype(np.float32)


def factors(rng, shape, choices, H_axis=None):
    f = rng.choice(np.asarray(choices, dtype=np.float64), size=shape)
    if H_axis is not None:  # heads h % 3 == 0: q = 0, the bias alone decides
        idx = [slice(None)] * len(shape)
        idx[H_axis] = slice(0, None, 3)
        f[tuple(idx)] = 0.0
    return f


def mask_bytes(rng, valid):
    """0 where masked, a byte from {1, 2, 255} where valid"""
    return np.where(valid, rng.choice(MASK_BYTES, size=valid.shape), 0).astype(np.uint8)


# ---- encoder
ENC_MASKS = ("all valid", "padded tail", "hole", "fully padded")


def enc_probe(L, H):
    rng = np.random.default_rng(1000 * L + H)
    M = len(ENC_MASKS)
    valid = np.ones((M, L), dtype=bool)
    valid[1, L - 13:] = False                 # 13 padded keys: not a multiple of 4
    valid[2, L // 2 - 5: L // 2 + 6] = False  # 11 keys in the middle
    valid[3] = False
    # (row factors: with 96+ keys the bias alone already spreads the weights down to 6e-4 -- 1 / (L e^2 mean(e^bias)))
    choices = (-0.25, -0.125, 0.125, 0.25) if L <= 64 else (-0.0625, -0.03125, 0.03125, 0.0625)
    p = dict(L=L, H=H, qf=factors(rng, (M, L, H), choices, H_axis=2),
             kv=np.stack([[grid_values(rng, L) for _ in range(H)] for _ in range(M)]), bias=raw_bias(rng, H, 255),
             mask=mask_bytes(rng, valid))
    p["ref"] = enc_weights(p)
    return p


def enc_weights(p, slot=lambda i: i, mask=None, kv=None):
    """[M][H][query][key]; slot maps the bias index key - query + 127 (the identity in the reference)"""
    L = p["L"]
    kv = p["kv"] if kv is None else kv
    mask = p["mask"] if mask is None else mask
    idx = slot(np.arange(L)[None, :] - np.arange(L)[:, None] + 127)
    score = p["qf"].transpose(0, 2, 1)[..., None] * kv[:, :, None, :] + p["bias"].astype(np.float64)[:, idx][None]
    return softmax_ref(score, (mask != 0)[:, None, None, :])


# ---- cross-attention
def xattn_valid(S, kind, rng):
    """The key mask of a cross-attention probe (shared by the users of the launch).  kind 0: runs of fully masked 32-key steps at the
    front, in the middle and at the end; between them fully valid steps, steps with a single valid key (the first or the last bit of
    the word) and sparse ones, an ODD number of valid steps, so that the two waves are dealt different numbers.  kind 1: every
    valid step at index >= 64 (the second word of the step ballot) where the bank has such steps.  At most 512 valid keys."""
    n = S // 32
    v = np.zeros((n, 32), dtype=bool)
    if n == 1:
        v[0] = rng.random(32) < 0.6
        v[0, 0], v[0, 31] = kind == 1, kind == 0
    elif n == 3:
        if kind == 0:
            v[0], v[2, 31] = True, True
        else:
            v[1, 0], v[2] = True, rng.random(32) < 0.5
    else:
        steps = np.arange(64, n) if (kind == 1 and n > 64) else np.arange(n)
        if steps.size == 1:
            v[steps[0]] = rng.random(32) < 0.6
        else:
            m = steps.size
            keep = np.ones(m, dtype=bool)
            keep[: m // 16 + 1] = False
            keep[m // 2 - m // 8: m // 2 + m // 8] = False
            keep[m - 3:] = False
            cand = rng.permutation(steps[keep])
            cand = cand[:29]  # 8 full + 5 first-bit + 5 last-bit + 11 sparse: 29 valid steps, <= 256 + 10 + 11 * 9 keys
            v[cand[:8]] = True
            v[cand[8:13], 0] = True
            v[cand[13:18], 31] = True
            for s in cand[18:]:
                v[s, rng.permutation(32)[: int(rng.integers(2, 10))]] = True
            assert int(v.any(1).sum()) % 2 == 1
    v = v.reshape(S)
    assert 1 <= int(v.sum()) <= 512
    return v


def xattn_probe(K, S, H=2, all_masked=False):
    rng = np.random.default_rng(100000 + 100 * S + K)
    valid = np.zeros(S, dtype=bool) if all_masked else xattn_valid(S, int(K in (16, 48)), rng)
    kv = np.empty((H, S))
    for h in range(H):  # distinct values on the valid keys; the masked ones repeat values of the same grid
        kv[h] = (rng.integers(0, 512, S) - 256) / 128.0
        if not all_masked:
            kv[h, valid] = grid_values(rng, int(valid.sum()))
    choices = (-1, -0.75, -0.5, -0.25, 0.25, 0.5, 0.75, 1) if S <= 96 else (-0.5, -0.375, -0.25, -0.125, 0.125, 0.25, 0.375, 0.5)
    p = dict(K=K, S=S, H=H, qf=factors(rng, (K, H), choices), kv=kv, mask=mask_bytes(rng, valid))
    p["ref"] = xattn_weights(p)
    return p


def xattn_weights(p, mask=None, kv=None):
    """[H][beam][key]"""
    kv = p["kv"] if kv is None else kv
    mask = p["mask"] if mask is None else mask
    return softmax_ref(p["qf"].T[:, :, None] * kv[:, None, :], (mask != 0)[None, None, :])


# ---- decoder step
def dec_probe(H, R=12, Tmax=DEC_LEN):
    rng = np.random.default_rng(7000 + H)
    # K of (position, row, head): rows of one position are at least 1/8 apart, so that a wrong ancestor row moves the score
    coarse = np.stack([[rng.permutation(16)[:R] for _ in range(H)] for _ in range(Tmax)]).transpose(0, 2, 1)  # [Tmax][R][H]
    kv = coarse / 4.0 - 2.0 + rng.integers(0, 16, (Tmax, R, H)) / 128.0
    p = dict(H=H, R=R, Tmax=Tmax, qf=factors(rng, (Tmax, R, H), (-0.25, -0.125, 0.125, 0.25), H_axis=2), kv=kv,
             bias=raw_bias(rng, H, DEC_LEN), parents=rng.integers(0, R, (Tmax, R)))
    p["ref"] = dec_weights(p)
    return p


def dec_weights(p, slot=lambda d: d, wrong=None):
    """[t][R][H][64]: the weights of step t over positions 0..t (zeros behind), the history reordered by parents[t] after every step
    as the reference index_selects its cache.  wrong = (t, row, position): that row reads the K of its ancestor's neighbour there."""
    H, R, Tmax = p["H"], p["R"], p["Tmax"]
    bias = p["bias"].astype(np.float64)
    hist = np.zeros((R, H, 0))
    src = np.zeros((R, 0), dtype=np.int64)  # the row that wrote the entry: what the kernel's ancestor table holds
    W = np.zeros((Tmax, R, H, DEC_LEN))
    for t in range(Tmax):
        hist = np.concatenate([hist, p["kv"][t][:, :, None]], axis=2)
        src = np.concatenate([src, np.arange(R)[:, None]], axis=1)
        k = hist
        if wrong is not None and wrong[0] == t:
            _, r0, j0 = wrong
            k = hist.copy()
            k[r0, :, j0] = p["kv"][j0][(src[r0, j0] + 1) % R]
        score = p["qf"][t][:, :, None] * k + bias[:, slot(t - np.arange(t + 1))][None]
        W[t, :, :, : t + 1] = softmax_ref(score, np.ones(t + 1, dtype=bool))
        hist, src = hist[p["parents"][t]], src[p["parents"][t]]
    return W


# ---- teacher-forced self-attention
def tf_probe(T, H=3, n_seq=5):
    rng = np.random.default_rng(9000 + T)
    p = dict(T=T, H=H, n_seq=n_seq, qf=factors(rng, (n_seq, T, H), (-0.25, -0.125, 0.125, 0.25), H_axis=2),
             kv=np.stack([[grid_values(rng, T) for _ in range(H)] for _ in range(n_seq)]), bias=raw_bias(rng, H, DEC_LEN))
    p["ref"] = tf_weights(p)
    return p


def tf_weights(p, slot=lambda d: d, limit=lambda t: t):
    """[n_seq][H][t][j]: query t over positions j <= limit(t) (the causal limit: t)"""
    T = p["T"]
    t, j = np.arange(T)[:, None], np.arange(T)[None, :]
    score = p["qf"].transpose(0, 2, 1)[..., None] * p["kv"][:, :, None, :] + p["bias"].astype(np.float64)[:, slot(np.abs(t - j))][None]
    return softmax_ref(score, (j <= np.minimum(limit(t), T - 1))[None, None])


ENC_CASES = [(32, 3), (64, 3), (96, 3), (128, 3), (128, 16)]
XATTN_K = [1, 16, 17, 33, 48, 49, 64]
XATTN_S = [32, 96, 2048, 2080, 4096]
TF_T = [1, 33, 64]


# ------------------------------------------------------------------------------------------------ device side
def _rtol(G, pieces):
    if pieces == 1 and not G.F16:
        pytest.skip("one-piece probes need IEEE half: bfloat16's 2^-8 cannot resolve bias values 4/254 apart with margin")
    if pieces == 1:
        return RTOL1
    from tests.test_gpu_split import tol
    return 10 * tol(G)


def _dev(G, a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(G.DEV, dtype)


def _pieces(G, x32, pieces):
    """[pieces][...] planar pieces of exactly representable values: the value and a zero remainder"""
    x = G.pieces_of(x32, pieces)
    assert torch.equal(x[0].float(), x32)
    return x


def _out64(G, out, pieces):
    return (G.join_inter(out) if pieces == 2 else out.double()).cpu().numpy()


def _report(name, what, pieces, ok, worst, rtol, wmin):
    print(f"\n[probe {name}] {what} pieces={pieces}: max relative weight error {worst:.2e} (bound {rtol:.2e}), smallest weight {wmin:.2e}")
    assert ok, (name, what, pieces, worst, rtol)


@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("L,H", ENC_CASES)
def test_probe_enc_self_attn(G, L, H, pieces):
    """gram_enc_self_attn_split: all four templates x both piece modes; passages (mask kind, group of 64 keys) in one launch."""
    rtol = _rtol(G, pieces)
    p = enc_probe(L, H)
    wmin = precondition(p["ref"], pieces)
    M, NG, inner = len(ENC_MASKS), (L + 63) // 64, H * 64
    P = M * NG
    x = torch.zeros(M, NG, L, 3, H, 64)
    x[:, :, :, 0, :, 0] = torch.from_numpy(p["qf"]).float()[:, None]
    x[:, :, :, 1, :, 0] = torch.from_numpy(p["kv"]).float().transpose(1, 2)[:, None]
    key = torch.arange(L)
    x[:, key // 64, key, 2, :, key % 64] = 1.0
    qkv = _pieces(G, x.view(P * L, 3 * inner).to(G.DEV), pieces)
    m8 = _dev(G, np.repeat(p["mask"], NG, axis=0), torch.uint8)
    bias = _dev(G, p["bias"])
    out = torch.full((P * L, pieces * inner), float("nan"), dtype=G.DT, device=G.DEV)
    _lib.check(G.lib().gram_enc_self_attn_split(G.p(qkv), G.p(bias), G.p(m8), G.p(out), P, L, H, pieces, qkv[0].numel(),
                                                G.stream()), "enc_attn")
    W = _out64(G, out, pieces).reshape(M, NG, L, H, 64).transpose(0, 3, 2, 1, 4).reshape(M, H, L, NG * 64)
    ref = np.zeros_like(W)
    ref[..., :L] = p["ref"]
    ok, worst = compare(W, ref, rtol)
    _report("enc", f"L={L} H={H}", pieces, ok, worst, rtol, wmin)


def _xattn_device(G, p, pieces):
    """q [pieces][B*K][inner], K bank, blocked V^T bank, mask [B][S], B = one user per group of 64 keys (same q, K and mask)"""
    K, S, H = p["K"], p["S"], p["H"]
    B, inner = (S + 63) // 64, H * 64
    q = torch.zeros(B, K, H, 64, device=G.DEV)
    q[..., 0] = _dev(G, p["qf"])[None]
    kb = torch.zeros(pieces, B, H, S, 64, dtype=G.DT, device=G.DEV)
    kb[0, :, :, :, 0] = _dev(G, p["kv"]).to(G.DT)[None]
    assert torch.equal(kb[0, 0, :, :, 0].double().cpu(), torch.from_numpy(p["kv"]))
    key = torch.arange(S, device=G.DEV)
    vt = torch.zeros(pieces, B, H, S // 32, 64, 32, dtype=G.DT, device=G.DEV)  # v[b][h][key] = e_(key % 64) for key // 64 == b
    vt[0, key // 64, :, key // 32, key % 64, key % 32] = 1.0
    m8 = _dev(G, np.tile(p["mask"], (B, 1)), torch.uint8)
    return _pieces(G, q.view(B * K, inner), pieces), kb, vt, m8, B


def _xattn_run(G, p, pieces, q, kb, vt, m8, n_users, users=None, rowpos=None, key_bits=None, rows=None):
    rows = n_users * p["K"] if rows is None else rows
    out = torch.full((rows, pieces * p["H"] * 64), float("nan"), dtype=G.DT, device=G.DEV)
    _lib.check(G.lib().gram_cross_attn_decode_split(G.p(q), G.p(kb), G.p(vt), G.p(m8), G.p(out), n_users, p["K"], p["H"], p["S"],
                                                    G.p(users), G.p(rowpos), pieces, q[0].numel(), kb[0].numel(), G.p(key_bits),
                                                    G.stream()), "xattn")
    return out


def _key_bits(G, m8, S):
    bits = torch.full((m8.shape[0], 128), -1, dtype=torch.int32, device=G.DEV)
    _lib.check(G.lib().gram_mask_key_bits(G.p(m8), G.p(bits), m8.shape[0], S, G.stream()), "bits")
    return bits


def _xattn_W(G, out, p, pieces, B):
    """[B*K][pieces * inner] -> [H][beam][B * 64]"""
    return _out64(G, out, pieces).reshape(B, p["K"], p["H"], 64).transpose(2, 1, 0, 3).reshape(p["H"], p["K"], B * 64)


def _xattn_live(G, p, pieces, q, kb, vt, m8, B, bits, out_all, seed):
    """the live-row form on a rowpos with -1 holes (one user without a live row when there are several): the all-rows bits"""
    K = p["K"]
    rng = np.random.default_rng(seed)
    live = rng.random((B, K)) < 0.6
    live[0, 0], live[0, K - 1] = True, False
    if B > 1:
        live[B // 2] = False
    rows = np.nonzero(live.reshape(-1))[0]
    rowpos = np.full(B * K, -1, dtype=np.int32)
    rowpos[rows] = np.arange(rows.size, dtype=np.int32)
    users = np.nonzero(live.any(1))[0].astype(np.int32)
    rows_d = _dev(G, rows, torch.int64)
    out = _xattn_run(G, p, pieces, q[:, rows_d].contiguous(), kb, vt, m8, users.size, _dev(G, users, torch.int32),
                     _dev(G, rowpos, torch.int32), bits, rows=rows.size)
    assert torch.equal(out.view(torch.int16), out_all[rows_d].view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("S", XATTN_S)
@pytest.mark.parametrize("K", XATTN_K)
def test_probe_cross_attn(G, K, S, pieces):
    """gram_cross_attn_decode_split: every beam-tile count, the two-wave and the one-wave kernel, short and long banks with skipped
    steps; key_bits NULL and precomputed give the same bits; K = 17 and 49 also through the live-row form."""
    rtol = _rtol(G, pieces)
    p = xattn_probe(K, S)
    wmin = precondition(p["ref"], pieces)
    q, kb, vt, m8, B = _xattn_device(G, p, pieces)
    out = _xattn_run(G, p, pieces, q, kb, vt, m8, B)
    bits = _key_bits(G, m8, S)
    assert torch.equal(out.view(torch.int16), _xattn_run(G, p, pieces, q, kb, vt, m8, B, key_bits=bits).view(torch.int16))
    if K in (17, 49):
        _xattn_live(G, p, pieces, q, kb, vt, m8, B, bits if S % 64 else None, out, K + S)
    W = _xattn_W(G, out, p, pieces, B)
    ref = np.zeros_like(W)
    ref[..., :S] = p["ref"]
    ok, worst = compare(W, ref, rtol)
    _report("cross", f"K={K} S={S} valid keys={int((p['mask'] != 0).sum())}", pieces, ok, worst, rtol, wmin)


@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("K", [4, 40])
@pytest.mark.parametrize("S", [64, 2048, 2080, 4096])
def test_probe_cross_attn_all_masked(G, S, K, pieces):
    """Users without a valid key keep every step (the step ballot rebuilt for nsteps = 2, 64, 65, 128): uniform weights 1/S, from the
    mask bytes and from precomputed key bits, two waves (K = 4) and one (K = 40); (S, K) = (2080, 40) also through the live form."""
    rtol = _rtol(G, pieces)
    p = xattn_probe(K, S, all_masked=True)
    assert np.allclose(p["ref"], 1.0 / S, rtol=1e-15, atol=0)
    wmin = precondition(p["ref"], 1)
    assert 1.0 / S >= FLOOR2 or S == 4096  # (2^-12 is a 16-bit number: its low piece is zero)
    q, kb, vt, m8, B = _xattn_device(G, p, pieces)
    bits = _key_bits(G, m8, S)
    assert not bool(bits[:, : S // 32].any())
    outs = [_xattn_run(G, p, pieces, q, kb, vt, m8, B), _xattn_run(G, p, pieces, q, kb, vt, m8, B, key_bits=bits)]
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    if (S, K) == (2080, 40):
        _xattn_live(G, p, pieces, q, kb, vt, m8, B, None, outs[0], S)
        _xattn_live(G, p, pieces, q, kb, vt, m8, B, bits, outs[0], S + 1)
    W = _xattn_W(G, outs[0], p, pieces, B)
    ref = np.zeros_like(W)
    ref[..., :S] = 1.0 / S
    ok, worst = compare(W, ref, rtol)
    _report("cross, no valid key", f"K={K} S={S}", pieces, ok, worst, rtol, wmin)


def _anc_advance(anc, t, parent):
    """the ancestor table after step t's beam reorder, as tests/test_gpu_kernels.py::test_dec_self_attn advances it"""
    new = anc.clone()
    new[:t, :] = anc[:t, parent]
    new[t, :] = parent.int()
    return new


@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("H", [3, 16])
def test_probe_dec_self_attn(G, H, pieces):
    """gram_dec_self_attn_split at every step t = 0..63 under a random ancestor table: the weights over positions 0..t (K differs
    by row and position, V is one-hot by position), zeros behind t, and slot t of both caches = this step's k and v bit for bit."""
    rtol = _rtol(G, pieces)
    p = dec_probe(H)
    wmin = precondition(p["ref"], pieces)
    R, Tmax, inner = p["R"], p["Tmax"], H * 64
    kc = torch.zeros(pieces, Tmax, R, inner, dtype=G.DT, device=G.DEV)
    vc = torch.zeros_like(kc)
    bias = _dev(G, p["bias"])
    anc = torch.arange(R, dtype=torch.int32).repeat(Tmax, 1)
    outs = []
    for t in range(Tmax):
        x = torch.zeros(R, 3, H, 64)
        x[:, 0, :, 0] = torch.from_numpy(p["qf"][t]).float()
        x[:, 1, :, 0] = torch.from_numpy(p["kv"][t]).float()
        x[:, 2, :, t] = 1.0
        qkv = _pieces(G, x.view(R, 3 * inner).to(G.DEV), pieces)
        out = torch.full((R, pieces * inner), float("nan"), dtype=G.DT, device=G.DEV)
        anc_d = anc.to(G.DEV)
        _lib.check(G.lib().gram_dec_self_attn_split(G.p(qkv), G.p(kc), G.p(vc), G.p(anc_d), G.p(bias), G.p(out), R, R, None, H, t,
                                                    Tmax, pieces, qkv[0].numel(), kc[0].numel(), G.stream()), "dec_attn")
        outs.append(out)
        assert torch.equal(kc[:, t].view(torch.int16), qkv[:, :, inner: 2 * inner].view(torch.int16)), t
        assert torch.equal(vc[:, t].view(torch.int16), qkv[:, :, 2 * inner:].view(torch.int16)), t
        anc = _anc_advance(anc, t, torch.from_numpy(p["parents"][t]))
    W = _out64(G, torch.cat(outs), pieces).reshape(Tmax, R, H, 64)
    worst = 0.0
    for t in range(Tmax):
        ok, e = compare(W[t], p["ref"][t], rtol)
        assert ok, (t, e, rtol)
        worst = max(worst, e)
    _report("dec step", f"H={H} t=0..{Tmax - 1}", pieces, True, worst, rtol, wmin)


@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("T", TF_T)
def test_probe_dec_self_attn_tf(G, T, pieces):
    """gram_dec_self_attn_tf_split: every (query, position) weight of n_seq sequences, exact zeros behind the causal limit."""
    rtol = _rtol(G, pieces)
    p = tf_probe(T)
    wmin = precondition(p["ref"], pieces)
    H, n_seq = p["H"], p["n_seq"]
    inner = H * 64
    x = torch.zeros(n_seq, T, 3, H, 64)
    x[:, :, 0, :, 0] = torch.from_numpy(p["qf"]).float()
    x[:, :, 1, :, 0] = torch.from_numpy(p["kv"]).float().transpose(1, 2)
    x[:, torch.arange(T), 2, :, torch.arange(T)] = 1.0
    qkv = _pieces(G, x.view(n_seq * T, 3 * inner).to(G.DEV), pieces)
    bias = _dev(G, p["bias"])
    out = torch.full((n_seq * T, pieces * inner), float("nan"), dtype=G.DT, device=G.DEV)
    _lib.check(G.lib().gram_dec_self_attn_tf_split(G.p(qkv), G.p(bias), G.p(out), n_seq, T, H, pieces, qkv[0].numel(),
                                                   G.stream()), "tf_attn")
    W = _out64(G, out, pieces).reshape(n_seq, T, H, 64).transpose(0, 2, 1, 3)
    ref = np.zeros_like(W)
    ref[..., :T] = p["ref"]
    ok, worst = compare(W, ref, rtol)
    _report("teacher-forced", f"T={T}", pieces, ok, worst, rtol, wmin)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [32, 2080, 4096])
def test_mask_key_bits_words(G, S):
    """gram_mask_key_bits: word st < S/32 of user b = the little-endian packing of mask[b][32 st ..] != 0, bytes from {0, 1, 2, 255}."""
    B = 3
    rng = np.random.default_rng(S)
    mask = rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), size=(B, S))
    mask[1, 32 * (S // 64): 32 * (S // 64) + 32] = 0  # a whole zero word
    bits = _key_bits(G, _dev(G, mask, torch.uint8), S)
    want = np.packbits(mask != 0, axis=1, bitorder="little").view("<u4")
    got = bits.cpu().numpy().view(np.uint32)[:, : S // 32]
    assert np.array_equal(got, want)


# ---- the instantiations no test compared with a reference, on random data (the style and the bounds of tests/test_gpu_split.py)
@pytest.mark.gpu
@pytest.mark.parametrize("L", [64, 96])
def test_split_enc_self_attn_two_and_three_key_steps(G, L):
    """enc_attn_kernel<2, 2> and <3, 2>: tests/test_gpu_split.py::test_split_enc_self_attn at the lengths it leaves out."""
    from tests import test_gpu_split as TS
    TS.test_split_enc_self_attn(G, L)


@pytest.mark.gpu
@pytest.mark.parametrize("K,S", [(40, 160), (64, 384)])
def test_split_cross_attn_one_wave(G, K, S):
    """cross_attn_kernel<3, *, 2, 1> and <4, *, 2, 1>: tests/test_gpu_split.py::test_split_cross_attn with more than 32 beams."""
    from tests import test_gpu_split as TS
    TS.test_split_cross_attn(G, K, S)


@pytest.mark.gpu
def test_dec_self_attn_one_piece_to_the_last_step(G):
    """dec_self_attn_kernel<1> at t = 0..63 (tests/test_gpu_kernels.py::test_dec_self_attn stops at t = 5) against fp64 on the
    rounded operands.  The kernel keeps P in fp32, so the output's one rounding is the only 16-bit step: rtol = 2 * eps16 (twice
    the rounding).  atol covers the fp32 arithmetic in front of it: per position one rounding each in the score sum, the running sum
    and the accumulator (2^-24) and two __expf (a few 2^-23 each, their arguments within 2^-24 * |s|, |s| < 16) -- 2^-21 per position,
    times the 64 positions, times the largest |v|."""
    from gram_amd.model.gram import relative_position_bucket
    R, H, Tmax = 12, 3, DEC_LEN
    inner = H * 64
    eps16 = EPS16 if G.F16 else 2.0 ** -8
    g = torch.Generator().manual_seed(22)
    table = torch.randn(32, H, generator=g) * 0.5
    bias = table[relative_position_bucket(-torch.arange(0, DEC_LEN), False, 32, 128)].t().contiguous()
    kc = torch.zeros(Tmax, R, inner, dtype=G.DT, device=G.DEV)
    vc = torch.zeros_like(kc)
    anc = torch.arange(R, dtype=torch.int32).repeat(Tmax, 1)
    bias_d = bias.to(G.DEV)
    ks, vs, worst = None, None, 0.0
    for t in range(Tmax):
        qkv = G.bf(torch.randn(R, 3 * inner, generator=g) * 0.5)
        out = torch.empty(R, inner, dtype=G.DT, device=G.DEV)
        anc_d = anc.to(G.DEV)
        _lib.check(G.lib().gram_dec_self_attn(G.p(qkv), G.p(kc), G.p(vc), G.p(anc_d), G.p(bias_d), G.p(out), R, H, t, Tmax,
                                              G.stream()), "dec_attn")
        x = qkv.double().cpu().view(R, 3, H, 64)
        q, k, v = x[:, 0], x[:, 1], x[:, 2]
        ks = k[:, :, None] if ks is None else torch.cat([ks, k[:, :, None]], 2)  # [R][H][t + 1][64]
        vs = v[:, :, None] if vs is None else torch.cat([vs, v[:, :, None]], 2)
        sc = torch.einsum("rhd,rhjd->rhj", q, ks) + bias.double()[:, t - torch.arange(t + 1)][None]
        ref = torch.einsum("rhj,rhjd->rhd", torch.softmax(sc, -1), vs).reshape(R, inner)
        err = (out.double().cpu() - ref).abs()
        bound = 2 * eps16 * ref.abs() + DEC_LEN * 2.0 ** -21 * float(vs.abs().max())
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (t, float((err / bound).max()))
        parent = torch.randint(0, R, (R,), generator=g)
        ks, vs = ks.index_select(0, parent), vs.index_select(0, parent)
        anc = _anc_advance(anc, t, parent)
    print(f"\n[dec step, one piece, random data] t=0..{Tmax - 1}: largest error / bound = {worst:.2f}")


@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("R,reorder", [pytest.param(5, False, id="identity"), pytest.param(6, True, id="reordered")])
def test_stepped_self_attn_bitwise_vs_the_sequence_kernel(G, R, reorder, pieces):
    """gram_dec_self_attn_split at t = 0..18 against gram_dec_self_attn_tf_split on the same prefixes, bit for bit: both kernels call
    the one row step of self_attn_row.h.  T = 19 is two full batches of 8 cached positions and a remainder of 3 at the last step, so
    every slot of the stepped kernel's batch and every remainder is met, t = 0 (no cached position) included; H = 3 is a 48-thread
    block.  identity: row r of step t is position t of sequence r, one sequence per row.  reordered: random beam parents after every
    step; for every (t, r) the explicit sequence qkv_j[anc_t[j][r]], j < t, then qkv_t[r], and position t of it is compared -- the
    ancestor indirection and the shared step together."""
    H, T = 3, 19
    inner = H * 64
    g = torch.Generator().manual_seed(190 + R)
    x = G.pieces_of((torch.randn(T, R, 3 * inner, generator=g) * 0.5).to(G.DEV), pieces)  # [pieces][step][row][q|k|v]
    bias = torch.randn(H, DEC_LEN, generator=g).to(G.DEV)
    kc = torch.zeros(pieces, T, R, inner, dtype=G.DT, device=G.DEV)
    vc = torch.zeros_like(kc)
    anc = torch.arange(R, dtype=torch.int32).repeat(T, 1)
    n_seq = T * R if reorder else R
    seqs = torch.zeros(pieces, n_seq, T, 3 * inner, dtype=G.DT, device=G.DEV)
    if not reorder:
        seqs.copy_(x.transpose(1, 2))
    outs = []
    for t in range(T):
        if reorder:  # the T-padded prefixes of step t's rows, through the table the step reads
            for j in range(t):
                seqs[:, t * R: (t + 1) * R, j] = x[:, j, anc[j].long().to(G.DEV)]
            seqs[:, t * R: (t + 1) * R, t] = x[:, t]
        qkv = x[:, t].contiguous()
        out = torch.full((R, pieces * inner), float("nan"), dtype=G.DT, device=G.DEV)
        anc_d = anc.to(G.DEV)
        _lib.check(G.lib().gram_dec_self_attn_split(G.p(qkv), G.p(kc), G.p(vc), G.p(anc_d), G.p(bias), G.p(out), R, R, None, H, t, T,
                                                    pieces, qkv[0].numel(), kc[0].numel(), G.stream()), "dec_attn")
        outs.append(out)
        if reorder:
            anc = _anc_advance(anc, t, torch.randint(0, R, (R,), generator=g))
    want = torch.full((n_seq * T, pieces * inner), float("nan"), dtype=G.DT, device=G.DEV)
    _lib.check(G.lib().gram_dec_self_attn_tf_split(G.p(seqs), G.p(bias), G.p(want), n_seq, T, H, pieces, seqs[0].numel(), G.stream()),
               "tf_attn")
    want = want.view(n_seq, T, pieces * inner)
    assert not bool(torch.isnan(want.float()).any())
    for t in range(T):
        rows = want[t * R: (t + 1) * R, t] if reorder else want[:, t]
        assert torch.equal(outs[t].view(torch.int16), rows.contiguous().view(torch.int16)), t


# ------------------------------------------------------------------------------------------------ no GPU: the probes can see it
def test_probes_reject_single_slot_errors():
    """Every probe's fp64 reference passes its own comparator, meets the weight floors, and the comparator -- at the WIDEST bound any
    probe uses, the one-piece 4 * eps16 -- rejects the weights of a kernel with one index error: the bias table read one slot further
    at distances >= 17 (everywhere, and at one distance only), one mask bit moved to the neighbouring key, two keys 64 apart swapped,
    one key dropped, an ancestor row replaced by its neighbour, the causal limit off by one.  For contrast: on the bucketed table the
    other tests use, the one-distance bias error changes nothing at all (the same bias bits, so no comparator can reject it) at all
    but the handful of distances where a log-spaced bucket ends."""
    rtol = RTOL1

    def accepted(W, ref):
        return compare(W, ref, rtol)[0]

    def dropped(ref, key):  # softmax without that key: its weight is 0, the others share its mass
        W = ref.copy()
        W[..., key] = 0.0
        with np.errstate(invalid="ignore"):  # (a row whose only key it was: NaN, which no comparator accepts)
            return W / W.sum(-1, keepdims=True)

    def swapped(ref, a, b):
        W = ref.copy()
        W[..., [a, b]] = ref[..., [b, a]]
        return W

    # ---- encoder
    for L, H in ENC_CASES:
        p = enc_probe(L, H)
        ref = p["ref"]
        precondition(ref)
        assert accepted(ref, ref)
        assert np.allclose(ref[3], 1.0 / L, rtol=1e-15, atol=0) and (ref[1][..., L - 13:] == 0).all()
        far = lambda i: np.where(np.abs(i - 127) >= 17, np.minimum(i + 1, 254), i)  # noqa: E731
        assert not accepted(enc_weights(p, slot=far), ref), L
        if L >= 64:
            for d in (17, L - 2):
                for sign in (1, -1):
                    one = lambda i, s=127 + sign * d: np.where(i == s, i + 1, i)  # noqa: E731
                    assert not accepted(enc_weights(p, slot=one), ref), (L, d, sign)
            assert not accepted(swapped(ref, 3, 67) if L > 67 else swapped(ref, 3, 63), ref), L
        for m, j in ((1, L - 14), (2, L // 2 - 6), (2, L // 2 + 5)):  # the mask's edges: bit j and bit j + 1 trade places
            mask = p["mask"].copy()
            assert (mask[m, j] != 0) != (mask[m, j + 1] != 0)
            mask[m, [j, j + 1]] = mask[m, [j + 1, j]]
            assert not accepted(enc_weights(p, mask=mask), ref), (L, m, j)
        assert not accepted(dropped(ref, L - 20), ref) and not accepted(dropped(ref, 0), ref), L
    # ---- cross-attention
    for S in XATTN_S:
        for K in XATTN_K:
            p = xattn_probe(K, S)
            ref = p["ref"]
            precondition(ref)
            assert accepted(ref, ref)
            valid = p["mask"] != 0
            edges = np.nonzero(valid[:-1] != valid[1:])[0]
            for j in edges[[0, len(edges) // 2, -1]]:
                mask = p["mask"].copy()
                mask[[j, j + 1]] = mask[[j + 1, j]]
                assert not accepted(xattn_weights(p, mask=mask), ref), (K, S, j)
            a = np.nonzero(valid)[0]
            assert not accepted(dropped(ref, a[0]), ref) and not accepted(dropped(ref, a[-1]), ref), (K, S)
            pairs = [j for j in a if j + 64 < S and valid[j + 64]]
            if pairs:  # two valid keys 64 apart: the same output dimension of neighbouring users
                kv = p["kv"].copy()
                kv[:, [pairs[0], pairs[0] + 64]] = kv[:, [pairs[0] + 64, pairs[0]]]
                assert not accepted(xattn_weights(p, kv=kv), ref), (K, S)
            if S >= 96:  # a valid key and a masked one 64 apart
                j = next(j for j in a if (j + 64 < S and not valid[j + 64]) or (j >= 64 and not valid[j - 64]))
                o = j + 64 if (j + 64 < S and not valid[j + 64]) else j - 64
                assert not accepted(swapped(ref, j, o), ref), (K, S)
    for S in (64, 2048, 2080, 4096):
        for K in (4, 40):
            ref = xattn_probe(K, S, all_masked=True)["ref"]
            precondition(ref, 1)
            assert accepted(ref, ref) and not accepted(dropped(ref, S - 1), ref)  # uniform over S - 1 keys: off by 1 / S
    # ---- decoder step
    for H in (3, 16):
        p = dec_probe(H)
        ref = p["ref"]
        precondition(ref)
        assert accepted(ref, ref)
        far = lambda d: np.where(d >= 17, np.minimum(d + 1, DEC_LEN - 1), d)  # noqa: E731
        W = dec_weights(p, slot=far)
        assert accepted(W[:17], ref[:17]) and not accepted(W[17], ref[17]) and not accepted(W[62], ref[62])
        for t, r, j in ((1, 0, 0), (40, 5, 17), (63, 11, 62)):
            W = dec_weights(p, wrong=(t, r, j))
            assert not accepted(W[t], ref[t]), (t, r, j)
            assert accepted(np.delete(W, t, 0), np.delete(ref, t, 0))
        assert not accepted(dropped(ref[63], 30), ref[63])
    # ---- teacher-forced
    for T in TF_T:
        p = tf_probe(T)
        ref = p["ref"]
        precondition(ref)
        assert accepted(ref, ref)
        if T > 1:
            assert not accepted(tf_weights(p, limit=lambda t: t + 1), ref), T  # looks one position ahead
            assert not accepted(tf_weights(p, limit=lambda t: np.maximum(t - 1, 0)), ref), T  # misses its own position
            assert not accepted(dropped(ref, 0)[:, :, 1:], ref[:, :, 1:]), T
        if T > 18:
            far = lambda d: np.where(d >= 17, np.minimum(d + 1, DEC_LEN - 1), d)  # noqa: E731
            assert not accepted(tf_weights(p, slot=far), ref), T
    # ---- the contrast: T5's bucketed tables
    from gram_amd.model.gram import relative_position_bucket
    table = torch.randn(32, 3, generator=torch.Generator().manual_seed(128)) * 0.5
    enc_b = table[relative_position_bucket(torch.arange(-127, 128), True, 32, 128)].t().contiguous().numpy()      # [H][255]
    dec_b = table[relative_position_bucket(-torch.arange(0, DEC_LEN), False, 32, 128)].t().contiguous().numpy()  # [H][64]
    enc_same = [d for d in range(17, 127) for s in (1, -1) if np.array_equal(enc_b[:, 127 + s * d], enc_b[:, 127 + s * d + 1])]
    dec_same = [d for d in range(17, DEC_LEN - 1) if np.array_equal(dec_b[:, d], dec_b[:, d + 1])]
    assert len(enc_same) >= 2 * 110 - 12 and len(dec_same) >= (DEC_LEN - 18) - 12, (len(enc_same), len(dec_same))
    p = dict(enc_probe(128, 3), bias=enc_b)  # the L = 128 probe on the bucketed table: the comparator accepts these mutants
    ref = enc_weights(p)
    for d in (17, 60, 100, 125):
        for sign in (1, -1):
            assert np.array_equal(enc_b[:, 127 + sign * d], enc_b[:, 127 + sign * d + 1])
            one = lambda i, s=127 + sign * d: np.where(i == s, i + 1, i)  # noqa: E731
            assert accepted(enc_weights(p, slot=one), ref), (d, sign)
    p = dict(tf_probe(64), bias=dec_b)
    ref = tf_weights(p)
    for d in (17, 28, 42, 61):
        assert np.array_equal(dec_b[:, d], dec_b[:, d + 1])
        assert accepted(tf_weights(p, slot=lambda i, s=d: np.where(i == s, i + 1, i)), ref), d
