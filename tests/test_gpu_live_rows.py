"""The live-row forms of the three decode-step kernels (include/gram_hip.h, gram_live_rows_t), each against its all-rows form through
the C ABI: gram_cross_attn_decode_split(users, rowpos), gram_dec_self_attn_split(rows) and gram_beam_step_sparse_live /
gram_beam_step_sparse_split(rowpos).  The header promises "bit-identical to running every row" with the cache, the ancestor table,
the bank and the beam state keeping their original indexing: outputs and state are compared bit for bit (as integers, so -0.0 and
NaN payloads count), buffers are prefilled with a sentinel to show every write, and the live outputs are also held against the
references and tolerances of the all-rows tests (tests/test_gpu_kernels.py, tests/test_gpu_split.py).

The live sets of the two attention tests come from live_schedule() below (numpy, checked on the CPU by the one unmarked test); the
beam step is driven through whole ragged searches and takes its live sets from gram_live_rows on the state it has reached."""
import ctypes as C

import numpy as np
import pytest
import torch

SENT = 0x5A5A  # 16-bit sentinel pattern (a finite number in IEEE half and in bfloat16)


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    return gpu_util


# ------------------------------------------------------------------------------------ the live-set generator (numpy)
def live_schedule(B, K, steps, seed, shrink_from=3):
    """Per-step live masks over the R = B * K rows and the beam parents that go with them.

    Returns (live bool [steps][R], parent i32 [steps][R]): row r of step t goes on from row parent[t][r] of step t - 1 (parent[0] is
    the identity), and a row live at step t has a parent that was live at step t - 1 -- the self-attention cache of a live-row search
    holds valid data only along such chains.  Parents stay inside their user, as the beam search's do.  Every row is live before
    `shrink_from`; then user u follows pattern u % 6, changing at s0 = shrink_from and s1 = shrink_from + 3:
        0  every beam live throughout            3  a random half that holds the last beam from s0, only the last beam from s1
        1  no beam live from s0                  4  alternating (even) beams from s1
        2  alternating beams from s0,            5  a random half from s1
           only beam 0 from s1
    so with B >= 6 step s1 shows all six patterns side by side.  The last step has ONE live row in the whole batch."""
    s0, s1 = shrink_from, shrink_from + 3
    assert steps >= s1 + 2 and B >= 1 and K >= 1
    rng = np.random.default_rng(seed)
    beams = np.arange(K)
    alt, first, last = beams % 2 == 0, beams == 0, beams == K - 1
    n_half = max(1, K // 2)
    live = np.ones((steps, B, K), dtype=bool)
    for u in range(B):
        half = np.zeros(K, dtype=bool)
        half[rng.permutation(K)[:n_half]] = True
        half_last = last.copy()
        half_last[rng.permutation(K - 1)[: n_half - 1]] = True
        kind = u % 6
        if kind == 1:
            live[s0:, u] = False
        elif kind == 2:
            live[s0:s1, u], live[s1:, u] = alt, first
        elif kind == 3:
            live[s0:s1, u], live[s1:, u] = half_last, last
        elif kind == 4:
            live[s1:, u] = alt
        elif kind == 5:
            live[s1:, u] = half
    u1 = max(u for u in range(B) if live[steps - 2, u].any())  # the single row: the last live beam of the last user that still has one
    k1 = int(np.nonzero(live[steps - 2, u1])[0][-1])
    live[steps - 1] = False
    live[steps - 1, u1, k1] = True
    parent = np.empty((steps, B * K), dtype=np.int32)
    parent[0] = np.arange(B * K)
    for t in range(1, steps):
        for u in range(B):
            pool = np.nonzero(live[t - 1, u])[0]
            p = rng.integers(0, K, K)  # rows that are not live go on from any row of their user
            if pool.size:
                p = np.where(live[t, u], pool[rng.integers(0, pool.size, K)], p)
            parent[t, u * K:(u + 1) * K] = u * K + p
    return live.reshape(steps, B * K), parent


def live_layout(mask, B, K):
    """gram_live_rows_t of a live mask: rows (original row of compact row i), rowpos (compact row of row r, -1 = not live), users
    (the users that own a live row), all ascending"""
    rows = np.nonzero(mask)[0].astype(np.int32)
    rowpos = np.full(B * K, -1, dtype=np.int32)
    rowpos[rows] = np.arange(rows.size, dtype=np.int32)
    users = np.nonzero(mask.reshape(B, K).any(1))[0].astype(np.int32)
    return rows, rowpos, users


def advance_anc(anc, parent, t):
    """The ancestor table [Tmax][R] after step t, when the rows of step t + 1 go on from the rows `parent` (what
    test_dec_self_attn does after each step, and beam_step_kernel on the device)"""
    new = anc.copy()
    new[:t] = anc[:t, parent]
    new[t] = parent
    return new


def _patterns(m):
    """names of the issue's patterns that a user's live mask [K] shows"""
    K, names = m.size, set()
    beams = np.arange(K)
    if m.all():
        names.add("all")
    if not m.any():
        names.add("none")
    if np.array_equal(m, beams == 0):
        names.add("first")
    if np.array_equal(m, beams == K - 1):
        names.add("last")
    if np.array_equal(m, beams % 2 == 0):
        names.add("alternating")
    if m.sum() == max(1, K // 2):
        names.add("half")
    return names


XATTN_K = [1, 8, 16, 20, 33, 50, 64]


@pytest.mark.parametrize("B,K,steps", [(6, K, 8) for K in XATTN_K] + [(4, 8, 12), (4, 8, 64)])
def test_live_schedule_invariants_and_layout(B, K, steps):
    """The generator the GPU tests below rely on: a live row's whole ancestor chain was live, the layout is gram_live_rows_t's, and
    the batch holds every pattern the live kernels must cope with."""
    R, s0, s1 = B * K, 3, 6
    live, parent = live_schedule(B, K, steps, seed=K)
    assert live.shape == (steps, R) and parent.shape == (steps, R) and live[:s0].all()
    counts = live.sum(1)
    assert (np.diff(counts) <= 0).all() and counts[s0] < counts[s0 - 1] and counts[-1] == 1
    if K > 1:
        assert counts[s1] < counts[s1 - 1]
    anc = np.tile(np.arange(R, dtype=np.int32), (steps, 1))
    for t in range(steps):
        assert (parent[t] // K == np.arange(R) // K).all()
        if t:
            assert live[t - 1][parent[t][live[t]]].all()  # a live row's parent was live
        for j in range(t):
            assert live[j][anc[j][live[t]]].all(), (t, j)  # ... and so was every ancestor: slot j of the cache holds its K/V
        if t + 1 < steps:
            anc = advance_anc(anc, parent[t + 1], t)
        rows, rowpos, users = live_layout(live[t], B, K)
        assert rows.size == counts[t] and (np.diff(rows) > 0).all() and live[t][rows].all()
        assert (rowpos[rows] == np.arange(rows.size)).all() and (rowpos[~live[t]] == -1).all()
        assert (np.diff(users) > 0).all() and set(users.tolist()) == set((rows // K).tolist())
    assert live_layout(live[-1], B, K)[2].size == 1
    per_user = live.reshape(steps, B, K)
    if B >= 6:  # all six patterns side by side at step s1
        for u, name in enumerate(("all", "none", "first", "last", "alternating", "half")):
            assert name in _patterns(per_user[s1, u]), (u, name)
        assert 1 not in live_layout(live[s1], B, K)[2]
        if K > 16:  # only the last beam: every 16-beam tile in front of its tile is empty
            assert not per_user[s1, 3, : 16 * ((K - 1) // 16)].any()
    seen = set().union(*(_patterns(per_user[t, u]) for t in range(steps) for u in range(B)))
    assert seen == {"all", "none", "first", "last", "alternating", "half"}


def _bits(t):
    """a 16-bit tensor as its bit patterns: equality of these is equality bit for bit"""
    return t.contiguous().view(torch.int16)


def _dev_i32(a, G):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(G.DEV)


# ------------------------------------------------------------------------------------ cross-attention
@pytest.mark.gpu
@pytest.mark.parametrize("S", [32, 160, 384])
@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("K", XATTN_K)  # beam tiles 1..4: two waves merged (K <= 32) and one wave, a partly filled last tile
def test_cross_attn_live_matches_all_rows(G, K, pieces, S):
    """gram_cross_attn_decode_split on the live rows of a batch that holds every live pattern (live_schedule), and on a single live
    row: the bits of the all-rows call on the same q, bank and mask, nothing written behind the live rows, the references of
    test_cross_attn_decode (one piece) / test_split_cross_attn (two), and the same bits with and without precomputed key bits."""
    from gram_amd import _lib
    from oracle import gram_oracle as O
    from tests.test_gpu_split import relerr, tol
    B, H = 6, 2
    R, inner = B * K, H * 64
    g = torch.Generator().manual_seed(K * 1000 + S)
    q32 = (torch.randn(R, inner, generator=g) * 0.3).to(G.DEV)
    k32 = torch.randn(B, H, S, 64, generator=g).to(G.DEV)
    v32 = torch.randn(B, H, S, 64, generator=g).to(G.DEV)
    vtb32 = G.vt_blocked(v32.transpose(2, 3).contiguous())
    # [pieces][...] planar pieces; one piece: the rounded values themselves
    q, kb, vt = (G.pieces_of(x, pieces) for x in (q32, k32, vtb32))
    mask = torch.rand(B, S, generator=g) > 0.3
    mask[0] = False            # a live user (every beam) whose whole bank is masked
    mask[2, : S // 2] = False  # leading masked steps (whole 32-key steps before any valid key)
    if S >= 64:
        mask[3, 32:] = False   # keys only in the first step
    m8 = mask.to(G.DEV).view(torch.uint8).contiguous()
    bits = torch.full((B, 128), -1, dtype=torch.int32, device=G.DEV)
    L_ = G.lib()
    _lib.check(L_.gram_mask_key_bits(G.p(m8), G.p(bits), B, S, G.stream()), "bits")

    def run(qq, n_users, users, rowpos, key_bits):
        out = torch.empty(R, pieces * inner, dtype=G.DT, device=G.DEV)
        _bits(out).fill_(SENT)
        _lib.check(L_.gram_cross_attn_decode_split(G.p(qq), G.p(kb), G.p(vt), G.p(m8), G.p(out), n_users, K, H, S, G.p(users),
                                                   G.p(rowpos), pieces, qq[0].numel(), kb[0].numel(), G.p(key_bits), G.stream()), "xattn")
        return out

    out_all = run(q, B, None, None, None)
    if pieces == 1:
        qh = q[0].float().cpu().view(B, K, H, 64).permute(0, 2, 1, 3)  # (B,H,K,64)
        ext = ((1.0 - mask.float()) * O.FMIN)[:, None, None, :]
        ref = O._attend(qh, kb[0].float().cpu(), G.vt_unblocked(vt[0]).float().cpu().transpose(2, 3), ext).reshape(R, inner)
    else:
        qh = q32.double().cpu().view(B, K, H, 64).permute(0, 2, 1, 3)
        ext = ((1.0 - mask.float()) * O.FMIN)[:, None, None, :].double()
        sc = torch.matmul(qh, k32.double().cpu().transpose(3, 2)) + ext
        ref = torch.matmul(torch.softmax(sc, -1), v32.double().cpu()).transpose(1, 2).reshape(R, inner)

    live, _ = live_schedule(B, K, 8, seed=K)
    for t in (6, 7):  # every pattern side by side / one live row in the whole batch
        rows, rowpos, users = live_layout(live[t], B, K)
        n = rows.size
        assert (t == 7) == (n == 1) and users.size == (1 if t == 7 else 5)
        rows_d, rowpos_d, users_d = (_dev_i32(a, G) for a in (rows, rowpos, users))
        q_live = q[:, rows_d.long()].contiguous()
        out_live = run(q_live, users.size, users_d, rowpos_d, None)
        out_live_bits = run(q_live, users.size, users_d, rowpos_d, bits)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out_live[:n]), _bits(out_all[rows_d.long()])), t
        assert (_bits(out_live[n:]) == SENT).all(), t  # a beam that is not live is skipped: nothing behind the compact rows
        assert torch.equal(_bits(out_live), _bits(out_live_bits)), t
        want = ref[torch.from_numpy(rows).long()]
        if pieces == 1:
            # bf16 P and bf16 output on O(1) values: 1e-2 abs (test_cross_attn_decode)
            assert torch.allclose(out_live[:n].float().cpu(), want, atol=1e-2, rtol=1e-2), t
        else:
            e = relerr(G.join_inter(out_live[:n]).cpu(), want)
            print(f"\n[live cross attn] K={K} S={S} step {t}: {e:.2e}")
            assert e < 10 * tol(G), t
    assert torch.equal(_bits(out_all), _bits(run(q, B, None, None, bits)))


# ------------------------------------------------------------------------------------ decoder self-attention
@pytest.mark.gpu
@pytest.mark.parametrize("H,pieces,steps", [(H, pc, 12) for H in (3, 8, 12, 16) for pc in (1, 2)] + [(12, 2, 64)])
def test_dec_self_attn_live_matches_all_rows(G, H, pieces, steps):
    """gram_dec_self_attn_split(rows) over a live set that shrinks from step 3 on (live_schedule: 4 users x 8 beams), next to the
    all-rows form on a cache of its own: the same output bits on the live rows, slot t of the cache written at the ORIGINAL rows
    (every piece) and nowhere else, and the fp64 reference of test_split_dec_self_attn (K/V history followed through the parents)."""
    from gram_amd import _lib
    from gram_amd.model.gram import relative_position_bucket
    from oracle import gram_oracle as O
    from tests.test_gpu_split import relerr, tol
    B, K, Tmax = 4, 8, 64
    R, inner = B * K, H * 64
    g = torch.Generator().manual_seed(100 * H + pieces)
    table = torch.randn(32, H, generator=g) * 0.5
    bias = table[relative_position_bucket(-torch.arange(0, _lib.GRAM_MAX_DEC_LEN), False, 32, 128)].t().contiguous().to(G.DEV)
    cfg = O.OracleConfig(num_heads=H)
    # two caches with the same (arbitrary) contents: A is stepped by the all-rows form, B by the live form
    kc_a = G.bf(torch.randn(pieces, Tmax, R, inner, generator=g))
    vc_a = G.bf(torch.randn(pieces, Tmax, R, inner, generator=g))
    kc_b, vc_b = kc_a.clone(), vc_a.clone()
    cache_ps = kc_a[0].numel()
    live, parent = live_schedule(B, K, steps, seed=H)
    anc = np.tile(np.arange(R, dtype=np.int32), (Tmax, 1))
    L_ = G.lib()
    ks, vs = None, None
    for t in range(steps):
        rows, _, _ = live_layout(live[t], B, K)
        n = rows.size
        rows_d = _dev_i32(rows, G)
        ri = rows_d.long()
        dead = torch.from_numpy(np.nonzero(~live[t])[0]).to(G.DEV)
        qkv32 = (torch.randn(R, 3 * inner, generator=g) * 0.5).to(G.DEV)
        qkv = G.pieces_of(qkv32, pieces)
        qkv_live = qkv[:, ri].contiguous()
        anc_d = _dev_i32(anc, G)
        out_all = torch.empty(R, pieces * inner, dtype=G.DT, device=G.DEV)
        out_live = torch.empty(R, pieces * inner, dtype=G.DT, device=G.DEV)
        _bits(out_live).fill_(SENT)
        for c in (kc_b, vc_b):
            _bits(c)[:, t] = SENT
        _lib.check(L_.gram_dec_self_attn_split(G.p(qkv), G.p(kc_a), G.p(vc_a), G.p(anc_d), G.p(bias), G.p(out_all), R, R, None, H, t,
                                               Tmax, pieces, qkv[0].numel(), cache_ps, G.stream()), "dec_attn")
        _lib.check(L_.gram_dec_self_attn_split(G.p(qkv_live), G.p(kc_b), G.p(vc_b), G.p(anc_d), G.p(bias), G.p(out_live), R, n,
                                               G.p(rows_d), H, t, Tmax, pieces, qkv_live[0].numel(), cache_ps, G.stream()), "dec_attn live")
        torch.cuda.synchronize()
        assert torch.equal(_bits(out_live[:n]), _bits(out_all[ri])), t
        assert (_bits(out_live[n:]) == SENT).all(), t
        for ca, cb in ((kc_a, kc_b), (vc_a, vc_b)):
            # slot t, every piece (cache_pstride apart): the live form wrote the ORIGINAL rows rows[i] and no other row
            assert torch.equal(_bits(cb)[:, t, ri], _bits(ca)[:, t, ri]), t
            assert (_bits(cb)[:, t, dead] == SENT).all(), t
        x = G.join(qkv).cpu().view(R, 1, 3, H, 64)
        q_, k_, v_ = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        ks = k_ if ks is None else torch.cat([ks, k_], 2)
        vs = v_ if vs is None else torch.cat([vs, v_], 2)
        b_ = O.position_bias(table, t + 1, t + 1, False, cfg)[:, :, -1:, :].double()
        sc = torch.matmul(q_, ks.transpose(3, 2)) + b_
        ref = torch.matmul(torch.softmax(sc, -1), vs).transpose(1, 2).reshape(R, inner)[torch.from_numpy(rows).long()]
        if pieces == 1:
            assert torch.allclose(out_live[:n].float().cpu().double(), ref, atol=2e-2, rtol=2e-2), t  # test_dec_self_attn's
        else:
            assert relerr(G.join_inter(out_live[:n]).cpu(), ref) < 10 * tol(G), t
        if t + 1 < steps:
            # beam reorder: the reference index_selects the K/V history, the device follows the ancestor table
            par = torch.from_numpy(parent[t + 1]).long()
            ks, vs = ks.index_select(0, par), vs.index_select(0, par)
            anc = advance_anc(anc, parent[t + 1], t)


# ------------------------------------------------------------------------------------ beam step
STATE = ("tokens", "node", "beam_scores", "seq", "anc", "done", "n_hyps", "hyp_score", "worst", "hyp_len", "hyp_tok")


def _raw(t):
    """a state array as integers of its element size (floats compared by their bits)"""
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


@pytest.mark.gpu
@pytest.mark.parametrize("scratch", [False, True])
@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("B,K", [(5, 4), (3, 20), (2, 64)])
@pytest.mark.parametrize("name", ["ragged", "rand"])
def test_beam_step_live_matches_all_rows(G, name, B, K, pieces, scratch):
    """A whole search on candidates of ragged lengths (beams leave the Trie at different steps, users finish early): at every step
    t >= 1 the state is stepped twice, by the all-rows sparse call on the full hidden / lse and by the rowpos form on hidden[rows] /
    lse[rows] of gram_live_rows' rows -- every state array bit-identical, error flag clear.  The compact buffers keep R rows, NaN
    behind the live ones.  The search goes on from the all-rows state; at its end the dense gram_beam_step path on the same hidden
    states returns the same sequences (scores within test_beam_step_sparse_equals_dense's 2e-5)."""
    from gram_amd import _lib
    from gram_amd.utils import generation_trie as gt
    if name == "ragged":
        from tests.test_gpu_kernels import _tries
        cands = _tries()["ragged"]
    else:
        from tests.test_gpu_configs import _rand_cands
        cands = _rand_cands(7, 120, 2, 6)
    flat = gt.FlatTrie(gt.Trie(cands))
    ctrie, _keep_trie = flat.to_device(torch.device(G.DEV))
    V, d = 256, 128
    R = B * K
    max_length = max(len(c) for c in cands)
    g = torch.Generator().manual_seed(1000 * B + 10 * K + pieces)
    E32 = torch.randn(V, d, generator=g).to(G.DEV)
    hidden32 = [(torch.randn(B if t == 0 else R, d, generator=g) * d ** -0.5 * 3).to(G.DEV) for t in range(max_length - 1)]
    if pieces == 2:
        W, hidden = G.inter(E32), [G.inter(h) for h in hidden32]  # interleaved [rows][2 d]
    else:
        W, hidden = G.bf(E32), [G.bf(h) for h in hidden32]
    sp = _lib.Split(pieces, 0, 0, 0, 1.0)
    L_ = G.lib()

    def lse_of(h, logits=None):
        rows = h.shape[0]
        part = torch.empty(rows, V // 64, 2, dtype=torch.float32, device=G.DEV)
        lse = torch.empty(rows, dtype=torch.float32, device=G.DEV)
        _lib.check(L_.gram_gemm_bf16_lse_split(G.p(h), G.p(W), G.p(logits), G.p(part), rows, V, d, pieces * d, V, C.byref(sp), G.stream()),
                   "gemm")
        _lib.check(L_.gram_lse_combine(G.p(part), G.p(lse), rows, V // 64, G.stream()), "lse")
        return lse

    def sparse_step(st, h, lse, t, rpu, rowpos):
        if pieces == 2:
            rc = L_.gram_beam_step_sparse_split(C.byref(st), C.byref(ctrie), G.p(h), G.p(E32), d, G.p(lse), V, t + 1, rpu, G.p(rowpos), 2,
                                                G.stream())
        elif rowpos is not None:
            rc = L_.gram_beam_step_sparse_live(C.byref(st), C.byref(ctrie), G.p(h), G.p(W), d, G.p(lse), V, t + 1, G.p(rowpos), G.stream())
        else:
            rc = L_.gram_beam_step_sparse(C.byref(st), C.byref(ctrie), G.p(h), G.p(W), d, G.p(lse), V, t + 1, rpu, G.stream())
        _lib.check(rc, "step_sparse")

    def finalize(st):
        seqs = torch.empty(R, max_length, dtype=torch.int64, device=G.DEV)
        scores = torch.empty(R, dtype=torch.float32, device=G.DEV)
        width = torch.zeros(4, dtype=torch.int32, device=G.DEV)
        _lib.check(L_.gram_beam_finalize(C.byref(st), K, max_length, G.p(seqs), G.p(scores), G.p(width), G.stream()), "fin")
        torch.cuda.synchronize()
        return seqs.cpu(), scores.cpu()

    st_a, a = G.make_beam_state(B, K, max_length, cand_scratch=scratch)  # all rows: the search itself
    st_b, b = G.make_beam_state(B, K, max_length, cand_scratch=scratch)  # its copy, stepped by the live form
    _lib.check(L_.gram_beam_init(C.byref(st_a), C.byref(ctrie), 0, G.stream()), "init")
    n_live = []
    for t in range(max_length - 1):
        lse = lse_of(hidden[t])
        if t == 0:  # all beams of a user are identical: one row per user
            sparse_step(st_a, hidden[0], lse, 0, 1, None)
            continue
        for k in STATE + ("error",):
            b[k].copy_(a[k])
        rows, rowpos, users = G.device_live_rows(st_a, ctrie)
        n = rows.numel()
        n_live.append(n)
        sparse_step(st_a, hidden[t], lse, t, K, None)
        if n == 0:  # nothing to decode: gram_generate launches nothing either (the ABI rejects n_rows < 1)
            continue
        h_live = torch.full_like(hidden[t], float("nan"))
        lse_live = torch.full_like(lse, float("nan"))
        h_live[:n], lse_live[:n] = hidden[t][rows.long()], lse[rows.long()]
        sparse_step(st_b, h_live, lse_live, t, K, rowpos)
        torch.cuda.synchronize()
        for k in STATE:
            assert torch.equal(_raw(a[k]), _raw(b[k])), (t, k)
        assert int(a["error"][0]) == 0 and int(b["error"][0]) == 0, t
    print(f"\n[live beam step] {name} B={B} K={K}: live rows per step {n_live} of {R}")
    assert any(0 < n < R for n in n_live)  # the search did run on a strict subset of its rows
    seqs, scores = finalize(st_a)
    err = int(a["error"][0])

    st_d, dd = G.make_beam_state(B, K, max_length)
    _lib.check(L_.gram_beam_init(C.byref(st_d), C.byref(ctrie), 0, G.stream()), "init")
    for t in range(max_length - 1):
        logits = torch.empty(hidden[t].shape[0], V, dtype=torch.float32, device=G.DEV)
        lse = lse_of(hidden[t], logits)
        _lib.check(L_.gram_beam_step(C.byref(st_d), C.byref(ctrie), G.p(logits), G.p(lse), V, t + 1, 1 if t == 0 else K, G.stream()), "step")
    dseqs, dscores = finalize(st_d)
    assert int(dd["error"][0]) == err
    assert dseqs.tolist() == seqs.tolist()
    assert torch.allclose(dscores, scores, atol=2e-5)
