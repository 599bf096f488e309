"""-m gpu: the row kernels of gram_amd/csrc/rowops.hip (and gram_trie_repeat_tokens), every launch form through the C ABI against an
fp64 restatement of the same operation on the same inputs.

Every output buffer is four rows (1-D outputs: 64 elements) longer than the call writes and prefilled with a sentinel (NaN for
floats, -7 for ints); after the call the tail must still hold the sentinel's bits.  Copies, pieces and row factors are identities
and compared bit for bit; sums and norms are held to the bounds stated at `_ratio16` and at each assert.  Every test prints the worst
error / bound ratio it saw."""
import pytest
import torch

from gram_amd import _lib
from tests.test_gpu_split import _host_row_xscale

pytestmark = pytest.mark.gpu

EPS = 1e-6
F32_TINY = 2.0 ** -126  # squares below fp32's normal range lose bits or vanish: the absolute floor of a sum-of-squares comparison


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    return gpu_util


# ------------------------------------------------------------------------------------ sentinels and bit comparisons
def _sent(G, shape, dtype):
    if dtype.is_floating_point:
        return torch.full(shape, float("nan"), dtype=dtype, device=G.DEV)
    return torch.full(shape, -7, dtype=dtype, device=G.DEV)


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()]) if t.dtype.is_floating_point else t


def _biteq(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a.contiguous()), _bits(b.contiguous())))


def _written(G, buf, n):
    """buf[:n] after checking that buf[n:] was left alone"""
    torch.cuda.synchronize()
    tail = buf[n:]
    assert tail.numel() > 0 and _biteq(tail, _sent(G, tuple(tail.shape), buf.dtype)), "the call wrote behind its output"
    return buf[:n]


# ------------------------------------------------------------------------------------ the 16-bit tolerance
def spacing16(G, v):
    """spacing of the library's 16-bit type at |v| (fp64 in, fp64 out)"""
    mant, emin = (10, -14) if G.F16 else (7, -126)
    v = v.double().abs().cpu()
    _, e = torch.frexp(v)  # v = m * 2^e, m in [0.5, 1): floor(log2 v) = e - 1
    fl = torch.where(v == 0, torch.full_like(e, emin), e - 1).clamp(min=emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (fl - mant).double())


def _ratio16(G, got, a, b, pieces):
    """worst |got - (a + b)| / bound over a 16-bit output (one piece) or the fp64 join of its two pieces.  a: the normalised term,
    b: the position term, both fp64.  One piece: half a spacing of the 16-bit type (round to nearest) plus 2e-6 (|a| + |b|) for the
    fp32 arithmetic in front of it.  Two pieces: the low piece rounds the residual, itself at most half a spacing of the high piece:
    2^-11 of that spacing on IEEE half (plus 2^-24: the low piece goes subnormal), 2^-8 on bfloat16."""
    got, a, b = got.double().cpu(), a.double().cpu(), b.double().cpu()
    ref = a + b
    sp = spacing16(G, torch.maximum(ref.abs(), got.abs()))
    slack = 2e-6 * (a.abs() + b.abs())
    if pieces == 1:
        bound = 0.5 * sp + slack
    elif G.F16:
        bound = sp * 2.0 ** -11 + 2.0 ** -24 + slack
    else:
        bound = sp * 2.0 ** -8 + slack
    assert bool(torch.isfinite(got).all())
    return float(((got - ref).abs() / bound).max())


def _off_the_edge(f):
    """rows of a row-factor argument f = min(want, cap) whose log2 lies within 0.002 of an integer (and that no clamp decides)"""
    lg = torch.log2(f.double())
    return torch.isfinite(lg) & (lg > -41) & (lg < 21) & ((lg - lg.round()).abs() < 0.002)


def _xscale_arg(ss):
    """min(want, cap) of common.h's row_xscale from 64-column partials [M][nblk], in fp64"""
    ss = ss.double()
    return torch.minimum(0.25 * torch.rsqrt(ss.min(dim=1).values / 64.0), 1024.0 * torch.rsqrt(ss.sum(dim=1)))


def _rel_ss(got, ref):
    """worst |got - ref| / (1e-6 ref + fp32's smallest normal)"""
    got, ref = got.double().cpu(), ref.double().cpu()
    return float(((got - ref).abs() / (1e-6 * ref + F32_TINY)).max())


# ------------------------------------------------------------------------------------ embedding
V_TAB = 9


def _embed_table(G, d, seed):
    """rows: 0 all zero | 1 magnitude 1e-30 | 2 magnitude 3e5, three columns x 300 | 3, 4, 5 zero in exactly one 64-column block (their
    cap, not the quietest block, sets the row factor; magnitudes a third of a binade apart) | 6 plain | 7 magnitude 1e-2 | 8 plain with
    three columns x 300"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(V_TAB, d, generator=g)
    cols = sorted({1 % d, d // 2, d - 1})
    nb = max(d // 64, 1)
    t[0] = 0.0
    t[1] *= 1e-30
    t[2] *= 3e5
    t[2, cols] *= 300.0
    for r, (blk, mag) in zip((3, 4, 5), ((0, 1.0), (nb - 1, 2.0 ** (1 / 3)), (nb // 2, 32.0 * 2.0 ** (2 / 3)))):
        t[r] *= mag
        t[r, 64 * blk:64 * blk + 64] = 0.0
    t[7] *= 1e-2
    t[8, cols] *= 300.0
    if d % 64 == 0:  # keep every row factor off the rounding edge of rsqrt
        for _ in range(8):
            edge = _off_the_edge(_xscale_arg((t.double() ** 2).view(V_TAB, d // 64, 64).sum(-1)))
            if not bool(edge.any()):
                break
            t[edge] *= 1.01
        else:
            raise AssertionError("a table row stays on a power-of-two edge")
    return t.to(G.DEV)


def _ids(G, rows, i64):
    base = [2, 0, V_TAB - 1, 3, 2, 1, 4, 5, 7, 6, 8, 8, 0]
    ids = torch.tensor([base[i % len(base)] for i in range(rows)], dtype=torch.int64 if i64 else torch.int32)
    if rows >= 5:
        assert 0 in ids and V_TAB - 1 in ids and len(set(ids.tolist())) < rows
    return ids.to(G.DEV)


def _embed_ex(G, table, ids, i64, d, nblk, pieces, xb=True, xs=True, entry="xs"):
    """one call of gram_embed_ex_xs / _split / gram_embed_ex -> (x, xb or None, ss, xs or None), tails checked"""
    rows = ids.numel()
    x = _sent(G, (rows + 4, d), torch.float32)
    b = _sent(G, (rows + 4, pieces * d), G.DT) if xb else None
    ss = _sent(G, (rows + 4, nblk), torch.float32)
    f = _sent(G, (rows + 64,), torch.float32) if xs else None
    L = G.lib()
    if entry == "xs":
        rc = L.gram_embed_ex_xs(G.p(table), G.p(ids), int(i64), G.p(x), G.p(b), G.p(ss), G.p(f), nblk, rows, d, pieces, G.stream())
    elif entry == "split":
        assert not xs
        rc = L.gram_embed_ex_split(G.p(table), G.p(ids), int(i64), G.p(x), G.p(b), G.p(ss), nblk, rows, d, pieces, G.stream())
    else:
        assert not xs and pieces == 1
        rc = L.gram_embed_ex(G.p(table), G.p(ids), int(i64), G.p(x), G.p(b), G.p(ss), nblk, rows, d, G.stream())
    _lib.check(rc, "gram_embed_" + entry)
    return (_written(G, x, rows), _written(G, b, rows) if xb else None, _written(G, ss, rows), _written(G, f, rows) if xs else None)


def _pieces(G, v, pieces):
    """the 16-bit copy of fp32 rows as the kernels lay it out: one piece plain, two pieces interleaved"""
    pc = G.pieces_of(v, pieces)
    return _lib.interleave(pc) if pieces == 2 else pc[0]


@pytest.mark.parametrize("d", [128, 512, 768, 1024])
def test_embed_plain(G, d):
    """gram_embed_i64 / gram_embed_i32: x = table[ids] bit for bit, nothing behind it"""
    table = _embed_table(G, d, d)
    for rows in (1, 5, 37):
        for i64 in (True, False):
            ids = _ids(G, rows, i64)
            x = _sent(G, (rows + 4, d), torch.float32)
            fn = G.lib().gram_embed_i64 if i64 else G.lib().gram_embed_i32
            _lib.check(fn(G.p(table), G.p(ids), G.p(x), rows, d, G.stream()), "embed")
            assert _biteq(_written(G, x, rows), table[ids.long()]), (rows, i64)


@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("d", [128, 512, 768, 1024])
def test_embed_ex_blocks_form(G, d, pieces):
    """gram_embed_ex_xs / _split / gram_embed_ex with nblk == d / 64: the fp32 copy, the 64-column partial sums of squares, the row's
    power-of-two factor and the 16-bit copy of x * factor."""
    table = _embed_table(G, d, 100 + d)
    nblk = d // 64
    worst = 0.0
    for rows in (1, 5, 37):
        for i64 in (True, False):
            ids = _ids(G, rows, i64)
            want_x = table[ids.long()]
            x, xb, ss, xs = _embed_ex(G, table, ids, i64, d, nblk, pieces)
            assert _biteq(x, want_x)
            # 4 products and 7 additions of non-negative terms per block: under 8 roundings of 2^-24
            r = _rel_ss(ss, (want_x.double() ** 2).view(rows, nblk, 64).sum(-1))
            worst = max(worst, r)
            assert r <= 1.0, (rows, i64, r)
            # the factor: what gram_row_rscale_xs publishes from the same partials, what the host restatement gives, a power of two
            rs = _sent(G, (rows + 64,), torch.float32)
            xs2 = _sent(G, (rows + 64,), torch.float32)
            _lib.check(G.lib().gram_row_rscale_xs(G.p(ss), G.p(rs), None, G.p(xs2), rows, nblk, d, EPS, G.stream()), "row_rscale_xs")
            assert _biteq(xs, _written(G, xs2, rows)), (rows, i64)
            assert _biteq(xs, _host_row_xscale(ss)), (rows, i64, xs, _host_row_xscale(ss))
            m, _ = torch.frexp(xs.cpu())
            assert bool((m == 0.5).all()) and float(xs.min()) >= 2.0 ** -40 and float(xs.max()) <= 2.0 ** 20
            # the product by a power of two and the residual subtraction are exact: an identity
            assert _biteq(xb, _pieces(G, x * xs[:, None], pieces)), (rows, i64)
            # without xs_out the copy is of x itself
            x1, xb1, ss1, _ = _embed_ex(G, table, ids, i64, d, nblk, pieces, xs=False, entry="split")
            assert _biteq(x1, x) and _biteq(ss1, ss) and _biteq(xb1, _pieces(G, x, pieces)), (rows, i64)
            # xb = NULL: everything else as before
            x2, _, ss2, xs3 = _embed_ex(G, table, ids, i64, d, nblk, pieces, xb=False)
            assert _biteq(x2, x) and _biteq(ss2, ss) and _biteq(xs3, xs), (rows, i64)
            if pieces == 1:
                x4, xb4, ss4, _ = _embed_ex(G, table, ids, i64, d, nblk, 1, xs=False, entry="plain")
                assert _biteq(x4, x1) and _biteq(xb4, xb1) and _biteq(ss4, ss1), (rows, i64)
    print(f"\n[embed_ex blocks] d={d} pieces={pieces}: worst ss error / (1e-6 rel) = {worst:.3f}")


@pytest.mark.parametrize("d,nblk", [(768, 1), (768, 3), (96, 1), (160, 2), (160, 1)])
def test_embed_ex_total_form(G, d, nblk):
    """nblk != d / 64, or a d that is no multiple of 64: the row's total in ss[row][0], exact zeros behind it, the copy unscaled."""
    table = _embed_table(G, d, 200 + d)
    worst = 0.0
    for pieces in (1, 2):
        for rows in (5, 37):
            ids = _ids(G, rows, rows == 5)
            x, xb, ss, _ = _embed_ex(G, table, ids, rows == 5, d, nblk, pieces, xs=False, entry="split")
            assert _biteq(x, table[ids.long()])
            r = _rel_ss(ss[:, 0], (x.double() ** 2).sum(-1))
            worst = max(worst, r)
            assert r <= 1.0, (pieces, rows, r)
            assert _biteq(ss[:, 1:], torch.zeros(rows, nblk - 1, device=G.DEV))
            assert _biteq(xb, _pieces(G, x, pieces))
    print(f"\n[embed_ex total] d={d} nblk={nblk}: worst ss[0] error / (1e-6 rel) = {worst:.3f}")


# ------------------------------------------------------------------------------------ T5LayerNorm
def _norm_inputs(G, rows, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, d, generator=g) * 3.0
    x[:, sorted({1 % d, d // 2, d - 1})] *= 300.0
    if rows > 1:
        x[2 % rows] = 0.0  # its output is the position term alone
    w = 1.0 + 0.1 * torch.randn(d, generator=g)
    return x.to(G.DEV), w.to(G.DEV)


def _norm_call(G, entry, x, w, rows, d, scale, pos, N, L, pmap, pieces):
    out = _sent(G, (rows + 4, pieces * d), G.DT)
    Lb = G.lib()
    if entry == "plain":
        assert pmap is None and pieces == 1
        rc = Lb.gram_rmsnorm_bf16(G.p(x), G.p(w), G.p(out), rows, d, EPS, scale, G.p(pos), N, L, G.stream())
    elif entry == "map":
        assert pieces == 1
        rc = Lb.gram_rmsnorm_bf16_map(G.p(x), G.p(w), G.p(out), rows, d, EPS, scale, G.p(pos), N, L, G.p(pmap), G.stream())
    else:
        rc = Lb.gram_rmsnorm_bf16_split(G.p(x), G.p(w), G.p(out), rows, d, EPS, scale, G.p(pos), N, L, G.p(pmap), pieces, G.stream())
    _lib.check(rc, "gram_rmsnorm_" + entry)
    return _written(G, out, rows)


@pytest.mark.parametrize("pieces,d", [(1, 4), (1, 128), (1, 260), (1, 768), (1, 1020), (1, 1024), (2, 32), (2, 288), (2, 768), (2, 1024)])
def test_rmsnorm_every_form(G, pieces, d):
    """gram_rmsnorm_bf16 / _map / _split against include/gram_hip.h's statement in fp64:
    out = r16(x * rsqrt(mean(x^2) + eps) * w * scale + pos[passage(row) % N]), passage(row) = row / L or passage_map[row / L]."""
    worst = 0.0
    for rows in (1, 5, 26):
        x, w = _norm_inputs(G, rows, d, 1000 * pieces + d + rows)
        x64, w64 = x.double(), w.double()
        normed = x64 * torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + EPS) * w64
        row = torch.arange(rows, device=G.DEV)
        for scale in (1.0, d ** -0.5):
            a = normed * float(torch.tensor(scale, dtype=torch.float32))  # (the kernel takes the scale as a float)
            forms = [(None, 1, 1, None)]
            g = torch.Generator().manual_seed(d + rows)
            for N, L in ((3, 4), (3, 1), (1, 5)):
                forms.append(((0.3 * torch.randn(N, d, generator=g)).to(G.DEV), N, L, None))
            N, L = 3, 4
            n_p = (rows + L - 1) // L
            pm = torch.randint(0, 3 * N, (n_p,), generator=g, dtype=torch.int32)
            pm[0] = 2 * N + 1  # beyond N, and not the passage row / L would give
            if n_p > 1:
                pm[1] = N + 1  # the same passage again, from another user
            forms.append(((0.3 * torch.randn(N, d, generator=g)).to(G.DEV), N, L, pm.to(G.DEV)))
            for pos, N, L, pmap in forms:
                if pos is None:
                    b = torch.zeros_like(a)
                else:
                    psg = row // L if pmap is None else pmap.long()[row // L]
                    b = pos.double()[psg % N]
                out = _norm_call(G, "split", x, w, rows, d, scale, pos, N, L, pmap, pieces)
                if pieces == 2:
                    pc = _lib.deinterleave(out)
                    lo_ok = pc[1].double().abs().cpu() <= 0.5 * spacing16(G, pc[0])
                    assert bool(lo_ok.all()), "the low piece is no residual of the high one"
                    got = G.join_inter(out)
                else:
                    got = out.double()
                r = _ratio16(G, got, a, b, pieces)
                worst = max(worst, r)
                assert r <= 1.0, (rows, scale, N, L, pmap is not None, r)
                if pieces == 1:  # the three entry points, where their arguments coincide
                    assert _biteq(out, _norm_call(G, "map", x, w, rows, d, scale, pos, N, L, pmap, 1))
                    if pmap is None:
                        assert _biteq(out, _norm_call(G, "plain", x, w, rows, d, scale, pos, N, L, None, 1))
                if pos is not None and pmap is None:  # the identity map is no map
                    ident = torch.arange((rows + L - 1) // L, dtype=torch.int32, device=G.DEV)
                    assert _biteq(out, _norm_call(G, "split", x, w, rows, d, scale, pos, N, L, ident, pieces))
    print(f"\n[rmsnorm] d={d} pieces={pieces}: worst error / bound = {worst:.3f}")


# ------------------------------------------------------------------------------------ 1/rms and row factors from the partials
@pytest.mark.parametrize("nblk", [2, 8, 12, 16])
def test_row_rscale(G, nblk):
    """gram_row_rscale / gram_row_rscale_xs on partials spread over 12 decades, with empty blocks and an all-zero row: rs against
    rsqrt(sum / d + eps) / xs_in in fp64, xs_out against the host restatement of the row factor, the entry points against each other."""
    d = 64 * nblk
    worst = 0.0
    for M in (1, 255, 256, 257):
        g = torch.Generator().manual_seed(nblk * 1000 + M)
        ss = torch.pow(10.0, torch.rand(M, 1, generator=g) * 12.0 - 6.0) * (torch.rand(M, nblk, generator=g) + 0.05)
        if M > 1:
            ss[3::7, 1] = 0.0  # rows with an empty block
            ss[5::11, nblk - 1] = 0.0
            ss[M // 2] = 0.0  # an all-zero row
        ss = ss.float()
        for _ in range(8):
            edge = _off_the_edge(_xscale_arg(ss))
            if not bool(edge.any()):
                break
            ss[edge] *= 1.01
        else:
            raise AssertionError("a row stays on a power-of-two edge")
        ss = ss.to(G.DEV)
        xs_in = torch.pow(2.0, torch.randint(-12, 13, (M,), generator=g).float()).to(G.DEV)

        def call(fn_xs, xin, want_xs):
            rs = _sent(G, (M + 64,), torch.float32)
            xo = _sent(G, (M + 64,), torch.float32) if want_xs else None
            if fn_xs:
                rc = G.lib().gram_row_rscale_xs(G.p(ss), G.p(rs), G.p(xin), G.p(xo), M, nblk, d, EPS, G.stream())
            else:
                rc = G.lib().gram_row_rscale(G.p(ss), G.p(rs), M, nblk, d, EPS, G.stream())
            _lib.check(rc, "gram_row_rscale")
            return _written(G, rs, M), _written(G, xo, M) if want_xs else None

        plain, _ = call(False, None, False)
        ref = torch.rsqrt(ss.double().sum(-1) / d + EPS)
        r = float(((plain.double() - ref).abs() / (1e-6 * ref)).max())  # a 1-ulp rsqrt and under 20 additions
        worst = max(worst, r)
        assert r <= 1.0, (M, r)
        same, _ = call(True, None, False)
        assert _biteq(plain, same), M
        rs2, xo = call(True, None, True)
        assert _biteq(plain, rs2) and _biteq(xo, _host_row_xscale(ss)), M
        rs3, xo3 = call(True, xs_in, True)
        assert _biteq(rs3, plain / xs_in) and _biteq(xo3, xo), M  # a power of two: the quotient is exact
        r = float(((rs3.double() - ref / xs_in.double()).abs() / (1e-6 * ref / xs_in.double())).max())
        assert r <= 1.0, (M, r)
    print(f"\n[row_rscale] nblk={nblk}: worst rs error / (1e-6 rel) = {worst:.3f}")


# ------------------------------------------------------------------------------------ log-sum-exp
NEG = float("-inf")


def _logit_rows(V, seed, dead_row):
    """fp32 logits [rows][V], one row per kind: random x 2 | one entry 40 above the rest at column 0, V - 1, the middle | all equal |
    near +-1e4 | -inf in a random 30 % | -inf everywhere but one column | (dead_row) -inf throughout"""
    g = torch.Generator().manual_seed(seed)
    rows = [torch.randn(V, generator=g) * 2.0, torch.randn(V, generator=g) * 5.0 - 3.0]
    for c in (0, V - 1, V // 2):
        r = torch.randn(V, generator=g)
        r[c] = float(r.max()) + 40.0
        rows.append(r)
    rows.append(torch.full((V,), 1.75))
    rows.append(torch.where(torch.rand(V, generator=g) < 0.5, -1.0, 1.0) * 1e4 + torch.randn(V, generator=g))
    r = torch.randn(V, generator=g) * 2.0
    r[torch.rand(V, generator=g) < 0.3] = NEG
    r[(3 * V) // 4] = 0.5  # (never dead, whatever the draw)
    rows.append(r)
    r = torch.full((V,), NEG)
    r[(2 * V) // 3] = -2.5
    rows.append(r)
    if dead_row:
        rows.append(torch.full((V,), NEG))
    return torch.stack(rows).float()


def _chunks(n, R):
    """index lists of R rows each that cover rows 0 .. n-1 (the last one wraps around)"""
    return [[(s + i) % n for i in range(R)] for s in range(0, n, R)]


def _lse_ratio(got, ref):
    """worst |got - ref| / (2e-5 + 1e-6 |ref|) over the finite rows; a row of -inf must be -inf exactly"""
    got, ref = got.double().cpu(), ref.double().cpu()
    dead = ref == NEG
    assert bool((got[dead] == NEG).all()), "a row of -inf throughout must give -inf"
    assert bool(torch.isfinite(got[~dead]).all()), got
    err = ((got - ref).abs() / (2e-5 + 1e-6 * ref.abs()))[~dead]
    return float(err.max()) if err.numel() else 0.0


@pytest.mark.parametrize("V", [4, 1020, 1024, 1028, 32128])
def test_row_lse(G, V):
    """gram_row_lse against the fp64 logsumexp, R rows per launch.  V <= 1024 is one pass of the block (at V = 4 a single thread has
    data), 1028 gives one thread a second pass, 32128 is the vocabulary.  The rows with -inf hold threads that see nothing else:
    their terms are exp(-inf + inf), which must not reach the sum."""
    lg = _logit_rows(V, V, dead_row=True)
    ref = torch.logsumexp(lg.double(), -1)
    dev = lg.to(G.DEV)
    worst = 0.0
    for R in (1, 5):
        for idx in _chunks(lg.shape[0], R):
            part = dev[idx].contiguous()
            lse = _sent(G, (R + 64,), torch.float32)
            _lib.check(G.lib().gram_row_lse(G.p(part), G.p(lse), R, V, G.stream()), "gram_row_lse")
            r = _lse_ratio(_written(G, lse, R), ref[idx])
            worst = max(worst, r)
            assert r <= 1.0, (R, idx, r)
    print(f"\n[row_lse] V={V}: worst error / (2e-5 + 1e-6 |ref|) = {worst:.3f}")


@pytest.mark.parametrize("nblk", [1, 2, 63, 64, 65, 502])
def test_lse_combine(G, nblk):
    """per-64-column partials (max, sum exp(x - max)) built in fp64 from the logits and rounded to fp32 -> the fp64 logsumexp of those
    logits.  Every block keeps a finite maximum, as the lm_head GEMM's do."""
    V = 64 * nblk
    lg = _logit_rows(V, 7000 + nblk, dead_row=False).double()
    lg[:, ::64] = torch.where(torch.isfinite(lg[:, ::64]), lg[:, ::64], torch.full_like(lg[:, ::64], -7.25))
    blk = lg.view(-1, nblk, 64)
    mx = blk.max(-1).values
    assert bool(torch.isfinite(mx).all())
    part = torch.stack([mx, torch.exp(blk - mx[..., None]).sum(-1)], -1).float().to(G.DEV)  # [rows][nblk][2]
    ref = torch.logsumexp(lg, -1)
    worst = 0.0
    for M in (1, 4, 5):
        for idx in _chunks(lg.shape[0], M):
            p = part[idx].contiguous()
            lse = _sent(G, (M + 64,), torch.float32)
            _lib.check(G.lib().gram_lse_combine(G.p(p), G.p(lse), M, nblk, G.stream()), "gram_lse_combine")
            r = _lse_ratio(_written(G, lse, M), ref[idx])
            worst = max(worst, r)
            assert r <= 1.0, (M, idx, r)
    print(f"\n[lse_combine] nblk={nblk}: worst error / (2e-5 + 1e-6 |ref|) = {worst:.3f}")


# ------------------------------------------------------------------------------------ passage cache gather, iota, token repeat
@pytest.mark.parametrize("n,L,cache_L,d", [(1, 32, 32, 128), (5, 128, 96, 768), (3, 64, 128, 1024)])
def test_gather_passage_x(G, n, L, cache_L, d):
    """x[i][l] = cache[slot[i]][l] for l < min(L, cache_L), exact zeros for l >= cache_L, nothing of the cache rows beyond L"""
    n_slots = 4
    g = torch.Generator().manual_seed(n * L + d)
    cache = torch.randn(n_slots, cache_L, d, generator=g).to(G.DEV)
    slot = torch.tensor([3, 1, 3, 0, 1][:n], dtype=torch.int32, device=G.DEV)  # out of order, repeated
    x = _sent(G, (n * L * d + 64,), torch.float32)
    _lib.check(G.lib().gram_gather_passage_x(G.p(cache), G.p(slot), G.p(x), n, L, cache_L, d, G.stream()), "gram_gather_passage_x")
    got = _written(G, x, n * L * d).view(n, L, d)
    want = torch.zeros(n, L, d, device=G.DEV)
    keep = min(L, cache_L)
    want[:, :keep] = cache[slot.long(), :keep]
    assert _biteq(got, want)


@pytest.mark.parametrize("n", [1, 256, 257, 32128])
def test_iota(G, n):
    out = _sent(G, (n + 64,), torch.int32)
    _lib.check(G.lib().gram_iota_i32(G.p(out), n, G.stream()), "gram_iota_i32")
    assert torch.equal(_written(G, out, n), torch.arange(n, dtype=torch.int32, device=G.DEV))


@pytest.mark.parametrize("B,Q", [(1, 1), (3, 255), (2, 257)])
def test_trie_repeat_tokens(G, B, Q):
    tokens = torch.randint(0, 32128, (Q,), generator=torch.Generator().manual_seed(Q), dtype=torch.int32).to(G.DEV)
    out = _sent(G, (B * Q + 64,), torch.int32)
    _lib.check(G.lib().gram_trie_repeat_tokens(G.p(tokens), G.p(out), B, Q, G.stream()), "gram_trie_repeat_tokens")
    assert torch.equal(_written(G, out, B * Q).view(B, Q), tokens[None].expand(B, Q))
