"""-m gpu: layer 0's q|k|v from per-token tables (include/gram_hip.h, gram_model_build_token_tables).

T5 has no absolute positions, so the first sublayer's q|k|v row of a token is a function of the token id and the weights; a handle
that has the two tables (encoder, decoder) skips layer 0's QKV GEMMs and lets the attention kernels read table rows by token id.
Everything here is a comparison of raw bits (torch.equal): table rows against the embedding -> layer-0 QKV GEMM launches on the same
ids, the row-indexed attention kernels against the plain ones on gathered buffers, and whole generate() calls with the tables
switched on against the same build with them switched off -- the path the rest of the suite holds against the oracle."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
SENT = 0x5A5A  # 16-bit sentinel pattern (a finite number in IEEE half and in bfloat16)


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    return gpu_util


@pytest.fixture(autouse=True)
def _default_switch():
    yield
    from gram_amd import _lib
    _lib.load().gram_debug_set_token_tables(-1)


def _bits(t):
    return t.view(torch.int16)


def _raw32(t):
    return t.view(torch.int32)


_MODELS = {}


def _model(G, pieces, heads=2, tables=True, monkeypatch=None):
    """The tiny model of the path tests (heads = 4: the same with 3 * inner = 768 columns, a shape the ping-pong GEMM takes), packed
    in the one- or two-piece mode.  tables False: a handle packed under GRAM_TOKEN_TABLES=0, which has none."""
    key = (pieces, heads, tables)
    if key not in _MODELS:
        import gram_amd
        from oracle import gram_oracle as O
        kw = dict(vocab_size=256, d_model=128, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=heads, max_item_num=5)
        oc = O.OracleConfig(d_kv=64, **kw)
        m = gram_amd.create_model("gram", gram_amd.T5Config(**kw))
        m.load_state_dict(O.init_state_dict(oc, 11))
        m = m.to(G.DEV).eval()
        m.set_precision(("f16" if G.F16 else "bf16") + ("x3" if pieces == 2 else ""))
        if not tables:
            monkeypatch.setenv("GRAM_TOKEN_TABLES", "0")
        m._pack()
        if not tables:
            monkeypatch.delenv("GRAM_TOKEN_TABLES")
        assert (m._token_tables is not None) == tables
        _MODELS[key] = m
    return _MODELS[key]


def _tables(G, m):
    """(encoder table, decoder table), each a [pieces][V][3 * inner] view of the handle's table memory"""
    c, P = m.config, m._PIECES[m.precision]
    n = P * c.vocab_size * 3 * c.num_heads * 64
    raw = m._token_tables.view(G.DT)
    second = (n + 127) // 128 * 128  # (each table is padded to 256 bytes)
    assert raw.numel() == 2 * second
    shape = (P, c.vocab_size, 3 * c.num_heads * 64)
    return raw[:n].view(shape), raw[second:second + n].view(shape)


def _w_qkv0(G, m, stack):
    """Layer 0's folded QKV weight of a stack as the GEMM reads it, and the GEMM's out_scale: what GRAM._pack hands the library."""
    pre, gain = {"enc": ("encoder.encoder.block.0.module.layer.0.SelfAttention", "encoder.encoder.block.0.module.layer.0.layer_norm.weight"),
                 "dec": ("decoder.block.0.layer.0.SelfAttention", "decoder.block.0.layer.0.layer_norm.weight")}[stack]
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    w = torch.cat([sd[pre + ".q.weight"], sd[pre + ".k.weight"], sd[pre + ".v.weight"]], 0).to(G.DEV, torch.float32)
    w = w * sd[gain].to(G.DEV, torch.float32)[None, :]
    scale = 2.0 ** (13 - math.floor(math.log2(float(w.abs().max())))) if G.F16 else 1.0
    w = w * scale
    return (G.inter(w) if m._PIECES[m.precision] == 2 else w.to(G.DT).contiguous()), 1.0 / scale


def _embed(G, table32, ids, d, pieces):
    """gram_embed_ex_xs on i64 ids -> (xb, ss, xs0)"""
    from gram_amd import _lib
    M = ids.numel()
    x = torch.empty(M, d, dtype=torch.float32, device=G.DEV)
    xb = torch.empty(M, pieces * d, dtype=G.DT, device=G.DEV)
    ss = torch.empty(M, d // 64, dtype=torch.float32, device=G.DEV)
    xs0 = torch.empty(M, dtype=torch.float32, device=G.DEV)
    _lib.check(G.lib().gram_embed_ex_xs(G.p(table32), G.p(ids), 1, G.p(x), G.p(xb), G.p(ss), G.p(xs0), d // 64, M, d, pieces, G.stream()),
               "embed")
    return xb, ss, xs0


def _qkv_gemm(G, xb, ss, xs0, W, out_scale, d, pieces, eps, xs_out=None):
    """The layer-0 QKV GEMM as generate.hip launches it on M rows: below 32 768 rows the GEMM adds the partials up itself and
    publishes the next row factor, from there on gram_row_rscale_xs runs in front.  Returns the planar output [pieces][M][N]."""
    from gram_amd import _lib
    M, N = xb.shape[0], W.shape[0]
    out = torch.empty(pieces, M, N, dtype=G.DT, device=G.DEV)
    xs1 = xs_out if xs_out is not None else torch.empty(M, dtype=torch.float32, device=G.DEV)
    if M >= 32768:
        rs = torch.empty(M, dtype=torch.float32, device=G.DEV)
        _lib.check(G.lib().gram_row_rscale_xs(G.p(ss), G.p(rs), G.p(xs0), G.p(xs1), M, d // 64, d, eps, G.stream()), "row_rscale_xs")
        nf = _lib.NormFusion(None, None, rs.data_ptr(), 0, d, eps)
    else:
        nf = _lib.NormFusion(None, None, ss.data_ptr(), d // 64, d, eps, 0, xs0.data_ptr(), xs1.data_ptr())
    sp = _lib.Split(pieces, 0, M * N, 0, out_scale)
    _lib.check(G.lib().gram_gemm_bf16_split(G.p(xb), G.p(W), G.p(out), M, N, d, pieces * d, N, _lib.EPI_BF16, None, C.byref(nf), C.byref(sp),
                                            G.stream()), "qkv gemm")
    return out


# ------------------------------------------------------------------------------------ 1. the table rows
@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("heads,m_big", [(2, 32768), (4, 65536)])
def test_table_rows_equal_the_gemm_path(G, heads, m_big, pieces):
    """64 token ids (0, 1 and V - 1 among them): their table rows are the planar output of gram_embed_ex_xs -> layer-0 QKV GEMM on
    those ids as a 64-row batch, and as rows scattered inside a batch of m_big >= 32 768 rows -- the side of the dispatch where
    gram_row_rscale_xs computes 1/rms in front of the GEMM (heads = 4, 65 536 rows, two pieces: the ping-pong kernel)."""
    m = _model(G, pieces, heads)
    c = m.config
    V, d, eps = c.vocab_size, c.d_model, float(c.layer_norm_epsilon)
    emb = m.state_dict()["shared.weight"].detach().to(G.DEV, torch.float32).contiguous()
    g = torch.Generator().manual_seed(17 + heads + pieces)
    ids = torch.cat([torch.tensor([0, 1, V - 1]), 2 + torch.randperm(V - 3, generator=g)[:61]]).to(G.DEV)
    big = torch.randint(0, V, (m_big,), generator=g).to(G.DEV)
    pos = torch.randperm(m_big, generator=g)[:64].to(G.DEV)
    big[pos] = ids
    for stack, table in zip(("enc", "dec"), _tables(G, m)):
        W, out_scale = _w_qkv0(G, m, stack)
        small = _qkv_gemm(G, *_embed(G, emb, ids, d, pieces), W, out_scale, d, pieces, eps)
        large = _qkv_gemm(G, *_embed(G, emb, big, d, pieces), W, out_scale, d, pieces, eps)
        torch.cuda.synchronize()
        assert torch.equal(_bits(table[:, ids]), _bits(small)), stack
        assert torch.equal(_bits(table[:, ids]), _bits(large[:, pos])), stack
        assert torch.equal(_bits(table[:, big]), _bits(large)), stack  # (and every other row of the big batch)


# ------------------------------------------------------------------------------------ 2. the published row factor
@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("rows", ["8", "past the streaming GEMM"])
def test_row_rscale_publishes_the_consumer_gemms_factor(G, rows, pieces):
    """Where a table stands in for the layer-0 QKV GEMM on the small path, gram_row_rscale_xs publishes the next producer's row factor
    in its place: the same bits the GEMM publishes, from the embedding's 64-column partials.  8 rows (the streaming GEMM), one of them
    scaled to ~3e5; and the same tokens repeated past the streaming GEMM's row limit (the tile kernels)."""
    from gram_amd import _lib
    m = _model(G, pieces)
    c = m.config
    V, d, eps = c.vocab_size, c.d_model, float(c.layer_norm_epsilon)
    emb = m.state_dict()["shared.weight"].detach().to(G.DEV, torch.float32).clone()
    emb[7] *= 3.0e5 / float(emb[7].abs().max())
    M = 8 if rows == "8" else G.lib().gram_gemm_stream_max_m() + 8
    ids = torch.tensor([0, 1, V - 1, 7, 100, 7, 33, 200], device=G.DEV).repeat((M + 7) // 8)[:M].contiguous()
    xb, ss, xs0 = _embed(G, emb, ids, d, pieces)
    W, out_scale = _w_qkv0(G, m, "enc")
    by_gemm = torch.zeros(M, dtype=torch.float32, device=G.DEV)
    _qkv_gemm(G, xb, ss, xs0, W, out_scale, d, pieces, eps, xs_out=by_gemm)
    by_kernel = torch.zeros(M, dtype=torch.float32, device=G.DEV)
    rs = torch.empty(M, dtype=torch.float32, device=G.DEV)
    _lib.check(G.lib().gram_row_rscale_xs(G.p(ss), G.p(rs), G.p(xs0), G.p(by_kernel), M, d // 64, d, eps, G.stream()), "row_rscale_xs")
    torch.cuda.synchronize()
    assert torch.equal(_raw32(by_kernel), _raw32(by_gemm))
    assert float(by_kernel[3]) < float(by_kernel[0]) and bool((by_kernel > 0).all())  # (the large row carries a smaller factor)


# ------------------------------------------------------------------------------------ 3. encoder attention by token id
@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("P,L", [(1, 32), (3, 32), (1, 128), (3, 128)])
def test_enc_attn_rows_matches_the_plain_kernel_on_gathered_rows(G, P, L, pieces):
    """gram_enc_self_attn_rows_split on a table against gram_enc_self_attn_split on the gathered buffer: ids that repeat inside a
    passage, the id V - 1, a masked tail of pad ids, and (P = 3) an all-masked passage."""
    from gram_amd import _lib
    H, V = 2, 256
    inner = H * 64
    g = torch.Generator().manual_seed(1000 * P + L + pieces)
    table = G.pieces_of((torch.randn(V, 3 * inner, generator=g) * 0.5).to(G.DEV), pieces)
    bias = (torch.randn(H, 255, generator=g) * 0.5).to(G.DEV)
    ids = torch.randint(2, 40, (P, L), generator=g)  # (38 values for 32 .. 128 positions: repeats)
    ids[:, 3] = V - 1
    ids[:, 5] = ids[:, 4]
    mask = torch.ones(P, L, dtype=torch.uint8)
    tail = L - L // 4
    ids[0, tail:], mask[0, tail:] = 0, 0
    if P == 3:
        ids[1], mask[1] = 0, 0
    ids, mask = ids.to(G.DEV), mask.to(G.DEV)
    gathered = table[:, ids.flatten()].contiguous()
    out = torch.empty(2, P * L, pieces * inner, dtype=G.DT, device=G.DEV)
    _bits(out).fill_(SENT)
    L_ = G.lib()
    _lib.check(L_.gram_enc_self_attn_split(G.p(gathered), G.p(bias), G.p(mask), G.p(out[0]), P, L, H, pieces, gathered[0].numel(), G.stream()),
               "enc_attn")
    _lib.check(L_.gram_enc_self_attn_rows_split(G.p(table), G.p(ids), G.p(bias), G.p(mask), G.p(out[1]), P, L, H, pieces, table[0].numel(),
                                                G.stream()), "enc_attn rows")
    torch.cuda.synchronize()
    assert not bool((_bits(out[0]) == SENT).all(dim=1).any())  # (every row was written)
    assert torch.equal(_bits(out[1]), _bits(out[0]))


# ------------------------------------------------------------------------------------ 4. decoder self-attention by token id
@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("live", [False, True])
@pytest.mark.parametrize("t", [0, 3])
def test_dec_self_attn_rows_matches_the_plain_kernel_on_gathered_rows(G, t, live, pieces):
    """gram_dec_self_attn_rows_split against gram_dec_self_attn_split on the gathered rows, R = 7 cache rows: all rows (rows NULL) and
    a live subset of 3 rows whose tokens repeat; output and both caches equal afterwards."""
    from gram_amd import _lib
    H, V, R, Tmax = 3, 256, 7, 8
    inner = H * 64
    g = torch.Generator().manual_seed(10 * t + 2 * pieces + live)
    table = G.pieces_of((torch.randn(V, 3 * inner, generator=g) * 0.5).to(G.DEV), pieces)
    bias = (torch.randn(H, _lib.GRAM_MAX_DEC_LEN, generator=g) * 0.5).to(G.DEV)
    anc = torch.randint(0, R, (Tmax, R), generator=g).to(torch.int32).to(G.DEV)
    caches = [G.bf(torch.randn(pieces, Tmax, R, inner, generator=g)) for _ in range(2)]
    kc, vc = [torch.stack([c, c.clone()]) for c in caches]  # [0]: the plain kernel's, [1]: the row-indexed kernel's
    if live:
        rows = torch.tensor([1, 4, 6], dtype=torch.int32, device=G.DEV)
        tokens = torch.tensor([5, 5, V - 1], dtype=torch.int32, device=G.DEV)
    else:
        rows = None
        tokens = torch.tensor([9, 0, 9, 1, V - 1, 77, 9], dtype=torch.int32, device=G.DEV)
    n = tokens.numel()
    gathered = table[:, tokens.long()].contiguous()
    out = torch.empty(2, R, pieces * inner, dtype=G.DT, device=G.DEV)
    _bits(out).fill_(SENT)
    L_ = G.lib()
    _lib.check(L_.gram_dec_self_attn_split(G.p(gathered), G.p(kc[0]), G.p(vc[0]), G.p(anc), G.p(bias), G.p(out[0]), R, n, G.p(rows), H, t,
                                           Tmax, pieces, gathered[0].numel(), kc[0, 0].numel(), G.stream()), "dec_attn")
    _lib.check(L_.gram_dec_self_attn_rows_split(G.p(table), G.p(tokens), G.p(kc[1]), G.p(vc[1]), G.p(anc), G.p(bias), G.p(out[1]), R, n,
                                                G.p(rows), H, t, Tmax, pieces, table[0].numel(), kc[0, 0].numel(), G.stream()),
               "dec_attn rows")
    torch.cuda.synchronize()
    assert not bool((_bits(out[0, :n]) == SENT).all(dim=1).any()) and bool((_bits(out[0, n:]) == SENT).all())
    assert torch.equal(_bits(out[1]), _bits(out[0]))
    assert torch.equal(_bits(kc[1]), _bits(kc[0])) and torch.equal(_bits(vc[1]), _bits(vc[0]))
    assert not torch.equal(_bits(kc[0]), _bits(caches[0]))  # (slot t was written)


# ------------------------------------------------------------------------------------ 5. the whole path
def _inputs(g, B, N, L, V, pad_passage):
    ids = torch.randint(2, V, (B, N, L), generator=g)
    mask = torch.ones(B, N, L, dtype=torch.bool)
    for b in range(B):
        for n in range(N):
            ln = int(torch.randint(max(2, L // 3), L + 1, (1,), generator=g))
            mask[b, n, ln:] = False
            ids[b, n, ln - 1] = 1
            ids[b, n, ln:] = 0
    if pad_passage:  # one fully padded passage: the encoder runs on the compacted batch (gram_compaction_t)
        mask[B - 1, N - 1] = False
        ids[B - 1, N - 1] = 0
    return ids, mask


def _generate(G, m, ids, mask, cands, K):
    from gram_amd.utils import generation_trie as gt
    fn = _generate.fns.setdefault(id(m), gt.prefix_allowed_tokens_fn(gt.Trie(cands)))
    out = m.generate(input_ids=ids.to(G.DEV), attention_mask=mask.to(G.DEV), max_length=max(len(c) for c in cands),
                     prefix_allowed_tokens_fn=fn, num_beams=K, num_return_sequences=K, length_penalty=1.0)
    scores = out["sequences_scores"]
    return out["sequences"].cpu(), None if scores is None else scores.cpu()


_generate.fns = {}


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("case,B,N,L,K,pad_passage", [("ragged Trie, live-row steps", 3, 2, 64, 4, False),
                                                      ("compacted encoder batch", 3, 2, 64, 4, True),
                                                      ("32 768 encoder rows", 128, 2, 128, 4, False),
                                                      ("greedy", 3, 2, 64, 1, False)])
def test_generate_is_bit_identical_with_and_without_the_tables(G, case, B, N, L, K, pad_passage, pieces):
    from tests.test_gpu_kernels import _tries
    m = _model(G, pieces)
    cands = _tries()["ragged"]
    ids, mask = _inputs(torch.Generator().manual_seed(5 + B + K), B, N, L, m.config.vocab_size, pad_passage)
    lib = G.lib()
    lib.gram_debug_set_token_tables(1)
    seq_on, sc_on = _generate(G, m, ids, mask, cands, K)
    lib.gram_debug_set_token_tables(0)
    seq_off, sc_off = _generate(G, m, ids, mask, cands, K)
    assert torch.equal(seq_on, seq_off), case
    if K > 1:
        assert torch.equal(_raw32(sc_on), _raw32(sc_off)), case
        assert bool(torch.isfinite(sc_on).all())
    else:
        assert sc_on is None and sc_off is None


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("P,L", [(5, 64), (256, 128)])
def test_encode_passages_is_bit_identical_with_and_without_the_tables(G, P, L, pieces):
    """gram_encode_passages (the passage-cache prefill) on 320 and on 32 768 rows"""
    from gram_amd import _lib
    m = _model(G, pieces)
    handle = m._pack()
    d = m.config.d_model
    ids, mask = _inputs(torch.Generator().manual_seed(P), P, 1, L, m.config.vocab_size, False)
    ids, mask = ids.view(P, L).to(G.DEV).contiguous(), mask.view(P, L).to(G.DEV).view(torch.uint8).contiguous()
    ws = m._get_workspace(handle, P, 1, L, 1, 2)
    x = torch.zeros(2, P, L, d, dtype=torch.float32, device=G.DEV)
    for on in (1, 0):
        G.lib().gram_debug_set_token_tables(on)
        _lib.check(G.lib().gram_encode_passages(handle, G.p(ids), G.p(mask), P, L, G.p(ws), ws.numel(), G.p(x[on]), G.stream()), "encode_passages")
    torch.cuda.synchronize()
    assert torch.equal(_raw32(x[1]), _raw32(x[0])) and bool(torch.isfinite(x[0]).all()) and bool((x[0] != 0).any())


# ------------------------------------------------------------------------------------ 6. launch counts
def _launch_counts(G, m, ids, mask, cands, K):
    """launches per kernel kind (gram_prof) of one generate()"""
    from gram_amd import _lib
    lib = G.lib()
    _lib.check(lib.gram_prof_enable((1 << 7) - 1, 4096), "prof")
    try:
        _generate(G, m, ids, mask, cands, K)
        counts = []
        for kind in range(7):
            ms, n, work, dropped = C.c_double(0), C.c_int64(0), C.c_double(0), C.c_int64(0)
            _lib.check(lib.gram_prof_collect(kind, C.byref(ms), C.byref(n), C.byref(work), C.byref(dropped)), "collect")
            assert dropped.value == 0
            counts.append(n.value)
    finally:
        lib.gram_prof_enable(0, 0)
    return counts


@pytest.mark.parametrize("pieces", [2, 1])
def test_without_tables_the_launch_sequence_is_the_one_with_the_gemms(G, pieces, monkeypatch):
    """A handle without tables, the switch off, and GRAM_TOKEN_TABLES=0 all launch the same kernels per kind: every sublayer's two
    GEMMs, the bank GEMM per encode and the lm_head per decode step.  With the tables one GEMM per encode and per decode step is gone
    and -- these are small batches, where that GEMM published the next row factor -- one gram_row_rscale_xs has taken its place."""
    from gram_amd import _lib
    from tests.test_gpu_kernels import _tries
    cands = _tries()["ragged"]
    B, N, L, K = 3, 2, 64, 4
    with_tables, without = _model(G, pieces), _model(G, pieces, tables=False, monkeypatch=monkeypatch)
    ids, mask = _inputs(torch.Generator().manual_seed(12), B, N, L, 256, False)
    lib = G.lib()
    lib.gram_debug_set_token_tables(-1)
    no_tables = _launch_counts(G, without, ids, mask, cands, K)
    lib.gram_debug_set_token_tables(0)
    switched_off = _launch_counts(G, with_tables, ids, mask, cands, K)
    lib.gram_debug_set_token_tables(-1)
    monkeypatch.setenv("GRAM_TOKEN_TABLES", "0")
    by_env = _launch_counts(G, with_tables, ids, mask, cands, K)
    monkeypatch.delenv("GRAM_TOKEN_TABLES")
    on = _launch_counts(G, with_tables, ids, mask, cands, K)
    assert no_tables == switched_off == by_env
    ne, nd = with_tables._n_enc, with_tables._n_dec
    steps, rest = divmod(no_tables[_lib.K_DEC_SELF_ATTN], nd)
    assert rest == 0 and steps >= 3
    assert no_tables[_lib.K_GEMM] == (4 * ne + 1) + steps * (6 * nd + 1)
    assert no_tables[_lib.K_ENC_ATTN] == ne
    want = list(no_tables)
    want[_lib.K_GEMM] -= 1 + steps
    want[_lib.K_ROWOPS] += 1 + steps
    assert on == want
