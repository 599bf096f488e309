"""-m gpu: passages of up to 512 tokens -- the tiled encoder self-attention (gram_enc_self_attn_long[_rows]_split) and the whole path
on a model raised by ``GRAM.set_max_passage_len``.

1. The kernel through the C ABI against an fp64 restatement on the kernel's own rounded operands, at L = 160 (a full and a partial key
   tile; the second query block has one live wave), 256 (two full tiles), 288 (two full and a partial) and 512, in both piece modes.
   The reference bias is O.position_bias at the TRUE distances (up to +-511) while the kernel gets the [H][255] table: that is what
   tests the clamp.  Masks: all valid; a valid prefix; valid keys in the first tile only; one valid key in the last 32 positions plus
   scattered holes; nothing valid (the uniform row over exactly L keys).  Tolerances are the project's own for the same roundings
   (tests/test_gpu_split.py::test_split_enc_self_attn at two pieces, tests/test_gpu_kernels.py::test_enc_self_attn at one).
2. Bias and mask alone (q = k = 0: the scores ARE the bias).
3. Bit equalities: the same passages at four padded lengths, one passage alone against five, the table form against the plain form.
4. The whole path against the oracle (fused encoder, generate, score_sequences) and its bit equalities in long mode: a batch against
   each user alone, L = 96 against the same users padded to 256, cold against warm passage cache with harvesting, two long passages
   that share their first 128 tokens, token tables on and off.  The refusals: a default model at L = 160, a config whose buckets are
   not constant beyond +-127."""
import functools
import types

import pytest
import torch

from gram_amd import _lib
from oracle import gram_oracle as O
from tests import test_gpu_path as TP
from tests.test_gpu_configs import ONE, TWO
from tests.test_gpu_path import DEV, SCORE_TOL, _check_generate, _inputs, _random_items
from tests.test_gpu_scale import _rescored
from tests.test_gpu_split import relerr, tol
from tests.test_gpu_teacher_forced import _labels, _tol

pytestmark = pytest.mark.gpu

P_, H_ = 5, 3
SENTINEL = 0x7D7D  # an IEEE-half NaN: no attention output


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
def _masks(L, g):
    """(5, L) bool: all valid | valid prefix | valid keys in the first tile only | one valid key in the last 32 positions plus
    scattered holes | nothing valid"""
    m = torch.zeros(P_, L, dtype=torch.bool)
    m[0] = True
    m[1, : int(torch.randint(1, L, (1,), generator=g))] = True
    n = min(128, L)
    m[2, :n] = torch.rand(n, generator=g) > 0.4
    m[2, 5] = True
    m[3, : L - 32] = torch.rand(L - 32, generator=g) > 0.5
    m[3, L - 32 + int(torch.randint(0, 32, (1,), generator=g))] = True
    return m


def _launch(G, qkv, bias, mask, P, L, H, pieces, ids=None):
    """the long kernel on planar pieces [pieces][rows][3 inner] -> the raw output ([P * L][pieces * inner]), every row checked written"""
    inner = H * 64
    out = torch.full((P * L, pieces * inner), SENTINEL, dtype=torch.int16, device=G.DEV).view(G.DT)
    m8 = mask.to(G.DEV).view(torch.uint8).contiguous()
    lib = G.lib()
    if ids is None:
        rc = lib.gram_enc_self_attn_long_split(G.p(qkv), G.p(bias), G.p(m8), G.p(out), P, L, H, pieces, qkv[0].numel(), G.stream())
    else:
        rc = lib.gram_enc_self_attn_long_rows_split(G.p(qkv), G.p(ids), G.p(bias), G.p(m8), G.p(out), P, L, H, pieces, qkv[0].numel(),
                                                    G.stream())
    _lib.check(rc, "gram_enc_self_attn_long")
    torch.cuda.synchronize()
    assert int((out.view(torch.int16) == SENTINEL).sum()) == 0, "rows left unwritten"
    return out


def _value(G, out, pieces):
    return (G.join_inter(out) if pieces == 2 else out.double()).cpu()


def _reference(x64, table, mask, L, H):
    """fp64 attention of q|k|v rows x64 (P * L, 3 inner) with the bias at the true distances; a masked key scores finfo.min exactly, as
    in the fp32 reference (the bias and q.k are absorbed), so a passage without a valid key gets the uniform row"""
    P = mask.shape[0]
    x = x64.view(P, L, 3, H, 64)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    b = O.position_bias(table, L, L, True, O.OracleConfig(num_heads=H)).double()
    sc = torch.matmul(q, k.transpose(3, 2)) + b
    sc = torch.where(mask[:, None, None, :], sc, torch.full((), float(O.FMIN), dtype=torch.float64))
    return torch.matmul(torch.softmax(sc, -1), v).transpose(1, 2).reshape(P * L, H * 64)


def _operands(G, L, pieces, seed, zero_qk=False):
    from gram_amd.model.gram import relative_position_bucket
    inner = H_ * 64
    g = torch.Generator().manual_seed(seed)
    qkv32 = torch.randn(P_ * L, 3 * inner, generator=g)
    if zero_qk:
        qkv32[:, : 2 * inner] = 0
    table = torch.randn(32, H_, generator=g) * 0.5
    bias = table[relative_position_bucket(torch.arange(-127, 128), True, 32, 128)].t().contiguous().to(G.DEV)
    qkv = G.pieces_of(qkv32.to(G.DEV), pieces)
    return types.SimpleNamespace(qkv=qkv, rounded=G.join(qkv).cpu(), table=table, bias=bias, mask=_masks(L, g))


def _check(G, got, ref, pieces, tag):
    e = relerr(got, ref)
    a = float((got - ref).abs().max())
    print(f"\n[long enc attn {tag}] pieces={pieces}: max err / rms {e:.2e}, max abs {a:.2e}")
    if pieces == 2:
        assert e < 10 * tol(G), e
    else:
        assert torch.allclose(got, ref, atol=2.5e-2, rtol=2e-2), a


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("L", [160, 256, 288, 512])
def test_kernel_against_fp64_on_its_own_operands(G, L, pieces):
    c = _operands(G, L, pieces, seed=L)
    out = _launch(G, c.qkv, c.bias, c.mask, P_, L, H_, pieces)
    _check(G, _value(G, out, pieces), _reference(c.rounded, c.table, c.mask, L, H_), pieces, f"L={L}")


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("L", [160, 512])
def test_bias_and_mask_alone(G, L, pieces):
    """q = k = 0: an index or clamp error cannot hide under q.k noise"""
    c = _operands(G, L, pieces, seed=7 * L, zero_qk=True)
    out = _launch(G, c.qkv, c.bias, c.mask, P_, L, H_, pieces)
    _check(G, _value(G, out, pieces), _reference(c.rounded, c.table, c.mask, L, H_), pieces, f"bias only, L={L}")


def _padded(G, qkv, mask, L0, L):
    """the passages of (qkv [pieces][P * L0][3 inner], mask [P][L0]) padded to L with masked rows of other values"""
    pieces, _, w = qkv.shape
    P = mask.shape[0]
    pad = G.pieces_of(torch.randn(P * (L - L0), w, generator=torch.Generator().manual_seed(L)).to(G.DEV), pieces).view(pieces, P, L - L0, w)
    q = torch.cat([qkv.view(pieces, P, L0, w), pad], 2).reshape(pieces, P * L, w).contiguous()
    return q, torch.nn.functional.pad(mask, (0, L - L0))


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("L0,lengths", [(64, (64, 160, 256, 512)), (160, (160, 256, 512))])
def test_rows_do_not_depend_on_the_padded_length(G, L0, lengths, pieces):
    """The same passages at several padded lengths: the rows below L0 of every passage with a valid key are the same bits (the padding
    holds other values: masked and excluded keys contribute exact zeros).  The passage without a valid key is left out: its row is
    uniform over L."""
    c = _operands(G, L0, pieces, seed=3 * L0)
    mask = c.mask
    rows = []
    for L in lengths:
        q, mk = (c.qkv, mask) if L == L0 else _padded(G, c.qkv, mask, L0, L)
        out = _launch(G, q, c.bias, mk, P_, L, H_, pieces)
        rows.append(out.view(torch.int16).view(P_, L, -1)[: P_ - 1, :L0].cpu())
    for r, L in zip(rows[1:], lengths[1:]):
        assert torch.equal(rows[0], r), (L0, L)


@pytest.mark.parametrize("pieces", [2, 1])
def test_one_passage_alone_and_among_five(G, pieces):
    L = 288
    c = _operands(G, L, pieces, seed=11)
    all5 = _launch(G, c.qkv, c.bias, c.mask, P_, L, H_, pieces).view(torch.int16).view(P_, L, -1).cpu()
    for p in range(P_):
        q1 = c.qkv.view(pieces, P_, L, -1)[:, p].contiguous()
        one = _launch(G, q1, c.bias, c.mask[p:p + 1], 1, L, H_, pieces).view(torch.int16).view(L, -1).cpu()
        assert torch.equal(one, all5[p]), p


@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("L", [160, 512])
def test_table_form_equals_plain_form_on_gathered_rows(G, L, pieces):
    V, inner = 97, H_ * 64
    g = torch.Generator().manual_seed(L + pieces)
    table = G.pieces_of(torch.randn(V, 3 * inner, generator=g).to(G.DEV), pieces)
    ids = torch.randint(0, V, (P_, L), generator=g).to(G.DEV)
    ids[0, :40] = 3  # a token that repeats inside a passage
    c = _operands(G, L, pieces, seed=L)
    gathered = table[:, ids.view(-1)].contiguous()
    plain = _launch(G, gathered, c.bias, c.mask, P_, L, H_, pieces)
    rows = _launch(G, table, c.bias, c.mask, P_, L, H_, pieces, ids=ids.contiguous())
    assert torch.equal(plain.view(torch.int16), rows.view(torch.int16))


def test_the_custom_op_and_its_validation(G):
    """torch.ops.gram.enc_self_attn_long: the entry point's bits, and a malformed tensor raises instead of reaching the C ABI"""
    import gram_amd.ops  # noqa: F401
    L = 160
    c = _operands(G, L, 1, seed=L)
    m8 = c.mask.to(G.DEV).view(torch.uint8).contiguous()
    out = torch.ops.gram.enc_self_attn_long(c.qkv[0], c.bias, m8, H_)
    assert out.shape == (P_ * L, H_ * 64)
    assert torch.equal(out.view(torch.int16), _launch(G, c.qkv, c.bias, c.mask, P_, L, H_, 1).view(torch.int16))
    for args in ((c.qkv[0][:, :256], c.bias, m8, H_), (c.qkv[0], c.bias[:, :200].contiguous(), m8, H_), (c.qkv[0].float(), c.bias, m8, H_),
                 (c.qkv[0], c.bias, m8[:, :144].contiguous(), H_), (c.qkv[0], c.bias, m8.bool(), H_),
                 (torch.zeros(2 * 544, 3 * H_ * 64, dtype=G.DT, device=G.DEV), c.bias, torch.ones(2, 544, dtype=torch.uint8, device=G.DEV), H_)):
        with pytest.raises((ValueError, RuntimeError)):
            torch.ops.gram.enc_self_attn_long(*args)


# ------------------------------------------------------------------------------------------------------------ the whole path
_MODELS = {}


def _model(gpu, name, mode):
    """a backbone of tests/test_gpu_path.py in long mode (one instance per mode)"""
    if (name, mode) not in _MODELS:
        oc, sd, m = TP._model(gpu, name, 11)
        m.set_precision(mode)
        m.set_max_passage_len(256)
        _MODELS[name, mode] = (oc, sd, m)
    return _MODELS[name, mode]


@functools.lru_cache(maxsize=None)
def _case(name, B, N, L):
    """inputs and oracle results of one (backbone, shape), computed once and shared (read only)"""
    oc, _gc = TP._cfgs(name)
    sd = O.init_state_dict(oc, 11)
    g = torch.Generator().manual_seed(B * 1000 + L)
    ids, mask = _inputs(g, B, N, L, min(oc.vocab_size, 32100))
    cands = _random_items(g, 30, 2, 3, 60)
    K = 4
    ref = O.generate(sd, oc, ids, mask, max(len(c) for c in cands), O.prefix_allowed_tokens_fn(O.Trie(cands)), K, K, 1.0)
    return types.SimpleNamespace(ids=ids, mask=mask, cands=cands, K=K, ref=ref, enc_ref=O.encode_fused(sd, oc, ids, mask))


def _fn(cands, _cache={}):
    from gram_amd.utils import generation_trie as gt
    if id(cands) not in _cache:
        _cache[id(cands)] = (cands, gt.prefix_allowed_tokens_fn(gt.Trie(cands)))
    return _cache[id(cands)][1]


def _gen(m, ids, mask, cands, K):
    return TP._gen(m, ids, mask, max(len(c) for c in cands), _fn(cands), K)


WHOLE = [("tiny", 2, 3, 160), ("tiny", 2, 2, 512), ("small", 2, 3, 160), ("small", 2, 2, 512)]


@pytest.mark.parametrize("name,B,N,L", WHOLE)
def test_fused_encoder_vs_oracle(gpu, name, B, N, L):
    """(2, 2, 512) needs the limit at 512: a long-mode model computes the same bits at either setting"""
    oc, sd, m = _model(gpu, name, TWO)
    c = _case(name, B, N, L)
    m.set_max_passage_len(max(256, L))
    try:
        TP._check_encoder(m, c.ids, c.mask, c.enc_ref, f"{name} {B}x{N}x{L}")
    finally:
        m.set_max_passage_len(256)


@pytest.mark.parametrize("mode", [TWO, ONE])
@pytest.mark.parametrize("name,B,N,L", WHOLE)
def test_generate_vs_oracle(gpu, name, B, N, L, mode):
    """Two pieces: the oracle's top-K at SCORE_TOL with tests/test_gpu_path.py's near-tie rule.  One piece: Trie members whose scores
    are the teacher-forced decoder's scores of the same rows (as tests/test_gpu_shapes.py)."""
    oc, sd, m = _model(gpu, name, mode)
    c = _case(name, B, N, L)
    m.set_max_passage_len(max(256, L))
    try:
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
            print(f"[long generate {name} {mode}] max |score - teacher-forced score of the same row| {audit:.2e}")
            assert audit < _tol(mode)["logp"], audit
    finally:
        m.set_max_passage_len(256)


@pytest.mark.parametrize("mode", [TWO, ONE])
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_score_sequences_vs_oracle(gpu, name, mode):
    from tests import tf_oracle as TF
    oc, sd, m = _model(gpu, name, mode)
    c = _case(name, 2, 3, 160)
    B, C, T = 2, 2, 5
    lab = _labels(torch.Generator().manual_seed(5), (B, C, T), min(oc.vocab_size, 32100))
    logits = TF.teacher_forced_logits(sd, oc, c.ids, c.mask, TF.shift_right(lab.view(B * C, T)))
    _, ref_tok = TF.loss_and_token_logp(logits, lab.view(B * C, T))
    seq, tok = m.score_sequences(c.ids.to(DEV), c.mask.to(DEV), lab.to(DEV), return_tokens=True)
    dt = float((tok.cpu().view(B * C, T).double() - ref_tok).abs().max())
    ds = float((seq.cpu().view(-1).double() - ref_tok.sum(-1)).abs().max())
    print(f"[long score_sequences {name} {mode}] token logp {dt:.2e}, sequence sums {ds:.2e}")
    assert dt < _tol(mode)["logp"] and ds < _tol(mode)["logp"] * T, (dt, ds)


# ---- bit for bit, long mode
def _run(m, ids, mask, cands, lab, K=4):
    out = _gen(m, ids, mask, cands, K)
    tok = m.score_sequences(ids.to(DEV), mask.to(DEV), lab.to(DEV), return_tokens=True, users_per_call=ids.shape[0])[1]
    assert bool(torch.isfinite(out["sequences_scores"]).all())
    return out["sequences"].cpu(), out["sequences_scores"].cpu(), tok.cpu()


def _same(a, b):
    return a[0].shape == b[0].shape and all(torch.equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _users(B, N, L, seed=21):
    g = torch.Generator().manual_seed(seed)
    ids, mask = _inputs(g, B, N, L, 250)
    return ids, mask, _random_items(g, 30, 2, 3, 60), _labels(g, (B, 2, 5), 250)


@pytest.mark.parametrize("mode", [TWO, ONE])
def test_a_batch_of_six_and_each_user_alone(gpu, mode):
    m = _model(gpu, "tiny", mode)[2]
    ids, mask, cands, lab = _users(6, 3, 160)
    seqs, scores, tok = _run(m, ids, mask, cands, lab)
    for u in range(6):
        s1, v1, t1 = _run(m, ids[u:u + 1], mask[u:u + 1], cands, lab[u:u + 1])
        w = min(s1.shape[1], seqs.shape[1])  # (a user alone may return fewer columns: the batch's width is its longest hypothesis)
        assert torch.equal(s1[:, :w], seqs[u * 4:(u + 1) * 4, :w]) and not bool(s1[:, w:].any()) and not bool(seqs[u * 4:(u + 1) * 4, w:].any())
        assert torch.equal(v1, scores[u * 4:(u + 1) * 4]) and torch.equal(t1[0], tok[u]), u


@pytest.mark.parametrize("mode", [TWO, ONE])
def test_a_batch_at_96_and_the_same_users_padded_to_256(gpu, mode):
    m = _model(gpu, "tiny", mode)[2]
    ids, mask, cands, lab = _users(3, 3, 96)
    a = _run(m, ids, mask, cands, lab)
    b = _run(m, torch.nn.functional.pad(ids, (0, 160)), torch.nn.functional.pad(mask, (0, 160)), cands, lab)
    assert _same(a, b)


@pytest.mark.parametrize("mode", [TWO, ONE])
def test_cold_model_and_warm_passage_cache_with_harvesting(gpu, mode):
    m = _model(gpu, "tiny", mode)[2]
    ids, mask, cands, lab = _users(3, 3, 160)
    ids, mask = ids.clone(), mask.clone()
    ids[1, 1], mask[1, 1] = ids[0, 2], mask[0, 2]  # an item prompt two users share
    m.clear_passage_cache()
    cold = _run(m, ids, mask, cands, lab)
    try:
        m.set_passage_harvest(True)
        first = _run(m, ids, mask, cands, lab)
        assert m._pcache is not None and m._pcache["n"] > 0 and m._pcache["x"].shape[1] == 256
        warm = _run(m, ids, mask, cands, lab)
    finally:
        m.set_passage_harvest(False)
        m.clear_passage_cache()
    assert _same(cold, first) and _same(cold, warm)


@pytest.mark.parametrize("mode", [TWO, ONE])
def test_two_cached_passages_that_share_their_first_128_tokens(gpu, mode):
    """200-token item prompts X and Y, equal in their first 128 tokens.  With X in the cache, Y must not be taken for it (a cache
    identity cut at 128 tokens would)."""
    m = _model(gpu, "tiny", mode)[2]
    ids, mask, cands, lab = _users(2, 3, 224, seed=22)
    ids, mask = ids.clone(), mask.clone()
    g = torch.Generator().manual_seed(9)
    x = torch.randint(2, 250, (200,), generator=g)
    y = x.clone()
    y[128:] = torch.randint(2, 250, (72,), generator=g)
    for b, row in ((0, x), (1, y)):
        ids[b, 1], mask[b, 1] = 0, False
        ids[b, 1, :200], mask[b, 1, :200] = row, True
    m.clear_passage_cache()
    cold = _run(m, ids, mask, cands, lab)
    assert not torch.equal(cold[1][:4], cold[1][4:])  # (the two users do differ)
    try:
        assert m.cache_passages(ids[0:1, 1].to(DEV), mask[0:1, 1].to(DEV)) == 1
        warm = _run(m, ids, mask, cands, lab)
        assert m.cache_passages(ids[:, 1].to(DEV), mask[:, 1].to(DEV)) == 2  # Y is a passage of its own
        both = _run(m, ids, mask, cands, lab)
    finally:
        m.clear_passage_cache()
    assert _same(cold, warm) and _same(cold, both)


@pytest.mark.parametrize("mode", [TWO, ONE])
def test_token_tables_on_and_off(gpu, mode):
    m = _model(gpu, "tiny", mode)[2]
    assert m._pack() and m._token_tables is not None
    ids, mask, cands, lab = _users(3, 3, 160)
    hook = _lib.load().gram_debug_set_token_tables
    try:
        hook(1)
        on = _run(m, ids, mask, cands, lab)
        hook(0)
        off = _run(m, ids, mask, cands, lab)
    finally:
        hook(-1)
    assert _same(on, off)


# ---- the refusals
def test_a_default_model_refuses_160_tokens_and_names_the_way_out(gpu):
    _oc, _sd, m = TP._model(gpu, "tiny", 11)
    ids, mask, cands, lab = _users(3, 3, 160)
    for call in (lambda: _gen(m, ids, mask, cands, 4), lambda: m.score_sequences(ids.to(DEV), mask.to(DEV), lab.to(DEV)),
                 lambda: m(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), labels=lab[:, 0].to(DEV))):
        with pytest.raises(ValueError, match=r"set_max_passage_len\(160\)"):
            call()
    handle = m._pack()
    assert _lib.load().gram_workspace_bytes(handle, 3, 3, 160, 4, 6) == _lib.E_ARG
    m.set_max_passage_len(160)
    assert _lib.load().gram_workspace_bytes(handle, 3, 3, 160, 4, 6) > 0  # (forwarded to the live handle)
    assert bool(torch.isfinite(_gen(m, ids, mask, cands, 4)["sequences_scores"]).all())


def test_buckets_that_vary_beyond_127_refuse_long_passages(gpu):
    from gram_amd import T5Config
    m = gpu.create_model("gram", T5Config(vocab_size=256, d_model=128, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2,
                                          max_item_num=5, relative_attention_max_distance=256))
    with pytest.raises(ValueError, match="not constant"):
        m.set_max_passage_len(256)
    m.set_max_passage_len(128)
