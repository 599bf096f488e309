"""The ``gram::`` PyTorch custom ops (gram_amd/ops.py): registered with schemas and meta implementations on any host; their
kernels exist for the ROCm device only -- a CPU tensor must fail loudly (no CPU path).  -m gpu: values through torch.ops."""
import pytest
import torch

import gram_amd  # noqa: F401
from gram_amd import _lib, ops  # noqa: F401

DT = _lib.piece_dtype()  # the loaded library's 16-bit operand type (float16; bfloat16 for the PIECE=bf16 build)


def test_ops_are_registered_with_fake_impls():
    for name in ("generate", "linear", "enc_self_attn", "cross_attn_decode", "trie_step"):
        assert hasattr(torch.ops.gram, name), name
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        a = torch.empty(20, 768, dtype=DT, device="cuda")
        w = torch.empty(2304, 768, dtype=DT, device="cuda")
        assert torch.ops.gram.linear(a, w).shape == (20, 2304)
        q = torch.empty(40, 768, dtype=DT, device="cuda")
        kb = torch.empty(2, 12, 384, 64, dtype=DT, device="cuda")
        vt = torch.empty(2, 12, 384 // 32, 64, 32, dtype=DT, device="cuda")
        mk = torch.empty(2, 384, dtype=torch.uint8, device="cuda")
        assert torch.ops.gram.cross_attn_decode(q, kb, vt, mk, 20).shape == (40, 768)
        ids = torch.empty(3, 2, 32, dtype=torch.int64, device="cuda")
        ws = torch.empty(1024, dtype=torch.uint8, device="cuda")
        t = torch.empty(8, dtype=torch.int32, device="cuda")
        s, sc, wd = torch.ops.gram.generate(ids, ids.to(torch.uint8), 0, ws, t, t, t, 4, 3, 5, 5, 7, 1.0, None, None, None, None, None, 0, 0)
        assert s.shape == (15, 7) and sc.shape == (15,) and wd.shape == (1,)


def test_no_cpu_kernels():
    a = torch.zeros(16, 64, dtype=DT)
    w = torch.zeros(128, 64, dtype=DT)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.gram.linear(a, w)


@pytest.mark.gpu
def test_ops_values_on_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import gram_oracle as O
    g = torch.Generator().manual_seed(4)
    a = torch.randn(77, 256, generator=g).to(DT).cuda()
    w = (torch.randn(384, 256, generator=g) / 16).to(DT).cuda()
    ref = a.float() @ w.float().T
    assert torch.allclose(torch.ops.gram.linear(a, w).float(), ref, atol=2e-2, rtol=1e-2)
    assert torch.allclose(torch.ops.gram.linear(a, w, True).float(), ref.clamp(min=0), atol=2e-2, rtol=1e-2)
    B, H, K, S = 2, 2, 5, 96
    q = (torch.randn(B * K, H * 64, generator=g) * 0.3).to(DT).cuda()
    kb = torch.randn(B, H, S, 64, generator=g).to(DT).cuda()
    v_t = torch.randn(B, H, 64, S, generator=g).to(DT)
    vt = v_t.unflatten(-1, (S // 32, 32)).transpose(-3, -2).contiguous().cuda()  # the bank's V^T, blocked by 32 keys
    mask = torch.rand(B, S, generator=g) > 0.3
    out = torch.ops.gram.cross_attn_decode(q, kb, vt, mask.cuda().view(torch.uint8).contiguous(), K)
    qh = q.float().cpu().view(B, K, H, 64).permute(0, 2, 1, 3)
    ext = ((1.0 - mask.float()) * O.FMIN)[:, None, None, :]
    ref = O._attend(qh, kb.float().cpu(), v_t.float().transpose(2, 3), ext).reshape(B * K, H * 64)
    assert torch.allclose(out.float().cpu(), ref, atol=1e-2, rtol=1e-2)


@pytest.mark.gpu
def test_ops_refuse_malformed_tensors():
    """The ops take raw data_ptr()s into the C ABI: a wrong dtype, a transposed or sliced view, a layout that is not the documented
    one or inconsistent shapes must raise instead of reading garbage or past the allocation."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    a = torch.zeros(32, 256, dtype=DT, device="cuda")
    w = torch.zeros(384, 256, dtype=DT, device="cuda")
    assert torch.ops.gram.linear(a, w).shape == (32, 384)
    assert torch.ops.gram.linear(torch.zeros(32, 512, dtype=DT, device="cuda")[:, :256], w).shape == (32, 384)  # row-strided A is fine
    for bad_a, bad_w in ((a.float(), w), (a, w.float()), (a.t().contiguous().t(), w), (a, torch.zeros(256, 384, dtype=DT, device="cuda").t()),
                         (a[:, ::2], w[:, ::2]), (a, w[:, :128]), (a[:, 1:65], w[:, :64]), (a, torch.zeros(100, 256, dtype=DT, device="cuda"))):
        with pytest.raises((ValueError, RuntimeError)):
            torch.ops.gram.linear(bad_a, bad_w)
    B, H, K, S = 2, 2, 5, 96
    q = torch.zeros(B * K, H * 64, dtype=DT, device="cuda")
    kb = torch.zeros(B, H, S, 64, dtype=DT, device="cuda")
    vt = torch.zeros(B, H, S // 32, 64, 32, dtype=DT, device="cuda")
    mk = torch.ones(B, S, dtype=torch.uint8, device="cuda")
    assert torch.ops.gram.cross_attn_decode(q, kb, vt, mk, K).shape == q.shape
    for args in ((q, kb, torch.zeros(B, H, 64, S, dtype=DT, device="cuda"), mk, K),      # plain [64][S] V^T, not blocked by 32 keys
                 (q[:-1], kb, vt, mk, K), (q, kb, vt, mk[:, :64].contiguous(), K), (q.float(), kb, vt, mk, K),
                 (q, kb.transpose(1, 2), vt, mk, K), (q, kb, vt, mk.bool(), K), (q, kb, vt, mk, 65)):
        with pytest.raises((ValueError, RuntimeError)):
            torch.ops.gram.cross_attn_decode(*args)
    qkv = torch.zeros(2 * 32, 3 * 128, dtype=DT, device="cuda")
    bias = torch.zeros(2, 255, device="cuda")
    m2 = torch.ones(2, 32, dtype=torch.uint8, device="cuda")
    assert torch.ops.gram.enc_self_attn(qkv, bias, m2, 2).shape == (64, 128)
    for args in ((qkv[:, :256], bias, m2, 2), (qkv, bias[:, :200].contiguous(), m2, 2), (qkv, bias, torch.ones(2, 48, dtype=torch.uint8, device="cuda"), 2)):
        with pytest.raises((ValueError, RuntimeError)):
            torch.ops.gram.enc_self_attn(*args)


@pytest.mark.gpu
def test_whole_path_ops_refuse_before_they_launch():
    """teacher_forced, teacher_forced_attn, teacher_forced_scores, score_trie and generate_items with one malformed argument at a
    time, at the smallest shapes and on ``handle = 0``: each must be refused in Python, as a ``ValueError``.  A call that slips past
    the Python checks reaches the C ABI, which answers a null handle with GRAM_E_ARG -- a ``GramHipError``, a ``RuntimeError`` -- so
    it fails here; the well-formed teacher-forced and score_trie calls show exactly that (no launch either: the C side refuses
    first).  Nothing runs on the device but the min / max reductions of the range checks."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    i32, i64, u8 = torch.int32, torch.int64, torch.uint8

    def dev(data, dtype=i32):
        return torch.tensor(data, dtype=dtype, device="cuda")

    def put(t, index, v):
        t = t.clone()
        t[index] = v
        return t

    V, L = 16, 32
    nocomp = (None, None, None, None, None, 0, 0)
    base = dict(input_ids=torch.zeros(1, 1, L, dtype=i64, device="cuda"), attention_mask=torch.ones(1, 1, L, dtype=u8, device="cuda"),
                handle=0, workspace=torch.zeros(1024, dtype=u8, device="cuda"))
    wide = torch.ones(1, 1, 2 * L, dtype=u8, device="cuda")
    bad_inputs = [dict(input_ids=base["input_ids"].to(i32)), dict(input_ids=torch.zeros(1, 1, 2 * L, dtype=i64, device="cuda")[:, :, ::2]),
                  dict(attention_mask=base["attention_mask"].bool()), dict(attention_mask=wide), dict(attention_mask=wide[:, :, ::2]),
                  dict(attention_mask=wide[:, :, 1:L + 1])]

    def refused(op, order, good, bads):
        for bad in bads:
            args = dict(good, **bad)
            with pytest.raises(ValueError):
                op(*(args[k] for k in order), *nocomp)
            assert sorted(args) == sorted(order)

    # ---- the three teacher-forced ops: B = 1, N = 1, L = 32, C = 1, T = 2
    dec, lab = dev([[[0, V - 1]]]), dev([[[V - 1, -100]]])
    tf = dict(base, decoder_input_ids=dec, labels=lab, vocab_size=V)
    long_T = torch.zeros(1, 1, _lib.GRAM_MAX_DEC_LEN + 1, dtype=i32, device="cuda")
    bad_tf = bad_inputs + [
        dict(decoder_input_ids=dec.to(i64)), dict(labels=lab.to(i64)), dict(labels=lab.float()),
        dict(decoder_input_ids=dev([[[0, 9, 1, 9]]])[:, :, ::2]), dict(labels=dev([[[0, 9, 1, 9]]])[:, :, ::2]),
        dict(decoder_input_ids=dev([[[9, 0, 1]]])[:, :, 1:]), dict(labels=dev([[[9, 0, 1]]])[:, :, 1:]),      # (not 16-byte aligned)
        dict(labels=dev([[[1, 2, 3]]])), dict(labels=dev([[[1, 2]], [[1, 2]]])), dict(labels=lab[0]), dict(decoder_input_ids=dec[0]),
        dict(decoder_input_ids=dec[:, :, :0], labels=lab[:, :, :0]), dict(decoder_input_ids=long_T, labels=long_T),
        dict(decoder_input_ids=put(dec, (0, 0, 1), -1)), dict(decoder_input_ids=put(dec, (0, 0, 0), V)), dict(labels=put(lab, (0, 0, 1), V)),
        dict(input_ids=base["input_ids"].cpu()), dict(labels=lab.cpu())]
    head = ("input_ids", "attention_mask", "handle", "workspace", "decoder_input_ids", "labels", "vocab_size")
    for op, extra, more in ((torch.ops.gram.teacher_forced, dict(want_logits=False), []),
                            (torch.ops.gram.teacher_forced_attn, dict(n_dec_layers=2, n_heads=2, want_probs=False, want_scores=True),
                             [dict(n_dec_layers=0), dict(n_heads=0), dict(want_scores=False)]),
                            (torch.ops.gram.teacher_forced_scores, {}, [])):
        good, order = dict(tf, **extra), head + tuple(extra)
        refused(op, order, good, bad_tf + more)
        with pytest.raises(_lib.GramHipError):  # well-formed: past the Python checks, refused by the C ABI for its null handle
            op(*(good[k] for k in order), *nocomp)

    # ---- a Trie of three nodes: root -5-> node 1 -1-> leaf 2 (one item); rows for the two internal nodes
    trie = dict(trie_child_off=dev([0, 1, 2, 2]), trie_child_tok=dev([5, 1]), trie_child_node=dev([1, 2]), trie_max_fanout=1,
                trie_min_seq_len=3)
    rows = dict(row_tokens=dev([0, 5]), row_pos=dev([0, 1]), row_anc=dev([[0, 0], [0, 1]]), row_node=dev([0, 1]), node_row=dev([0, 1, -1]),
                node_tok=dev([-1, 5, 1]), node_leaf=dev([-1, -1, 0]), n_leaves=1, vocab_size=V, want_nodes=True)
    good = dict(base, **trie, **rows)
    order = tuple(base) + tuple(trie) + tuple(rows)
    bad_rows = bad_inputs + [
        dict(row_tokens=rows["row_tokens"].to(i64)), dict(node_leaf=rows["node_leaf"].float()), dict(trie_child_off=trie["trie_child_off"].to(i64)),
        dict(row_anc=rows["row_anc"].t()), dict(row_anc=rows["row_anc"][0]), dict(row_pos=dev([0, 9, 1, 9])[::2]),
        dict(row_node=dev([9, 0, 1])[1:]), dict(node_row=dev([0, 1, -1, -1])), dict(node_tok=dev([-1, 5])), dict(row_tokens=dev([0, 5, 1])),
        dict(trie_child_node=dev([1, 2, 2])), dict(trie_child_off=dev([0, 1, 2])), dict(n_leaves=0), dict(n_leaves=3),
        dict(row_tokens=dev([0, V])), dict(row_tokens=dev([-1, 5])), dict(row_pos=dev([0, 2])), dict(row_pos=dev([-1, 1])),
        dict(row_anc=dev([[0, 0], [0, 2]])), dict(row_anc=dev([[0, -1], [0, 1]])), dict(row_node=dev([0, 3])), dict(row_node=dev([-1, 1])),
        dict(node_row=dev([0, 2, -1])), dict(node_row=dev([0, 1, -2])), dict(node_tok=dev([-1, V, 1])), dict(node_tok=dev([-2, 5, 1])),
        dict(node_leaf=dev([-1, -1, 1])), dict(node_leaf=dev([-2, -1, 0])), dict(node_leaf=rows["node_leaf"].cpu())]
    refused(torch.ops.gram.score_trie, order, good, bad_rows)
    with pytest.raises(_lib.GramHipError):
        torch.ops.gram.score_trie(*(good[k] for k in order), *nocomp)

    # ---- generate_items: one candidate (n_items = 1), M = 2 list entries (the well-formed call would prepare the lists on the device
    #      before the C ABI sees the handle, so it is not made here)
    search = dict(num_beams=2, num_return_sequences=2, max_length=3, length_penalty=1.0)
    filt = dict(leaf_lo=dev([0, 0, 0]), leaf_hi=dev([1, 1, 1]), item_rank=dev([0]), items=dev([[0, -1]]), allow=False)
    comp = dict(zip(("comp_map", "comp_ids", "comp_mask", "cache_slot", "cache_x", "n_cached", "cache_L"), nocomp))
    good = dict(base, **trie, **search, **comp, **filt)
    order = tuple(base) + tuple(trie) + tuple(search) + tuple(comp) + tuple(filt)
    bad_items = bad_inputs + [
        dict(items=filt["items"].to(i64)), dict(items=dev([[0, 9, -1, 9]])[:, ::2]), dict(items=dev([[9, 0, -1]])[:, 1:]),
        dict(items=dev([0, -1])), dict(items=dev([[0, -1], [0, -1]])), dict(items=torch.zeros(1, 0, dtype=i32, device="cuda")),
        dict(items=torch.zeros(1, _lib.GRAM_MAX_USER_ITEMS + 1, dtype=i32, device="cuda")), dict(items=dev([[0, 1]])), dict(items=dev([[0, -2]])),
        dict(item_rank=torch.zeros(0, dtype=i32, device="cuda")), dict(item_rank=dev([[0]])), dict(item_rank=dev([0], i64)),
        dict(leaf_lo=dev([0, 0])), dict(leaf_hi=dev([1, 1, 1, 1])), dict(leaf_hi=filt["leaf_hi"].to(i64)),
        dict(trie_child_node=dev([1, 2, 2])), dict(trie_child_tok=dev([5, 1], i64)), dict(trie_child_off=torch.zeros(1, dtype=i32, device="cuda")),
        dict(items=filt["items"].cpu())]
    for bad in bad_items:
        args = dict(good, **bad)
        with pytest.raises(ValueError):
            torch.ops.gram.generate_items(*(args[k] for k in order))
