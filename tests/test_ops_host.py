"""CPU: the host side of the ``gram::`` custom ops (gram_amd/ops.py) -- the twelve schemas (public: INTEGRATION.md and the callers
pass arguments by position), every meta implementation's shapes and dtypes under ``FakeTensorMode``, and the private helpers that
state the shared argument handling once: the teacher-forced validator with each of its refusals, the gram_compaction_t and
gram_trie_t builders field by field.  Needs the built library (the 16-bit operand type is its), no GPU."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import gram_amd  # noqa: F401
from gram_amd import _lib, ops

DT = _lib.piece_dtype()
I32, I64, U8, F32 = torch.int32, torch.int64, torch.uint8, torch.float32

_HEAD = "Tensor input_ids, Tensor attention_mask, SymInt handle, Tensor(a3!) workspace, "
_TRIE = "Tensor trie_child_off, Tensor trie_child_tok, Tensor trie_child_node, SymInt trie_max_fanout, SymInt trie_min_seq_len, "
_SEARCH = "SymInt num_beams, SymInt num_return_sequences, SymInt max_length, float length_penalty, "
_COMP = "Tensor? comp_map, Tensor? comp_ids, Tensor? comp_mask, Tensor? cache_slot, Tensor? cache_x, SymInt n_cached, SymInt cache_L"
_DEC = "Tensor decoder_input_ids, Tensor labels, SymInt vocab_size, "

# str(torch.ops.gram.<name>.default._schema), recorded before the shared argument handling was factored out of the op bodies
SCHEMAS = {
    "generate": "gram::generate(" + _HEAD + _TRIE + _SEARCH + _COMP
                + ", Tensor? trie_sub_rows=None, SymInt trie_d_tail=0, SymInt trie_tail_steps=0) -> (Tensor, Tensor, Tensor)",
    "generate_items": "gram::generate_items(" + _HEAD + _TRIE + _SEARCH + _COMP
                      + ", Tensor leaf_lo, Tensor leaf_hi, Tensor item_rank, Tensor items, bool allow) -> (Tensor, Tensor, Tensor)",
    "teacher_forced": "gram::teacher_forced(" + _HEAD + _DEC + "bool want_logits, " + _COMP + ") -> (Tensor, Tensor, Tensor)",
    "teacher_forced_attn": "gram::teacher_forced_attn(" + _HEAD + _DEC
                           + "SymInt n_dec_layers, SymInt n_heads, bool want_probs, bool want_scores, " + _COMP
                           + ") -> (Tensor, Tensor, Tensor)",
    "teacher_forced_scores": "gram::teacher_forced_scores(" + _HEAD + _DEC + _COMP + ") -> (Tensor, Tensor)",
    "score_trie": "gram::score_trie(" + _HEAD + _TRIE
                  + "Tensor row_tokens, Tensor row_pos, Tensor row_anc, Tensor row_node, Tensor node_row, Tensor node_tok, "
                  "Tensor node_leaf, SymInt n_leaves, SymInt vocab_size, bool want_nodes, " + _COMP + ") -> (Tensor, Tensor)",
    "linear": "gram::linear(Tensor a, Tensor w, bool relu=False) -> Tensor",
    "enc_self_attn": "gram::enc_self_attn(Tensor qkv, Tensor bias, Tensor mask, SymInt num_heads) -> Tensor",
    "enc_self_attn_long": "gram::enc_self_attn_long(Tensor qkv, Tensor bias, Tensor mask, SymInt num_heads) -> Tensor",
    "cross_attn_decode": "gram::cross_attn_decode(Tensor q, Tensor k_bank, Tensor vt_bank, Tensor mask, SymInt num_beams) -> Tensor",
    "cross_attn_long": "gram::cross_attn_long(Tensor q, Tensor k_bank, Tensor vt_bank, Tensor mask, SymInt num_beams) -> Tensor",
    "trie_step": "gram::trie_step(Tensor logits, Tensor(a1!) tokens, Tensor(a2!) node, Tensor(a3!) beam_scores, Tensor(a4!) seq, "
                 "Tensor(a5!) anc, Tensor(a6!) done, Tensor(a7!) n_hyps, Tensor(a8!) hyp_score, Tensor(a9!) worst, Tensor(a10!) hyp_len, "
                 "Tensor(a11!) hyp_tok, Tensor(a12!) error, Tensor trie_child_off, Tensor trie_child_tok, Tensor trie_child_node, "
                 "SymInt trie_max_fanout, SymInt num_beams, SymInt cur_len, float length_penalty) -> Tensor",
}


def test_schemas_are_the_recorded_ones():
    assert sorted(SCHEMAS) == sorted(ops.__all__) and len(SCHEMAS) == 12
    for name, want in SCHEMAS.items():
        assert str(getattr(torch.ops.gram, name).default._schema) == want, name


# ---------------------------------------------------------------------------------------------- meta implementations
def _is(t, shape, dtype):
    return tuple(t.shape) == tuple(shape) and t.dtype == dtype


def _e(*shape, dtype=I32):
    return torch.empty(*shape, dtype=dtype, device="cuda")


NOCOMP = (None, None, None, None, None, 0, 0)


def test_fakes_of_the_search_ops():
    """generate / generate_items: (B*nret, max_length) i64, (B*nret,) f32 -- empty for greedy search --, width i32 (1,) on the host;
    with compaction tensors and with the tail tables alike."""
    with FakeTensorMode():
        ids, ws, t, items = _e(3, 2, 32, dtype=I64), _e(1024, dtype=U8), _e(8), _e(3, 6)
        comp = (_e(4), _e(4, 32, dtype=I64), _e(4, 32, dtype=U8), _e(2), _e(9, 128, 64, dtype=F32), 2, 128)
        for K, nret, n_sc in ((5, 5, 15), (5, 2, 6), (1, 1, 0)):
            head = (ids, ids.to(U8), 0, ws, t, t, t, 4, 3, K, nret, 7, 1.0)
            for out in (torch.ops.gram.generate(*head, *NOCOMP), torch.ops.gram.generate(*head, *comp),
                        torch.ops.gram.generate(*head, *NOCOMP, t, 2, 3), torch.ops.gram.generate_items(*head, *NOCOMP, t, t, t, items, True),
                        torch.ops.gram.generate_items(*head, *comp, t, t, t, items, False)):
                s, sc, wd = out
                assert _is(s, (3 * nret, 7), I64) and _is(sc, (n_sc,), F32) and _is(wd, (1,), I32), (K, nret)
                assert s.device.type == sc.device.type == "cuda" and wd.device.type == "cpu"


def test_fakes_of_the_teacher_forced_ops():
    B, N, L, Cn, T, V, nl, H = 2, 3, 64, 3, 4, 256, 2, 4
    Q, S = Cn * T, N * L
    with FakeTensorMode():
        ids, ws, dec = _e(B, N, L, dtype=I64), _e(1024, dtype=U8), _e(B, Cn, T)
        head = (ids, ids.to(U8), 0, ws, dec, dec, V)
        for want_logits in (False, True):
            lg, tok, seq = torch.ops.gram.teacher_forced(*head, want_logits, *NOCOMP)
            assert _is(lg, (B, Cn, T, V) if want_logits else (0,), F32) and _is(tok, (B, Cn, T), F32) and _is(seq, (B, Cn), F32)
        for want_probs, want_scores in ((True, False), (False, True), (True, True)):
            pr, tsc, psc = torch.ops.gram.teacher_forced_attn(*head, nl, H, want_probs, want_scores, *NOCOMP)
            assert _is(pr, (nl, B, H, Q, S) if want_probs else (0,), F32), (want_probs, want_scores)
            assert _is(tsc, (B, Q, S) if want_scores else (0,), F32) and _is(psc, (B, Q, N) if want_scores else (0,), F32)
        tsc, psc = torch.ops.gram.teacher_forced_scores(*head, *NOCOMP)
        assert _is(tsc, (B, Q, S), F32) and _is(psc, (B, Q, N), F32)


def test_fake_of_score_trie():
    B, n_nodes, n_leaves, Qr, Tq = 2, 9, 5, 4, 3
    with FakeTensorMode():
        ids, ws = _e(B, 3, 32, dtype=I64), _e(1024, dtype=U8)
        for want_nodes in (False, True):
            leaf, nodes = torch.ops.gram.score_trie(ids, ids.to(U8), 0, ws, _e(n_nodes + 1), _e(8), _e(8), 4, 3, _e(Qr), _e(Qr), _e(Qr, Tq),
                                                    _e(Qr), _e(n_nodes), _e(n_nodes), _e(n_nodes), n_leaves, 256, want_nodes, *NOCOMP)
            assert _is(leaf, (B, n_leaves), F32) and _is(nodes, (B, n_nodes) if want_nodes else (0,), F32)


def test_fakes_of_the_kernel_ops():
    with FakeTensorMode():
        a, w = _e(20, 768, dtype=DT), _e(2304, 768, dtype=DT)
        assert _is(torch.ops.gram.linear(a, w), (20, 2304), DT) and _is(torch.ops.gram.linear(a, w, True), (20, 2304), DT)
        P, L, H = 3, 64, 2
        qkv, bias, m2 = _e(P * L, 3 * H * 64, dtype=DT), _e(H, 255, dtype=F32), _e(P, L, dtype=U8)
        assert _is(torch.ops.gram.enc_self_attn(qkv, bias, m2, H), (P * L, H * 64), DT)
        assert _is(torch.ops.gram.enc_self_attn_long(qkv, bias, m2, H), (P * L, H * 64), DT)
        B, K, S = 2, 5, 96
        q, kb, vt, mk = _e(B * K, H * 64, dtype=DT), _e(B, H, S, 64, dtype=DT), _e(B, H, S // 32, 64, 32, dtype=DT), _e(B, S, dtype=U8)
        assert _is(torch.ops.gram.cross_attn_decode(q, kb, vt, mk, K), (B * K, H * 64), DT)
        assert _is(torch.ops.gram.cross_attn_long(q, kb, vt, mk, K), (B * K, H * 64), DT)
        R, V, Tq = B * K, 256, 6
        f64 = torch.float64
        lse = torch.ops.gram.trie_step(_e(R, V, dtype=F32), _e(R), _e(R), _e(R, dtype=F32), _e(R, Tq), _e(Tq, R), _e(B), _e(B),
                                       _e(B, K + 1, dtype=f64), _e(B, dtype=f64), _e(B, K + 1), _e(B, K + 1, Tq), _e(1), _e(8), _e(8), _e(8), 4,
                                       K, 2, 1.0)
        assert _is(lse, (R,), F32)


# ---------------------------------------------------------------------------------------------- the shared helpers
V = 16


def _tf_good(T=2):
    ids = torch.zeros(1, 1, 32, dtype=I64)
    dec = torch.tensor([[[0, V - 1] + [1] * (T - 2)]], dtype=I32)[:, :, :T].contiguous()
    lab = torch.tensor([[[V - 1, -100] + [-1] * (T - 2)]], dtype=I32)[:, :, :T].contiguous()
    return dict(input_ids=ids, attention_mask=torch.ones(1, 1, 32, dtype=U8), decoder_input_ids=dec, labels=lab)


def _tf_bad():
    g = _tf_good()
    dec, lab = g["decoder_input_ids"], g["labels"]

    def at(t, v):
        t = t.clone()
        t[0, 0, 1] = v
        return t

    long_T = _lib.GRAM_MAX_DEC_LEN + 1
    return {
        "input_ids not 3-D": dict(input_ids=g["input_ids"][0], attention_mask=g["attention_mask"][0]),
        "decoder_input_ids not 3-D": dict(decoder_input_ids=dec[0], labels=lab[0]),
        "input_ids dtype": dict(input_ids=g["input_ids"].to(I32)),
        "attention_mask dtype": dict(attention_mask=g["attention_mask"].bool()),
        "decoder_input_ids dtype": dict(decoder_input_ids=dec.to(I64)),
        "labels dtype": dict(labels=lab.to(I64)),
        "labels shape": dict(labels=torch.zeros(1, 1, 3, dtype=I32)),
        "labels users": dict(labels=torch.zeros(2, 1, 2, dtype=I32)),
        "mask shape": dict(attention_mask=torch.ones(1, 1, 64, dtype=U8)),
        "decoder users": dict(decoder_input_ids=torch.zeros(2, 1, 2, dtype=I32), labels=torch.zeros(2, 1, 2, dtype=I32)),
        "T = 0": dict(decoder_input_ids=torch.zeros(1, 1, 0, dtype=I32), labels=torch.zeros(1, 1, 0, dtype=I32)),
        "T too long": dict(decoder_input_ids=torch.zeros(1, 1, long_T, dtype=I32), labels=torch.zeros(1, 1, long_T, dtype=I32)),
        "C = 0": dict(decoder_input_ids=torch.zeros(1, 0, 2, dtype=I32), labels=torch.zeros(1, 0, 2, dtype=I32)),
        "decoder id -1": dict(decoder_input_ids=at(dec, -1)),
        "decoder id = vocab": dict(decoder_input_ids=at(dec, V)),
        "label = vocab": dict(labels=at(lab, V)),
        "mask not contiguous": dict(attention_mask=torch.ones(1, 1, 64, dtype=U8)[:, :, ::2]),
        "labels not aligned": dict(labels=torch.zeros(1, 1, 3, dtype=I32)[:, :, 1:]),
    }


def test_tf_inputs_accepts_and_returns_the_dimensions():
    assert ops._tf_inputs("teacher_forced", vocab_size=V, **_tf_good()) == (1, 1, 32, 1, 2)
    assert ops._tf_inputs("teacher_forced", vocab_size=V, **_tf_good(_lib.GRAM_MAX_DEC_LEN)) == (1, 1, 32, 1, _lib.GRAM_MAX_DEC_LEN)
    g = _tf_good()
    g["labels"] = torch.full((1, 1, 2), -100, dtype=I32)  # every label ignored: labels < 0 are fine
    g["input_ids"] = torch.zeros(1, 3, 64, dtype=I64)
    g["attention_mask"] = torch.ones(1, 3, 64, dtype=U8)
    assert ops._tf_inputs("teacher_forced_scores", vocab_size=V, **g) == (1, 3, 64, 1, 2)


@pytest.mark.parametrize("what", sorted(_tf_bad()))
def test_tf_inputs_refuses(what):
    args = dict(_tf_good(), **_tf_bad()[what])
    with pytest.raises(ValueError) as e:
        ops._tf_inputs("teacher_forced_attn", vocab_size=V, **args)
    ranges = ("decoder id -1", "decoder id = vocab", "label = vocab")
    if "3-D" in what or what in ("T = 0", "T too long", "C = 0") + ranges:
        assert str(e.value).startswith("teacher_forced_attn: ")  # the op's own refusals carry its name (the others name the tensor)
    if what in ("T = 0", "T too long"):
        assert str(_lib.GRAM_MAX_DEC_LEN) in str(e.value)
    if what in ranges:
        assert f"[0, {V})" in str(e.value)


def test_tf_inputs_reads_back_once(monkeypatch):
    """The range check is the one device-to-host read of a call: three reductions stacked into one tensor, one ``tolist``."""
    calls = []
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda t: calls.append(tuple(t.shape)) or real(t))
    ops._tf_inputs("teacher_forced", vocab_size=V, **_tf_good())
    assert calls == [(3,)]


def test_compaction_builder_fills_the_named_fields():
    assert ops._compaction(*NOCOMP) is None and ops._ref(None) is None
    cmap, cids, cmask = torch.zeros(5, dtype=I32), torch.zeros(3, 32, dtype=I64), torch.zeros(3, 32, dtype=U8)
    slot, x = torch.zeros(2, dtype=I32), torch.zeros(4, 128, 8)
    comp = ops._compaction(cmap, cids, cmask, slot, x, 2, 128)
    want = dict(n_active=cmap.numel(), passage_map=cmap.data_ptr(), ids=cids.data_ptr(), mask=cmask.data_ptr(), n_cached=2, cache_L=128,
                cache_x=x.data_ptr(), cache_slot=slot.data_ptr())
    assert isinstance(comp, _lib.Compaction) and set(want) == {n for n, _ in _lib.Compaction._fields_}
    assert {n: getattr(comp, n) for n in want} == want
    assert len({v for n, v in want.items() if n not in ("n_active", "n_cached", "cache_L")}) == 5  # (five distinct pointers)
    assert ops._ref(comp) is not None
    comp = ops._compaction(cmap, cids, cmask, None, None, 0, 0)  # nothing cached
    want.update(cache_x=None, cache_slot=None, n_cached=0, cache_L=0)
    assert {n: getattr(comp, n) for n in want} == want


def test_trie_builder_fills_the_named_fields():
    off, tok, node = torch.zeros(10, dtype=I32), torch.zeros(8, dtype=I32), torch.zeros(8, dtype=I32)
    trie = ops._trie(off, tok, node, 4, 3)
    want = dict(child_off=off.data_ptr(), child_tok=tok.data_ptr(), child_node=node.data_ptr(), n_nodes=off.numel() - 1,
                n_edges=tok.numel(), max_fanout=4, min_seq_len=3)
    assert isinstance(trie, _lib.Trie) and set(want) == {n for n, _ in _lib.Trie._fields_}
    assert {n: getattr(trie, n) for n in want} == want
    assert len({want["child_off"], want["child_tok"], want["child_node"]}) == 3
