"""CPU: fused contexts of up to 16 384 tokens at the boundaries that need no device -- gram_model_set_max_fused_len and the shape
checks of the whole-path entry points through the C ABI (descriptors on dummy pointers, as tests/test_long_passages_host.py: every
refusal comes back before any launch), the argument checks of the long cross-attention's entry points, the KV-bank GEMM's host
guard and the multiply-high division bound it states, ``GRAM.set_max_fused_tokens`` with the error texts that name it, the fake
implementation of torch.ops.gram.cross_attn_long and the runner's setting.  The launch trains of a raised handle
(tests/golden/launch_train/*fused*.txt) are held against the tool by tests/test_launch_train.py."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from gram_amd import _lib

FAKE = 0x1000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_train")


def _create(max_passages=40, pieces=1):
    """gram_model_create on a tiny descriptor over dummy pointers -> (lib, handle)"""
    lib = _lib.load()
    keep = []

    def arr(n):
        a = (C.c_void_p * n)(*([FAKE] * n))
        keep.append(a)
        return C.cast(a, C.POINTER(C.c_void_p))

    desc = _lib.ModelDesc(vocab=384, d_model=128, d_ff=256, n_heads=2, n_enc_layers=2, n_dec_layers=2, max_passages=max_passages,
                          tie_word_embeddings=1, use_position_embedding=1, fold_norm=1, eps=1e-6, embed_f32=FAKE, lm_head_bf16=FAKE,
                          pos_emb_f32=FAKE, enc_bias_f32=FAKE, dec_bias_f32=FAKE, enc_final_ln=FAKE, dec_final_ln=FAKE,
                          enc_ln1=arr(2), enc_wqkv=arr(2), enc_wo=arr(2), enc_ln2=arr(2), enc_wi=arr(2), enc_wo2=arr(2), dec_ln1=arr(2),
                          dec_wqkv=arr(2), dec_wo=arr(2), dec_ln2=arr(2), dec_wq_x=arr(2), dec_wo_x=arr(2), dec_ln3=arr(2), dec_wi=arr(2),
                          dec_wo2=arr(2), dec_wkv_x_all=FAKE, pieces=pieces, lm_head_f32=FAKE)
    h = lib.gram_model_create(C.byref(desc))
    assert h
    return lib, h


@pytest.fixture()
def handle():
    lib, h = _create()
    yield lib, h
    lib.gram_model_destroy(h)


def _sizes(lib, h, B, N, L):
    """every workspace query of the C ABI at one (B, N, L)"""
    return [lib.gram_workspace_bytes(h, B, N, L, 4, 6), lib.gram_workspace_encoder_x_offset(h, B, N, L, 4, 6),
            lib.gram_workspace_bytes_tf(h, B, N, L, 2, 6), lib.gram_workspace_bytes_trie(h, B, N, L, 12)]


# ------------------------------------------------------------------------------------------------------------ the setter
def test_constants():
    assert _lib.GRAM_MAX_FUSED_LEN == 4096 and _lib.GRAM_MAX_LONG_FUSED_LEN == 16384 and _lib.ABI_VERSION == 7
    assert _lib.GRAM_KEY_BITS_LONG_WORDS == 512 and _lib.GRAM_KEY_BITS_LONG_STRIDE >= 513 and _lib.GRAM_KEY_BITS_LONG_STRIDE % 4 == 0


@pytest.mark.parametrize("n", [4096, 4128, 10752, 16384])
def test_setter_accepts(handle, n):
    lib, h = handle
    assert lib.gram_model_set_max_fused_len(h, n) == 0
    assert lib.gram_workspace_bytes(h, 2, 32, 128, 4, 6) > 0
    assert (lib.gram_workspace_bytes(h, 2, 33, 128, 4, 6) > 0) == (n >= 33 * 128)


@pytest.mark.parametrize("n", [0, 4095, 4100, 16416, 32768, -4096])
def test_setter_refuses_and_leaves_the_limit(handle, n):
    lib, h = handle
    assert lib.gram_model_set_max_fused_len(h, n) == _lib.E_ARG
    assert lib.gram_workspace_bytes(h, 2, 32, 128, 4, 6) > 0 and lib.gram_workspace_bytes(h, 2, 33, 128, 4, 6) == _lib.E_ARG
    assert lib.gram_model_set_max_fused_len(h, 8192) == 0
    assert lib.gram_model_set_max_fused_len(h, n) == _lib.E_ARG
    assert lib.gram_workspace_bytes(h, 2, 33, 128, 4, 6) > 0 and lib.gram_workspace_bytes(h, 2, 40, 224, 4, 6) == _lib.E_ARG  # 8960: still 8192


def test_setter_refuses_a_null_handle():
    assert _lib.load().gram_model_set_max_fused_len(None, 8192) == _lib.E_ARG


# ------------------------------------------------------------------------------------------------------------ workspace queries
@pytest.mark.parametrize("N,L", [(9, 512), (33, 128)])
def test_default_and_long_passage_handles_still_stop_at_4096(handle, N, L):
    lib, h = handle
    if L <= 128:
        assert all(v == _lib.E_ARG for v in _sizes(lib, h, 2, N, L))
    assert lib.gram_model_set_max_passage_len(h, 512) == 0
    assert all(v == _lib.E_ARG for v in _sizes(lib, h, 2, N, L))


@pytest.mark.parametrize("N,L", [(21, 224), (21, 512), (32, 512), (33, 128)])
def test_a_raised_handle_takes_up_to_16384(handle, N, L):
    lib, h = handle
    assert lib.gram_model_set_max_passage_len(h, 512) == 0
    assert lib.gram_model_set_max_fused_len(h, 16384) == 0
    sizes = _sizes(lib, h, 2, N, L)
    assert all(v >= 0 and v % 256 == 0 for v in sizes), sizes
    assert all(v == _lib.E_ARG for v in _sizes(lib, h, 2, 33, 512))  # 16 896
    assert lib.gram_model_set_max_fused_len(h, 4096) == 0  # back to the default
    assert all(v == _lib.E_ARG for v in _sizes(lib, h, 2, N, L))


def test_a_raised_handle_carves_the_wider_key_bits_and_the_scratch(handle):
    lib, h = handle
    B, K, H = 3, 4, 2
    short = lib.gram_workspace_bytes(h, B, 32, 128, K, 6)
    assert lib.gram_model_set_max_fused_len(h, 16384) == 0
    long_ = lib.gram_workspace_bytes(h, B, 32, 128, K, 6)
    # S = 4096: one segment, no scratch -- the rows of key bits grow from 128 to the long stride, rounded to the carve's 256 B
    grow = B * (_lib.GRAM_KEY_BITS_LONG_STRIDE - 128) * 4
    assert 0 <= long_ - short - grow < 512, (short, long_, grow)
    assert lib.gram_cross_attn_long_scratch_bytes(B * K, H, 4096) == 0
    assert lib.gram_cross_attn_long_scratch_bytes(B * K, H, 4128) == B * K * H * 2 * 68 * 4
    assert lib.gram_cross_attn_long_scratch_bytes(B * K, H, 16384) == B * K * H * 4 * 68 * 4
    for bad in ((0, H, 4128), (4, 0, 4128), (4, H, 0), (4, H, 4100), (4, H, 16416)):
        assert lib.gram_cross_attn_long_scratch_bytes(*bad) == _lib.E_ARG


# ------------------------------------------------------------------------------------------------------------ whole-path calls
def test_whole_path_calls_refuse_before_any_launch(handle):
    """No device here: a call that got as far as a launch would come back with a HIP error, not GRAM_E_ARG."""
    lib, h = handle
    trie = _lib.Trie(FAKE, FAKE, FAKE, 40, 39, 3, 2)
    assert lib.gram_model_set_max_passage_len(h, 512) == 0
    for N, L, smax in ((21, 224, 4096), (33, 128, 4096), (21, 512, 8192), (33, 512, 16384)):
        assert lib.gram_model_set_max_fused_len(h, smax) == 0
        assert lib.gram_encode_fused(h, FAKE, FAKE, 2, N, L, FAKE, 1 << 40, 4, 6, None, None) == _lib.E_ARG
        assert lib.gram_generate(h, FAKE, FAKE, 2, N, L, 4, 4, 6, 1.0, C.byref(trie), FAKE, 1 << 40, FAKE, FAKE, None, None) == _lib.E_ARG
        assert lib.gram_generate_ex(h, FAKE, FAKE, 2, N, L, 4, 4, 6, 1.0, C.byref(trie), None, FAKE, 1 << 40, FAKE, FAKE, None, None) == _lib.E_ARG
        assert lib.gram_decode_step(h, FAKE, FAKE, FAKE, 2, N, L, 4, 6, 1, FAKE, 1 << 40, FAKE, None) == _lib.E_ARG
        assert lib.gram_teacher_forced(h, FAKE, FAKE, 2, N, L, None, FAKE, FAKE, 2, 6, FAKE, 1 << 40, None, FAKE, FAKE, None) == _lib.E_ARG
        assert lib.gram_teacher_forced_ex(h, FAKE, FAKE, 2, N, L, None, FAKE, FAKE, 2, 6, FAKE, 1 << 40, None, FAKE, FAKE, None, None) == _lib.E_ARG


def test_attention_outputs_stop_at_4096_on_a_raised_handle(handle):
    lib, h = handle
    assert lib.gram_model_set_max_passage_len(h, 512) == 0 and lib.gram_model_set_max_fused_len(h, 16384) == 0
    attn = _lib.XattnOut(FAKE, None, None, None)
    # a workspace that is too small is what an ACCEPTED shape answers before any launch: (21, 160) = 3360 keys gets that far ...
    assert lib.gram_teacher_forced_ex(h, FAKE, FAKE, 2, 21, 160, None, FAKE, FAKE, 2, 6, FAKE, 16, None, FAKE, FAKE, C.byref(attn), None) == _lib.E_WORKSPACE
    # ... (21, 224) = 4704 is refused with the attention struct, and accepted without
    assert lib.gram_teacher_forced_ex(h, FAKE, FAKE, 2, 21, 224, None, FAKE, FAKE, 2, 6, FAKE, 16, None, FAKE, FAKE, C.byref(attn), None) == _lib.E_ARG
    assert lib.gram_teacher_forced_ex(h, FAKE, FAKE, 2, 21, 224, None, FAKE, FAKE, 2, 6, FAKE, 16, None, FAKE, FAKE, None, None) == _lib.E_WORKSPACE


# ------------------------------------------------------------------------------------------------------------ the kernel entry points
B_, K_, H_, S_ = 2, 20, 2, 8192
GOOD = dict(q=FAKE, k=FAKE, vt=FAKE, mask=FAKE, out=FAKE, B=B_, K=K_, H=H_, S=S_, users=None, rowpos=None, pieces=2, qps=B_ * K_ * H_ * 64,
            bps=H_ * S_ * 64, bits=FAKE, scratch=FAKE)
BAD = [dict(q=None), dict(k=None), dict(vt=None), dict(out=None), dict(bits=None), dict(scratch=None), dict(B=0), dict(K=0), dict(K=65), dict(H=0),
       dict(S=0), dict(S=16), dict(S=8200), dict(S=16416), dict(S=-32), dict(pieces=0), dict(pieces=3), dict(users=FAKE), dict(rowpos=FAKE),
       dict(qps=B_ * K_ * H_ * 64 - 8), dict(qps=0), dict(bps=H_ * S_ * 64 - 1), dict(q=FAKE + 8), dict(k=FAKE + 8), dict(vt=FAKE + 8),
       dict(out=FAKE + 4), dict(bits=FAKE + 2), dict(scratch=FAKE + 8)]


def _long_split(lib, a):
    return lib.gram_cross_attn_long_split(a["q"], a["k"], a["vt"], a["mask"], a["out"], a["B"], a["K"], a["H"], a["S"], a["users"], a["rowpos"],
                                          a["pieces"], a["qps"], a["bps"], a["bits"], a["scratch"], None)


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_long_cross_attention_argument_errors_before_any_launch(kw):
    lib = _lib.load()
    a = dict(GOOD, **kw)
    assert _long_split(lib, a) == _lib.E_ARG
    if not ({"users", "rowpos", "K"} & set(kw)):  # the rows form: Q rows per user, 130 of them in three groups
        Q = 130
        qps = a["qps"] if "qps" in kw else B_ * Q * H_ * 64
        if kw.get("qps") == B_ * K_ * H_ * 64 - 8:
            qps = B_ * Q * H_ * 64 - 8
        assert lib.gram_cross_attn_rows_long_split(a["q"], a["k"], a["vt"], a["mask"], a["out"], a["B"], Q, a["H"], a["S"], a["pieces"], qps,
                                                   a["bps"], a["bits"], a["scratch"], FAKE, None) == _lib.E_ARG


def test_rows_form_needs_its_row_tables_and_a_row():
    lib = _lib.load()
    a = GOOD
    for Q, rowmap in ((130, None), (0, FAKE), (-1, FAKE)):
        assert lib.gram_cross_attn_rows_long_split(a["q"], a["k"], a["vt"], a["mask"], a["out"], B_, Q, H_, S_, 2, B_ * 130 * H_ * 64, a["bps"],
                                                   a["bits"], a["scratch"], rowmap, None) == _lib.E_ARG


@pytest.mark.parametrize("kw", [dict(mask=None), dict(bits=None), dict(B=0), dict(S=0), dict(S=48), dict(S=16416), dict(mask=FAKE + 8), dict(bits=FAKE + 2)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_long_key_bits_argument_errors(kw):
    a = dict(dict(mask=FAKE, bits=FAKE, B=2, S=8192), **kw)
    assert _lib.load().gram_mask_key_bits_long(a["mask"], a["bits"], a["B"], a["S"], None) == _lib.E_ARG


def test_the_short_entry_points_keep_their_limit():
    lib = _lib.load()
    assert lib.gram_cross_attn_decode_split(FAKE, FAKE, FAKE, FAKE, FAKE, 2, 4, 2, 4128, None, None, 1, 0, 0, None, None) == _lib.E_ARG
    assert lib.gram_cross_attn_rows_split(FAKE, FAKE, FAKE, FAKE, FAKE, 2, 4, 2, 4128, 1, 0, 0, None, None, None) == _lib.E_ARG
    assert lib.gram_mask_key_bits(FAKE, FAKE, 2, 4128, None) == _lib.E_ARG
    assert lib.gram_cross_attn_probs_split(FAKE, FAKE, FAKE, FAKE, 2, 4, 2, 4128, 1, 0, 0, None, None) == _lib.E_ARG


# ------------------------------------------------------------------------------------------------------------ the KV-bank GEMM's guard
def _bank_gemm(lib, B, S, H=4, pieces=1):
    """gram_gemm_bf16_split with the KV-bank epilogue on dummy pointers: M = B * S rows, one layer, K = 256 (the ping-pong kernel
    wants four 64-column steps at least)"""
    bank = _lib.KVBank(FAKE, FAKE, 1, B, H, S, None, 0, 0)
    split = _lib.Split(pieces, 0, 0, B * H * S * 64, 1.0)
    M, N, kc = B * S, 2 * H * 64, 256
    return lib.gram_gemm_bf16_split(FAKE, FAKE, None, M, N, kc, pieces * kc, N, _lib.EPI_KV_BANK, C.byref(bank), None, C.byref(split), None)


V_PP = 22  # gemm.hip's id of the ping-pong kernel (gram_debug_set_gemm_variant)


@pytest.mark.parametrize("pieces", [1, 2])
def test_the_bank_gemm_refuses_what_its_divisions_cannot_take(pieces):
    """The guard is the ping-pong kernel's (the only one that divides by multiply-high; unforced, a shape it declines falls back to
    the 128-row kernel, which divides exactly): with that kernel forced the refusal is the call's answer, before any launch.  Without a device an accepted
    shape ends in the same code one step later (no device to count the CUs of), so that the kernel TAKES S = 16 384, and refuses
    exactly these, is checked again on the GPU: tests/test_gpu_fused_len.py."""
    lib = _lib.load()
    lib.gram_debug_set_gemm_variant(V_PP)
    try:
        assert _bank_gemm(lib, 2, 16416, pieces=pieces) == _lib.E_ARG  # S above 16 384
        assert _bank_gemm(lib, 1 << 14, 16384, pieces=pieces) == _lib.E_ARG  # M = 2^28: (M / 32) * (S / 32) = 2^32
    finally:
        lib.gram_debug_set_gemm_variant(-1)


def _mulhi_div(x, d):
    """kv_locate's division: multiply-high by floor(2^32 / d) + 1"""
    return (x * ((1 << 32) // d + 1)) >> 32


def test_magic_division_is_exact_inside_the_guard():
    """x / d by multiply-high is exact iff x * e < 2^32, e = d - (2^32 mod d) <= d, and the estimate is monotone in x: the
    boundaries x = k d - 1 and x = k d decide.  Every d = S / 32 <= 512 and every boundary below 2^23 -- what (M / 32) * (S / 32) < 2^32
    lets through at d = 512."""
    for d in range(1, 513):
        mg = np.uint64((1 << 32) // d + 1)
        k = np.arange(1, ((1 << 23) - 1) // d + 1, dtype=np.uint64)
        x = k * np.uint64(d)  # (x < 2^23, mg <= 2^32 + 1: the product stays inside uint64)
        assert np.array_equal((x * mg) >> np.uint64(32), k), d
        assert np.array_equal(((x - np.uint64(1)) * mg) >> np.uint64(32), k - np.uint64(1)), d


def test_magic_division_can_fail_past_the_guard():
    """d = 512 (e = d): the first boundary whose x * d reaches 2^32 is off by one -- the guard is needed, and it is tight."""
    d = 512
    x_last = (1 << 23) - 1  # the largest x with x * d < 2^32
    assert x_last * d < 1 << 32 and _mulhi_div(x_last, d) == x_last // d
    x = ((1 << 14) + 1) * d - 1  # the first k d - 1 at or above 2^32 / d
    assert x * d >= 1 << 32 and _mulhi_div(x, d) == x // d + 1


# ------------------------------------------------------------------------------------------------------------ Python
def _gram(**kw):
    import gram_amd
    kw.setdefault("max_item_num", 31)
    return gram_amd.create_model("gram", gram_amd.T5Config(vocab_size=256, d_model=128, d_ff=256, num_layers=2, num_decoder_layers=2,
                                                           num_heads=2, **kw))


def test_set_max_fused_tokens_values():
    m = _gram()
    assert m._max_fused_tokens == 4096
    for bad in (0, 4095, 4100, 16416, 32768):
        with pytest.raises(ValueError, match="multiple of 32"):
            m.set_max_fused_tokens(bad)
        assert m._max_fused_tokens == 4096
    m._pcache = sentinel = object()
    for good in (4128, 10752, 16384, 4096):
        m.set_max_fused_tokens(good)
        assert m._max_fused_tokens == good
    assert m._pcache is sentinel  # cached passages do not depend on N * L
    assert type(m)._max_fused_tokens == 4096  # (the setting is the model's own)


def test_entry_points_name_the_setter():
    from gram_amd.utils import generation_trie as gt
    m = _gram()
    m.set_max_passage_len(256)
    ids = torch.zeros(2, 21, 224, dtype=torch.long)
    mask = torch.ones(2, 21, 224, dtype=torch.bool)
    fn = gt.prefix_allowed_tokens_fn(gt.Trie([[0, 2, 1]]))
    want = r"set_max_fused_tokens\(4704\) first"
    with pytest.raises(ValueError, match=want):
        m.generate(input_ids=ids, attention_mask=mask, max_length=3, prefix_allowed_tokens_fn=fn, num_beams=2)
    with pytest.raises(ValueError, match=want):
        m._tf_chunks(ids, mask, None, None, None)
    with pytest.raises(ValueError, match=want):
        m._tf_chunks(ids, mask, None, None, None, trie_rows=(12, 4))  # score_all_items' pass
    for query in (lambda: m.max_users_per_call(21, 224, 4, 6), lambda: m.max_users_per_call_tf(21, 224, 2, 6),
                  lambda: m.max_users_per_call_trie(21, 224, 12, 4)):
        with pytest.raises(ValueError, match=want):
            query()
    assert m._check_fused_len(32, 128) == 4096 and m._check_fused_len(16, 225) == 4096
    with pytest.raises(ValueError, match=r"set_max_fused_tokens\(4704\)"):
        m._check_fused_len(21, 200)  # padded to 224
    m.set_max_fused_tokens(4704)
    assert m._check_fused_len(21, 224) == 4704
    with pytest.raises(ValueError, match=r"set_max_fused_tokens\(10752\)"):
        m._check_fused_len(21, 512)
    with pytest.raises(ValueError, match="goes up to 16384"):
        m._check_fused_len(33, 512)


def test_attention_probabilities_say_they_stop_at_4096():
    m = _gram()
    m.set_max_passage_len(256)
    m.set_max_fused_tokens(16384)
    ids = torch.zeros(2, 21, 224, dtype=torch.long)
    mask = torch.ones(2, 21, 224, dtype=torch.bool)
    dec = torch.zeros(2, 1, 1, dtype=torch.long)
    with pytest.raises(ValueError, match="limited to 4096 fused tokens"):
        m._teacher_forced_attn(ids, mask, dec, dec, True, False)


def test_the_custom_op_is_registered_with_a_fake_impl():
    import gram_amd.ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert hasattr(torch.ops.gram, "cross_attn_long")
    dt = _lib.piece_dtype()
    with FakeTensorMode():
        B, K, H, S = 2, 20, 2, 8192
        out = torch.ops.gram.cross_attn_long(torch.empty(B * K, H * 64, dtype=dt, device="cuda"), torch.empty(B, H, S, 64, dtype=dt, device="cuda"),
                                             torch.empty(B, H, S // 32, 64, 32, dtype=dt, device="cuda"),
                                             torch.empty(B, S, dtype=torch.uint8, device="cuda"), K)
        assert out.shape == (B * K, H * 64) and out.dtype == dt
    with pytest.raises((NotImplementedError, RuntimeError)):  # no CPU kernel
        torch.ops.gram.cross_attn_long(torch.zeros(4, 128, dtype=dt), torch.zeros(1, 2, 32, 64, dtype=dt), torch.zeros(1, 2, 1, 64, 32, dtype=dt),
                                       torch.ones(1, 32, dtype=torch.uint8), 4)


@pytest.mark.parametrize("prompt_len,max_his,want_L,want_S", [(256, 20, 256, 5376), (128, 20, None, None), (512, 20, 512, 10752),
                                                              (512, 40, 512, 16384), (200, 20, 224, 4704), (128, 31, None, None)])
def test_the_runner_raises_the_limits_from_its_arguments(prompt_len, max_his, want_L, want_S):
    from gram_amd.runner.base import BaseRunner

    class Model:
        _max_passage_len, _max_fused_tokens = 128, 4096
        calls = None

        def set_max_passage_len(self, n):
            self.calls.append(("L", n))
            self._max_passage_len = n

        def set_max_fused_tokens(self, n):
            self.calls.append(("S", n))
            self._max_fused_tokens = n

    model = Model()
    model.calls = []
    runner = BaseRunner.__new__(BaseRunner)
    runner.args = types.SimpleNamespace(item_prompt_max_len=prompt_len, max_his=max_his)
    runner.model_rec = model
    loader = types.SimpleNamespace(collate_fn=None)
    runner._raise_model_limits(loader)
    assert model.calls == ([("L", want_L)] if want_L else []) + ([("S", want_S)] if want_S else [])
    runner._raise_model_limits(loader)  # (again: nothing to do)
    assert len(model.calls) == (want_L is not None) + (want_S is not None)


# ------------------------------------------------------------------------------------------------------------ the launch trains
def _train(case):
    with open(os.path.join(GOLDEN, case + ".txt")) as f:
        return f.read().splitlines()


def test_a_raised_handles_train_differs_in_the_cross_attention_only():
    short, long_ = _train("generate_p1_folded"), _train("generate_fused_32")
    assert long_[0] == "gram_model_set_max_fused_len 0"
    long_ = long_[1:]
    assert len(short) == len(long_)
    names = {"gram_mask_key_bits": "gram_mask_key_bits_long", "gram_cross_attn_decode_split": "gram_cross_attn_long_split"}
    n = {k: 0 for k in names}
    for a, b in zip(short, long_):
        fa, fb = a.split(), b.split()
        if fa[0] in names:
            assert fb[0] == names[fa[0]]
            if fa[0] == "gram_cross_attn_decode_split":
                assert fb[1:-2] == fa[1:-1] and fb[-2] == "0" and fb[-1] == fa[-1]  # the same operands, no scratch at S <= 4096
            else:
                assert fb[1:] == fa[1:]
            n[fa[0]] += 1
        elif a != b:
            assert fa[0].startswith("gram_workspace_bytes") and fb[0] == fa[0] and int(fb[1]) > int(fa[1])  # wider key bits
    assert n == {"gram_mask_key_bits": 1, "gram_cross_attn_decode_split": 6}  # 3 steps x 2 layers


@pytest.mark.parametrize("case,name,count", [("generate_fused_4704", "gram_cross_attn_long_split", 6), ("tf_fused_4704", "gram_cross_attn_rows_long_split", 2),
                                             ("score_trie_fused_4704", "gram_cross_attn_rows_long_split", 2)])
def test_the_trains_at_4704_fused_tokens(case, name, count):
    got = _train(case)
    assert got[-1] == "return 0"
    calls = [l.split() for l in got]
    assert [c[0] for c in calls if "key_bits" in c[0]] == ["gram_mask_key_bits_long"]
    xa = [c for c in calls if "cross_attn" in c[0]]
    assert [c[0] for c in xa] == [name] * count
    for c in xa:
        assert c[9] == "4704" and c[-2 if name.endswith("_long_split") and "rows" not in name else -3].startswith("ws+"), c  # S; the scratch is carved
