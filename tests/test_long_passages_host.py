"""CPU: passages of up to 512 tokens at the boundaries that need no device -- gram_model_set_max_passage_len and the shape checks of
the whole-path entry points through the C ABI (descriptors on dummy pointers, as tests/test_model_shapes_host.py: nothing reads a
weight, and every refusal comes back before any launch), the argument checks of gram_enc_self_attn_long[_rows]_split, the widths of
the passage cache's identities and keys, the ValueErrors of ``GRAM.set_max_passage_len`` and of the entry points, and the launch
trains of a long-mode handle (tests/golden/launch_train/generate_long_*.txt; tests/test_launch_train.py holds them against the tool)."""
import ctypes as C
import os

import pytest
import torch

from gram_amd import _lib

FAKE = 0x1000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_train")


def _create(max_passages=16):
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
                          dec_wo2=arr(2), dec_wkv_x_all=FAKE, pieces=1, lm_head_f32=FAKE)
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


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_constants():
    assert _lib.GRAM_MAX_PASSAGE_LEN == 128 and _lib.GRAM_MAX_LONG_PASSAGE_LEN == 512 and _lib.ABI_VERSION == 7


@pytest.mark.parametrize("n", [128, 160, 256, 480, 512])
def test_setter_accepts(handle, n):
    lib, h = handle
    assert lib.gram_model_set_max_passage_len(h, n) == 0
    assert lib.gram_workspace_bytes(h, 2, 2, n, 4, 6) > 0


@pytest.mark.parametrize("n", [0, -128, 32, 96, 127, 129, 144, 500, 544, 1024])
def test_setter_refuses(handle, n):
    lib, h = handle
    assert lib.gram_model_set_max_passage_len(h, n) == _lib.E_ARG
    assert lib.gram_workspace_bytes(h, 2, 2, 128, 4, 6) > 0 and lib.gram_workspace_bytes(h, 2, 2, 160, 4, 6) == _lib.E_ARG  # (unchanged)


def test_setter_refuses_a_null_handle():
    assert _lib.load().gram_model_set_max_passage_len(None, 256) == _lib.E_ARG


@pytest.mark.parametrize("N,L", [(8, 512), (16, 256), (1, 512), (3, 160)])
def test_a_long_handle_takes_long_passages_up_to_4096_fused_tokens(handle, N, L):
    lib, h = handle
    assert all(v == _lib.E_ARG for v in _sizes(lib, h, 2, N, L))  # (a default handle)
    assert lib.gram_model_set_max_passage_len(h, 512) == 0
    sizes = _sizes(lib, h, 2, N, L)
    assert all(v >= 0 for v in sizes) and sizes[0] % 256 == 0, sizes


def test_the_limit_is_the_handles_own(handle):
    lib, h = handle
    assert lib.gram_model_set_max_passage_len(h, 256) == 0
    assert all(v >= 0 for v in _sizes(lib, h, 2, 3, 256)) and all(v == _lib.E_ARG for v in _sizes(lib, h, 2, 3, 288))
    assert lib.gram_model_set_max_passage_len(h, 128) == 0  # back to the default
    assert all(v == _lib.E_ARG for v in _sizes(lib, h, 2, 3, 160)) and all(v >= 0 for v in _sizes(lib, h, 2, 3, 128))


@pytest.mark.parametrize("N,L", [(9, 512), (16, 512), (16, 288), (13, 320)])
def test_more_than_4096_fused_tokens_are_refused_on_a_long_handle(handle, N, L):
    lib, h = handle
    assert lib.gram_model_set_max_passage_len(h, 512) == 0
    assert all(v == _lib.E_ARG for v in _sizes(lib, h, 2, N, L))


def test_more_than_4096_fused_tokens_are_refused_on_a_default_handle():
    lib, h = _create(max_passages=40)
    try:
        assert all(v >= 0 for v in _sizes(lib, h, 2, 32, 128)) and all(v == _lib.E_ARG for v in _sizes(lib, h, 2, 33, 128))
    finally:
        lib.gram_model_destroy(h)


def test_whole_path_calls_refuse_before_any_launch(handle):
    """No device here: a call that got as far as a launch would come back with a HIP error, not GRAM_E_ARG."""
    lib, h = handle
    trie = _lib.Trie(FAKE, FAKE, FAKE, 40, 39, 3, 2)
    for N, L, lmax in ((3, 160, 128), (9, 512, 512), (3, 288, 256)):
        assert lib.gram_model_set_max_passage_len(h, lmax) == 0
        assert lib.gram_encode_fused(h, FAKE, FAKE, 2, N, L, FAKE, 1 << 40, 4, 6, None, None) == _lib.E_ARG
        if L > lmax:
            assert lib.gram_encode_passages(h, FAKE, FAKE, 2, L, FAKE, 1 << 40, FAKE, None) == _lib.E_ARG
        assert lib.gram_generate_ex(h, FAKE, FAKE, 2, N, L, 4, 4, 6, 1.0, C.byref(trie), None, FAKE, 1 << 40, FAKE, FAKE, None, None) == _lib.E_ARG
        assert lib.gram_decode_step(h, FAKE, FAKE, FAKE, 2, N, L, 4, 6, 1, FAKE, 1 << 40, FAKE, None) == _lib.E_ARG
        assert lib.gram_teacher_forced(h, FAKE, FAKE, 2, N, L, None, FAKE, FAKE, 2, 6, FAKE, 1 << 40, None, FAKE, FAKE, None) == _lib.E_ARG


GOOD = dict(qkv=FAKE, bias=FAKE, mask=FAKE, out=FAKE, P=2, L=160, H=2, pieces=2, ps=2 * 160 * 3 * 128)
BAD = [dict(qkv=None), dict(bias=None), dict(mask=None), dict(out=None), dict(P=0), dict(H=0), dict(L=0), dict(L=16), dict(L=176), dict(L=544),
       dict(L=-32), dict(pieces=0), dict(pieces=3), dict(ps=2 * 160 * 3 * 128 - 8), dict(ps=0), dict(qkv=FAKE + 8), dict(out=FAKE + 2)]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_long_kernel_argument_errors_before_any_launch(kw):
    lib = _lib.load()
    a = dict(GOOD, **kw)
    assert lib.gram_enc_self_attn_long_split(a["qkv"], a["bias"], a["mask"], a["out"], a["P"], a["L"], a["H"], a["pieces"], a["ps"], None) == _lib.E_ARG
    if "ps" not in kw:  # (the table form's stride is the table's: one row per piece at least)
        assert lib.gram_enc_self_attn_long_rows_split(a["qkv"], FAKE, a["bias"], a["mask"], a["out"], a["P"], a["L"], a["H"], a["pieces"],
                                                      a["ps"], None) == _lib.E_ARG
    assert lib.gram_enc_self_attn_long_rows_split(FAKE, None, FAKE, FAKE, FAKE, 2, 160, 2, 2, 384, None) == _lib.E_ARG  # no ids
    assert lib.gram_enc_self_attn_long_rows_split(FAKE, FAKE, FAKE, FAKE, FAKE, 2, 160, 2, 2, 376, None) == _lib.E_ARG  # less than one row


def test_the_short_entry_points_keep_their_limit():
    lib = _lib.load()
    assert lib.gram_enc_self_attn_split(FAKE, FAKE, FAKE, FAKE, 2, 160, 2, 1, 0, None) == _lib.E_ARG
    assert lib.gram_enc_self_attn_rows_split(FAKE, FAKE, FAKE, FAKE, FAKE, 2, 160, 2, 1, 0, None) == _lib.E_ARG


# ------------------------------------------------------------------------------------------------------------ Python
def _gram(**kw):
    import gram_amd
    return gram_amd.create_model("gram", gram_amd.T5Config(vocab_size=256, d_model=128, d_ff=256, num_layers=2, num_decoder_layers=2,
                                                           num_heads=2, max_item_num=5, **kw))


def test_canonical_identities_follow_the_width():
    from gram_amd.model.gram import GRAM
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(2, 250, (2, 224), generator=g)
    ids[1, :128] = ids[0, :128]  # equal in their first 128 tokens
    mask = torch.ones(2, 224, dtype=torch.bool)
    mask[:, 200:] = False
    canon = GRAM._canonical(ids, mask, 256)
    assert canon.shape == (2, 256) and canon.dtype == torch.int32
    assert bool((canon[:, 200:] == -1).all()) and torch.equal(canon[:, :200], ids[:, :200].int())
    assert not torch.equal(canon[0], canon[1])
    keys = GRAM._passage_keys(canon)
    assert keys.dtype == torch.int64 and int(keys[0]) != int(keys[1])
    with pytest.raises(ValueError):
        GRAM._canonical(ids, mask)  # 224 tokens do not fit rows of 128: refused, never cut
    short = GRAM._canonical(ids[:, :96], mask[:, :96])
    assert short.shape == (2, 128)
    # the keys of a width are their own (a cache never mixes widths), and the largest possible sum stays inside int64
    assert GRAM._passage_keys(short).shape == (2,) and (torch.device("cpu"), 128) in GRAM._KEY_MULT and (torch.device("cpu"), 256) in GRAM._KEY_MULT
    worst = GRAM._passage_keys(torch.full((1, 512), 2 ** 15 - 2, dtype=torch.int32))
    assert 0 < int(worst[0]) < 2 ** 15 * 2 ** 31 * 2 ** 9 < 2 ** 63


def test_set_max_passage_len_values():
    m = _gram()
    assert m._max_passage_len == 128 and m._CACHE_L == 128
    for bad in (0, 96, 100, 130, 544, 1024):
        with pytest.raises(ValueError, match="multiple of 32"):
            m.set_max_passage_len(bad)
    m.set_max_passage_len(256)
    assert m._max_passage_len == 256 and m._CACHE_L == 256 and m._pcache is None
    assert type(m)._CACHE_L == 128  # (the setting is the model's own)


@pytest.mark.parametrize("nb,md,ok", [(32, 128, True), (64, 128, True), (16, 64, True), (32, 100, True), (32, 256, False), (32, 192, False), (32, 129, True)])
def test_long_passages_need_buckets_constant_beyond_127(nb, md, ok):
    from gram_amd.model.gram import relative_position_bucket
    m = _gram(relative_attention_num_buckets=nb, relative_attention_max_distance=md)
    rel = torch.arange(-511, 512)
    b = relative_position_bucket(rel, True, nb, md)
    constant = bool((b[rel <= -127] == b[rel == -127]).all() and (b[rel >= 127] == b[rel == 127]).all())
    assert constant == ok
    if ok:
        m.set_max_passage_len(512)
    else:
        with pytest.raises(ValueError, match="not constant"):
            m.set_max_passage_len(256)
        assert m._max_passage_len == 128
    m.set_max_passage_len(128)  # (always allowed)


def test_entry_points_name_the_setter():
    from gram_amd.utils import generation_trie as gt
    m = _gram()
    ids = torch.zeros(2, 3, 150, dtype=torch.long)
    mask = torch.ones(2, 3, 150, dtype=torch.bool)
    fn = gt.prefix_allowed_tokens_fn(gt.Trie([[0, 2, 1]]))
    with pytest.raises(ValueError, match=r"set_max_passage_len\(160\)"):
        m.generate(input_ids=ids, attention_mask=mask, max_length=3, prefix_allowed_tokens_fn=fn, num_beams=2)
    with pytest.raises(ValueError, match=r"set_max_passage_len\(160\)"):
        m._tf_chunks(ids, mask, None, None, None)
    assert m._check_passage_len(128) == 128 and m._check_passage_len(97) == 128
    m.set_max_passage_len(256)
    assert m._check_passage_len(150) == 160
    with pytest.raises(ValueError, match=r"set_max_passage_len\(288\)"):
        m._check_passage_len(260)
    with pytest.raises(ValueError, match="goes up to 512"):
        m._check_passage_len(513)


def test_the_custom_op_is_registered_with_a_fake_impl():
    import gram_amd.ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert hasattr(torch.ops.gram, "enc_self_attn_long")
    with FakeTensorMode():
        qkv = torch.empty(2 * 512, 3 * 128, dtype=_lib.piece_dtype(), device="cuda")
        out = torch.ops.gram.enc_self_attn_long(qkv, torch.empty(2, 255, device="cuda"), torch.empty(2, 512, dtype=torch.uint8, device="cuda"), 2)
        assert out.shape == (1024, 128)
    with pytest.raises((NotImplementedError, RuntimeError)):  # no CPU kernel
        torch.ops.gram.enc_self_attn_long(torch.zeros(64, 384, dtype=_lib.piece_dtype()), torch.zeros(2, 255), torch.ones(2, 32, dtype=torch.uint8), 2)


# ------------------------------------------------------------------------------------------------------------ the launch trains
def _train(case):
    with open(os.path.join(GOLDEN, case + ".txt")) as f:
        return f.read().splitlines()


def test_a_long_handles_train_differs_in_the_encoder_attention_only():
    short, long_ = _train("generate_p1_folded"), _train("generate_long_32")
    assert long_[0] == "gram_model_set_max_passage_len 0"
    long_ = long_[1:]
    assert len(short) == len(long_)
    n = 0
    for a, b in zip(short, long_):
        if a != b:
            assert a.startswith("gram_enc_self_attn_split ") and b == a.replace("gram_enc_self_attn_split", "gram_enc_self_attn_long_split", 1)
            n += 1
    assert n == 2  # one per encoder layer


@pytest.mark.parametrize("case,names", [("generate_long_160", ["gram_enc_self_attn_long_split"] * 2),
                                        ("generate_p2_tables_long_160", ["gram_enc_self_attn_long_rows_split", "gram_enc_self_attn_long_split"])])
def test_the_train_at_160_tokens(case, names):
    """generate at L = 160 on a long handle: the calls of the default train (same names, same order, as generate_p1_folded /
    generate_p2_tables at L = 32) with the encoder attention replaced; with token tables layer 0 reads them"""
    base = _train("generate_p1_folded" if case == "generate_long_160" else "generate_p2_tables")
    got = _train(case)
    assert got[-1] == "return 0"
    calls = [l.split()[0] for l in got if l.split()[0] != "gram_model_set_max_passage_len"]
    assert [c for c in calls if c.startswith("gram_enc_self_attn")] == names
    assert [c.replace("_long", "") for c in calls] == [l.split()[0] for l in base]
    for l in got:
        if l.startswith("gram_enc_self_attn"):
            f = l.split()
            assert f[-6:-3] == ["6", "160", "2"], l  # P, L, H
