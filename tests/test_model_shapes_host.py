"""CPU: the acceptance boundary of gram_model_create through the C ABI (include/gram_hip.h).

The library takes any model with vocab, d_model and d_ff positive multiples of 128, d_model <= 1024, an even n_heads <= 16
(inner = 64 * n_heads a multiple of 128, independent of d_model), at least one layer per stack and pieces in {0, 1, 2}; two pieces need
the fp32 lm_head and folded norms.  A shape is either computed correctly (tests/test_gpu_shapes.py holds the accepted side against the
oracle) or refused here with a NULL handle, before anything reads a weight or touches the device.  The descriptors stand on dummy
pointers, as in tests/test_teacher_forced_host.py: create copies the descriptor and reads no weight."""
import ctypes as C

import pytest

from gram_amd import _lib

FAKE = 0x1000
# (d_model, n_heads, d_ff): the shapes tests/test_gpu_shapes.py runs
SHAPES = [(128, 4, 384), (384, 2, 640), (256, 6, 128), (128, 16, 256), (1024, 2, 128), (640, 14, 896)]
BACKBONES = {"tiny": (128, 2, 256), "t5-small": (512, 8, 2048), "t5-base": (768, 12, 3072), "t5-large": (1024, 16, 4096)}


def _create(d_model=128, n_heads=2, d_ff=256, vocab=384, n_enc=2, n_dec=2, pieces=1, lm_head_f32=True, fold_norm=1):
    """gram_model_create on a descriptor over dummy pointers -> (lib, handle or None)"""
    lib = _lib.load()
    keep = []

    def arr(n):
        a = (C.c_void_p * max(n, 1))(*([FAKE] * max(n, 1)))
        keep.append(a)
        return C.cast(a, C.POINTER(C.c_void_p))

    desc = _lib.ModelDesc(vocab=vocab, d_model=d_model, d_ff=d_ff, n_heads=n_heads, n_enc_layers=n_enc, n_dec_layers=n_dec, max_passages=6,
                          tie_word_embeddings=1, use_position_embedding=1, fold_norm=fold_norm, eps=1e-6, embed_f32=FAKE, lm_head_bf16=FAKE,
                          pos_emb_f32=FAKE, enc_bias_f32=FAKE, dec_bias_f32=FAKE, enc_final_ln=FAKE, dec_final_ln=FAKE,
                          enc_ln1=arr(n_enc), enc_wqkv=arr(n_enc), enc_wo=arr(n_enc), enc_ln2=arr(n_enc), enc_wi=arr(n_enc),
                          enc_wo2=arr(n_enc), dec_ln1=arr(n_dec), dec_wqkv=arr(n_dec), dec_wo=arr(n_dec), dec_ln2=arr(n_dec),
                          dec_wq_x=arr(n_dec), dec_wo_x=arr(n_dec), dec_ln3=arr(n_dec), dec_wi=arr(n_dec), dec_wo2=arr(n_dec),
                          dec_wkv_x_all=FAKE, pieces=pieces, lm_head_f32=FAKE if lm_head_f32 else None)
    return lib, lib.gram_model_create(C.byref(desc))


ACCEPTED = ([pytest.param(dict(d_model=d, n_heads=h, d_ff=f), id=f"{d}-{h}-{f}") for d, h, f in SHAPES]
            + [pytest.param(dict(d_model=d, n_heads=h, d_ff=f, vocab=256 if name == "tiny" else 32128), id=name)
               for name, (d, h, f) in BACKBONES.items()]
            + [pytest.param(dict(n_heads=2), id="n_heads=2"), pytest.param(dict(n_heads=16), id="n_heads=16"),
               pytest.param(dict(d_model=1024), id="d_model=1024")])


@pytest.mark.parametrize("pieces", [0, 1, 2])
@pytest.mark.parametrize("kw", ACCEPTED)
def test_accepted_shapes(kw, pieces):
    lib, h = _create(pieces=pieces, **kw)
    assert h, (kw, pieces)
    try:
        ws = lib.gram_workspace_bytes(h, 2, 2, 32, 4, 6)
        assert ws > 0 and ws % 256 == 0, ws
        assert lib.gram_workspace_bytes_tf(h, 2, 2, 32, 4, 6) > 0
    finally:
        lib.gram_model_destroy(h)


REFUSED = [pytest.param(dict(d_model=1152), id="d_model=1152"), pytest.param(dict(d_model=192), id="d_model=192"),
           pytest.param(dict(d_model=0), id="d_model=0"), pytest.param(dict(d_model=-128), id="d_model=-128"),
           pytest.param(dict(d_ff=0), id="d_ff=0"), pytest.param(dict(vocab=0), id="vocab=0"), pytest.param(dict(d_ff=192), id="d_ff=192"),
           pytest.param(dict(vocab=200), id="vocab=200"), pytest.param(dict(n_heads=0), id="n_heads=0"),
           pytest.param(dict(n_heads=3), id="n_heads=3"),  # inner = 192: not a multiple of 128
           pytest.param(dict(n_heads=18), id="n_heads=18"), pytest.param(dict(n_enc=0), id="n_enc_layers=0"),
           pytest.param(dict(n_dec=0), id="n_dec_layers=0"), pytest.param(dict(pieces=3), id="pieces=3"),
           pytest.param(dict(pieces=2, lm_head_f32=False), id="pieces=2 without lm_head_f32"),
           pytest.param(dict(pieces=2, fold_norm=0), id="pieces=2 with fold_norm=0")]


@pytest.mark.parametrize("kw", REFUSED)
def test_refused_shapes(kw):
    lib, h = _create(**kw)
    if h:
        lib.gram_model_destroy(h)
    assert not h, kw
