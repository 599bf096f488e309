"""CPU: the teacher-forced forward's host side -- shift-right semantics, the C ABI's argument checks (no GPU needed: shapes are
refused before any launch), and the CPU restatement the GPU tests use (tests/tf_oracle.py) against the reference's own
forward(labels, return_dict=False) in tests/golden/ref_forward.npz."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from gram_amd import _lib
from gram_amd.model.gram import shift_right
from oracle import gram_oracle as O
from tests import tf_oracle as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shift_right_semantics():
    lab = torch.tensor([[5, 6, 1, -100, -100], [7, 1, -100, -100, -100], [-100, 9, 1, 3, 4]])
    want = torch.tensor([[0, 5, 6, 1, 0], [0, 7, 1, 0, 0], [0, 0, 9, 1, 3]])
    assert torch.equal(shift_right(lab), want)
    assert torch.equal(TF.shift_right(lab), want)
    assert torch.equal(shift_right(lab[None]), want[None])  # (B, C, T): along the last dimension


def _fake_model():
    """A gram_model_t over dummy weight pointers: gram_model_create copies the descriptor and reads no weight."""
    lib = _lib.load()
    fake = 0x1000
    keep = []

    def arr(n):
        a = (C.c_void_p * n)(*([fake] * n))
        keep.append(a)
        return C.cast(a, C.POINTER(C.c_void_p))

    desc = _lib.ModelDesc(vocab=256, d_model=128, d_ff=256, n_heads=2, n_enc_layers=1, n_dec_layers=1, max_passages=4,
                          tie_word_embeddings=1, use_position_embedding=1, fold_norm=1, eps=1e-6, embed_f32=fake, lm_head_bf16=fake,
                          pos_emb_f32=fake, enc_bias_f32=fake, dec_bias_f32=fake, enc_final_ln=fake, dec_final_ln=fake,
                          enc_ln1=arr(1), enc_wqkv=arr(1), enc_wo=arr(1), enc_ln2=arr(1), enc_wi=arr(1), enc_wo2=arr(1), dec_ln1=arr(1),
                          dec_wqkv=arr(1), dec_wo=arr(1), dec_ln2=arr(1), dec_wq_x=arr(1), dec_wo_x=arr(1), dec_ln3=arr(1),
                          dec_wi=arr(1), dec_wo2=arr(1), dec_wkv_x_all=fake, pieces=1, lm_head_f32=None)
    h = lib.gram_model_create(C.byref(desc))
    assert h
    return lib, h


def test_teacher_forced_argument_errors_without_gpu():
    lib, h = _fake_model()
    try:
        assert lib.gram_workspace_bytes_tf(h, 2, 3, 32, 20, 64) > 0
        assert lib.gram_workspace_bytes_tf(h, 2, 3, 32, 20, 65) == _lib.E_ARG  # T > GRAM_MAX_DEC_LEN
        assert lib.gram_workspace_bytes_tf(h, 2, 3, 32, 0, 10) == _lib.E_ARG  # C < 1
        assert lib.gram_workspace_bytes_tf(h, 2, 3, 48, 1, 10) == _lib.E_ARG  # L % 32
        assert lib.gram_workspace_bytes_tf(None, 2, 3, 32, 1, 10) == _lib.E_ARG
        # more rows than one call shares with the decoder's workspace: refused, not carved
        assert lib.gram_workspace_bytes_tf(h, 1 << 24, 1, 32, 64, 64) == _lib.E_ARG
        fake = 0x1000
        ws = 1 << 40
        args = lambda C_, T, tok, seq: (h, fake, fake, 2, 3, 32, None, fake, fake, C_, T, fake, ws, None, tok, seq, None)  # noqa: E731
        assert lib.gram_teacher_forced(*args(1, 65, fake, fake)) == _lib.E_ARG
        assert lib.gram_teacher_forced(*args(0, 10, fake, fake)) == _lib.E_ARG
        assert lib.gram_teacher_forced(*args(1, 10, None, fake)) == _lib.E_ARG  # null token_logp
        assert lib.gram_teacher_forced(*args(1, 10, fake, None)) == _lib.E_ARG
        # a workspace too small is GRAM_E_WORKSPACE, also before any launch
        small = (h, fake, fake, 2, 3, 32, None, fake, fake, 1, 10, fake, 1024, None, fake, fake, None)
        assert lib.gram_teacher_forced(*small) == _lib.E_WORKSPACE
    finally:
        lib.gram_model_destroy(h)
    lib = _lib.load()
    f = 0x1000
    assert lib.gram_dec_self_attn_tf_split(f, f, f, 4, 65, 2, 1, 0, None) == _lib.E_ARG
    assert lib.gram_dec_self_attn_tf_split(f, f, f, 4, 10, 2, 2, 10, None) == _lib.E_ARG  # piece stride below the planar size
    assert lib.gram_cross_attn_rows_split(f, f, f, f, f, 2, 200, 2, 96, 1, 0, 0, None, None, None) == _lib.E_ARG  # Q > 64 needs rowmap
    assert lib.gram_label_logprob_split(f, f, None, 128, f, f, 4, 10, 256, 1, None, f, None) == _lib.E_ARG  # null token_logp
    assert lib.gram_label_logprob_split(f, f, None, 128, f, f, 4, 65, 256, 1, f, f, None) == _lib.E_ARG
    assert lib.gram_label_logprob_split(f, f, None, 128, f, f, 4, 10, 256, 2, f, f, None) == _lib.E_ARG  # 2 pieces need the fp32 table


def test_forward_refuses_cpu_and_bad_calls():
    import gram_amd
    cfg = gram_amd.T5Config(vocab_size=256, d_model=128, d_ff=256, num_layers=1, num_decoder_layers=1, num_heads=2, max_item_num=3)
    m = gram_amd.create_model("gram", cfg)
    ids = torch.zeros(1, 1, 32, dtype=torch.long)
    mask = torch.ones(1, 1, 32, dtype=torch.bool)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        m(input_ids=ids, attention_mask=mask, labels=torch.tensor([[5, 1]]), return_dict=False)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        m.score_sequences(ids, mask, torch.tensor([[[5, 1]]]))


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_forward.npz"))


def test_oracle_composition_reproduces_the_reference_forward():
    """Stepped O.decoder_step over _shift_right(labels) + CrossEntropyLoss(ignore_index=-100) = the reference's forward(labels)."""
    z = _golden()
    oc = O.OracleConfig(vocab_size=256, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2, max_item_num=5)
    assert [int(v) for v in z["cfg"]] == [256, 128, 64, 256, 2, 2, 2, 5]
    sd = O.init_state_dict(oc, int(z["seed"]))
    ids, mask, lab = (torch.from_numpy(z["tiny_" + k]) for k in ("ids", "mask", "labels"))
    logits = TF.teacher_forced_logits(sd, oc, ids, mask, TF.shift_right(lab))
    ref = torch.from_numpy(z["tiny_logits"])
    dev = float((logits - ref).abs().max())
    loss, _ = TF.loss_and_token_logp(logits, lab)
    print(f"tiny: max |logit diff| {dev:.2e}, loss {float(loss):.8f} vs {float(z['tiny_loss']):.8f}")
    assert dev < 2e-5
    assert abs(float(loss) - float(z["tiny_loss"])) < 1e-5


def test_oracle_composition_reproduces_the_reference_t5_base():
    z = _golden()
    oc = O.OracleConfig.named("t5-base")
    sd = O.init_state_dict(oc, int(z["base_seed"]))
    ids, mask, lab = (torch.from_numpy(z["base_" + k]) for k in ("ids", "mask", "labels"))
    logits = TF.teacher_forced_logits(sd, oc, ids, mask, TF.shift_right(lab))
    loss, tok = TF.loss_and_token_logp(logits, lab)
    cols = torch.from_numpy(z["base_cols"])
    dl = float((logits[..., cols] - torch.from_numpy(z["base_logits_cols"])).abs().max())
    dt = float((tok - torch.from_numpy(z["base_token_logp"]).double()).abs().max())
    print(f"t5-base: logits slice {dl:.2e}, token logp {dt:.2e}, loss {float(loss):.8f} vs {float(z['base_loss']):.8f}")
    assert dl < 1e-4 and dt < 1e-4
    assert abs(float(loss) - float(z["base_loss"])) < 1e-5 * abs(float(z["base_loss"]))
