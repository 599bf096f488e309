"""CPU: the host side of the cross-attention probabilities and per-passage scores -- the CPU restatement the GPU tests use
(tests/xattn_oracle.py) and GRAM.get_crossattention_scores against the reference's own outputs (tests/golden/ref_xattn.npz, written by
tools/make_xattn_golden.py), the C ABI's argument checks (refused before any launch: no GPU needed) and the ctypes mirror of
gram_xattn_out_t against the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

import gram_amd
from gram_amd import _lib
from oracle import gram_oracle as O
from tests import xattn_oracle as XO
from tests.test_teacher_forced_host import _fake_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_xattn.npz"))


def _tiny(z):
    oc = O.OracleConfig(vocab_size=256, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2, max_item_num=5)
    assert [int(v) for v in z["cfg"]] == [256, 128, 64, 256, 2, 2, 2, 5]
    return oc, O.init_state_dict(oc, int(z["seed"]))


def test_oracle_reproduces_the_reference_cross_attentions():
    """forward(decoder_input_ids, output_attentions=True).cross_attentions of the reference, T = 4 and the T = 1 first-token pass:
    within 2e-6 max abs (fp32 against fp32: the margin covers thread-count-dependent summation; measured 3.4e-7), masked keys exactly 0."""
    z = _golden()
    oc, sd = _tiny(z)
    ids, mask, dec = (torch.from_numpy(z[k]) for k in ("ids", "mask", "dec"))
    B, N, L = ids.shape
    assert not bool(mask[B - 1, N - 1].any())  # the fully padded passage
    for name, d in (("cross_attentions", dec), ("first_cross_attentions", torch.zeros(B, 1, dtype=torch.long))):
        ref = torch.from_numpy(z[name])
        got = torch.stack(XO.cross_attentions(sd, oc, ids, mask, d))
        assert got.shape == ref.shape == (oc.num_decoder_layers, B, oc.num_heads, d.shape[1], N * L)
        err = float((got - ref).abs().max())
        print(f"{name}: max abs deviation from the reference {err:.2e}")
        assert err <= 2e-6
        masked = ~mask.reshape(1, B, 1, 1, N * L).expand_as(ref)
        assert bool((got[masked] == 0).all()) and bool((ref[masked] == 0).all())
        assert float((got.double().sum(-1) - 1).abs().max()) < 1e-6


def test_get_crossattention_scores_matches_the_reference():
    """gram_amd.GRAM.get_crossattention_scores on the reference's own cross_attentions = the reference's get_crossattention_scores, per
    user of a B = 3 batch: token and passage scores within 1e-6 relative (fp32 sums), NaN where the reference has NaN."""
    z = _golden()
    ca = [list(torch.from_numpy(z["first_cross_attentions"]))]  # [token][layer] of (B, H, 1, N*L)
    mask = torch.from_numpy(z["mask"])
    B, N, L = mask.shape
    for b in range(B):
        tok, sc = gram_amd.GRAM.get_crossattention_scores(ca, mask[b:b + 1], b_idx=b)
        assert isinstance(tok, list) and len(tok) == N and all(len(r) == L for r in tok)
        assert isinstance(sc, torch.Tensor) and sc.shape == (1, N)
        ref_tok, ref_sc = z["first_token_scores"][b], z["first_scores"][b]
        np.testing.assert_allclose(np.asarray(tok, dtype=np.float64), ref_tok, rtol=1e-6, atol=0)
        assert np.array_equal(np.isnan(sc.numpy()[0]), np.isnan(ref_sc))
        ok = ~np.isnan(ref_sc)
        np.testing.assert_allclose(sc.numpy()[0][ok], ref_sc[ok], rtol=1e-6, atol=0)
    assert np.isnan(z["first_scores"][B - 1, N - 1]) and int(np.isnan(z["first_scores"]).sum()) == 1
    # the oracle's fp64 reduction (what the GPU tests compare passage_attention with) agrees with the reference's too
    tok64, sc64 = XO.passage_scores(ca[0], mask)
    np.testing.assert_allclose(tok64[:, 0].numpy(), z["first_token_scores"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(sc64[:, 0].numpy(), z["first_scores"], rtol=1e-6, atol=0, equal_nan=True)
    # an instance method too, as in the reference
    cfg = gram_amd.T5Config(vocab_size=256, d_model=128, d_ff=256, num_layers=1, num_decoder_layers=1, num_heads=2, max_item_num=3)
    tok_m, sc_m = gram_amd.create_model("gram", cfg).get_crossattention_scores(ca, mask[:1], 0)
    assert torch.equal(sc_m, gram_amd.GRAM.get_crossattention_scores(ca, mask[:1], 0)[1])


def test_xattn_argument_errors_without_gpu():
    lib = _lib.load()
    f = 0x1000
    E = _lib.E_ARG
    # (q, k_layer, mask, probs, B, Q, H, S, pieces, q_pstride, bank_pstride, key_bits, stream)
    assert lib.gram_cross_attn_probs_split(f, f, f, f, 2, 0, 2, 96, 1, 0, 0, None, None) == E  # Q < 1
    assert lib.gram_cross_attn_probs_split(f, f, f, f, 2, 5, 2, 100, 1, 0, 0, None, None) == E  # S % 32
    assert lib.gram_cross_attn_probs_split(f, f, f, f, 2, 5, 2, 4128, 1, 0, 0, None, None) == E  # S > 4096
    assert lib.gram_cross_attn_probs_split(f, f, f, f, 2, 5, 2, 96, 3, 1 << 20, 1 << 20, None, None) == E  # pieces 3
    planar_q, planar_k = 2 * 5 * 2 * 64, 2 * 96 * 64
    assert lib.gram_cross_attn_probs_split(f, f, f, f, 2, 5, 2, 96, 2, planar_q - 1, planar_k, None, None) == E  # piece strides below
    assert lib.gram_cross_attn_probs_split(f, f, f, f, 2, 5, 2, 96, 2, planar_q, planar_k - 1, None, None) == E  # the planar sizes
    assert lib.gram_cross_attn_probs_split(f, f, f, None, 2, 5, 2, 96, 1, 0, 0, None, None) == E  # null probs
    assert lib.gram_cross_attn_probs_split(None, f, f, f, 2, 5, 2, 96, 1, 0, 0, None, None) == E
    assert lib.gram_cross_attn_probs_split(f, f, f, f + 4, 2, 5, 2, 96, 1, 0, 0, None, None) == E  # probs not 16-byte aligned
    assert lib.gram_xattn_head_sum(None, f, 2, 5, 2, 96, 1, None) == E
    assert lib.gram_xattn_head_sum(f, f, 2, 5, 2, 98, 1, None) == E  # S % 4
    assert lib.gram_xattn_passage_scores(f, f, None, 2, 5, 3, 32, 4.0, None) == E
    assert lib.gram_xattn_passage_scores(f, f, f, 2, 5, 3, 32, 0.0, None) == E  # denom
    lib, h = _fake_model()
    try:
        ws = 1 << 40

        def args(attn, T=10):
            return (h, f, f, 2, 3, 32, None, f, f, 1, T, f, ws, None, f, f, C.byref(attn) if attn is not None else None, None)

        assert lib.gram_teacher_forced_ex(*args(_lib.XattnOut(None, None, f, None))) == E  # probs and layer_probs both null
        assert lib.gram_teacher_forced_ex(*args(_lib.XattnOut(f, None, None, f))) == E  # passage_scores without token_scores
        assert lib.gram_teacher_forced_ex(*args(_lib.XattnOut(f, None, None, None), T=65)) == E  # the pass's own shape checks first
        small = (h, f, f, 2, 3, 32, None, f, f, 1, 10, f, 1024, None, f, f, C.byref(_lib.XattnOut(f, None, None, None)), None)
        assert lib.gram_teacher_forced_ex(*small) == _lib.E_WORKSPACE  # (a valid request reaches the workspace check: no launch either)
    finally:
        lib.gram_model_destroy(h)


def test_xattn_out_struct_matches_the_header(tmp_path):
    """gram_xattn_out_t against its ctypes mirror: total size and the offset of every field, from a C program compiled against the header."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gram_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(gram_xattn_out_t));']
    for fname, _ in _lib.XattnOut._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(gram_xattn_out_t, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines() if ln.strip())
    assert int(got["size"]) == C.sizeof(_lib.XattnOut) == 32
    assert [f for f, _ in _lib.XattnOut._fields_] == ["probs", "layer_probs", "token_scores", "passage_scores"]
    for fname, _ in _lib.XattnOut._fields_:
        assert int(got[fname]) == getattr(_lib.XattnOut, fname).offset, fname


def test_attention_methods_refuse_cpu():
    import pytest
    cfg = gram_amd.T5Config(vocab_size=256, d_model=128, d_ff=256, num_layers=1, num_decoder_layers=1, num_heads=2, max_item_num=3)
    m = gram_amd.create_model("gram", cfg)
    ids = torch.zeros(1, 1, 32, dtype=torch.long)
    mask = torch.ones(1, 1, 32, dtype=torch.bool)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        m.cross_attentions(ids, mask, decoder_input_ids=torch.zeros(1, 1, dtype=torch.long))
    with pytest.raises(NotImplementedError, match="no CPU path"):
        m.passage_attention(ids, mask, torch.tensor([[[5, 1]]]))
