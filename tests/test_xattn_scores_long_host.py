"""CPU: the host side of the head-summed token scores over up to 16 384 fused keys -- every refusal of
gram_cross_attn_token_scores_split and gram_teacher_forced_scores through the C ABI on dummy pointers (each comes back before any
launch: no GPU needed), the workspace check behind them, gram_xattn_scores_t against its ctypes mirror, ``GRAM.passage_attention``'s
``fused`` argument with its error texts, and the fake implementation of torch.ops.gram.teacher_forced_scores.  The launch trains
(tests/golden/launch_train/tf_scores_fused_*.txt) are held against the tool by tests/test_launch_train.py."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from gram_amd import _lib
from tests.test_fused_len_host import FAKE, _create, _gram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = _lib.E_ARG


def _kernel(lib, q=FAKE, k=FAKE, acc=FAKE, B=2, Q=5, H=2, S=4128, pieces=1, q_ps=0, bank_ps=0, bits=FAKE, first=1):
    return lib.gram_cross_attn_token_scores_split(q, k, acc, B, Q, H, S, pieces, q_ps, bank_ps, bits, first, None)


def test_token_scores_kernel_argument_errors_without_gpu():
    lib = _lib.load()
    for name in ("q", "k", "acc", "bits"):
        assert _kernel(lib, **{name: None}) == E, name  # a null pointer
        assert _kernel(lib, **{name: FAKE + 8}) == E, name  # not 16-byte aligned
    for S in (0, 16, 100, 4100, 16416, 32768):
        assert _kernel(lib, S=S) == E, S
    assert _kernel(lib, Q=0) == E and _kernel(lib, Q=-3) == E
    assert _kernel(lib, H=0) == E and _kernel(lib, H=17) == E
    assert _kernel(lib, B=0) == E and _kernel(lib, B=65536) == E  # users are a grid dimension
    assert _kernel(lib, pieces=0) == E and _kernel(lib, pieces=3, q_ps=1 << 30, bank_ps=1 << 30) == E
    planar_q, planar_k = 2 * 5 * 2 * 64, 2 * 4128 * 64
    assert _kernel(lib, pieces=2, q_ps=planar_q - 8, bank_ps=planar_k) == E  # piece strides shorter than the rows
    assert _kernel(lib, pieces=2, q_ps=planar_q, bank_ps=planar_k - 8) == E
    assert _kernel(lib, B=1, Q=32 * 65535 + 1) == E  # more than 65 535 row tiles


def _tf_args(h, scores, N=21, L=224, T=6, ws=1 << 40, mask=FAKE, labels=FAKE):
    return (h, FAKE, mask, 2, N, L, None, FAKE, labels, 2, T, FAKE, ws, None, FAKE, FAKE, C.byref(scores) if scores is not None else None, None)


def test_teacher_forced_scores_argument_errors_without_gpu():
    ok = _lib.XattnScores(FAKE, FAKE)
    lib, h = _create()
    try:
        # a default handle: its workspace holds the short key bits (refused at a shape it takes and at one it does not)
        assert lib.gram_teacher_forced_scores(*_tf_args(h, ok, N=3, L=32)) == E
        assert lib.gram_teacher_forced_scores(*_tf_args(h, ok)) == E
        before = lib.gram_workspace_bytes_tf(h, 2, 3, 32, 2, 6)
        assert lib.gram_model_set_max_fused_len(h, 16384) == 0
        assert lib.gram_model_set_max_passage_len(h, 512) == 0
        assert lib.gram_teacher_forced_scores(*_tf_args(h, None)) == E  # no outputs
        assert lib.gram_teacher_forced_scores(*_tf_args(h, _lib.XattnScores(None, FAKE))) == E  # token_scores is required
        assert lib.gram_teacher_forced_scores(*_tf_args(h, _lib.XattnScores(FAKE + 4, None))) == E  # and 16-byte aligned
        assert lib.gram_teacher_forced_scores(*_tf_args(None, ok)) == E
        # the pass's own checks
        assert lib.gram_teacher_forced_scores(*_tf_args(h, ok, T=65)) == E
        assert lib.gram_teacher_forced_scores(*_tf_args(h, ok, N=33, L=512)) == E  # 16 896 fused keys
        assert lib.gram_teacher_forced_scores(*_tf_args(h, ok, mask=None)) == E
        assert lib.gram_teacher_forced_scores(*_tf_args(h, ok, labels=None)) == E
        big = list(_tf_args(h, ok, N=3, L=32, T=1, ws=16))  # more users than the kernel's grid takes: refused here, not in layer 0
        big[3], big[9] = 65536, 1
        assert lib.gram_teacher_forced_scores(*big) == E
        big[3] = 65535
        assert lib.gram_teacher_forced_scores(*big) == _lib.E_WORKSPACE
        # accepted shapes reach the workspace check (no launch either): below and above 4096 keys, with and without passage scores
        for N, L in ((3, 32), (21, 160), (21, 224), (32, 512)):
            assert lib.gram_teacher_forced_scores(*_tf_args(h, ok, N=N, L=L, ws=16)) == _lib.E_WORKSPACE, (N, L)
        assert lib.gram_teacher_forced_scores(*_tf_args(h, _lib.XattnScores(FAKE, None), ws=16)) == _lib.E_WORKSPACE
        # the attention struct of gram_teacher_forced_ex keeps its limit on the same handle
        attn = _lib.XattnOut(FAKE, None, None, None)
        assert lib.gram_teacher_forced_ex(h, FAKE, FAKE, 2, 21, 224, None, FAKE, FAKE, 2, 6, FAKE, 16, None, FAKE, FAKE, C.byref(attn), None) == E
        assert lib.gram_cross_attn_probs_split(FAKE, FAKE, FAKE, FAKE, 2, 4, 2, 4128, 1, 0, 0, None, None) == E
        assert before > 0 and lib.gram_workspace_bytes_tf(h, 2, 21, 224, 2, 6) > 0
    finally:
        lib.gram_model_destroy(h)
    assert _lib.ABI_VERSION == 7


def test_xattn_scores_struct_matches_the_header(tmp_path):
    """gram_xattn_scores_t against its ctypes mirror (size and every offset, from a C program compiled against the header);
    gram_xattn_out_t keeps its 32 bytes."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gram_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(gram_xattn_scores_t));', '  printf("out %zu\\n", sizeof(gram_xattn_out_t));']
    for fname, _ in _lib.XattnScores._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(gram_xattn_scores_t, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines() if ln.strip())
    assert int(got["size"]) == C.sizeof(_lib.XattnScores) == 16 and int(got["out"]) == C.sizeof(_lib.XattnOut) == 32
    assert [f for f, _ in _lib.XattnScores._fields_] == ["token_scores", "passage_scores"]
    for fname, _ in _lib.XattnScores._fields_:
        assert int(got[fname]) == getattr(_lib.XattnScores, fname).offset, fname


def test_passage_attention_refusals():
    ids = torch.zeros(2, 21, 224, dtype=torch.long)
    mask = torch.ones(2, 21, 224, dtype=torch.bool)
    lab = torch.ones(2, 1, 2, dtype=torch.long)
    m = _gram()
    m.set_max_passage_len(256)
    # a default model: fused=True names the way out at any S; above 4096 keys the default path does too, with the size
    with pytest.raises(ValueError, match=r"fused=True.*set_max_fused_tokens"):
        m.passage_attention(ids[:, :3], mask[:, :3], lab, fused=True)
    with pytest.raises(ValueError, match=r"set_max_fused_tokens\(4704\) first"):
        m.passage_attention(ids, mask, lab)
    with pytest.raises(ValueError, match="limited to 4096 fused tokens"):
        m.passage_attention(ids, mask, lab, fused=False)
    m.set_max_fused_tokens(16384)
    with pytest.raises(ValueError, match="limited to 4096 fused tokens"):  # a raised model: fused=False keeps its limit
        m.passage_attention(ids, mask, lab, fused=False)
    with pytest.raises(ValueError, match="limited to 4096 fused tokens"):
        m._teacher_forced_attn(ids, mask, lab, lab, False, True)
    # everything else passed: the CPU device is what stops these
    for kw in (dict(), dict(fused=True), dict(fused=None)):
        with pytest.raises(NotImplementedError, match="no CPU path"):
            m.passage_attention(ids, mask, lab, **kw)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        m.passage_attention(ids[:, :3], mask[:, :3], lab, fused=False)
    with pytest.raises(ValueError, match="set_max_fused_tokens"):  # (the helper itself, on a model that was not raised)
        _gram()._teacher_forced_scores(ids[:, :3], mask[:, :3], lab, lab)


def test_the_custom_op_is_registered_with_a_fake_implementation():
    import gram_amd.ops as ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert hasattr(torch.ops.gram, "teacher_forced_scores") and "teacher_forced_scores" in ops.__all__
    with FakeTensorMode():
        ids = torch.empty(2, 21, 224, dtype=torch.int64, device="cuda")
        dec = torch.empty(2, 3, 4, dtype=torch.int32, device="cuda")
        ws = torch.empty(1024, dtype=torch.uint8, device="cuda")
        tok, sc = torch.ops.gram.teacher_forced_scores(ids, ids.to(torch.uint8), 0, ws, dec, dec, 256, None, None, None, None, None, 0, 0)
        assert tok.shape == (2, 12, 4704) and sc.shape == (2, 12, 21) and tok.dtype == sc.dtype == torch.float32
    with pytest.raises((NotImplementedError, RuntimeError)):  # no CPU kernel
        ids = torch.zeros(1, 3, 32, dtype=torch.int64)
        dec = torch.zeros(1, 1, 2, dtype=torch.int32)
        torch.ops.gram.teacher_forced_scores(ids, ids.to(torch.uint8), 0, torch.zeros(16, dtype=torch.uint8), dec, dec, 256, None, None, None,
                                             None, None, 0, 0)
