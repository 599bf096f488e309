"""The CPU restatement of the teacher-forced pass's cross-attention weights (test infrastructure, not a test module): the oracle's
decoder stepped over the decoder inputs (tests/tf_oracle.py) with oracle.gram_oracle._attend wrapped so that every CROSS-attention
call records softmax(q k^T + bias) -- HF's `cross_attentions`.  tests/test_xattn_scores_host.py pins it against the reference's own
forward(output_attentions=True) (tests/golden/ref_xattn.npz)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import gram_oracle as O  # noqa: E402
from tests import tf_oracle as TF  # noqa: E402


@torch.no_grad()
def cross_attentions(sd, oc, ids, mask, dec, fp64=False):
    """ids / mask (B, N, L); dec (B * C, T) decoder inputs, user-major -> a list of num_decoder_layers tensors (B * C, H, T, N * L):
    the weights of every decoder position over the fused keys.  fp64: the oracle on double weights, the weights recorded in double
    (the reference the device results are compared with); otherwise fp32 throughout, as the reference model computes."""
    if fp64:
        sd = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    rec = []
    inner = O._attend

    def attend(q, k, v, bias):
        # a cross-attention call: its additive bias is the encoder mask alone, one row per key of the bank (the self-attention's
        # carries the relative position bias over the decoded positions)
        cross = bias.dim() == 4 and bias.shape[1] == 1 and bias.shape[2] == 1 and bias.shape[-1] == k.shape[2] == mask[0].numel()
        s = torch.matmul(q, k.transpose(3, 2)) + bias
        w = torch.softmax(s.double() if fp64 else s.float(), dim=-1)
        if cross:
            rec.append(w)
        if not fp64:
            return inner(q, k, v, bias)
        o = torch.matmul(w, v)  # (_attend itself keeps its softmax in fp32: restated here for double operands)
        b, H, ql, dk = o.shape
        return o.transpose(1, 2).contiguous().view(b, ql, H * dk)

    O._attend = attend
    try:
        TF.teacher_forced_logits(sd, oc, ids, mask, dec)
    finally:
        O._attend = inner
    nl, T = oc.num_decoder_layers, dec.shape[1]
    assert len(rec) == nl * T, (len(rec), nl, T)
    # recorded step by step, layer by layer: (R, H, 1, S) each
    return [torch.cat([rec[t * nl + i] for t in range(T)], dim=2) for i in range(nl)]


def passage_scores(ca, mask):
    """get_crossattention_scores' two reductions at every position, in fp64: ca a list of (B, H, T, N * L) weights, mask (B, N, L)
    -> (token_scores (B, T, N, L), scores (B, T, N): NaN for a passage without a valid key)"""
    B, N, L = mask.shape
    w = torch.stack([c.double() for c in ca])  # (nl, B, H, T, S)
    nl, _, H, T, _ = w.shape
    valid = mask.ne(0)
    tok = w.sum(dim=(0, 2)).view(B, T, N, L).masked_fill(~valid[:, None], 0.0)
    return tok, tok.sum(-1) / (valid.sum(-1)[:, None].double() * (nl * H))
