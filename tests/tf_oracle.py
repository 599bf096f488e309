"""The CPU restatement of the teacher-forced forward the tests compare the HIP path with (test infrastructure, not a test module):
the oracle's cached decoder stepped over the decoder inputs with one bank per row (rows_per_bank = 1), then CrossEntropyLoss
(ignore_index=-100).  tests/test_teacher_forced_host.py pins it against the reference's own forward (tests/golden/ref_forward.npz).

    python tests/tf_oracle.py --child OUT.pt     one fixed score_sequences case in a process of its own (GRAM_LIB selects the
                                                 library): the race screen of tests/test_gpu_teacher_forced.py"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import gram_oracle as O  # noqa: E402


def shift_right(labels):
    """_shift_right (gram_t5_modeling.py:935-964), restated: start token 0, -100 -> pad 0."""
    out = torch.zeros_like(labels)
    out[..., 1:] = labels[..., :-1]
    return out.masked_fill(out == -100, 0)


@torch.no_grad()
def teacher_forced_logits(sd, oc, ids, mask, dec):
    """ids / mask (B, N, L); dec (B * C, T) decoder inputs, user-major -> logits f32 (B * C, T, V)."""
    B = ids.shape[0]
    R, T = dec.shape
    C = R // B
    enc = O.encode_fused(sd, oc, ids, mask).repeat_interleave(C, 0)
    m = mask.reshape(B, -1).repeat_interleave(C, 0).float()
    ext = ((1.0 - m) * O.FMIN)[:, None, None, :]
    st = O.DecodeState(cross=O.cross_kv(sd, oc, enc), enc_mask_ext=ext, rows_per_bank=1)
    return torch.stack([O.decoder_step(sd, oc, dec[:, t], st) for t in range(T)], 1)


def loss_and_token_logp(logits, labels):
    """CrossEntropyLoss(ignore_index=-100) (gram_t5.py:256-260) and log_softmax(logits)[label] (0 where ignored)."""
    loss = torch.nn.functional.cross_entropy(logits.reshape(-1, logits.shape[-1]).double(), labels.reshape(-1), ignore_index=-100)
    lp = torch.log_softmax(logits.double(), -1).gather(-1, labels.clamp(min=0)[..., None])[..., 0]
    return loss, torch.where(labels >= 0, lp, torch.zeros((), dtype=lp.dtype))


def _child(out_path):
    import gram_amd
    cfg = gram_amd.T5Config.named("t5-small")
    torch.manual_seed(7)
    model = gram_amd.create_model("gram", cfg).to("cuda:0").eval()
    g = torch.Generator().manual_seed(8)
    B, N, L, C, T = 24, 3, 64, 20, 10
    ids = torch.randint(2, cfg.vocab_size, (B, N, L), generator=g)
    mask = torch.ones(B, N, L, dtype=torch.bool)
    lens = torch.randint(16, L + 1, (B, N), generator=g)
    for b in range(B):
        for n in range(N):
            mask[b, n, lens[b, n]:] = False
    labels = torch.randint(2, cfg.vocab_size, (B, C, T), generator=g)
    labels[:, :, 7:] = -100
    seq, tok = model.score_sequences(ids.cuda(), mask.cuda(), labels.cuda(), return_tokens=True)
    torch.save(dict(seq=seq.cpu(), tok=tok.cpu()), out_path)


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(sys.argv[2])
