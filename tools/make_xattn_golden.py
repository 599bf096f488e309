"""Generate tests/golden/ref_xattn.npz by running THE REFERENCE's forward with output_attentions=True and its own
GRAM.get_crossattention_scores (imported read-only, build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_xattn_golden.py

The tiny config of tools/make_forward_golden.py (seed 11), B = 3 users, N = 3 passages of L = 32, ragged masks with the last user's last
passage fully padded, T = 4 decoder positions.  The fixture keeps
  ids, mask, dec        the inputs (dec = the decoder_input_ids: start token, then random tokens)
  cross_attentions      f32 [n_dec_layers][B][H][T][N*L]: forward(decoder_input_ids=dec, output_attentions=True).cross_attentions
  first_*               the T = 1 pass (decoder_input_ids = zeros(B, 1)): first_cross_attentions [n_dec_layers][B][H][1][N*L], and per
                        user b the reference's get_crossattention_scores([ca], mask[b:b+1], b_idx=b): first_token_scores [B][N][L],
                        first_scores [B][N] (NaN for the fully padded passage: its 0 / 0)
Nothing at test, smoke or bench time imports this script; the tests read only the .npz.
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gram_oracle as O  # noqa: E402
from oracle.make_golden import cfg_arrays, import_reference, ragged_inputs, ref_model  # noqa: E402


def main():
    gram_mod, T5Config, _trie, _eval = import_reference()
    torch.set_num_threads(8)
    cfg = O.OracleConfig(vocab_size=256, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2, max_item_num=5)
    seed = 11
    sd = O.init_state_dict(cfg, seed)
    m = ref_model(gram_mod, T5Config, cfg, sd)
    g = torch.Generator().manual_seed(29)
    B, N, L, T = 3, 3, 32, 4
    ids, mask = ragged_inputs(g, B, N, L, cfg.vocab_size)  # the last user's last passage is fully padded
    dec = torch.randint(2, cfg.vocab_size, (B, T), generator=g)
    dec[:, 0] = 0
    with torch.no_grad():
        res = m(input_ids=ids, attention_mask=mask, decoder_input_ids=dec, output_attentions=True, return_dict=True)
        ca = res.cross_attentions
        assert len(ca) == cfg.num_decoder_layers and tuple(ca[0].shape) == (B, cfg.num_heads, T, N * L), [tuple(c.shape) for c in ca]
        first = m(input_ids=ids, attention_mask=mask, decoder_input_ids=torch.zeros(B, 1, dtype=torch.long), output_attentions=True,
                  return_dict=True).cross_attentions
        tok, sc = [], []
        for b in range(B):
            t, s = m.get_crossattention_scores([first], mask[b:b + 1], b_idx=b)
            tok.append(np.asarray(t, dtype=np.float32))
            sc.append(s.numpy()[0])
    out = dict(cfg_arrays(cfg, seed, sd))
    out.update(ids=ids.numpy(), mask=mask.numpy(), dec=dec.numpy(), cross_attentions=torch.stack(list(ca)).numpy(),
               first_cross_attentions=torch.stack(list(first)).numpy(), first_token_scores=np.stack(tok), first_scores=np.stack(sc))
    for k in ("cross_attentions", "first_cross_attentions", "first_token_scores", "first_scores"):
        print(k, out[k].shape, out[k].dtype)
    print("first_scores", out["first_scores"])
    masked = ~mask.reshape(B, 1, 1, N * L).expand(B, cfg.num_heads, T, N * L).numpy()
    assert all((c.numpy()[masked] == 0).all() for c in ca), "masked keys are exact zeros in the reference"
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ref_xattn.npz"), **out)


if __name__ == "__main__":
    main()
