"""Generate tests/golden/ref_forward.npz by running THE REFERENCE's teacher-forced forward (imported read-only, build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_forward_golden.py

The reference runners' loss call -- ``model(input_ids=(B,N,L), attention_mask=(B,N,L), labels=(B,T), return_dict=False)``
(single_runner_gram.py:188-193) -- returns (loss, logits, past_key_values, encoder_last_hidden_state); the fixture keeps the inputs,
the loss and the logits:
  tiny_*   the smoke() tiny config (oracle/make_golden.py's), ragged masks with a fully padded passage, labels with -100 tails
  base_*   one T5-base-shaped case: the loss, a logits slice (64 vocabulary columns) and the per-token log-probs of the labels
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


def labels_with_tails(g, B, T, V, lens):
    lab = torch.randint(2, V, (B, T), generator=g)
    for b, n in enumerate(lens):
        lab[b, n - 1] = 1  # EOS ends the item id
        lab[b, n:] = -100
    return lab


def main():
    gram_mod, T5Config, _trie, _eval = import_reference()
    torch.set_num_threads(8)
    out = {}

    cfg = O.OracleConfig(vocab_size=256, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2, max_item_num=5)
    seed = 11
    sd = O.init_state_dict(cfg, seed)
    m = ref_model(gram_mod, T5Config, cfg, sd)
    g = torch.Generator().manual_seed(29)
    B, N, L, T = 3, 3, 32, 7
    ids, mask = ragged_inputs(g, B, N, L, cfg.vocab_size)  # the last user's last passage is fully padded
    lab = labels_with_tails(g, B, T, cfg.vocab_size, [7, 4, 1])
    with torch.no_grad():
        res = m(input_ids=ids, attention_mask=mask, labels=lab, return_dict=False)
    assert len(res) == 4, len(res)
    out.update({k: v for k, v in cfg_arrays(cfg, seed, sd).items()})
    out.update(tiny_ids=ids.numpy(), tiny_mask=mask.numpy(), tiny_labels=lab.numpy(), tiny_loss=res[0].numpy(),
               tiny_logits=res[1].numpy())
    print("tiny: loss", float(res[0]), "logits", tuple(res[1].shape))

    cfgb = O.OracleConfig.named("t5-base")
    seedb = 2023
    sdb = O.init_state_dict(cfgb, seedb)
    mb = ref_model(gram_mod, T5Config, cfgb, sdb)
    g = torch.Generator().manual_seed(31)
    B, N, L, T = 2, 3, 32, 10
    ids, mask = ragged_inputs(g, B, N, L, 32100, pad_passage=False)
    lab = labels_with_tails(g, B, T, 32100, [10, 6])
    with torch.no_grad():
        res = mb(input_ids=ids, attention_mask=mask, labels=lab, return_dict=False)
        logp = torch.log_softmax(res[1].float(), -1)
        tok = torch.where(lab >= 0, logp.gather(-1, lab.clamp(min=0)[..., None])[..., 0], torch.zeros(()))
    cols = torch.randint(0, cfgb.vocab_size, (64,), generator=g)
    arr = cfg_arrays(cfgb, seedb, sdb)
    out.update(base_cfg=arr["cfg"], base_seed=arr["seed"], base_sd_sha256=arr["sd_sha256"], base_ids=ids.numpy(), base_mask=mask.numpy(),
               base_labels=lab.numpy(), base_loss=res[0].numpy(), base_cols=cols.numpy(), base_logits_cols=res[1][..., cols].numpy(),
               base_token_logp=tok.numpy())
    print("t5-base: loss", float(res[0]))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ref_forward.npz"), **out)


if __name__ == "__main__":
    main()
