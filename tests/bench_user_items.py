"""Per-user item filters at the bench shape: milliseconds per generate() call at T5-base, beam 20, 3 passages of 128 tokens, the
Beauty Trie (12 101 items), unfiltered, with 20 excluded items per user (a history) and with 1 000 allowed items per user (a
retrieval stage's output) -- what the alive test (two binary searches in the user's sorted list per candidate) costs.  The list
preparation (host validation, upload, gram_user_items_prepare) is inside the filtered calls, as a runner would pay it.  Not
collected by pytest.
    python tests/bench_user_items.py [--batch 4096] [--iters 5] [--precision f16x3] [--runs unfiltered,exclude_20,allow_1000]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--runs", default="unfiltered,exclude_20,allow_1000", help="which of the three runs, comma-separated")
    args = ap.parse_args()
    import gram_amd
    from gram_amd.utils import generation_trie as gt
    dev = torch.device("cuda:0")
    torch.manual_seed(2023)
    model = gram_amd.create_model("gram", gram_amd.T5Config.named("t5-base")).to(dev).eval()
    model.set_precision(args.precision)
    z = np.load(os.path.join(ROOT, "tests", "golden", "tries.npz"))
    cands = [[int(x) for x in row if x >= 0] for row in z["Beauty_cands"]]
    fn = gt.prefix_allowed_tokens_fn(gt.Trie(cands))
    max_length = max(len(c) for c in cands)
    B, K, n = args.batch, 20, len(cands)
    g = torch.Generator().manual_seed(1000)
    ids = torch.randint(2, 32100, (B, 3, 128), generator=g)
    ids[:, :, -1] = 1
    ids_d, mask_d = ids.to(dev), torch.ones(B, 3, 128, dtype=torch.bool, device=dev)
    # distinct items per user: the first columns of a per-user random order
    order = torch.rand(B, n, generator=g).argsort(dim=1)
    runs = (("unfiltered", {}), ("exclude_20", dict(exclude_items=order[:, :20].contiguous(), candidates=cands)),
            ("allow_1000", dict(allowed_items=order[:, :1000].contiguous(), candidates=cands)))
    res = {}
    for name, kw in runs:
        if name not in args.runs.split(","):
            continue

        def call():
            return model.generate(input_ids=ids_d, attention_mask=mask_d, max_length=max_length, prefix_allowed_tokens_fn=fn, num_beams=K,
                                  num_return_sequences=K, output_scores=True, return_dict_in_generate=True, length_penalty=1.0, **kw)
        for _ in range(2):
            out = call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            call()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / args.iters * 1e3
        res[name] = {"generate_ms": round(ms, 2), "users_per_s": round(B / ms * 1e3, 1)}
        # what came back respects the lists
        items = model.sequence_items(out["sequences"], fn, cands).view(B, K).cpu()
        if name == "exclude_20":
            assert not bool((items[:, :, None] == order[:, None, :20]).any()), "an excluded item was returned"
        if name == "allow_1000":
            assert bool(((items[:, :, None] == order[:, None, :1000]).any(dim=2) | (items < 0)).all()), "an item outside the list was returned"
    for name in ("exclude_20", "allow_1000"):
        if name not in res or "unfiltered" not in res:
            continue
        res[name]["over_unfiltered"] = round(res[name]["generate_ms"] / res["unfiltered"]["generate_ms"], 4)
    print(json.dumps({"precision": args.precision, "batch": B, "beams": K, "items": n, **res}))


if __name__ == "__main__":
    main()
