"""Per-user item masks at a serving shape: milliseconds per generate() call at T5-base, beam 20, 3 passages of 128 tokens, the Beauty
Trie (12 101 items), B = 256 users, f16x3 -- plain beam search with its tail pass switched off (the yardstick: the filtered calls
take none, so this is the same launch train), ``allowed_items`` with 1 000 items per user (two binary searches per alive test),
``item_mask`` with the same 1 000 and ``item_mask`` keeping a random half of the catalogue (two record loads per alive test; the
half is a set no list can say) -- and gram_user_mask_prepare alone at B = 1 and B = 256.  The filters' preparation (host checks,
upload, the preparation kernel) is inside the filtered calls, as a runner would pay it.  Median of --iters calls after a warm-up,
one process, with the spread (min .. max).  Not collected by pytest.
    python tests/bench_item_mask.py [--batch 256] [--iters 5] [--precision f16x3] [--runs plain,allow_1000,mask_1000,mask_half,prepare]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(call, iters, warmup=2):
    """median, min and max of `iters` synchronised calls, in milliseconds; the last call's result"""
    for _ in range(warmup):
        out = call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--runs", default="plain,allow_1000,mask_1000,mask_half,prepare", help="which of the runs, comma-separated")
    args = ap.parse_args()
    import gram_amd
    from gram_amd import _lib
    from gram_amd.utils import generation_trie as gt
    dev = torch.device("cuda:0")
    torch.manual_seed(2023)
    lib = _lib.load()
    z = np.load(os.path.join(ROOT, "tests", "golden", "tries.npz"))
    cands = [[int(x) for x in row if x >= 0] for row in z["Beauty_cands"]]
    trie = gt.Trie(cands)
    fn = gt.prefix_allowed_tokens_fn(trie)
    max_length = max(len(c) for c in cands)
    B, K, n = args.batch, 20, len(cands)
    g = torch.Generator().manual_seed(1000)
    order = torch.rand(B, n, generator=g).argsort(dim=1)  # distinct items per user: the first columns of a per-user random order
    first = order[:, :1000].contiguous()
    mask_1000 = torch.zeros(B, n, dtype=torch.bool).scatter_(1, first, True).to(dev)
    mask_half = torch.zeros(B, n, dtype=torch.bool).scatter_(1, order[:, : n // 2].contiguous(), True).to(dev)
    runs = args.runs.split(",")
    res = {}
    if set(runs) - {"prepare"}:
        model = gram_amd.create_model("gram", gram_amd.T5Config.named("t5-base")).to(dev).eval()
        model.set_precision(args.precision)
        ids = torch.randint(2, 32100, (B, 3, 128), generator=g)
        ids[:, :, -1] = 1
        ids_d, mask_d = ids.to(dev), torch.ones(B, 3, 128, dtype=torch.bool, device=dev)
        cases = (("plain", {}), ("allow_1000", dict(allowed_items=first.to(dev), candidates=cands)),
                 ("mask_1000", dict(item_mask=mask_1000, candidates=cands)), ("mask_half", dict(item_mask=mask_half, candidates=cands)))
        outs = {}
        for name, kw in cases:
            if name not in runs:
                continue

            def call():
                return model.generate(input_ids=ids_d, attention_mask=mask_d, max_length=max_length, prefix_allowed_tokens_fn=fn, num_beams=K,
                                      num_return_sequences=K, output_scores=True, return_dict_in_generate=True, length_penalty=1.0, **kw)
            try:
                if name == "plain":
                    lib.gram_debug_set_tail_pass(0)  # (the filtered calls take no tail pass: the same launch train)
                res[name], outs[name] = timed(call, args.iters)
            finally:
                lib.gram_debug_set_tail_pass(-1)
            res[name]["users_per_s"] = round(B / res[name]["median_ms"] * 1e3, 1)
            items = model.sequence_items(outs[name]["sequences"], fn, cands).view(B, K)
            kept = {"allow_1000": mask_1000, "mask_1000": mask_1000, "mask_half": mask_half}.get(name)
            if kept is not None:  # what came back respects the sets
                assert bool((kept.gather(1, items.clamp(min=0).long()) | (items < 0)).all()), "an item outside the set was returned"
        if "allow_1000" in outs and "mask_1000" in outs:  # the same sets: the same bits
            assert torch.equal(outs["allow_1000"]["sequences"], outs["mask_1000"]["sequences"])
            assert torch.equal(outs["allow_1000"]["sequences_scores"], outs["mask_1000"]["sequences_scores"])
        for name in ("allow_1000", "mask_1000", "mask_half"):
            if name in res and "plain" in res:
                res[name]["over_plain"] = round(res[name]["median_ms"] / res["plain"]["median_ms"], 4)
    if "prepare" in runs:  # the preparation kernel alone, CUDA-event time of 20 back-to-back launches per sample
        flat = gt.FlatTrie(trie)
        leaf_item = flat.leaf_items_on(dev, cands)
        n_leaves = leaf_item.numel()
        stride = int(lib.gram_user_mask_words(n_leaves))
        st = torch.cuda.current_stream(dev).cuda_stream
        for b in sorted({1, B}):
            m8 = mask_half[:b].to(torch.uint8).contiguous()
            words = torch.empty(b, stride, 2, dtype=torch.int32, device=dev)
            count = torch.empty(b, dtype=torch.int32, device=dev)

            def launch():
                _lib.check(lib.gram_user_mask_prepare(m8.data_ptr(), n, b, n, leaf_item.data_ptr(), n_leaves, words.data_ptr(), stride,
                                                      count.data_ptr(), st), "gram_user_mask_prepare")
            for _ in range(5):
                launch()
            us = []
            for _ in range(args.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    launch()
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) / 20 * 1e3)
            assert n_leaves != n or count.tolist() == mask_half[:b].sum(dim=1).tolist()
            res[f"prepare_B{b}"] = {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
                                    "record_bytes": b * stride * 8}
    print(json.dumps({"precision": args.precision, "batch": B, "beams": K, "items": n, "iters": args.iters, **res}))


if __name__ == "__main__":
    main()
