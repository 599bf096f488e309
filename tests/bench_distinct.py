"""Sampling without replacement against sampling with replacement and beam search at one shape, in one process: T5-base, 3 passages
of 128 tokens, the Beauty Trie (12 101 items), f16x3, B users, 20 rows per user -- ``generate(do_sample=True, replacement=False)``,
``generate(do_sample=True)`` and ``generate(num_beams=20)`` alternating, the median of ``--reps`` calls each after a warm-up at the
full shape, and the spread of each.  Sampling of either kind decodes every row at every step; beam search drops finished rows and,
at this batch, decodes the Trie's tail in one pass.  A second pass with per-kind event timing on (gram_prof, kind BEAM: every
launch of beam.hip, sample.hip and sbs.hip) reports the step kernels' own time in each of the three.  Not collected by pytest.
    python tests/bench_distinct.py [--batch 256] [--reps 5] [--precision f16x3]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import gram_amd
    from gram_amd import _lib
    from gram_amd.utils import generation_trie as gt
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(2023)
    model = gram_amd.create_model("gram", gram_amd.T5Config.named("t5-base")).to(dev).eval()
    model.set_precision(args.precision)
    z = np.load(os.path.join(ROOT, "tests", "golden", "tries.npz"))
    cands = [[int(x) for x in row if x >= 0] for row in z["Beauty_cands"]]
    fn = gt.prefix_allowed_tokens_fn(gt.Trie(cands))
    max_length = max(len(c) for c in cands)
    B, K = args.batch, 20
    g = torch.Generator().manual_seed(1000)
    ids = torch.randint(2, 32100, (B, 3, 128), generator=g)
    ids[:, :, -1] = 1
    ids_d, mask_d = ids.to(dev), torch.ones(B, 3, 128, dtype=torch.bool, device=dev)
    uniforms = torch.rand(B, K, max_length - 1, generator=g).to(dev)
    keys = torch.arange(B, dtype=torch.int64, device=dev)
    common = dict(input_ids=ids_d, attention_mask=mask_d, max_length=max_length, prefix_allowed_tokens_fn=fn, return_dict_in_generate=True)
    calls = {
        "distinct": lambda: model.generate(do_sample=True, num_beams=1, num_return_sequences=K, replacement=False, seed=7, user_keys=keys,
                                           **common),
        "sample": lambda: model.generate(do_sample=True, num_beams=1, num_return_sequences=K, uniforms=uniforms, **common),
        "beam": lambda: model.generate(num_beams=K, num_return_sequences=K, output_scores=True, length_penalty=1.0, **common),
    }

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(2):  # warm-up of all three at the full shape (the workspace is sized once: the largest of the three)
        outs = {k: c() for k, c in calls.items()}
    items = model.sequence_items(outs["distinct"]["sequences"], fn, cands).view(B, K)
    assert bool((items >= 0).all()), "a returned row is not a candidate"
    assert all(len(set(r)) == K for r in items.tolist()), "a user's rows are not distinct"
    distinct_with = statistics.mean(len(set(r)) for r in model.sequence_items(outs["sample"]["sequences"], fn, cands).view(B, K).tolist())
    times = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, c in calls.items():
            times[k].append(timed(c)[0])

    def step_kernels(call):  # event-timed launches of kind BEAM in one call
        lib.gram_prof_enable(1 << _lib.K_BEAM, 1 << 12)
        lib.gram_prof_reset()
        call()
        ms, n, work, dropped = C.c_double(), C.c_int64(), C.c_double(), C.c_int64()
        lib.gram_prof_collect(_lib.K_BEAM, C.byref(ms), C.byref(n), C.byref(work), C.byref(dropped))
        lib.gram_prof_enable(0, 0)
        return {"ms_per_call": round(ms.value, 3), "launches": n.value, "dropped": dropped.value}

    res = {"precision": args.precision, "batch": B, "rows_per_user": K, "items": len(cands), "max_length": max_length, "reps": args.reps,
           "distinct_items_per_user_with_replacement": round(distinct_with, 2)}
    for k in calls:
        res[k + "_ms_median"] = round(statistics.median(times[k]), 2)
        res[k + "_ms_all"] = [round(t, 2) for t in times[k]]
        res[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 2)
    res["distinct_over_sample"] = round(res["distinct_ms_median"] / res["sample_ms_median"], 4)
    res["distinct_over_beam"] = round(res["distinct_ms_median"] / res["beam_ms_median"], 4)
    for k, c in calls.items():
        res["step_kernels_" + k] = step_kernels(c)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
