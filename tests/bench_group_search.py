"""Group (diverse) beam search against plain beam search at one shape, in one process: T5-base, 3 passages of 128 tokens, the Beauty
Trie (12 101 items), f16x3, B users, K = 20 -- ``generate(num_beams=20)`` (the unchanged plain path, with the tail pass as shipped and
with it switched off: the group search never takes it) and ``generate(num_beams=20, num_beam_groups=G, diversity_penalty=1.0)`` for
G in 2, 4, 5, 10, 20, alternating: the median of ``--reps`` calls each after a warm-up at the full shape, and every call's time, so
that the run-to-run spread is on the page.  A second pass with per-kind event timing on (gram_prof, kind BEAM: every launch of
beam.hip) gives the search steps' own time per call and per launch, and a last one with the ping-pong GEMM's clock stamps on the
clock the chip held.  No threshold: the expected cost of a group step is G dependent selection rounds, plus the missing tail pass.
Not collected by pytest.
    python tests/bench_group_search.py [--batch 256] [--reps 5] [--precision f16x3]"""
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
GROUPS = (2, 4, 5, 10, 20)


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
    common = dict(input_ids=ids.to(dev), attention_mask=torch.ones(B, 3, 128, dtype=torch.bool, device=dev), max_length=max_length,
                  prefix_allowed_tokens_fn=fn, return_dict_in_generate=True, num_beams=K, num_return_sequences=K, length_penalty=1.0)

    def plain():
        return model.generate(**common)

    def plain_no_tail():
        lib.gram_debug_set_tail_pass(0)
        try:
            return model.generate(**common)
        finally:
            lib.gram_debug_set_tail_pass(-1)

    def groups(G):
        return lambda: model.generate(num_beam_groups=G, diversity_penalty=1.0, **common)

    calls = {"plain": plain, "plain_no_tail": plain_no_tail, **{f"G{G}": groups(G) for G in GROUPS}}

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    distinct = {}
    for name, call in calls.items():  # warm-up of every call at the full shape
        call()
        out = call()
        items = model.sequence_items(out["sequences"], fn, cands).view(B, K)
        # distinct items per user's list of 20 (a group search can return one item twice; -1: a -inf filler row)
        distinct[name] = round(float(torch.tensor([len(set(r.tolist()) - {-1}) for r in items.cpu()], dtype=torch.float32).mean()), 2)
    times = {name: [] for name in calls}
    for _ in range(args.reps):
        for name, call in calls.items():
            times[name].append(timed(call)[0])

    def step_kernels(call):  # event-timed launches of kind BEAM in one call
        lib.gram_prof_enable(1 << _lib.K_BEAM, 1 << 12)
        lib.gram_prof_reset()
        call()
        ms, n, work, dropped = C.c_double(), C.c_int64(), C.c_double(), C.c_int64()
        lib.gram_prof_collect(_lib.K_BEAM, C.byref(ms), C.byref(n), C.byref(work), C.byref(dropped))
        lib.gram_prof_enable(0, 0)
        return {"ms_per_call": round(ms.value, 3), "launches": n.value, "dropped": dropped.value}

    kernels = {name: step_kernels(call) for name, call in calls.items()}
    lib.gram_prof_pp_clock_enable(1)
    _lib.check(lib.gram_prof_pp_clock(None, 1), "pp_clock reset")
    plain()
    groups(5)()
    ghz = C.c_double(0.0)
    _lib.check(lib.gram_prof_pp_clock(C.byref(ghz), 1), "pp_clock")
    lib.gram_prof_pp_clock_enable(0)
    med = {name: statistics.median(t) for name, t in times.items()}
    print(json.dumps({
        "precision": args.precision, "batch": B, "num_beams": K, "items": len(cands), "max_length": max_length, "reps": args.reps,
        "ms_median": {n: round(v, 2) for n, v in med.items()},
        "over_plain": {n: round(v / med["plain"], 4) for n, v in med.items()},
        "over_plain_no_tail": {n: round(v / med["plain_no_tail"], 4) for n, v in med.items()},
        "ms_all": {n: [round(x, 2) for x in t] for n, t in times.items()},
        "spread_ms": {n: round(max(t) - min(t), 2) for n, t in times.items()},
        "step_kernels": kernels, "distinct_items_per_user": distinct,
        "clock_ghz_in_gemm": round(ghz.value, 4) if ghz.value > 0 else None}))


if __name__ == "__main__":
    main()
