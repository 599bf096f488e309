"""Beam search with per-item score biases against plain beam search at one shape, in one process: T5-base, 3 passages of 128 tokens,
the Beauty Trie (12 101 items), f16x3, B users, K = 20 -- ``generate(num_beams=20)`` (the unchanged plain path, with the tail pass
as shipped and with it switched off: the biased search never takes it, so THAT is its yardstick: the same launch train),
``exclude_items`` with 20 entries per user, and ``generate(item_bias=T)`` with a zero bias (the biased code on the plain search's
decisions), with one bias row shared by all users and with one per user, alternating: the median of ``--reps`` calls each after a warm-up at the full shape, and every call's time, so that the
run-to-run spread is on the page.  Then gram_item_bias_table alone (torch.ops.gram.item_bias_table, event-timed) at rows = 1 and
rows = B, and a pass with per-kind event timing on (gram_prof, kind BEAM: every launch of beam.hip) for the search steps' own time
per call.  No threshold.  Not collected by pytest.
    python tests/bench_item_bias.py [--batch 256] [--reps 5] [--precision f16x3]"""
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
    common = dict(input_ids=ids.to(dev), attention_mask=torch.ones(B, 3, 128, dtype=torch.bool, device=dev), max_length=max_length,
                  prefix_allowed_tokens_fn=fn, return_dict_in_generate=True, num_beams=K, num_return_sequences=K, length_penalty=1.0)
    shared = (torch.randn(len(cands), generator=g) * 1.5).clamp_(-4, 4).to(dev)
    per_user = (torch.randn(B, len(cands), generator=g) * 1.5).clamp_(-4, 4).to(dev)
    excl = torch.stack([torch.randperm(len(cands), generator=g)[:20] for _ in range(B)]).to(torch.int32)

    def plain():
        return model.generate(**common)

    def plain_no_tail():
        lib.gram_debug_set_tail_pass(0)
        try:
            return model.generate(**common)
        finally:
            lib.gram_debug_set_tail_pass(-1)

    calls = {"plain": plain, "plain_no_tail": plain_no_tail,
             "exclude_20": lambda: model.generate(exclude_items=excl, candidates=cands, **common),
             # a zero bias takes the biased kernels and the plain search's decisions: the cost of the code alone
             "bias_zero": lambda: model.generate(item_bias=torch.zeros_like(shared), candidates=cands, **common),
             "bias_shared": lambda: model.generate(item_bias=shared, candidates=cands, **common),
             "bias_per_user": lambda: model.generate(item_bias=per_user, candidates=cands, **common)}

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    changed = {}
    base = None
    for name, call in calls.items():  # warm-up of every call at the full shape
        call()
        items = model.sequence_items(call()["sequences"], fn, cands).view(B, K).cpu()
        base = items if base is None else base
        changed[name] = int((items != base).any(dim=1).sum())  # users whose list differs from the plain one
    times = {name: [] for name in calls}
    for _ in range(args.reps):
        for name, call in calls.items():
            times[name].append(timed(call)[0])

    # the potentials kernel alone
    flat = model._flat_trie(fn)
    _c, (t_off, t_tok, t_node) = flat.to_device(dev)
    lo, hi = flat.leaf_ranges_on(dev)
    li = flat.leaf_items_on(dev, cands)
    table = {}
    for rows, T in ((1, shared.view(1, -1)), (B, per_user)):
        def run():
            return torch.ops.gram.item_bias_table(T, li, lo, hi, t_off, t_tok, t_node, int(flat.max_fanout), int(flat.min_seq_len), 0, True)
        run()
        torch.cuda.synchronize()
        us = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            phi = run()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        table[f"rows_{rows}"] = {"us_median": round(statistics.median(us), 1), "us_all": [round(x, 1) for x in us],
                                 "phi_bytes": phi.numel() * 4}

    def step_kernels(call):  # event-timed launches of kind BEAM in one call
        lib.gram_prof_enable(1 << _lib.K_BEAM, 1 << 12)
        lib.gram_prof_reset()
        call()
        ms, n, work, dropped = C.c_double(), C.c_int64(), C.c_double(), C.c_int64()
        lib.gram_prof_collect(_lib.K_BEAM, C.byref(ms), C.byref(n), C.byref(work), C.byref(dropped))
        lib.gram_prof_enable(0, 0)
        return {"ms_per_call": round(ms.value, 3), "launches": n.value, "dropped": dropped.value}

    kernels = {name: step_kernels(call) for name, call in calls.items()}
    med = {name: statistics.median(t) for name, t in times.items()}
    print(json.dumps({
        "precision": args.precision, "batch": B, "num_beams": K, "items": len(cands), "n_nodes": int(flat.n_nodes),
        "max_length": max_length, "reps": args.reps,
        "ms_median": {n: round(v, 2) for n, v in med.items()},
        "over_plain": {n: round(v / med["plain"], 4) for n, v in med.items()},
        "over_plain_no_tail": {n: round(v / med["plain_no_tail"], 4) for n, v in med.items()},
        "ms_all": {n: [round(x, 2) for x in t] for n, t in times.items()},
        "spread_ms": {n: round(max(t) - min(t), 2) for n, t in times.items()},
        "item_bias_table": table, "step_kernels": kernels, "users_with_a_changed_list": changed}))


if __name__ == "__main__":
    main()
