"""Trie-constrained sampling against beam search at one shape, in one process: T5-base, 3 passages of 128 tokens, the Beauty Trie
(12 101 items), f16x3, B users -- ``generate(num_beams=20)`` and ``generate(do_sample=True, num_return_sequences=20)`` alternating,
the median of ``--reps`` calls each after a warm-up at the full shape, and the spread between the beam repetitions (the margin a
difference has to exceed to mean anything).  Beam search drops finished rows from its late steps (live-row compaction) and, at this
batch, decodes the Trie's tail in one pass; sampling does neither, so a third call -- beam search with both switched off
(gram_debug_set_live_rows / gram_debug_set_tail_pass) -- is the one that launches the same kernels as sampling except for the step.
A second pass with per-kind event timing on (gram_prof, kind BEAM: every launch of beam.hip and sample.hip) reports the step
kernels' own time in each of the three, and a last one with the ping-pong GEMM's clock stamps on reports the clock the chip held.
Not collected by pytest.
    python tests/bench_sample.py [--batch 256] [--reps 5] [--precision f16x3]"""
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
    common = dict(input_ids=ids_d, attention_mask=mask_d, max_length=max_length, prefix_allowed_tokens_fn=fn, return_dict_in_generate=True)

    def beam():
        return model.generate(num_beams=K, num_return_sequences=K, output_scores=True, length_penalty=1.0, **common)

    def sample():
        return model.generate(do_sample=True, num_beams=1, num_return_sequences=K, uniforms=uniforms, **common)

    def beam_stepwise():  # every row decoded at every step, as sampling does
        lib.gram_debug_set_live_rows(0)
        lib.gram_debug_set_tail_pass(0)
        try:
            return beam()
        finally:
            lib.gram_debug_set_live_rows(-1)
            lib.gram_debug_set_tail_pass(-1)

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(2):  # warm-up of both at the full shape (the workspace is sized once: the larger of the two)
        beam()
        beam_stepwise()
        out = sample()
    items = model.sequence_items(out["sequences"], fn, cands)
    assert bool((items >= 0).all()), "a sampled row is not a candidate"
    t_beam, t_step, t_sample = [], [], []
    for _ in range(args.reps):
        t_beam.append(timed(beam)[0])
        t_step.append(timed(beam_stepwise)[0])
        t_sample.append(timed(sample)[0])

    def step_kernels(call):  # event-timed launches of kind BEAM in one call
        lib.gram_prof_enable(1 << _lib.K_BEAM, 1 << 12)
        lib.gram_prof_reset()
        call()
        ms, n, work, dropped = C.c_double(), C.c_int64(), C.c_double(), C.c_int64()
        lib.gram_prof_collect(_lib.K_BEAM, C.byref(ms), C.byref(n), C.byref(work), C.byref(dropped))
        lib.gram_prof_enable(0, 0)
        return {"ms_per_call": round(ms.value, 3), "launches": n.value, "dropped": dropped.value}

    k_beam, k_step, k_sample = step_kernels(beam), step_kernels(beam_stepwise), step_kernels(sample)
    lib.gram_prof_pp_clock_enable(1)
    _lib.check(lib.gram_prof_pp_clock(None, 1), "pp_clock reset")
    beam()
    sample()
    ghz = C.c_double(0.0)
    _lib.check(lib.gram_prof_pp_clock(C.byref(ghz), 1), "pp_clock")
    lib.gram_prof_pp_clock_enable(0)
    mb, ms_ = statistics.median(t_beam), statistics.median(t_sample)
    print(json.dumps({
        "precision": args.precision, "batch": B, "rows_per_user": K, "items": len(cands), "max_length": max_length, "reps": args.reps,
        "beam_ms_median": round(mb, 2), "sample_ms_median": round(ms_, 2), "sample_over_beam": round(ms_ / mb, 4),
        "beam_ms_all": [round(t, 2) for t in t_beam], "sample_ms_all": [round(t, 2) for t in t_sample],
        "beam_spread_ms": round(max(t_beam) - min(t_beam), 2),
        "beam_stepwise_ms_median": round(statistics.median(t_step), 2), "beam_stepwise_ms_all": [round(t, 2) for t in t_step],
        "sample_over_beam_stepwise": round(ms_ / statistics.median(t_step), 4),
        "step_kernels_beam": k_beam, "step_kernels_beam_stepwise": k_step, "step_kernels_sample": k_sample,
        "clock_ghz_in_gemm": round(ghz.value, 4) if ghz.value > 0 else None}))


if __name__ == "__main__":
    main()
