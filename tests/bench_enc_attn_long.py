"""GPU micro-benchmark (not a test): the long-passage encoder self-attention (gram_enc_self_attn_long_split) against the shipped kernel.
T5-base heads (H = 12), two-piece operands, every key valid, P passages of L tokens with P * L = 49 152 at every L: the bytes are the
same in every row, the flops grow with L.  The shipped kernel at L = 128 and the long kernel at L = 128, 256, 512 alternate in one
process; the figure is the median ms per launch after a warm-up, per token and as the 16-bit-MFMA flop rate (three piece products per
product).  The yardstick is the shipped kernel's L = 128 time at the same token count.
    python tests/bench_enc_attn_long.py [--tokens 49152] [--rounds 15] [--out profiles/enc_attn_long_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gram_amd import _lib  # noqa: E402
from tests import gpu_util as G  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=49152)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "enc_attn_long_bench.json"))
    a = ap.parse_args()
    lib = _lib.load()
    H, T = 12, a.tokens
    inner = H * 64
    g = torch.Generator(device=G.DEV).manual_seed(0)
    qkv = torch.stack([(torch.randn(T, 3 * inner, generator=g, device=G.DEV) * s).to(G.DT) for s in (1.0, 2.0 ** -11)]).contiguous()
    bias = (torch.randn(H, 255, generator=g, device=G.DEV) * 0.5).contiguous()
    mask = torch.ones(T, dtype=torch.uint8, device=G.DEV)
    out = torch.empty(T, 2 * inner, dtype=G.DT, device=G.DEV)
    cases = [("shipped", 128, lib.gram_enc_self_attn_split)] + [("long", L, lib.gram_enc_self_attn_long_split) for L in (128, 256, 512)]

    def launch(fn, L):
        _lib.check(fn(G.p(qkv), G.p(bias), G.p(mask), G.p(out), T // L, L, H, 2, qkv[0].numel(), G.stream()), "enc_attn")

    times = {(k, L): [] for k, L, _ in cases}
    for r in range(a.warmup + a.rounds):
        for k, L, fn in cases:  # alternating: every kernel sees the same clocks and the same neighbours
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            launch(fn, L)
            e.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[k, L].append(s.elapsed_time(e))
    base = statistics.median(times["shipped", 128])
    rows = []
    for k, L, _ in cases:
        ms = statistics.median(times[k, L])
        flops = 4.0 * T * L * H * 64 * 3
        rows.append(dict(kernel=k, L=L, P=T // L, ms=round(ms, 4), ms_min=round(min(times[k, L]), 4), ms_max=round(max(times[k, L]), 4),
                         ns_per_token=round(ms * 1e6 / T, 2), tflops=round(flops / ms / 1e9, 1), vs_shipped_128=round(ms / base, 3)))
        print(f"{k:8s} L={L:3d} P={T // L:4d}: {ms:7.4f} ms (min {min(times[k, L]):.4f}, max {max(times[k, L]):.4f}), "
              f"{ms * 1e6 / T:6.2f} ns/token, {flops / ms / 1e9:6.1f} TFLOP/s, {ms / base:5.2f}x the shipped kernel at 128", flush=True)
    res = dict(device=torch.cuda.get_device_name(0), H=H, pieces=2, tokens=T, rounds=a.rounds, warmup=a.warmup, rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
