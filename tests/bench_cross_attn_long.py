"""GPU micro-benchmark (not a test): the segmented cross-attention for fused contexts of up to 16 384 keys
(gram_cross_attn_long_split) against the shipped kernel (gram_cross_attn_decode_split).  T5-base heads (H = 12), two-piece operands,
K = 20 beams, every key valid.  The shipped kernel and the long form alternate in one process at S = 2688 and 4096 for B = 64 and 1024;
the long form alone at S = 5376, 10 752 and 16 384 with a B whose bank fits.  The figure is the event-timed median ms per launch
after a warm-up (the long form's time includes its merge kernel above 4096 keys), and the bank bytes per second against the
algorithmic 4 * B * H * S * 64 * pieces.  The shader clock is read once before and once after, where the platform reports it.
    python tests/bench_cross_attn_long.py [--rounds 15] [--out profiles/cross_attn_long_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gram_amd import _lib  # noqa: E402
from tests import gpu_util as G  # noqa: E402


def _clock_mhz():
    try:
        return int(torch.cuda.clock_rate())
    except Exception:  # (needs the platform's management library)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "cross_attn_long_bench.json"))
    a = ap.parse_args()
    lib = _lib.load()
    H, K, P = 12, 20, 2
    inner = H * 64
    shapes = [(64, 2688), (64, 4096), (1024, 2688), (1024, 4096), (512, 5376), (256, 10752), (256, 16384)]
    cases = [(k, B, S) for B, S in shapes for k in (("shipped", "long") if S <= 4096 else ("long",))]
    per_piece = max(B * H * S * 64 for B, S in shapes)  # elements of the largest bank, per piece: every case is a prefix of it
    kb = torch.empty(P, per_piece, dtype=G.DT, device=G.DEV).normal_()
    vt = torch.empty(P, per_piece, dtype=G.DT, device=G.DEV).normal_()
    kb[1] *= 2.0 ** -11
    vt[1] *= 2.0 ** -11
    Bmax, Smax = max(B for B, _ in shapes), max(S for _, S in shapes)
    q = (torch.empty(P, Bmax * K, inner, dtype=G.DT, device=G.DEV).normal_() * 0.3).contiguous()
    out = torch.empty(Bmax * K, P * inner, dtype=G.DT, device=G.DEV)
    mask = torch.ones(Bmax * Smax, dtype=torch.uint8, device=G.DEV)
    bits_s = torch.empty(Bmax, 128, dtype=torch.int32, device=G.DEV)
    bits_l = torch.empty(Bmax, _lib.GRAM_KEY_BITS_LONG_STRIDE, dtype=torch.int32, device=G.DEV)
    scratch = torch.empty(max(4, max(lib.gram_cross_attn_long_scratch_bytes(B * K, H, S) for B, S in shapes) // 4), dtype=torch.float32,
                          device=G.DEV)

    def launch(kind, B, S):
        if kind == "shipped":
            _lib.check(lib.gram_cross_attn_decode_split(G.p(q), G.p(kb), G.p(vt), G.p(mask), G.p(out), B, K, H, S, None, None, P, q[0].numel(),
                                                        per_piece, G.p(bits_s), G.stream()), "shipped")
        else:
            _lib.check(lib.gram_cross_attn_long_split(G.p(q), G.p(kb), G.p(vt), G.p(mask), G.p(out), B, K, H, S, None, None, P, q[0].numel(),
                                                      per_piece, G.p(bits_l), G.p(scratch), G.stream()), "long")

    clock0 = _clock_mhz()
    times = {c: [] for c in cases}
    for r in range(a.warmup + a.rounds):
        for c in cases:  # alternating: every kernel sees the same clocks and the same neighbours
            kind, B, S = c
            # (the key bits belong to the (B, S) they were packed for: outside the timed region, as once per generate)
            if kind == "shipped":
                _lib.check(lib.gram_mask_key_bits(G.p(mask), G.p(bits_s), B, S, G.stream()), "bits")
            else:
                _lib.check(lib.gram_mask_key_bits_long(G.p(mask), G.p(bits_l), B, S, G.stream()), "bits")
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            launch(kind, B, S)
            e.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[c].append(s.elapsed_time(e))
    clock1 = _clock_mhz()
    rows = []
    for c in cases:
        kind, B, S = c
        ms = statistics.median(times[c])
        nbytes = 4.0 * B * H * S * 64 * P
        base = statistics.median(times["shipped", B, S]) if ("shipped", B, S) in times else None
        rows.append(dict(kernel=kind, B=B, S=S, ms=round(ms, 4), ms_min=round(min(times[c]), 4), ms_max=round(max(times[c]), 4),
                         tb_per_s=round(nbytes / ms / 1e9, 3), vs_shipped=None if base is None else round(ms / base, 3)))
        print(f"{kind:8s} B={B:5d} S={S:6d}: {ms:8.4f} ms (min {min(times[c]):.4f}, max {max(times[c]):.4f}), {nbytes / ms / 1e9:6.3f} TB/s"
              + ("" if base is None else f", {ms / base:5.2f}x the shipped kernel"), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), H=H, K=K, pieces=P, rounds=a.rounds, warmup=a.warmup, shader_clock_mhz=[clock0, clock1],
               rows=rows)
    print(f"shader clock before / after: {clock0} / {clock1} MHz")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
