"""GPU micro-benchmark (not a test): the head-summed token scores kernel (gram_cross_attn_token_scores_split, xattn_scores.hip) at
T5-base heads (H = 12), two pieces, one layer, Q = 180 rows per user (20 candidates x 9 positions).
    python tests/bench_xattn_scores.py [--out profiles/xattn_scores_bench.json]
* S = 4096, B = 16: the shipped pair (gram_cross_attn_probs_split + gram_xattn_head_sum, through its [B][H][Q][S] scratch) against the
  fused kernel in the same run -- each side warmed up once, then the median of 5 launches;
* the fused kernel alone at S = 10 752 and 16 384 (B = 16, Q = 180) and at B = 1, Q = 1.
One JSON line per shape (us per launch) and the whole list, with the shader clock read before and after where the platform reports it,
in --out.  `first` = 0 throughout: the accumulator is read and written, as in every layer but the first."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gram_amd import _lib  # noqa: E402

H, PIECES = 12, 2


def _clock_mhz():
    try:
        return int(torch.cuda.clock_rate())
    except Exception:  # (needs the platform's management library)
        return None


def _timed(fn, reps=5):
    fn()  # warm-up
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(t), min(t)


def one(B, Q, S, pair):
    lib = _lib.load()
    DT = _lib.piece_dtype()
    dev = "cuda:0"
    inner = H * 64
    g = torch.Generator(device=dev).manual_seed(S + Q)
    q = (torch.randn(PIECES, B * Q, inner, device=dev, generator=g) * 0.3).to(DT)
    kb = torch.randn(PIECES, B, H, S, 64, device=dev, generator=g).to(DT)
    mask = torch.ones(B, S, dtype=torch.uint8, device=dev)
    acc = torch.zeros(B, Q, S, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    bits = torch.zeros(B, _lib.GRAM_KEY_BITS_LONG_STRIDE, dtype=torch.int32, device=dev)
    _lib.check(lib.gram_mask_key_bits_long(mask.data_ptr(), bits.data_ptr(), B, S, st), "bits")

    def fused():
        _lib.check(lib.gram_cross_attn_token_scores_split(q.data_ptr(), kb.data_ptr(), acc.data_ptr(), B, Q, H, S, PIECES, q[0].numel(),
                                                          kb[0].numel(), bits.data_ptr(), 0, st), "token scores")

    res = {"B": B, "Q": Q, "H": H, "S": S, "pieces": PIECES}
    if pair:
        probs = torch.empty(B, H, Q, S, dtype=torch.float32, device=dev)

        def shipped():
            _lib.check(lib.gram_cross_attn_probs_split(q.data_ptr(), kb.data_ptr(), mask.data_ptr(), probs.data_ptr(), B, Q, H, S, PIECES,
                                                       q[0].numel(), kb[0].numel(), None, st), "probs")
            _lib.check(lib.gram_xattn_head_sum(probs.data_ptr(), acc.data_ptr(), B, Q, H, S, 0, st), "head sum")

        med, mn = _timed(shipped)
        res.update(pair_us=round(med, 1), pair_min_us=round(mn, 1), pair_scratch_MB=round(probs.numel() * 4 / 1e6, 1))
    med, mn = _timed(fused)
    res.update(fused_us=round(med, 1), fused_min_us=round(mn, 1))
    if pair:
        res["fused_over_pair"] = round(res["fused_us"] / res["pair_us"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xattn_scores_bench.json"))
    a = ap.parse_args()
    clock0 = _clock_mhz()
    rows = []
    for B, Q, S, pair in ((16, 180, 4096, True), (16, 180, 10752, False), (16, 180, 16384, False), (1, 1, 4096, False), (1, 1, 10752, False),
                          (1, 1, 16384, False)):
        rows.append(one(B, Q, S, pair))
        print(json.dumps(rows[-1]), flush=True)
    clock1 = _clock_mhz()
    res = dict(device=torch.cuda.get_device_name(0), warmup=1, launches=5, statistic="median", shader_clock_mhz=[clock0, clock1], cases=rows)
    print(f"shader clock before / after: {clock0} / {clock1} MHz")
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
