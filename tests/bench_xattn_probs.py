"""GPU micro-benchmark (not a test): the cross-attention probabilities kernel (gram_cross_attn_probs_split) next to the shipped
cross-attention kernel (gram_cross_attn_decode_split) at the same (B, K = Q, H, S), both in one process, alternating round by round.
    python tests/bench_xattn_probs.py                    # T5-base (H 12), B 512: S = 384 and 2688, Q = 1 and 20, one and two pieces
    python tests/bench_xattn_probs.py pieces B H S Q     # one shape
One JSON line per shape: median and minimum per-launch time of both kernels (us), their ratio, and the probabilities kernel's
algorithmic traffic (K read twice + the fp32 output written once) over its median time.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one(pieces, B=512, H=12, S=384, Q=20, rounds=9, reps=10):
    import torch
    from gram_amd import _lib
    DT = _lib.piece_dtype()
    lib = _lib.load()
    dev = "cuda:0"
    inner = H * 64
    g = torch.Generator(device=dev).manual_seed(S + Q)
    q = (torch.randn(pieces, B * Q, inner, device=dev, generator=g) * 0.3).to(DT)
    kb = torch.randn(pieces, B, H, S, 64, device=dev, generator=g).to(DT)
    vt = torch.randn(pieces, B, H, S // 32, 64, 32, device=dev, generator=g).to(DT)
    mask = torch.ones(B, S, dtype=torch.uint8, device=dev)
    out = torch.empty(B * Q, pieces * inner, dtype=DT, device=dev)
    probs = torch.empty(B, H, Q, S, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    bits = torch.zeros(B, 128, dtype=torch.int32, device=dev)
    _lib.check(lib.gram_mask_key_bits(mask.data_ptr(), bits.data_ptr(), B, S, st), "bits")

    def shipped():
        _lib.check(lib.gram_cross_attn_decode_split(q.data_ptr(), kb.data_ptr(), vt.data_ptr(), mask.data_ptr(), out.data_ptr(), B, Q, H, S,
                                                    None, None, pieces, q[0].numel(), kb[0].numel(), bits.data_ptr(), st), "xattn")

    def new():
        _lib.check(lib.gram_cross_attn_probs_split(q.data_ptr(), kb.data_ptr(), mask.data_ptr(), probs.data_ptr(), B, Q, H, S, pieces,
                                                   q[0].numel(), kb[0].numel(), bits.data_ptr(), st), "probs")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    for _ in range(3):
        shipped()
        new()
    t = {"shipped": [], "probs": []}
    for _ in range(rounds):  # alternating rounds: both kernels see the same clocks and the same neighbours
        t["shipped"].append(timed(shipped))
        t["probs"].append(timed(new))
    med = {k: statistics.median(v) for k, v in t.items()}
    nbytes = 2.0 * (2.0 * B * H * S * 64 * pieces) + 4.0 * B * H * Q * S
    return {"pieces": pieces, "B": B, "H": H, "S": S, "Q": Q, "shipped_us": round(med["shipped"], 1), "shipped_min_us": round(min(t["shipped"]), 1),
            "probs_us": round(med["probs"], 1), "probs_min_us": round(min(t["probs"]), 1), "ratio": round(med["probs"] / med["shipped"], 2),
            "probs_GBps": round(nbytes / (med["probs"] * 1e-6) / 1e9, 1)}


if __name__ == "__main__":
    if len(sys.argv) not in (1, 6):
        sys.exit(__doc__)
    if len(sys.argv) > 1:
        pieces, B, H, S, Q = (int(x) for x in sys.argv[1:6])
        print(json.dumps(one(pieces, B=B, H=H, S=S, Q=Q)), flush=True)
    else:
        for S in (384, 2688):
            for Q in (1, 20):
                for pieces in (1, 2):
                    print(json.dumps(one(pieces, S=S, Q=Q)), flush=True)
