"""Teacher-forced scoring throughput (not collected by pytest, not part of bench.py; run on an MI355X).

    python tests/bench_teacher_forced.py [--users 4096] [--reps 3] [--precision f16x3]

Shape: T5-base, 3 x 128-token passages, C = 20 Beauty Trie items per user as candidates (label form, -100 after EOS), scored by
GRAM.score_sequences; then forward(labels) at a training-size batch (B = 32, T = 10).  Prints one JSON line: users/s, candidate tokens/s,
GEMM TFLOP/s (fp32-problem flops), cross-attention GB/s (algorithmic bytes, per launch kind) and the forward(labels) time."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gram_amd  # noqa: E402
from gram_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precision", default="f16x3")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = gram_amd.T5Config.named("t5-base")
    torch.manual_seed(2023)
    model = gram_amd.create_model("gram", cfg).to(dev).eval()
    model.set_precision(a.precision)
    z = np.load(os.path.join(ROOT, "tests", "golden", "tries.npz"))
    cands = [[int(x) for x in row if x >= 0] for row in z["Beauty_cands"]]
    T = max(len(c) for c in cands) - 1  # label form: no start token
    B, N, L, Cn = a.users, 3, 128, 20
    g = torch.Generator().manual_seed(99)
    ids = torch.randint(2, 32100, (B, N, L), generator=g)
    ids[:, :, -1] = 1
    mask = torch.ones(B, N, L, dtype=torch.bool)
    pick = torch.randint(0, len(cands), (B, Cn), generator=g)
    lab = torch.full((B, Cn, T), -100, dtype=torch.long)
    for b in range(B):
        for c in range(Cn):
            s = cands[int(pick[b, c])][1:]
            lab[b, c, :len(s)] = torch.tensor(s)
    ids, mask, lab = ids.to(dev), mask.to(dev), lab.to(dev)
    n_tok = int((lab >= 0).sum())
    lib = _lib.load()
    model.score_sequences(ids[:64], mask[:64], lab[:64])  # warm-up (packing, workspace)
    upc = model.max_users_per_call_tf(N, L, Cn, T, limit=B)
    kinds = (1 << _lib.K_GEMM) | (1 << _lib.K_CROSS_ATTN) | (1 << _lib.K_DEC_SELF_ATTN) | (1 << _lib.K_ENC_ATTN)
    times = []
    for rep in range(a.reps + 1):
        if rep == 1:
            lib.gram_prof_enable(kinds, 1 << 16)
            lib.gram_prof_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.score_sequences(ids, mask, lab, users_per_call=upc)
        torch.cuda.synchronize()
        if rep:
            times.append(time.perf_counter() - t0)
    prof = {}
    for k, name in ((_lib.K_GEMM, "gemm"), (_lib.K_CROSS_ATTN, "cross_attn"), (_lib.K_DEC_SELF_ATTN, "self_attn_tf"),
                    (_lib.K_ENC_ATTN, "enc_attn")):
        ms, n, work, dropped = C.c_double(), C.c_int64(), C.c_double(), C.c_int64()
        lib.gram_prof_collect(k, C.byref(ms), C.byref(n), C.byref(work), C.byref(dropped))
        prof[name] = dict(ms_per_rep=ms.value / a.reps, launches=n.value // a.reps, dropped=dropped.value)
        if k == _lib.K_GEMM:
            prof[name]["tflops"] = work.value / (ms.value * 1e-3) / 1e12 if ms.value else 0.0
        elif k == _lib.K_CROSS_ATTN:
            prof[name]["gb_s"] = work.value / (ms.value * 1e-3) / 1e9 if ms.value else 0.0
    lib.gram_prof_enable(0, 0)
    best = min(times)
    # forward(labels) at a training-size batch
    Bt, Tt = 32, 10
    lt = lab[:Bt, 0, :Tt].contiguous()
    with torch.no_grad():
        model(input_ids=ids[:Bt], attention_mask=mask[:Bt], labels=lt, return_dict=False)
        torch.cuda.synchronize()
        fw = []
        for _ in range(5):
            t0 = time.perf_counter()
            model(input_ids=ids[:Bt], attention_mask=mask[:Bt], labels=lt, return_dict=False)
            torch.cuda.synchronize()
            fw.append(time.perf_counter() - t0)
    print(json.dumps(dict(users=B, candidates=Cn, T=T, precision=a.precision, users_per_call=upc, best_s=best, all_s=times,
                          users_per_s=B / best, candidate_tokens_per_s=n_tok / best, kernels=prof,
                          forward_labels_B32_T10_ms=min(fw) * 1e3)))


if __name__ == "__main__":
    main()
