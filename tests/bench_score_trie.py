"""Every catalogue item in one decoder pass against score_sequences over the same candidates (not collected by pytest, not part of
bench.py; run on an MI355X).

    python tests/bench_score_trie.py [--users 16] [--reps 5] [--precision f16x3] [--dataset Beauty]

Shape: T5-base, 3 x 128-token passages, the dataset's item Trie of tests/golden/tries.npz (Beauty: 12 101 items, ids of <= 10 tokens).
GRAM.score_all_items runs Q decoder rows per user (the Trie's internal nodes), GRAM.score_sequences n_items * T; both pick their own
chunk size.  Each side is warmed up once at the full batch (workspace growth, tables, packing), then timed `reps` times.  Prints one
JSON line: the median seconds per user of both with the spread (min, max) of the repetitions, the ratio of the medians beside the row
ratio, whether the scores are bit-equal, and per kernel kind (gram_prof_*) the milliseconds per user and the share of the profiled
time."""
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
from gram_amd.utils import generation_trie as gt  # noqa: E402

KINDS = ((_lib.K_GEMM, "gemm"), (_lib.K_ENC_ATTN, "enc_attn"), (_lib.K_CROSS_ATTN, "cross_attn"), (_lib.K_DEC_SELF_ATTN, "self_attn"),
         (_lib.K_ROWOPS, "rowops"), (_lib.K_LSE, "lse_and_logprob"))


def timed(lib, fn, reps, users):
    """one warm-up call at the full batch, the wall times of `reps` calls, then one profiled call:
    (median seconds, all seconds, {kind: ms per user, launches, share})"""
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    lib.gram_prof_enable(sum(1 << k for k, _ in KINDS), 1 << 17)
    lib.gram_prof_reset()
    fn()
    torch.cuda.synchronize()
    prof, total = {}, 0.0
    for k, name in KINDS:
        ms, n, work, dropped = C.c_double(), C.c_int64(), C.c_double(), C.c_int64()
        lib.gram_prof_collect(k, C.byref(ms), C.byref(n), C.byref(work), C.byref(dropped))
        prof[name] = dict(ms_per_user=ms.value / users, launches=n.value, dropped=dropped.value)
        total += ms.value
    lib.gram_prof_enable(0, 0)
    for v in prof.values():
        v["share"] = v["ms_per_user"] * users / total if total else 0.0
    return float(np.median(times)), times, prof


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--dataset", default="Beauty")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = gram_amd.T5Config.named("t5-base")
    torch.manual_seed(2023)
    model = gram_amd.create_model("gram", cfg).to(dev).eval()
    model.set_precision(a.precision)
    z = np.load(os.path.join(ROOT, "tests", "golden", "tries.npz"))
    cands = [[int(x) for x in row if x >= 0] for row in z[f"{a.dataset}_cands"]]
    trie = gt.Trie(cands)
    fn = gt.prefix_allowed_tokens_fn(trie)
    rows = gt.FlatTrie(trie).decoder_rows()
    T = max(len(c) for c in cands) - 1  # label form: no start token
    B, N, L = a.users, 3, 128
    g = torch.Generator().manual_seed(99)
    ids = torch.randint(2, 32100, (B, N, L), generator=g)
    ids[:, :, -1] = 1
    mask = torch.ones(B, N, L, dtype=torch.bool)
    lab1 = torch.full((len(cands), T), -100, dtype=torch.long)
    for i, c in enumerate(cands):
        lab1[i, : len(c) - 1] = torch.tensor(c[1:])
    ids, mask = ids.to(dev), mask.to(dev)
    lab = lab1.to(dev)[None].expand(B, -1, -1).contiguous()
    lib = _lib.load()
    tree = model.score_all_items(ids[:1], mask[:1], fn, cands)  # the first user of both: are the bits equal?
    seqs = model.score_sequences(ids[:1], mask[:1], lab[:1])
    equal = bool(torch.equal(tree, seqs))
    max_diff = float((tree.double() - seqs.double()).abs().max())
    upc_tree = model.max_users_per_call_trie(N, L, rows.Q, rows.n_leaves, limit=B)
    upc_seq = model.max_users_per_call_tf(N, L, len(cands), T, limit=B)
    t_tree, all_tree, prof_tree = timed(lib, lambda: model.score_all_items(ids, mask, fn, cands), a.reps, B)
    t_seq, all_seq, prof_seq = timed(lib, lambda: model.score_sequences(ids, mask, lab), a.reps, B)
    print(json.dumps(dict(dataset=a.dataset, users=B, precision=a.precision, n_items=len(cands), T=T, Q=rows.Q, Tq=rows.Tq,
                          rows_sequences=len(cands) * T, row_ratio=len(cands) * T / rows.Q, bit_equal_first_user=equal,
                          max_abs_diff_first_user=max_diff, users_per_call=dict(tree=upc_tree, sequences=upc_seq),
                          s_per_user=dict(tree=t_tree / B, sequences=t_seq / B),
                          s_per_user_min_max=dict(tree=[min(all_tree) / B, max(all_tree) / B], sequences=[min(all_seq) / B, max(all_seq) / B]),
                          time_ratio=t_seq / t_tree, time_ratio_min_max=[min(all_seq) / max(all_tree), max(all_seq) / min(all_tree)], reps=a.reps,
                          all_s=dict(tree=all_tree, sequences=all_seq), kernels=dict(tree=prof_tree, sequences=prof_seq))))


if __name__ == "__main__":
    main()
