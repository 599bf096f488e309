"""The search step on a wide Trie: milliseconds per search step (the kernel alone, on random operands) and per generate() call at
T5-base, beam 20, 256 users, on a synthetic Trie whose root has 4 000 children (chunked kernel: K * fan-out = 80 000) and on the
Beauty Trie (one-shot kernel), and the chunked kernel forced onto Beauty (gram_debug_set_beam_chunked) -- the one pair with a
baseline.  Not collected by pytest.
    python tests/bench_wide_trie.py [--batch 256] [--iters 10] [--precision f16x3]"""
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


def step_ms(lib, _lib, flat, B, K, iters, dev):
    """median ms of step 0 (shared row, K * root fan-out candidates) and of step 1 of a sparse search on random operands"""
    from tests import gpu_util as G
    V, d, T = 32128, 768, 12
    g = torch.Generator().manual_seed(7)
    E = G.bf(torch.randn(V, d, generator=g) * 0.05)
    ctrie, _keep = flat.to_device(dev)
    st, t = G.make_beam_state(B, K, T)
    out = []
    for step in (0, 1):
        rows = B if step == 0 else B * K
        h = G.bf(torch.randn(rows, d, generator=g))
        lse = torch.logsumexp(h.float() @ E.float().t(), dim=1).contiguous()
        if step == 0:
            _lib.check(lib.gram_beam_init(C.byref(st), C.byref(ctrie), 0, G.stream()), "init")
        saved = {k: v.clone() for k, v in t.items()}
        ms = []
        for _ in range(iters + 2):
            for k, v in t.items():
                v.copy_(saved[k])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(lib.gram_beam_step_sparse(C.byref(st), C.byref(ctrie), G.p(h), G.p(E), d, G.p(lse), V, step + 1, 1 if step == 0 else K,
                                                 G.stream()), "step")
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        assert int(t["error"][0]) == 0
        out.append(round(float(np.median(ms[2:])), 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
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
    beauty = [[int(x) for x in row if x >= 0] for row in z["Beauty_cands"]]
    rng = np.random.default_rng(5)
    wide = sorted({(0, a) + tuple(int(x) for x in rng.integers(2, 32100, int(rng.integers(2, 8)))) + (1,)
                   for a in range(2, 4002) for _ in range(3)})
    B, K = args.batch, 20
    g = torch.Generator().manual_seed(1000)
    ids = torch.randint(2, 32100, (B, 3, 128), generator=g)
    ids[:, :, -1] = 1
    ids_d, mask_d = ids.to(dev), torch.ones(B, 3, 128, dtype=torch.bool, device=dev)
    res = {}
    for name, cands, chunked in (("wide4000", [list(c) for c in wide], -1), ("beauty", beauty, -1), ("beauty_chunked", beauty, 1)):
        trie = gt.Trie(cands)
        flat = gt.FlatTrie(trie)
        fn = gt.prefix_allowed_tokens_fn(trie)
        max_length = max(len(c) for c in cands)
        lib.gram_debug_set_beam_chunked(chunked)
        try:
            s0, s1 = step_ms(lib, _lib, flat, B, K, args.iters, dev)

            def call():
                return model.generate(input_ids=ids_d, attention_mask=mask_d, max_length=max_length, prefix_allowed_tokens_fn=fn, num_beams=K,
                                      num_return_sequences=K, output_scores=True, return_dict_in_generate=True, length_penalty=1.0)
            for _ in range(2):
                call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                call()
            torch.cuda.synchronize()
            gen = (time.perf_counter() - t0) / args.iters * 1e3
        finally:
            lib.gram_debug_set_beam_chunked(-1)
        res[name] = {"max_fanout": flat.max_fanout, "K_x_fanout": K * flat.max_fanout, "search_step0_ms": s0, "search_step1_ms": s1,
                     "generate_ms": round(gen, 3), "generate_ms_per_step": round(gen / (max_length - 1), 3), "decode_steps": max_length - 1}
    res["chunked_over_one_shot_beauty"] = {k: round(res["beauty_chunked"][k] / res["beauty"][k], 4)
                                           for k in ("search_step0_ms", "search_step1_ms", "generate_ms")}
    print(json.dumps({"precision": args.precision, "batch": B, "beams": K, **res}))


if __name__ == "__main__":
    main()
