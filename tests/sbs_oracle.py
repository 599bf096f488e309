"""The CPU restatement of sampling without replacement on the Trie -- stochastic beam search (Kool, van Hoof, Welling, ICML 2019;
DESIGN.md section 4.10) -- that the tests compare the HIP path with (test infrastructure, not a test module).

``philox`` is Philox4x32-10 in Python integers; ``expand`` is ONE step for one user in float64 (or, with ``dtype=np.float32``, in
numpy float32: the device's arithmetic, to measure how far rounding moves a perturbed score): every candidate of the user's rows,
ranked, and the smallest gap between adjacent perturbed scores among the first R + 1.  ``run`` is the loop over any function that
returns the logits of a prefix's children (the host tests' small Tries); ``walk`` is the loop over the oracle's decoder
(``oracle.gram_oracle``), free-running or teacher-forced along given rows."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import gram_oracle as O  # noqa: E402

M32 = 0xFFFFFFFF
EOS = 1

# delta of tests/test_gpu_sbs.py's selection test per precision mode: 4 x the largest |dG| the restatement shows when every logit
# moves by up to +-TOL[mode]["logit"] and when it runs in float32 (``measure_delta``; tests/test_sbs_host.py asserts that the
# constants cover the measurement).  Measured on ``sample_oracle.whole_path_case()`` at SEED / USER_KEYS below, 4 draws: f16x3
# (logit tolerance 1e-4) 4 x 3.04e-4 = 1.21e-3, bf16x3 (1.6e-3) 4 x 4.87e-3 = 1.95e-2; the smallest gap of any (user, step) there is
# 2.66e-2, so every pair is decidable in both.  The one-piece modes (3e-2) measure 4 x 9.5e-2 = 0.38: 11 of the 12 (user, step)
# pairs have a gap below that, far beyond the 10 % that may be left out, so they get the property tests only.
DELTA = {"f16x3": 1.3e-3, "bf16x3": 2.0e-2}
SEED = 2019
USER_KEYS = (1001, 77, 123456789012)


def philox(counter, key):
    """Philox4x32-10: counter (c0, c1, c2, c3) and key (k0, k1) as 32-bit ints -> four 32-bit ints"""
    c0, c1, c2, c3 = (int(c) & M32 for c in counter)
    k0, k1 = (int(k) & M32 for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def seed_key(seed):
    seed = int(seed) % (1 << 64)
    return seed & M32, seed >> 32


def uniform(w2):
    return ((w2 >> 8) + 0.5) * 2.0 ** -24


def gumbel(w2):
    return -math.log(-math.log(uniform(w2)))


def root(seed, user_key):
    """the row every user starts from: prefix [0], phi = 0, G = the root's Gumbel"""
    uk = int(user_key) % (1 << 64)
    w = philox((uk & M32, uk >> 32, 0, 0), seed_key(seed))
    return dict(prefix=(0,), phi=0.0, G=gumbel(w[2]), model=0.0, path=(w[0], w[1]), fin=False)


def expand(rows, kids, temperature, seed, R, dtype=np.float64):
    """One step for one user.  rows: the live and finished rows (dicts as ``root``'s; dead rows are simply absent); kids(prefix) ->
    (tokens in ascending order, their raw logits z, the row's full-vocabulary lse).  Returns (ranked, gap): every candidate in
    descending order of G, ties to the lower (row, token), each a row dict with ``parent`` (index into rows) and ``tok``; gap = the
    smallest difference between adjacent G among the first R + 1 (inf with fewer than two)."""
    f = dtype
    key = seed_key(seed)
    out = []
    for k, row in enumerate(rows):
        if row["fin"]:
            out.append(dict(row, parent=k, tok=0))
            continue
        toks, z, lse_row = kids(row["prefix"])
        if not len(toks):
            continue
        cur_len = len(row["prefix"])
        y = np.asarray(z, dtype=f) / f(temperature)
        m = y.max()
        lse_k = m + np.log(np.exp(y - m).sum(dtype=f))
        phi_c = f(row["phi"]) + (y - lse_k)
        ws = [philox((row["path"][0], row["path"][1], int(t), cur_len), key) for t in toks]
        gt = phi_c + np.asarray([gumbel(w[2]) for w in ws], dtype=f)
        Z, T = gt.max(), f(row["G"])
        with np.errstate(divide="ignore"):
            v = (T - gt) + np.log1p(-np.exp(gt - Z))
            G = (T - np.maximum(f(0), v)) - np.log1p(np.exp(-np.abs(v)))
        G = np.where(gt == Z, T, G)
        for i, t in enumerate(toks):
            out.append(dict(prefix=row["prefix"] + (int(t),), phi=float(phi_c[i]), G=float(G[i]),
                            model=row["model"] + float(z[i]) - float(lse_row), path=(ws[i][0], ws[i][1]), fin=int(t) == EOS,
                            parent=k, tok=int(t)))
    out.sort(key=lambda c: (-c["G"], c["parent"], c["tok"]))
    g = [c["G"] for c in out[:R + 1]]
    gap = min((a - b for a, b in zip(g, g[1:])), default=math.inf)
    return out, gap


def run(kids, R, max_length, seed, user_key, temperature=1.0, dtype=np.float64):
    """The whole search for one user over ``kids``: the R rows after max_length - 1 steps, best G first (fewer where the Trie has
    fewer items), and the per-step (ranked, gap) lists."""
    rows, steps = [root(seed, user_key)], []
    for _ in range(max_length - 1):
        ranked, gap = expand(rows, kids, temperature, seed, R, dtype)
        steps.append((ranked, gap))
        rows = ranked[:R]
    return rows, steps


def table_kids(trie, logits):
    """kids() over an ``O.Trie`` and a dict prefix -> {token: logit} (lse: over the children themselves)"""
    def kids(prefix):
        toks = sorted(trie.get(list(prefix)))
        z = np.asarray([logits[prefix][t] for t in toks], dtype=np.float64)
        return toks, z, float(np.log(np.exp(z).sum())) if len(toks) else 0.0
    return kids


# ---------------------------------------------------------------------------------------------- the loop over the oracle's decoder
@torch.no_grad()
def prefix_logits(sd, oc, bank, mask, prefixes):
    """float64 logits (rows, V) behind each of ``prefixes`` (one list of equal-length token tuples per user, the same count for
    every user): the oracle's cached decoder over ``bank`` = O.cross_kv(...) fed the prefixes position by position."""
    B, n = mask.shape[0], len(prefixes[0])
    ext = ((1.0 - mask.reshape(B, -1).float().repeat_interleave(n, 0)) * O.FMIN)[:, None, None, :]
    st = O.DecodeState(bank, ext, n)
    seq = torch.tensor([list(p) for u in prefixes for p in u], dtype=torch.int64)
    for t in range(seq.shape[1]):
        logits = O.decoder_step(sd, oc, seq[:, t].clone(), st)
    return logits.double()


def walk(sd, oc, ids, mask, tries, R, max_length, seed, user_keys, temperature=1.0, forced=None, shift=None, dtype=np.float64):
    """The search over the oracle's decoder for B users.  tries: one Trie-like object with ``get(prefix)`` per user.
    forced: None (free-running), or per step t = 0 .. max_length - 2 and per user the list of prefixes (tuples of t + 1 tokens;
    finished ones padded with 0 behind EOS) that are the rows BEFORE step t, in any order -- the device's rows: the restatement
    then expands exactly those, with its own phi / G / path for them (they are candidates of its previous step).
    shift: None or a function (user, step, tokens) -> array added to the children's logits (the delta measurement).
    Returns per user a list over the steps of dict(rows=the rows expanded, ranked=every candidate best first, gap=...)."""
    B = ids.shape[0]
    state = [[root(seed, user_keys[b])] for b in range(B)]
    bank = O.cross_kv(sd, oc, O.encode_fused(sd, oc, ids, mask))
    hist = [[] for _ in range(B)]
    for t in range(max_length - 1):
        if forced is not None and t > 0:
            for b in range(B):
                known = {_strip(c["prefix"]): c for c in hist[b][-1]["ranked"]}
                state[b] = [known[_strip(p)] for p in forced[t][b]]
        n = max(1, max(len(s) for s in state))
        pre = [[_pad(s[i]["prefix"], t + 1) if i < len(s) else (0,) * (t + 1) for i in range(n)] for s in state]
        logits = prefix_logits(sd, oc, bank, mask, pre)
        lse = torch.logsumexp(logits, -1)
        for b in range(B):
            index = {_strip(p): b * n + i for i, p in enumerate(pre[b])}

            def kids(prefix, b=b, index=index):
                toks = sorted(tries[b].get(list(prefix)))
                r = index[_strip(prefix)]
                z = logits[r, toks].numpy() if toks else np.zeros(0)
                if shift is not None and len(toks):
                    z = z + shift(b, t, toks)
                return toks, z, float(lse[r])
            ranked, gap = expand(state[b], kids, temperature, seed, R, dtype)
            hist[b].append(dict(rows=state[b], ranked=ranked, gap=gap))
            state[b] = ranked[:R]
    return hist


def _strip(prefix):
    """a prefix without the padding behind its EOS"""
    p = tuple(int(x) for x in prefix)
    return p[: p.index(EOS) + 1] if EOS in p else p


def _pad(prefix, n):
    p = tuple(prefix)
    return (p + (0,) * n)[:n]


def final_rows(hist, R):
    """per user the R best rows after the last step (fewer where there are fewer)"""
    return [h[-1]["ranked"][:R] for h in hist]


def measure_delta(case, tries, R, max_length, logit_tol, draws=4, temperature=1.0, seed=SEED, user_keys=USER_KEYS):
    """The largest |dG| of any candidate of the first R + 1 of any (user, step) of the free-running restatement when (a) every
    logit moves by a uniform random amount in [-logit_tol, logit_tol] (``draws`` draws; the rows are forced to stay the exact run's)
    and (b) the arithmetic is numpy float32.  Returns (largest |dG|, the exact run's history)."""
    a = (case["sd"], case["oc"], case["ids"], case["mask"], tries, R, max_length, seed, user_keys, temperature)
    exact = walk(*a)
    forced = [[[_pad(r["prefix"], t + 1) for r in exact[b][t]["rows"]] for b in range(len(tries))] for t in range(max_length - 1)]
    worst = 0.0
    runs = [walk(*a, forced=forced, dtype=np.float32)]
    for d in range(draws):
        rng = np.random.default_rng(1000 + d)
        runs.append(walk(*a, forced=forced, shift=lambda b, t, toks, rng=rng: rng.uniform(-logit_tol, logit_tol, len(toks))))
    for other in runs:
        for hb, ob in zip(exact, other):
            for he, ho in zip(hb, ob):
                got = {c["prefix"]: c["G"] for c in ho["ranked"]}
                for c in he["ranked"][:R + 1]:
                    worst = max(worst, abs(c["G"] - got[c["prefix"]]))
    return worst, exact


# ---------------------------------------------------------------------------------------------- the distribution check
# One 5-child node whose logits are exact in every number format, 4 096 users with distinct keys: the token of a user's first row
# is the argmax of its children's perturbed scores, so its counts follow softmax(DIST_LOGITS).  tests/test_gpu_sbs_step.py runs it on
# the device, tests/test_sbs_host.py on the restatement, with the same seed and keys.
DIST_LOGITS = (1.5, 1.0, 0.5, 0.0, -0.25)
DIST_TOKENS = (11, 57, 100, 163, 201)
DIST_USERS = 4096
DIST_SEED = 20190609


def dist_keys():
    return [7919 * i + 13 for i in range(DIST_USERS)]


def dist_z(counts):
    """per child, (count - n p) / sqrt(n p (1 - p)) against p = softmax(DIST_LOGITS)"""
    p = np.exp(np.asarray(DIST_LOGITS))
    p /= p.sum()
    n = float(np.sum(counts))
    return (np.asarray(counts, dtype=np.float64) - n * p) / np.sqrt(n * p * (1 - p))
