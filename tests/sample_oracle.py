"""The CPU restatement of Trie-constrained sampling the tests compare the HIP path with (test infrastructure, not a test module).

``warp`` / ``pick`` are DESIGN.md section 4.8 for ONE row in float64: the HF 4.26 ``sample`` step on the row's Trie children --
temperature, top_k (ties at the threshold all stay), top_p (ascending cumulative softmax mass, ``min_tokens_to_keep = 1``, equal
values stay or go together), then the inverse-CDF draw from a uniform.  ``walk`` is the sampling loop over the oracle's cached
decoder (``oracle.gram_oracle``: encode_fused / cross_kv / DecodeState / decoder_step): it either CONSTRUCTS uniforms that land in
the middle of wide CDF intervals, or follows given sequences and reports, per step, what the restatement picks for a given uniform
and how far that uniform is from the nearest decision boundary.  ``whole_path_case`` is the one set of inputs tests/test_gpu_sample.py
runs and tests/test_sample_host.py checks on the CPU first."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import gram_oracle as O  # noqa: E402


# ---------------------------------------------------------------------------------------------- one row, float64
def warp(z, temperature=1.0, top_k=0, top_p=1.0):
    """z: the raw logits of a row's children in token order.  Returns (y, kept, cum_k): y = z / temperature, the kept mask after
    top_k and top_p, and for every child the cumulative softmax mass S_i = sum_{j kept by top_k, y_j <= y_i} p_j that top_p compares
    with 1 - top_p (NaN for a child top_k dropped)."""
    y = np.asarray(z, dtype=np.float64) / float(temperature)
    F = y.shape[0]
    kept = np.ones(F, dtype=bool)
    if top_k and top_k > 0:
        kk = min(max(int(top_k), 1), F)
        kept = y >= np.sort(y)[::-1][kk - 1]
    w = np.where(kept, np.exp(y - y.max()), 0.0)
    p = w / w.sum()
    cum = np.array([p[kept & (y <= y[i])].sum() if kept[i] else np.nan for i in range(F)])
    if top_p < 1.0:
        stay = kept & (cum > 1.0 - float(top_p))
        stay[int(np.argmax(y))] = True
        stay |= kept & (y == y.max())
        kept = stay
    return y, kept, cum


def cdf(y, kept):
    """(lo, hi, logq): the CDF interval [lo_i, hi_i) of every kept child in token order (NaN for the others) and its log-probability
    under the distribution sampled from, (y_i - y_max) - log W."""
    w = np.where(kept, np.exp(y - y.max()), 0.0)
    W = w.sum()
    hi = np.cumsum(w) / W
    lo = hi - w / W
    nan = np.full_like(hi, np.nan)
    return np.where(kept, lo, nan), np.where(kept, hi, nan), np.where(kept, (y - y.max()) - np.log(W), nan)


def pick(z, u, temperature=1.0, top_k=0, top_p=1.0):
    """index of the drawn child: the first kept child in token order whose running sum exceeds u * W, else the last kept one"""
    y, kept, _ = warp(z, temperature, top_k, top_p)
    _, hi, _ = cdf(y, kept)
    idx = np.nonzero(kept)[0]
    over = idx[hi[idx] > float(u)]
    return int(over[0]) if over.size else int(idx[-1])


# ---------------------------------------------------------------------------------------------- the loop over the oracle's decoder
@torch.no_grad()
def walk(sd, oc, ids, mask, tries, R, max_length, temperature=1.0, top_k=0, top_p=1.0, delta=0.0, rng=None, uniforms=None, forced=None):
    """R rows per user, max_length - 1 steps.  tries: one Trie-like object with ``get(prefix)`` per user (the same one for all
    without filters).  Two uses:
      construct (rng given): every step picks, with ``rng``, one kept child whose CDF interval is wider than 4 * delta and emits
        the interval's midpoint as that step's uniform; a step without such a child raises.
      follow (uniforms given; forced = sequences (B*R, width) or None = the restatement's own picks): every step records the
        restatement's pick for the uniform and the uniform's distance from the nearest interior CDF boundary, then follows
        ``forced`` (or the pick).
    Returns dict(seq i64 (B*R, max_length), model_lp / sample_lp f64 (B*R,) along the followed path, uniforms f32 (B, R, T-1),
    want i64 (B*R, T-1) the restatement's token (-1 for a finished row), margin f64 (B*R, T-1) (inf for a finished row))."""
    B = ids.shape[0]
    rows, T = B * R, max_length
    enc = O.encode_fused(sd, oc, ids, mask)
    ext = ((1.0 - mask.reshape(B, -1).float().repeat_interleave(R, 0)) * O.FMIN)[:, None, None, :]
    st = O.DecodeState(O.cross_kv(sd, oc, enc), ext, R)
    seq = torch.zeros(rows, T, dtype=torch.int64)
    fin = [False] * rows
    model_lp, sample_lp = np.zeros(rows), np.zeros(rows)
    uni = np.zeros((rows, T - 1), dtype=np.float32) if uniforms is None else uniforms.reshape(rows, T - 1).numpy().astype(np.float32)
    want = np.full((rows, T - 1), -1, dtype=np.int64)
    margin = np.full((rows, T - 1), np.inf)
    for t in range(T - 1):
        logits = O.decoder_step(sd, oc, seq[:, t].clone(), st).double()
        lse = torch.logsumexp(logits, -1)
        for r in range(rows):
            if fin[r]:
                continue
            children = sorted(tries[r // R].get(seq[r, : t + 1].tolist()))
            assert children, ("a live row without children", r, t)
            z = logits[r, children].numpy()
            y, kept, _ = warp(z, temperature, top_k, top_p)
            lo, hi, logq = cdf(y, kept)
            if rng is not None:
                wide = [i for i in np.nonzero(kept)[0] if hi[i] - lo[i] > 4 * delta]
                if not wide:
                    raise ValueError(f"row {r} step {t}: no kept child with a CDF interval wider than {4 * delta:.3g} ({hi - lo})")
                i = int(wide[int(rng.integers(len(wide)))])
                uni[r, t] = np.float32(0.5 * (lo[i] + hi[i]))
            else:
                u = float(uni[r, t])
                i = pick(z, u, temperature, top_k, top_p)
                inner = hi[np.nonzero(kept)[0][:-1]]  # (0 and 1 decide nothing: u lies in [0, 1))
                margin[r, t] = np.abs(inner - u).min() if inner.size else np.inf
            want[r, t] = children[i]
            if forced is not None:
                tok = int(forced[r, t + 1]) if t + 1 < forced.shape[1] else 0
                assert tok in children, ("the followed sequence leaves the Trie", r, t, tok, children)
                i = children.index(tok)
            seq[r, t + 1] = children[i]
            model_lp[r] += z[i] - float(lse[r])
            sample_lp[r] += logq[i] if kept[i] else -np.inf
            fin[r] = children[i] == 1
    return dict(seq=seq, model_lp=model_lp, sample_lp=sample_lp, uniforms=torch.from_numpy(uni.reshape(B, R, T - 1).copy()), want=want,
                margin=margin)


# ---------------------------------------------------------------------------------------------- the whole-path case
B, N, L, R, MAX_LENGTH = 3, 3, 32, 8, 5
SEED = 31


def _candidates():
    """28 candidates [0, a, b(, c), 1] over spread-out token ids: fan-out <= 4 at every node (three letters and, where one candidate
    is a prefix of another, EOS)"""
    letters = [5, 411, 7003]
    g = torch.Generator().manual_seed(SEED)
    two = [[a, b] for a in letters for b in letters]
    three = [[a, b, c] for a in letters for b in letters for c in letters]
    chosen = [two[i] for i in torch.randperm(len(two), generator=g)[:5].tolist()]
    chosen += [three[i] for i in torch.randperm(len(three), generator=g)[:23].tolist()]
    return [[0] + s + [1] for s in sorted(chosen)]


@functools.lru_cache(maxsize=None)
def whole_path_case():
    """dict(oc, sd, ids, mask, cands, cands_thin, uniforms): t5-small (OracleConfig.named), B = 3 users of N = 3 passages of L = 32 tokens,
    R = 8 samples, max_length 5, and the seeded random uniforms of the capped test"""
    oc = O.OracleConfig.named("t5-small", max_item_num=4)
    sd = O.init_state_dict(oc, SEED)
    g = torch.Generator().manual_seed(SEED + 1)
    ids = torch.randint(2, 32100, (B, N, L), generator=g)
    mask = torch.ones(B, N, L, dtype=torch.bool)
    for b in range(B):
        for n in range(N):
            ln = int(torch.randint(L // 3, L + 1, (1,), generator=g))
            mask[b, n, ln:] = False
            ids[b, n, ln:] = 0
    cands = _candidates()
    # the one-piece mode's logit tolerance is 3e-2, so its delta is 0.12: a uniform is undecidable within 0.12 of every interior CDF
    # boundary, 0.24 of the unit interval per boundary.  On the Trie above (up to 3 boundaries per step) no input keeps the undecidable
    # share below 10 %; this thin Trie -- one binary choice at step 0, one at step 2 under one branch -- does
    cands_thin = [[0, 5, 411, 7003, 1], [0, 411, 5, 411, 1], [0, 411, 5, 5, 1]]
    uniforms = torch.rand(B, R, MAX_LENGTH - 1, generator=torch.Generator().manual_seed(SEED + 2))
    return dict(oc=oc, sd=sd, ids=ids, mask=mask, cands=cands, cands_thin=cands_thin, uniforms=uniforms)


def case_candidates(case, mode):
    """the Trie of the two delta-dependent whole-path tests in a precision mode: the wide one for two pieces, the thin one for one"""
    return case["cands"] if mode.endswith("x3") else case["cands_thin"]


def skipped_share(res, delta):
    """share of the live steps of a follow-mode ``walk`` whose uniform is within delta of an interior CDF boundary"""
    live = res["want"] >= 0
    return float(((res["margin"] <= delta) & live).sum()) / float(live.sum())
