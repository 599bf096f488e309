"""Beam search with per-item score biases restated over oracle.gram_oracle -- not a test module (compare tests/group_oracle.py).

``generate(num_beams=K >= 2, item_bias=T, bias_lookahead=...)`` as DESIGN.md section 4.11 specifies it: HF 4.26 ``beam_search``
with the runners' kwargs, over a Trie, with one more term per candidate.  Potentials phi[r][n] (fp32; r = 0 for a shared bias, the
user otherwise; n a Trie node of ``FlatTrie``'s numbering): a leaf's is T[r][its item] -- the FIRST candidate that spells the leaf's
sequence --, an internal node's the max over the leaves below it (lookahead) or 0, the root's and the start node's 0.  The candidate
that moves a beam from node p to its child c scores, all fp32 and in this order,

    s = (logit - lse) + (phi[c] - phi[p]);   s = s + beam_score

and everything else is the plain search on these scores.  ``keep`` (one boolean array over the leaf ranks per user) restricts a
user to the leaves it keeps, as ``exclude_items`` / ``allowed_items`` do; the potentials ignore it.

The search also measures its *decision margin* (``group_oracle.Margin``): ``whole_path_cases`` are inputs whose margin is well
above the deviation of a device's scores.
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional

import numpy as np
import torch

from gram_amd.utils import generation_trie as gt
from oracle import gram_oracle as O
from tests import group_oracle as GO
from tests.group_oracle import BIG, Margin, _Heap  # noqa: F401  (the Margin of the group search's restatement)

MIN_MARGIN = 5e-4  # the bar of the group search's cases, above 10 x SCORE_TOL of tests/test_gpu_path.py


def flat_trie(cands) -> gt.FlatTrie:
    return gt.FlatTrie(gt.Trie(cands))


def potentials(cands, T, lookahead: bool, start_token: int = 0, flat: Optional[gt.FlatTrie] = None) -> np.ndarray:
    """phi float32 [rows][n_nodes] over FlatTrie(Trie(cands)) from T float32 [n_items] or [rows][n_items] (numpy).  The max is
    numpy's over float32 values: exact (the test data holds no -0.0, the one pair of equal values with different bits)."""
    flat = flat or flat_trie(cands)
    T = np.asarray(T, dtype=np.float32).reshape(-1, len(cands))
    lo, hi = flat.leaf_ranges()
    item = flat.node_items(cands)
    fan = np.diff(flat.child_off)
    leaf = (fan == 0) & (np.arange(flat.n_nodes) > 0)
    leaf_item = np.full(int(hi[0]), -1, dtype=np.int64)
    leaf_item[lo[leaf]] = item[leaf]
    vals = np.where(leaf_item[None, :] >= 0, T[:, np.maximum(leaf_item, 0)], np.float32(0)).astype(np.float32)  # [rows][n_leaves]
    phi = np.zeros((T.shape[0], flat.n_nodes), dtype=np.float32)
    for n in range(1, flat.n_nodes):
        if (leaf[n] or lookahead) and hi[n] > lo[n]:
            phi[:, n] = vals[:, lo[n]:hi[n]].max(axis=1)
    phi[:, 0] = 0
    s = flat.leaf_of([start_token])
    if s > 0:
        phi[:, s] = 0
    return phi


def bias_beam_search(step_fn: Callable, reorder_fn: Callable, batch_size: int, num_beams: int, max_length: int, flat: gt.FlatTrie,
                     phi: Optional[np.ndarray], length_penalty: float = 1.0, num_return_sequences: Optional[int] = None,
                     pad_token_id: int = 0, eos_token_id: int = 1, decoder_start_token_id: int = 0, early_exit: bool = True,
                     trace: Optional[list] = None, lse_fn: Optional[Callable] = None, margin: Optional[Margin] = None,
                     keep: Optional[List[np.ndarray]] = None):
    """step_fn(last tokens (R,)) -> logits (R, V); reorder_fn(beam_idx (R,)).  phi: potentials [1 or B][n_nodes], None = all zero.
    lse_fn(step, logits) -> the normaliser (R,) fp32 (log-probabilities are then logit - lse, the kernel's arithmetic).  trace: one
    dict per step with tokens (B, K), beam_scores (B, K), done [B], input_ids after the step.  Returns (sequences (B * nret, width)
    int64, sequences_scores (B * nret,) fp32) as O.beam_search does."""
    B, K = batch_size, num_beams
    nret = num_return_sequences or K
    R = B * K
    lo, hi = flat.leaf_ranges()
    off, ctok, cnode = flat.child_off, flat.child_tok, flat.child_node
    if phi is None:
        phi = np.zeros((1, flat.n_nodes), dtype=np.float32)
    phi_t = torch.from_numpy(np.ascontiguousarray(phi, dtype=np.float32))
    input_ids = torch.full((R, 1), decoder_start_token_id, dtype=torch.long)
    node = [flat.leaf_of([decoder_start_token_id])] * R  # the Trie node of every beam, -1 once it has left the Trie
    beam_scores = torch.full((B, K), -1e9, dtype=torch.float32)
    beam_scores[:, 0] = 0
    beam_scores = beam_scores.view(R)
    hyps = [_Heap(K, length_penalty, margin) for _ in range(B)]
    done = [False] * B
    step = 0

    def alive(b, n):
        return keep is None or bool(keep[b][lo[n]:hi[n]].any())

    while True:
        cur_len = input_ids.shape[1]
        logits = step_fn(input_ids[:, -1]).float().cpu()
        V = logits.shape[-1]
        if lse_fn is None:
            logp = torch.log_softmax(logits, dim=-1)
        else:
            logp = logits - lse_fn(step, logits).float().cpu()[:, None]
        nb_scores = torch.zeros(B, K, dtype=torch.float32)
        nb_tokens = torch.full((B, K), pad_token_id, dtype=torch.long)
        nb_idx = torch.arange(R, dtype=torch.long).view(B, K).clone()
        nb_node = [-1] * R
        for b in range(B):
            if done[b]:
                continue  # score 0, token pad; parents are never read
            r = b if phi_t.shape[0] > 1 else 0
            s = torch.full((K, V), -math.inf, dtype=torch.float32)
            child_of = {}
            for j in range(K):
                n = node[b * K + j]
                if n < 0:
                    continue
                edges = [e for e in range(int(off[n]), int(off[n + 1])) if alive(b, int(cnode[e]))]
                if not edges:
                    continue
                toks = torch.from_numpy(ctok[edges].astype(np.int64))
                ch = torch.from_numpy(cnode[edges].astype(np.int64))
                child_of.update({(j, int(t)): int(c) for t, c in zip(toks, ch)})
                s[j, toks] = logp[b * K + j, toks] + (phi_t[r, ch] - phi_t[r, n])  # fp32: one rounding per operation
            s = (s + beam_scores[b * K:(b + 1) * K][:, None]).view(K * V)
            top, flat_idx = O.topk_candidates(s, 2 * K + 1 if K * V > 2 * K else 2 * K)
            if margin is not None:
                for rk in range(top.numel() - 1):
                    if top[rk + 1] > BIG:
                        margin.see(float(top[rk] - top[rk + 1]), ("rank", cur_len, b, rk))
            j = 0
            for rank in range(2 * K):
                tok = int(flat_idx[rank] % V)
                k = int(flat_idx[rank] // V)
                sc = top[rank]
                row = b * K + k
                if tok == eos_token_id:
                    if rank >= K:
                        continue
                    hyps[b].add(input_ids[row].tolist(), float(sc))
                else:
                    nb_scores[b, j] = sc
                    nb_tokens[b, j] = tok
                    nb_idx[b, j] = row
                    nb_node[b * K + j] = child_of.get((k, tok), -1)  # (-1: a -inf filler, no Trie edge)
                    j += 1
                if j == K:
                    break
            if j < K:
                raise ValueError("fewer than num_beams non-EOS candidates in the top 2 * num_beams")
            done[b] = done[b] or hyps[b].is_done(float(top[0]), cur_len)
        beam_scores = nb_scores.view(R)
        beam_idx = nb_idx.view(R)
        input_ids = torch.cat([input_ids[beam_idx], nb_tokens.view(R, 1)], dim=-1)
        node = nb_node
        reorder_fn(beam_idx)
        if trace is not None:
            trace.append(dict(cur_len=cur_len, tokens=nb_tokens.clone(), beam_scores=nb_scores.clone(), done=list(done),
                              input_ids=input_ids.clone()))
        step += 1
        if (early_exit and all(done)) or input_ids.shape[1] >= max_length:
            break

    for b in range(B):  # BeamSearchScorer.finalize
        if done[b]:
            continue
        for k in range(K):
            hyps[b].add(input_ids[b * K + k].tolist(), float(beam_scores[b * K + k]))
    best: List[List[int]] = []
    best_scores = torch.zeros(B * nret, dtype=torch.float32)
    for b in range(B):
        ordered = sorted(hyps[b].beams, key=lambda x: x[0])
        if margin is not None:
            for a, c in zip(ordered, ordered[1:]):
                if a[0] > BIG:
                    margin.see(c[0] - a[0], ("final", b))
        for j in range(nret):
            sc, h = ordered.pop()
            best.append(h)
            best_scores[b * nret + j] = sc
    width = min(max(len(h) for h in best) + 1, max_length)
    decoded = torch.full((B * nret, width), pad_token_id, dtype=torch.long)
    for i, h in enumerate(best):
        decoded[i, : len(h)] = torch.tensor(h, dtype=torch.long)
        if len(h) < width:
            decoded[i, len(h)] = eos_token_id
    return decoded, best_scores


def keep_masks(flat: gt.FlatTrie, cands, lists, allow: bool) -> List[np.ndarray]:
    """per user: the leaf ranks it keeps under an exclude (allow=False) or allow list of candidate indices"""
    ranks = flat.item_ranks(cands)
    n_leaves = int(flat.leaf_ranges()[1][0])
    out = []
    for r in lists:
        m = np.zeros(n_leaves, dtype=bool) if allow else np.ones(n_leaves, dtype=bool)
        m[ranks[np.asarray(r, dtype=np.int64)]] = allow
        out.append(m)
    return out


def logits_search(logits_per_step, lse_per_step, cands, B, K, T, lookahead=True, lp=1.0, early_exit=False, trace=None, margin=None,
                  nret=None, keep=None, phi=None):
    """The search on given logits [T][B * K][V] and normalisers [T][B * K] over Trie(cands) with bias T (None: the plain search;
    phi: ready-made potentials instead) -- the kernel-level tests' restatement"""
    flat = flat_trie(cands)
    if phi is None and T is not None:
        phi = potentials(cands, T, lookahead, flat=flat)
    it = iter(logits_per_step)
    return bias_beam_search(lambda tok: next(it), lambda idx: None, B, K, max(len(c) for c in cands), flat, phi, lp, nret,
                            early_exit=early_exit, trace=trace, lse_fn=None if lse_per_step is None else (lambda t, lg: lse_per_step[t]),
                            margin=margin, keep=keep)


def generate(sd, cfg, input_ids, attention_mask, max_length, cands, num_beams, T, lookahead=True, length_penalty=1.0,
             num_return_sequences=None, early_exit=True, trace=None, margin=None, keep=None):
    """O.generate with the biased search in beam_search's place (the bank shared by a user's beams); T = None: the plain search"""
    B, N, L = input_ids.shape
    K = num_beams
    flat = flat_trie(cands)
    phi = None if T is None else potentials(cands, T, lookahead, cfg.decoder_start_token_id, flat)
    with torch.no_grad():
        enc = O.encode_fused(sd, cfg, input_ids, attention_mask)
        mask_rows = attention_mask.reshape(B, N * L).to(torch.float32).repeat_interleave(K, dim=0)
        ext = ((1.0 - mask_rows) * O.FMIN)[:, None, None, :]
        st = O.DecodeState(cross=O.cross_kv(sd, cfg, enc), enc_mask_ext=ext, rows_per_bank=K)
        return bias_beam_search(lambda tok: O.decoder_step(sd, cfg, tok, st), st.reorder, B, K, max_length, flat, phi, length_penalty,
                                num_return_sequences, cfg.pad_token_id, cfg.eos_token_id, cfg.decoder_start_token_id, early_exit, trace,
                                None, margin, keep)


# ---- the inputs of the whole-path GPU test ------------------------------------------------------------------------------------------
def make_case(B, N, L, K, per_user, seed):
    """One whole-path case from its shape, bias kind and seed: group_oracle's weights, inputs and random Trie of 40-200 items of
    depth 2-4, and a bias drawn from N(0, 1.5^2), clipped to +-4"""
    case = GO.make_case(B, N, L, K, 1, 0.0, seed)
    g = torch.Generator().manual_seed(7000 + 100 * seed + 2 * K + int(per_user))
    n = len(case["cands"])
    bias = (torch.randn((B, n) if per_user else (n,), generator=g) * 1.5).clamp_(-4.0, 4.0).to(torch.float32)
    case.update(per_user=per_user, bias=bias)
    del case["G"], case["lam"]
    return case


def run_case(case, bias="case", lookahead=True, **kw):
    """The restatement on a whole-path case -> (sequences, scores); bias=None: the plain search"""
    sd = O.init_state_dict(case["cfg"], case["model_seed"])
    T = case["bias"].numpy() if isinstance(bias, str) else bias
    return generate(sd, case["cfg"], case["input_ids"], case["attention_mask"], case["max_length"], case["cands"], case["K"], T,
                    lookahead, case["length_penalty"], **kw)


def case_properties(case):
    """(margin with lookahead, margin without, the bias changes a list, the lookahead changes a list)"""
    m1, m0 = Margin(), Margin()
    look, _ = run_case(case, lookahead=True, margin=m1, early_exit=False)
    leaf, _ = run_case(case, lookahead=False, margin=m0, early_exit=False)
    plain, _ = run_case(case, bias=None)
    differs = lambda a, b: a.shape != b.shape or not torch.equal(a, b)  # noqa: E731
    return m1.value, m0.value, differs(look, plain), differs(look, leaf)


def find_seed(B, N, L, K, per_user, limit=32):
    """the first of the seeds 0, 1, 2, ... whose case has (a) both margins >= MIN_MARGIN, (b) a list the bias changes and (c) a list
    the lookahead changes; how WHOLE_PATH_SEEDS was filled"""
    for seed in range(limit):
        m1, m0, b, c = case_properties(make_case(B, N, L, K, per_user, seed))
        if min(m1, m0) >= MIN_MARGIN and b and c:
            return seed
    raise ValueError("no seed found")


# (B, N, L, K, per-user bias) -> the seed: find_seed's answer, the FIRST of 0, 1, 2, ... with the three properties
# (tests/test_item_bias_host.py checks both: the properties of every entry, and that no earlier seed has them).  A seed fixes the
# weights, inputs and Trie as group_oracle.make_case(B, N, L, K, 1, 0.0, seed) does, and the bias through a generator of its own
# seeded 7000 + 100 * seed + 2 * K + per_user (make_case above): with these draws the per-user cases needed seeds 0, 1, 4, 0 and the
# shared ones 0, 1, 5, 0.
WHOLE_PATH_SEEDS = {(3, 2, 32, 4, False): 0, (3, 2, 32, 4, True): 0, (2, 3, 32, 6, False): 1, (2, 3, 32, 6, True): 1,
                    (2, 1, 32, 20, False): 5, (2, 1, 32, 20, True): 4, (2, 2, 32, 8, False): 0, (2, 2, 32, 8, True): 0}


def whole_path_cases():
    return [make_case(*shape, seed) for shape, seed in WHOLE_PATH_SEEDS.items()]
