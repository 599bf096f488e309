"""Group (diverse) beam search restated over oracle.gram_oracle -- not a test module (compare tests/sample_oracle.py).

HF 4.26 ``group_beam_search`` + ``HammingDiversityLogitsProcessor`` with the runners' other kwargs (early_stopping=False,
do_sample=False), as DESIGN.md section 4.9 specifies it.  HF 4.26 is not installed here; where it turns out to differ, section 4.9
and this restatement of it are what the HIP path implements.

K beams = G groups of gs = K / G; group g owns beams [g gs, (g + 1) gs) of every user.  One BeamHypotheses heap of capacity K and
one done flag per user, shared by its groups.  Per step the decoder runs once over all K rows, then for g = 0 .. G - 1 and every
user (all fp32, in this order):

    s = logit - lse;   s = s - fl(lambda) * float(c_v);   s = -inf outside the Trie;   s = s + beam_score

c_v = the beams of groups 0 .. g - 1 of this user whose token chosen in this step is v.  The best 2 gs of the gs * V candidates
(ties to the lower flat index j * V + v) go through BeamSearchScorer.process with group size gs; done |= heap.is_done(the group's
rank-0 score, cur_len).  A user can finish at group g of a step: its later groups are padded (score 0, token pad) in that step.

``group_beam_search`` also measures the search's *decision margin* (see ``Margin``): how far the closest decision of the whole
search was from going the other way.  A whole-path test on a device whose scores deviate by e from these needs inputs whose margin
is well above e; ``whole_path_cases`` are such inputs.
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional

import torch

from oracle import gram_oracle as O

BIG = -1e8  # scores at or below this are the -1e9-class start scores and -inf fillers: ordered by index, or 1e8 away


class Margin:
    """The smallest of (a) the gaps between consecutive entries of every group's sorted candidate list, rank 0 down to rank 2 gs
    against the first one left out, over pairs with both scores above -1e8; (b) |new - worst| at every insertion into a full heap;
    (c) |worst - best / cur_len^lp| at every is_done on a full heap -- an exact 0 is exempt: the step's best candidate is the EOS
    hypothesis just stored as the heap's worst, compared with itself; (d) the adjacent gaps of every user's final sorted heap among
    scores above -1e8."""

    def __init__(self):
        self.value = math.inf
        self.where = None

    def see(self, gap: float, where) -> None:
        if gap < self.value:
            self.value, self.where = gap, where


class _Heap(O.BeamHypotheses):
    """BeamHypotheses that reports (b) and (c) to a Margin"""

    def __init__(self, num_beams, length_penalty, margin: Optional[Margin]):
        super().__init__(num_beams, length_penalty)
        self.margin = margin

    def add(self, hyp, sum_logprobs):
        if self.margin is not None and len(self) >= self.num_beams:
            score = sum_logprobs / (len(hyp) ** self.length_penalty)
            if score > BIG and self.worst_score > BIG:
                self.margin.see(abs(score - self.worst_score), ("heap", len(hyp)))
        super().add(hyp, sum_logprobs)

    def is_done(self, best_sum_logprobs, cur_len):
        if self.margin is not None and len(self) >= self.num_beams:
            cur = best_sum_logprobs / cur_len ** self.length_penalty
            gap = abs(self.worst_score - cur)
            if gap != 0.0 and cur > BIG and self.worst_score > BIG:
                self.margin.see(gap, ("is_done", cur_len))
        return super().is_done(best_sum_logprobs, cur_len)


def group_beam_search(step_fn: Callable, reorder_fn: Callable, batch_size: int, num_beams: int, num_beam_groups: int,
                      diversity_penalty: float, max_length: int, prefix_fn: Callable, length_penalty: float = 1.0,
                      num_return_sequences: Optional[int] = None, pad_token_id: int = 0, eos_token_id: int = 1,
                      decoder_start_token_id: int = 0, early_exit: bool = True, trace: Optional[list] = None,
                      lse_fn: Optional[Callable] = None, margin: Optional[Margin] = None):
    """step_fn(last tokens (R,)) -> logits (R, V); reorder_fn(beam_idx (R,)); prefix_fn(b, input_ids row) -> allowed tokens.
    lse_fn(step, logits) -> the normaliser (R,) fp32: log-probabilities are then logit - lse instead of torch.log_softmax (a test hands a kernel the
    same one).  trace: one dict per step with tokens (B, K), beam_scores (B, K), done [B] after the step.  Returns (sequences
    (B * nret, width) int64, sequences_scores (B * nret,) fp32) as O.beam_search does."""
    B, K, G = batch_size, num_beams, num_beam_groups
    assert G >= 1 and K % G == 0
    gs = K // G
    nret = num_return_sequences or K
    R = B * K
    lam = torch.tensor(float(diversity_penalty), dtype=torch.float32)
    input_ids = torch.full((R, 1), decoder_start_token_id, dtype=torch.long)
    beam_scores = torch.full((B, K), -1e9, dtype=torch.float32)
    beam_scores[:, ::gs] = 0
    beam_scores = beam_scores.view(R)
    hyps = [_Heap(K, length_penalty, margin) for _ in range(B)]
    done = [False] * B
    step = 0
    while True:
        cur_len = input_ids.shape[1]
        logits = step_fn(input_ids[:, -1]).float().cpu()
        V = logits.shape[-1]
        if lse_fn is None:  # HF's own op (what O.beam_search calls); with a given normaliser: logit - lse, the kernel's arithmetic
            logp = torch.log_softmax(logits, dim=-1)
        else:
            logp = logits - lse_fn(step, logits).float().cpu()[:, None]
        nb_scores = torch.zeros(B, K, dtype=torch.float32)
        nb_tokens = torch.full((B, K), pad_token_id, dtype=torch.long)
        nb_idx = torch.arange(R, dtype=torch.long).view(B, K).clone()
        for g in range(G):
            k0 = g * gs
            for b in range(B):
                if done[b]:
                    continue  # score 0, token pad; parents are never read
                rows = torch.arange(b * K + k0, b * K + k0 + gs)
                s = logp[rows]
                if g > 0:
                    cnt = torch.bincount(nb_tokens[b, :k0], minlength=V).to(torch.float32)
                    s = s - lam * cnt
                allowed = torch.zeros(gs, V, dtype=torch.bool)
                for j in range(gs):
                    a = prefix_fn(b, input_ids[b * K + k0 + j])
                    if a:
                        allowed[j, torch.tensor([int(x) for x in a], dtype=torch.long)] = True
                s = torch.where(allowed, s, torch.tensor(-math.inf))
                s = (s + beam_scores[rows][:, None]).view(gs * V)
                top, flat = O.topk_candidates(s, 2 * gs + 1 if gs * V > 2 * gs else 2 * gs)
                if margin is not None:
                    for r in range(top.numel() - 1):
                        if top[r + 1] > BIG:
                            margin.see(float(top[r] - top[r + 1]), ("rank", cur_len, b, g, r))
                j = 0
                for rank in range(2 * gs):
                    tok = int(flat[rank] % V)
                    sc = top[rank]
                    row = b * K + k0 + int(flat[rank] // V)
                    if tok == eos_token_id:
                        if rank >= gs:
                            continue
                        hyps[b].add(input_ids[row].tolist(), float(sc))
                    else:
                        nb_scores[b, k0 + j] = sc
                        nb_tokens[b, k0 + j] = tok
                        nb_idx[b, k0 + j] = row
                        j += 1
                    if j == gs:
                        break
                if j < gs:
                    raise ValueError("fewer than group-size non-EOS candidates in the group's top 2 * group size")
                done[b] = done[b] or hyps[b].is_done(float(top[0]), cur_len)
        beam_scores = nb_scores.view(R)
        beam_idx = nb_idx.view(R)
        input_ids = torch.cat([input_ids[beam_idx], nb_tokens.view(R, 1)], dim=-1)
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
            for lo, hi in zip(ordered, ordered[1:]):
                if lo[0] > BIG:
                    margin.see(hi[0] - lo[0], ("final", b))
        for j in range(nret):
            s, h = ordered.pop()
            best.append(h)
            best_scores[b * nret + j] = s
    width = min(max(len(h) for h in best) + 1, max_length)
    decoded = torch.full((B * nret, width), pad_token_id, dtype=torch.long)
    for i, h in enumerate(best):
        decoded[i, : len(h)] = torch.tensor(h, dtype=torch.long)
        if len(h) < width:
            decoded[i, len(h)] = eos_token_id
    return decoded, best_scores


def logits_search(logits_per_step, lse_per_step, cands, B, K, G, lam, lp=1.0, early_exit=False, trace=None, margin=None, nret=None):
    """The search on given logits [T][B * K][V] and normalisers [T][B * K] over Trie(cands) (the kernel-level tests' restatement)"""
    trie = O.Trie(cands)
    it = iter(logits_per_step)
    return group_beam_search(lambda tok: next(it), lambda idx: None, B, K, G, lam, max(len(c) for c in cands),
                             O.prefix_allowed_tokens_fn(trie), lp, nret, early_exit=early_exit, trace=trace,
                             lse_fn=None if lse_per_step is None else (lambda t, lg: lse_per_step[t]), margin=margin)


def generate(sd, cfg, input_ids, attention_mask, max_length, prefix_fn, num_beams, num_beam_groups, diversity_penalty,
             length_penalty=1.0, num_return_sequences=None, early_exit=True, trace=None, margin=None):
    """O.generate with the group search in beam_search's place (the bank shared by a user's beams)"""
    B, N, L = input_ids.shape
    K = num_beams
    with torch.no_grad():
        enc = O.encode_fused(sd, cfg, input_ids, attention_mask)
        mask_rows = attention_mask.reshape(B, N * L).to(torch.float32).repeat_interleave(K, dim=0)
        ext = ((1.0 - mask_rows) * O.FMIN)[:, None, None, :]
        st = O.DecodeState(cross=O.cross_kv(sd, cfg, enc), enc_mask_ext=ext, rows_per_bank=K)
        return group_beam_search(lambda tok: O.decoder_step(sd, cfg, tok, st), st.reorder, B, K, num_beam_groups, diversity_penalty,
                                 max_length, prefix_fn, length_penalty, num_return_sequences, cfg.pad_token_id, cfg.eos_token_id,
                                 cfg.decoder_start_token_id, early_exit, trace, None, margin)


# ---- the inputs of the whole-path GPU test ------------------------------------------------------------------------------------------
def tiny_config() -> O.OracleConfig:
    """the tiny model of tests/test_gpu_path.py"""
    return O.OracleConfig(vocab_size=256, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2, max_item_num=5)


def random_cands(g: torch.Generator, n_items: int, depth_lo: int, depth_hi: int, V: int, first: int = 6):
    """n_items distinct item ids of depth_lo .. depth_hi pieces (tokens in [2, V); `first` distinct first pieces, so that the
    items share prefixes as hierarchical ids do), as sequences [0, pieces ..., 1]; no id is a prefix of another"""
    seen, out = set(), []
    heads = torch.randperm(V - 2, generator=g)[:first].add(2).tolist()
    while len(out) < n_items:
        depth = int(torch.randint(depth_lo, depth_hi + 1, (1,), generator=g))
        toks = [heads[int(torch.randint(0, first, (1,), generator=g))]]
        toks += torch.randint(2, 2 + 12, (depth - 1,), generator=g).tolist()
        t = tuple(toks)
        if any(t[:i] in seen for i in range(1, len(t) + 1)) or any(s[: len(t)] == t for s in seen):
            continue
        seen.add(t)
        out.append([0, *t, 1])
    return out


def make_case(B, N, L, K, G, lam, seed):
    """One whole-path case from its shape and seed: weights, inputs and a random Trie of 40-200 items of depth 2-4"""
    cfg = tiny_config()
    g = torch.Generator().manual_seed(1000 * seed + 17 * K + G)
    n_items = int(torch.randint(max(40, 2 * K), 201, (1,), generator=g))
    cands = random_cands(g, n_items, 2, 4, cfg.vocab_size)
    ids = torch.randint(2, cfg.vocab_size, (B, N, L), generator=g)
    mask = torch.ones(B, N, L, dtype=torch.bool)
    for b in range(B):
        for n in range(N):
            ln = int(torch.randint(L // 3, L + 1, (1,), generator=g))
            mask[b, n, ln:] = False
            ids[b, n, ln - 1] = 1
            ids[b, n, ln:] = 0
    return dict(B=B, N=N, L=L, K=K, G=G, lam=lam, seed=seed, cfg=cfg, model_seed=100 + seed, cands=cands, input_ids=ids,
                attention_mask=mask, max_length=max(len(c) for c in cands), length_penalty=1.0)


# (B, N, L, K, G, lambda) -> the seed: the first of seeds 0, 1, 2, ... whose decision margin on the oracle model is >= 5e-4 and at
# which the penalty changes some user's list (tests/test_group_search_host.py checks both properties of every entry)
WHOLE_PATH_SHAPES = {(3, 2, 32, 4, 2, 0.5): 0, (2, 3, 32, 6, 3, 1.0): 0, (2, 1, 32, 20, 5, 0.5): 0, (2, 2, 32, 8, 8, 1.0): 0}


def whole_path_cases():
    return [make_case(*shape, seed) for shape, seed in WHOLE_PATH_SHAPES.items()]


def run_case(case, lam=None, **kw):
    """The restatement on a whole-path case -> (sequences, scores)"""
    sd = O.init_state_dict(case["cfg"], case["model_seed"])
    trie = O.Trie(case["cands"])
    return generate(sd, case["cfg"], case["input_ids"], case["attention_mask"], case["max_length"], O.prefix_allowed_tokens_fn(trie),
                    case["K"], case["G"], case["lam"] if lam is None else lam, case["length_penalty"], **kw)
