"""-m gpu: sampling without replacement through the whole path -- ``GRAM.generate(do_sample=True, replacement=False)`` on t5-small
against stochastic beam search over the CPU oracle (tests/sbs_oracle.py): the case of ``sample_oracle.whole_path_case()``, N = 3
passages of L = 32 tokens, max_length 5, B = 3 users, R = 8 rows, 28 candidates of unequal depth, in every precision mode.

The selection test teacher-forces the restatement along the DEVICE's rows.  The rows before step t are what the same call returns
with max_length = t + 1 (the search is nested in its length as it is in R: the uniforms depend on the token prefix only), so the test
runs the call at every length, hands the restatement those rows and compares what each makes of them.  A (user, step) whose
smallest gap between adjacent perturbed scores among the first R + 1 candidates exceeds ``sbs_oracle.DELTA[mode]`` must select and
order exactly as the restatement; at most 10 % may be left out.  DELTA is measured on the restatement (``sbs_oracle.measure_delta``;
tests/test_sbs_host.py asserts the constants and that the restatement alone stays within the cap); modes without an entry there are
not decidable and get the log-probability and property tests only."""
import pytest
import torch

from gram_amd.utils import generation_trie as gt
from oracle import gram_oracle as O
from tests import sample_oracle as S
from tests import sbs_oracle as X
from tests.test_gpu_path import DEV, _model
from tests.test_gpu_teacher_forced import _modes, _tol

pytestmark = pytest.mark.gpu
B, R, T = S.B, S.R, S.MAX_LENGTH
NEG = float("-inf")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gram_amd
    return gram_amd


@pytest.fixture(scope="module")
def world(gpu):
    c = S.whole_path_case()
    _, _, m = _model(gpu, c["oc"], S.SEED, sd=c["sd"])
    return dict(c, m=m, fns={id(c["cands"]): gt.prefix_allowed_tokens_fn(gt.Trie(c["cands"]))})


def _draw(w, cands=None, ids=None, mask=None, r=R, seed=X.SEED, keys=X.USER_KEYS, max_length=T, fn=None, **kw):
    cands = w["cands"] if cands is None else cands
    fn = fn or w["fns"].get(id(cands)) or gt.prefix_allowed_tokens_fn(gt.Trie(cands))
    ids = w["ids"] if ids is None else ids
    mask = w["mask"] if mask is None else mask
    out = w["m"].generate(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), max_length=max_length, prefix_allowed_tokens_fn=fn,
                          do_sample=True, num_beams=1, num_return_sequences=r, replacement=False, seed=seed,
                          user_keys=torch.tensor(list(keys), dtype=torch.int64), **kw)
    assert out["sequences_scores"] is None
    return out, fn


def _pad(seqs, n=T):
    seqs = seqs.cpu()
    return torch.nn.functional.pad(seqs, (0, n - seqs.shape[1]))


FIELDS = ("sequence_logprobs", "sample_logprobs", "perturbed_scores")


def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    return (torch.equal(_pad(a["sequences"])[rows_a], _pad(b["sequences"])[rows_b])
            and all(torch.equal(a[k].cpu()[rows_a].view(torch.int32), b[k].cpu()[rows_b].view(torch.int32)) for k in FIELDS))


def _user_rows(out, n, r=R):
    """per user the live rows of a call's result as token tuples of length n, in the order returned"""
    seqs, G = _pad(out["sequences"], n).view(B, r, n), out["perturbed_scores"].cpu().view(B, r)
    return [[tuple(seqs[b, j].tolist()) for j in range(r) if G[b, j] > NEG] for b in range(B)]


@pytest.fixture(scope="module")
def forced(world):
    """per mode: the call at every length 2 .. T and the restatement teacher-forced along those rows"""
    w, res = world, {}
    for mode in _modes():
        w["m"].set_precision(mode)
        runs = {n: _draw(w, max_length=n)[0] for n in range(2, T + 1)}
        before = [[[(0,)] for _ in range(B)]] + [_user_rows(runs[t + 1], t + 1) for t in range(1, T - 1)]
        hist = X.walk(w["sd"], w["oc"], w["ids"], w["mask"], [O.Trie(w["cands"])] * B, R, T, X.SEED, X.USER_KEYS, forced=before)
        res[mode] = (runs, hist)
    return res


def test_selection_against_the_restatement(world, forced):
    decided_modes = [m for m in _modes() if m in X.DELTA]
    assert decided_modes
    for mode in decided_modes:
        runs, hist = forced[mode]
        delta, left_out, wrong = X.DELTA[mode], 0, []
        for t in range(T - 1):
            got = _user_rows(runs[t + 2], t + 2)
            for b in range(B):
                if not hist[b][t]["gap"] > delta:
                    left_out += 1
                    continue
                want = [X._strip(c["prefix"]) for c in hist[b][t]["ranked"][:R]]
                if [X._strip(p) for p in got[b]] != want:
                    wrong.append((b, t, got[b], want))
        print(f"[{mode}] delta {delta:.1e}: {B * (T - 1)} (user, step) pairs, {left_out} left out, {len(wrong)} wrong; "
              f"smallest gap {min(h['gap'] for hb in hist for h in hb):.3e}")
        assert not wrong, (mode, wrong[:2])
        assert left_out <= 0.10 * B * (T - 1)


def test_log_probabilities(world, forced):
    """sample_logprobs / sequence_logprobs against the restatement along the device's own rows, in every mode; sequence_logprobs is
    what score_sequences returns for the rows; the perturbed scores descend and stay below the user's root"""
    w = world
    for mode in _modes():
        w["m"].set_precision(mode)
        runs, hist = forced[mode]
        out, tol = runs[T], _tol(mode)["logp"]
        seqs = _pad(out["sequences"]).view(B, R, T)
        G, phi, lm = (out[k].cpu().double().view(B, R) for k in ("perturbed_scores", "sample_logprobs", "sequence_logprobs"))
        worst = 0.0
        for b in range(B):
            known = {X._strip(c["prefix"]): c for c in hist[b][-1]["ranked"]}
            assert bool((G[b, :-1] >= G[b, 1:]).all())
            for j in range(R):
                c = known[X._strip(seqs[b, j].tolist())]
                worst = max(worst, abs(float(phi[b, j]) - c["phi"]), abs(float(lm[b, j]) - c["model"]))
        lab = seqs[:, :, 1:].clone()
        after = (lab == 1).cumsum(-1) - (lab == 1).long()
        lab = lab.masked_fill(after > 0, -100)
        sc = w["m"].score_sequences(w["ids"].to(DEV), w["mask"].to(DEV), lab.to(DEV)).cpu().view(B, R)
        d = float((sc.double() - lm).abs().max())
        print(f"[{mode}] |log-prob - restatement| {worst:.2e}, |sequence_logprobs - score_sequences| {d:.2e} (tolerance {tol:.0e})")
        assert worst < tol and d < tol
        assert bool((phi <= 0).all()) and bool((lm < phi + tol).all())  # (the Trie-renormalised probability is the larger one)


def test_rows_are_distinct_items(world, forced):
    w = world
    for mode in _modes():
        out = forced[mode][0][T]
        items = w["m"].sequence_items(out["sequences"], w["fns"][id(w["cands"])], w["cands"]).cpu().view(B, R)
        assert bool((items >= 0).all())
        for b in range(B):
            assert len(set(items[b].tolist())) == R, (mode, b, items[b])


def test_bit_exact_invariance(world, forced):
    """A user's rows depend on (seed, its key, its passages) only: the user alone, R' = 3 against the first 3 rows of R = 8, the
    batch padded to a longer L and with ragged masks, the passage cache; another seed or key is another draw"""
    w = world
    m = w["m"]
    for mode in _modes():
        m.set_precision(mode)
        full = forced[mode][0][T]
        for b in range(B):
            one, _ = _draw(w, ids=w["ids"][b:b + 1], mask=w["mask"][b:b + 1], keys=X.USER_KEYS[b:b + 1])
            assert _same(one, full, rows_b=slice(b * R, (b + 1) * R)), (mode, "user alone", b)
        three, _ = _draw(w, r=3)
        for b in range(B):
            assert _same(three, full, slice(b * 3, b * 3 + 3), slice(b * R, b * R + 3)), (mode, "R' = 3", b)
        swapped, _ = _draw(w, ids=w["ids"].flip(0), mask=w["mask"].flip(0), keys=X.USER_KEYS[::-1])
        for b in range(B):
            assert _same(swapped, full, slice((B - 1 - b) * R, (B - b) * R), slice(b * R, (b + 1) * R)), (mode, "place in the batch", b)
        ids64 = torch.nn.functional.pad(w["ids"], (0, 32))
        mask64 = torch.nn.functional.pad(w["mask"], (0, 32))
        longer, _ = _draw(w, ids=ids64, mask=mask64)
        assert _same(longer, full), (mode, "padded to L = 64")
        try:
            m.cache_passages(w["ids"].to(DEV), w["mask"].to(DEV))
            cached, _ = _draw(w)
        finally:
            m.clear_passage_cache()
        assert _same(cached, full), (mode, "passage cache")
        other_seed, _ = _draw(w, seed=X.SEED + 1)
        other_keys, _ = _draw(w, keys=[k + 1 for k in X.USER_KEYS])
        for other in (other_seed, other_keys):
            assert not torch.equal(other["perturbed_scores"].cpu(), full["perturbed_scores"].cpu())
            assert not torch.equal(_pad(other["sequences"]), _pad(full["sequences"]))


def test_item_filters_equal_per_user_tries(world):
    """exclude_items / allowed_items: bit for bit what the user gets alone with Trie(A_b) -- the uniforms are keyed by the token
    prefix, not by the Trie's nodes; no excluded item is ever returned"""
    w = world
    m, cands = w["m"], w["cands"]
    n = len(cands)
    g = torch.Generator().manual_seed(S.SEED + 3)
    first = cands[0][1]
    lists = [[i for i, c in enumerate(cands) if c[1] == first],  # an inner node dies
             torch.randperm(n, generator=g)[:15].tolist(),
             [i for i in range(n) if i % 3 == 0]]
    keep = [sorted(set(range(n)) - set(r)) for r in lists]
    assert all(len(k) >= R for k in keep)
    for mode in _modes():
        m.set_precision(mode)
        for kind, kw in (("exclude", dict(exclude_items=lists)), ("allow", dict(allowed_items=keep))):
            out, fn = _draw(w, candidates=cands, **kw)
            items = m.sequence_items(out["sequences"], fn, cands).cpu().view(B, R)
            for b in range(B):
                assert set(items[b].tolist()) <= set(keep[b]) and len(set(items[b].tolist())) == R, (mode, kind, b, items[b])
                alone, _ = _draw(w, [cands[i] for i in keep[b]], ids=w["ids"][b:b + 1], mask=w["mask"][b:b + 1], keys=X.USER_KEYS[b:b + 1])
                assert _same(alone, out, rows_b=slice(b * R, (b + 1) * R)), (mode, kind, b)


def test_too_few_items_leave_dead_rows(world):
    """a user left with 3 items gets them all, in some order, then rows of the start token and padding with -inf -- and no error"""
    w = world
    m, cands = w["m"], w["cands"]
    m.set_precision(_modes()[0])
    keep = [[3, 17, 20], list(range(len(cands))), [5]]
    out, fn = _draw(w, candidates=cands, allowed_items=keep)
    seqs = _pad(out["sequences"]).view(B, R, T)
    items = m.sequence_items(out["sequences"], fn, cands).cpu().view(B, R)
    for b, n in enumerate((3, R, 1)):
        assert sorted(items[b, :n].tolist()) == sorted(keep[b]) if n < R else len(set(items[b].tolist())) == R
        assert bool((seqs[b, n:] == 0).all())
        for k in FIELDS:
            v = out[k].cpu().view(B, R)[b]
            assert bool(torch.isfinite(v[:n]).all()) and bool((v[n:] == NEG).all()), (b, k, v)
    # the three items of user 0 carry their whole Trie-renormalised mass
    p = out["sample_logprobs"].cpu().double().view(B, R)[0, :3].exp().sum()
    assert abs(float(p) - 1.0) < 1e-3
