"""-m gpu: Trie-constrained sampling through the whole path -- ``GRAM.generate(do_sample=True)`` on t5-small against the sampling loop
over the CPU oracle (tests/sample_oracle.py): N = 3 passages of L = 32 tokens, max_length 5, B = 3 users, R = 8 samples, Tries of at
most 30 candidates with fan-out <= 4, in every precision mode.

delta = 4 * TOL[mode]['logit'] / temperature is how far a uniform must be from a boundary of the oracle's CDF for the device to have
to agree: TOL's logit entry bounds the device's logits against the oracle's, a boundary is a ratio of sums of exp(logit), and the
derivative of such a ratio with respect to any one logit is at most 1/4, so the factor 4 covers every child moving at once with
room to spare.  The two delta-dependent tests run on the Trie that is decidable at their mode's delta (sample_oracle.case_candidates;
tests/test_sample_host.py checks the choice on the CPU); the bit-exact tests run on the wide Trie in every mode."""
import numpy as np
import pytest
import torch

from gram_amd.utils import generation_trie as gt
from oracle import gram_oracle as O
from tests import sample_oracle as S
from tests.test_gpu_path import DEV, _model
from tests.test_gpu_teacher_forced import _modes, _tol

pytestmark = pytest.mark.gpu
B, R, T = S.B, S.R, S.MAX_LENGTH


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
    fns = {id(c[k]): gt.prefix_allowed_tokens_fn(gt.Trie(c[k])) for k in ("cands", "cands_thin")}
    return dict(c, m=m, fns=fns)


def _sample(w, cands=None, ids=None, mask=None, uniforms=None, r=R, fn=None, **kw):
    cands = w["cands"] if cands is None else cands
    fn = fn or w["fns"].get(id(cands)) or gt.prefix_allowed_tokens_fn(gt.Trie(cands))
    ids = w["ids"] if ids is None else ids
    mask = w["mask"] if mask is None else mask
    args = dict(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), max_length=T, prefix_allowed_tokens_fn=fn, do_sample=True,
                num_beams=1, num_return_sequences=r, uniforms=uniforms)
    args.update(kw)
    out = w["m"].generate(**args)
    assert out["sequences_scores"] is None
    return out, fn


def _pad(seqs):
    seqs = seqs.cpu()
    return torch.nn.functional.pad(seqs, (0, T - seqs.shape[1]))


def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    return (torch.equal(_pad(a["sequences"])[rows_a], _pad(b["sequences"])[rows_b])
            and torch.equal(a["sequence_logprobs"].cpu()[rows_a], b["sequence_logprobs"].cpu()[rows_b])
            and torch.equal(a["sample_logprobs"].cpu()[rows_a], b["sample_logprobs"].cpu()[rows_b]))


def _mode_delta(mode, tau=1.0):
    return 4 * _tol(mode)["logit"] / tau


@pytest.mark.parametrize("tau,top_k,top_p", [(1.0, 50, 1.0), (2.0, 3, 0.9)])
def test_constructed_trajectories(world, tau, top_k, top_p):
    """The oracle walks every (user, sample) along children a seeded RNG picks among those with a CDF interval wider than 4 delta and
    emits the midpoints as uniforms: the device returns exactly these sequences, with both log-probabilities within TOL's logp."""
    w = world
    for mode in _modes():
        w["m"].set_precision(mode)
        cands = S.case_candidates(w, mode)
        delta = _mode_delta(mode, tau)
        ref = S.walk(w["sd"], w["oc"], w["ids"], w["mask"], [O.Trie(cands)] * B, R, T, tau, top_k, top_p, delta=delta,
                     rng=np.random.default_rng(S.SEED))
        out, _ = _sample(w, cands, uniforms=ref["uniforms"], temperature=tau, top_k=top_k, top_p=top_p)
        assert torch.equal(_pad(out["sequences"]), ref["seq"]), (mode, _pad(out["sequences"]), ref["seq"])
        width = 1 + max(len([t for t in row if t]) for row in ref["seq"][:, 1:].tolist())
        assert out["sequences"].shape[1] == min(width, T)
        dm = float((out["sequence_logprobs"].cpu().double() - torch.from_numpy(ref["model_lp"])).abs().max())
        ds = float((out["sample_logprobs"].cpu().double() - torch.from_numpy(ref["sample_lp"])).abs().max())
        print(f"[{mode}] tau={tau} top_k={top_k} top_p={top_p}: model logp {dm:.2e}, sample logp {ds:.2e}; "
              f"{len({tuple(r) for r in ref['seq'].tolist()})} distinct sequences")
        tol = _tol(mode)["logp"]
        assert dm < tol and ds < tol


def test_random_uniforms_capped(world):
    """torch.rand uniforms with a fixed seed; the oracle is teacher-forced along the device's own sequences.  Every step whose u is
    further than delta from every boundary of the oracle's CDF must be the oracle's pick; at most 10 % of the steps may be skipped."""
    w = world
    for mode in _modes():
        w["m"].set_precision(mode)
        cands = S.case_candidates(w, mode)
        out, _ = _sample(w, cands, uniforms=w["uniforms"])
        seqs = _pad(out["sequences"])
        res = S.walk(w["sd"], w["oc"], w["ids"], w["mask"], [O.Trie(cands)] * B, R, T, 1.0, 50, 1.0, uniforms=w["uniforms"], forced=seqs)
        delta = _mode_delta(mode)
        live = res["want"] >= 0
        decided = live & (res["margin"] > delta)
        got = seqs[:, 1:].numpy()
        share = 1.0 - decided.sum() / live.sum()
        print(f"[{mode}] {int(live.sum())} steps, {int((live & ~decided).sum())} skipped ({share:.3f}), "
              f"{int((got != res['want'])[decided].sum())} wrong")
        assert np.array_equal(got[decided], res["want"][decided]), (mode, np.argwhere(decided & (got != res["want"])))
        assert share <= 0.10
        dm = float((out["sequence_logprobs"].cpu().double() - torch.from_numpy(res["model_lp"])).abs().max())
        assert dm < _tol(mode)["logp"]


def test_sequence_logprobs_are_score_sequences(world):
    """sequence_logprobs is what score_sequences returns for the returned rows, and every row is a candidate"""
    w = world
    for mode in _modes():
        w["m"].set_precision(mode)
        out, fn = _sample(w, uniforms=w["uniforms"])
        items = w["m"].sequence_items(out["sequences"], fn, w["cands"]).cpu()
        assert bool((items >= 0).all())
        lab = _pad(out["sequences"])[:, 1:].clone()
        after = (lab == 1).cumsum(-1) - (lab == 1).long()  # positions behind the EOS
        lab = lab.masked_fill(after > 0, -100).view(B, R, T - 1)
        sc = w["m"].score_sequences(w["ids"].to(DEV), w["mask"].to(DEV), lab.to(DEV)).cpu().view(-1)
        d = float((sc.double() - out["sequence_logprobs"].cpu().double()).abs().max())
        print(f"[{mode}] |sequence_logprobs - score_sequences| {d:.2e}")
        assert d < _tol(mode)["logp"]
        assert bool((out["sample_logprobs"].cpu() <= 0).all()) and bool((out["sequence_logprobs"].cpu() < 0).all())


def test_bit_exact_invariance(world):
    """A row's draw depends on its user, its uniforms and the parameters only: user b alone, sample r alone at R = 1, the batch
    padded to a longer L, the passage cache on and off"""
    w = world
    m = w["m"]
    for mode in _modes():
        m.set_precision(mode)
        kw = dict(temperature=1.5, top_k=3, top_p=0.95)
        full, _ = _sample(w, uniforms=w["uniforms"], **kw)
        assert len({tuple(r) for r in _pad(full["sequences"]).tolist()}) > B  # (the samples of a user differ)
        for b in range(B):
            one, _ = _sample(w, ids=w["ids"][b:b + 1], mask=w["mask"][b:b + 1], uniforms=w["uniforms"][b:b + 1], **kw)
            assert _same(one, full, rows_b=slice(b * R, (b + 1) * R)), (mode, "user alone", b)
        for b, r in ((0, 0), (1, 5), (2, 7)):
            one, _ = _sample(w, ids=w["ids"][b:b + 1], mask=w["mask"][b:b + 1], uniforms=w["uniforms"][b:b + 1, r:r + 1], r=1, **kw)
            assert _same(one, full, rows_b=slice(b * R + r, b * R + r + 1)), (mode, "sample alone", b, r)
        ids64 = torch.nn.functional.pad(w["ids"], (0, 32))
        mask64 = torch.nn.functional.pad(w["mask"], (0, 32))
        longer, _ = _sample(w, ids=ids64, mask=mask64, uniforms=w["uniforms"], **kw)
        assert _same(longer, full), (mode, "padded to L = 64")
        try:
            m.cache_passages(w["ids"].to(DEV), w["mask"].to(DEV))
            cached, _ = _sample(w, uniforms=w["uniforms"], **kw)
        finally:
            m.clear_passage_cache()
        assert _same(cached, full), (mode, "passage cache")


def test_item_filters_equal_per_user_tries(world):
    """exclude_items / allowed_items: bit for bit what the user gets alone with Trie(A_b); no excluded item is ever returned"""
    w = world
    m, cands = w["m"], w["cands"]
    n = len(cands)
    g = torch.Generator().manual_seed(S.SEED + 3)
    first = cands[0][1]
    lists = [[i for i, c in enumerate(cands) if c[1] == first],  # an inner node dies
             torch.randperm(n, generator=g)[:15].tolist(),
             [i for i in range(n) if i not in (3, 17)]]             # two items left
    keep = [sorted(set(range(n)) - set(r)) for r in lists]
    for mode in _modes():
        m.set_precision(mode)
        for kind, kw in (("exclude", dict(exclude_items=lists)), ("allow", dict(allowed_items=keep))):
            out, fn = _sample(w, uniforms=w["uniforms"], candidates=cands, **kw)
            items = m.sequence_items(out["sequences"], fn, cands).cpu().view(B, R)
            for b in range(B):
                assert set(items[b].tolist()) <= set(keep[b]), (mode, kind, b, items[b])
                alone, _ = _sample(w, [cands[i] for i in keep[b]], ids=w["ids"][b:b + 1], mask=w["mask"][b:b + 1],
                                   uniforms=w["uniforms"][b:b + 1])
                assert _same(alone, out, rows_b=slice(b * R, (b + 1) * R)), (mode, kind, b)


def test_top_k_one_and_tiny_top_p_are_the_mode(world):
    """top_k = 1 returns one sequence per user whatever the uniforms; top_p = 1e-6 returns the same sequence"""
    w = world
    w["m"].set_precision(_modes()[0])
    other = torch.rand(B, R, T - 1, generator=torch.Generator().manual_seed(99))
    a, _ = _sample(w, uniforms=w["uniforms"], top_k=1)
    b, _ = _sample(w, uniforms=other, top_k=1)
    c, _ = _sample(w, uniforms=other, top_k=0, top_p=1e-6)
    sa = _pad(a["sequences"]).view(B, R, T)
    assert bool((sa == sa[:, :1]).all())
    assert _same(a, b) and torch.equal(_pad(a["sequences"]), _pad(c["sequences"]))
    assert bool((a["sample_logprobs"].cpu() == 0).all())  # (one kept child per step: log 1)


def test_seeded_generator(world):
    w = world
    w["m"].set_precision(_modes()[0])

    def run(seed, dev):
        out, _ = _sample(w, generator=torch.Generator(device=dev).manual_seed(seed))
        return out
    for dev in ("cpu", DEV):
        a, b, c = run(5, dev), run(5, dev), run(6, dev)
        assert _same(a, b) and not torch.equal(_pad(a["sequences"]), _pad(c["sequences"])), dev
    plain, _ = _sample(w)  # (no generator: torch's global one)
    assert plain["sequences"].shape[0] == B * R and plain["sequence_logprobs"].shape == (B * R,)
