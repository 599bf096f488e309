"""-m gpu: per-user item masks of GRAM.generate (item_mask=): every user searches its own view of the one shared device Trie, its
set of ANY size given as a row of a (B, len(candidates)) tensor.

The definition is tests/test_gpu_user_items.py's: user b with kept candidates A_b gets exactly what ``generate`` returns for that
user ALONE with ``prefix_allowed_tokens_fn(Trie(A_b))`` and the same ``max_length``, -inf fillers included.  The reference is the
unmodified fast path on one-user batches with per-user Tries, and every equality is ``torch.equal`` on sequences and scores: the
path is batch-invariant bit for bit, and a dead candidate only removes a key from a selection whose keys are unique and totally
ordered."""
import pytest
import torch

from tests.test_gpu_path import DEV, _inputs, _model, _random_items
from tests.test_gpu_user_items import _gen, _pad, _per_user_reference

pytestmark = pytest.mark.gpu

B, N, L, K = 6, 2, 32, 5
N_ITEMS = 60


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gram_amd
    return gram_amd


def _mask(keep, n):
    m = torch.zeros(len(keep), n, dtype=torch.bool)
    for b, kp in enumerate(keep):
        m[b, sorted(kp)] = True
    return m


@pytest.fixture(scope="module")
def world(gpu):
    """Model, inputs, 60 candidates, the unfiltered result, the six users' sets and their per-user reference: computed once"""
    oc, sd, m = _model(gpu, "tiny", 11)
    g = torch.Generator().manual_seed(2025)
    ids, mask = _inputs(g, B, N, L, min(oc.vocab_size, 32100))
    cands = _random_items(g, N_ITEMS, 2, 4, 40)
    n = len(cands)
    max_length = max(len(c) for c in cands)
    plain, fn = _gen(m, ids, mask, max_length, cands)
    plain_items = m.sequence_items(plain["sequences"], fn, cands).cpu().view(B, K)
    assert bool((plain_items >= 0).all())
    first = cands[int(plain_items[4][0])][1]  # the first token of user 4's best item: user 4 loses it, user 3 keeps nothing else
    under = {i for i, c in enumerate(cands) if c[1] == first}
    assert 0 < len(under) < n
    keep = [
        set(range(n)),                                           # 0: all items
        {int(plain_items[1][1])},                                # 1: one item
        set(torch.randperm(n, generator=g)[: n // 2].tolist()) - {int(plain_items[2][0])},  # 2: a random half, without its best item
        under,                                                   # 3: exactly the items under one first token
        set(range(n)) - under,                                   # 4: the complement of that: an inner node dies
        {4, 17, 33},                                             # 5: three items, fewer than K
    ]
    ref_seqs, ref_scores = _per_user_reference(m, ids, mask, max_length, cands, keep)
    return dict(oc=oc, sd=sd, m=m, ids=ids, mask=mask, cands=cands, max_length=max_length, plain=plain, plain_items=plain_items, fn=fn,
                keep=keep, ref_seqs=ref_seqs, ref_scores=ref_scores)


def _masked(w, item_mask=None, k=K, **kw):
    item_mask = _mask(w["keep"], len(w["cands"])) if item_mask is None else item_mask
    out, _ = _gen(w["m"], w["ids"], w["mask"], w["max_length"], w["cands"], k, fn=w["fn"], item_mask=item_mask, candidates=w["cands"], **kw)
    return out


def _assert_equals_reference(w, out, tag):
    seqs, scores = _pad(out["sequences"], w["max_length"]), out["sequences_scores"].cpu()
    for b in range(B):
        rows = slice(b * K, (b + 1) * K)
        assert torch.equal(seqs[rows], w["ref_seqs"][rows]), (tag, "sequences of user", b, seqs[rows], w["ref_seqs"][rows])
        assert torch.equal(scores[rows], w["ref_scores"][rows]), (tag, "scores of user", b, scores[rows], w["ref_scores"][rows])


def test_item_mask_changes_the_result(world):
    """The call with item_mask returns other rows than the call without it for the users that lose items of their unfiltered result
    (without the feature the keyword is ignored with a warning and the rows are the same), and the rows of the user that keeps all"""
    import warnings
    w = world
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (no "ignores the keyword argument 'item_mask'")
        out = _masked(w)
    seqs, scores = _pad(out["sequences"], w["max_length"]), out["sequences_scores"].cpu()
    pseqs, pscores = _pad(w["plain"]["sequences"], w["max_length"]), w["plain"]["sequences_scores"].cpu()
    assert torch.equal(seqs[:K], pseqs[:K]) and torch.equal(scores[:K], pscores[:K])
    for b in range(1, B):
        assert set(w["plain_items"][b].tolist()) - w["keep"][b], f"user {b}'s set holds its unfiltered top-{K}: the test is vacuous"
        assert not torch.equal(seqs[b * K:(b + 1) * K], pseqs[b * K:(b + 1) * K]), b


def test_six_users_equal_per_user_tries_and_both_list_forms(world):
    w = world
    n = len(w["cands"])
    out = _masked(w)  # (a non-finite candidate or an impossible beam state raises here: GRAM_E_NONFINITE / GRAM_E_BEAM)
    _assert_equals_reference(w, out, "item_mask")
    allowed, _ = _gen(w["m"], w["ids"], w["mask"], w["max_length"], w["cands"], fn=w["fn"], allowed_items=[sorted(k) for k in w["keep"]],
                      candidates=w["cands"])
    excluded, _ = _gen(w["m"], w["ids"], w["mask"], w["max_length"], w["cands"], fn=w["fn"],
                       exclude_items=[sorted(set(range(n)) - k) for k in w["keep"]], candidates=w["cands"])
    for other in (allowed, excluded):
        assert torch.equal(out["sequences"], other["sequences"]) and torch.equal(out["sequences_scores"], other["sequences_scores"])
    # every returned item lies in its user's set; user 5 keeps 3 items < K: they come first
    items = w["m"].sequence_items(out["sequences"], w["fn"], w["cands"]).cpu().view(B, K)
    for b in range(B):
        got = [i for i in items[b].tolist() if i >= 0]
        assert got and set(got) <= w["keep"][b], (b, got)
    assert sorted(items[5].tolist()[:3]) == sorted(w["keep"][5]) and items[1, 0] == next(iter(w["keep"][1]))


@pytest.mark.parametrize("variant", ["chunked_cap7", "live_rows_off"])
def test_chunked_and_without_live_rows(world, variant):
    """The chunked search step (7 fresh candidates per round) and the step without the live-row compaction: the default path's bits"""
    from gram_amd import _lib
    lib = _lib.load()
    try:
        if variant == "chunked_cap7":
            assert lib.gram_debug_set_beam_chunked(1) == 0 and lib.gram_debug_set_beam_chunk_capacity(7) == 0
        else:
            assert lib.gram_debug_set_live_rows(0) == 0
        out = _masked(world)
    finally:
        lib.gram_debug_set_beam_chunked(-1)
        lib.gram_debug_set_beam_chunk_capacity(0)
        lib.gram_debug_set_live_rows(-1)
    _assert_equals_reference(world, out, variant)


def test_one_piece_precision(gpu, world):
    """The one-piece arithmetic against per-user Tries in the same mode"""
    from gram_amd import _lib
    w = world
    _, _, m = _model(gpu, "tiny", 11)
    m.set_precision("f16" if _lib.piece_dtype() == torch.float16 else "bf16")
    out, _ = _gen(m, w["ids"], w["mask"], w["max_length"], w["cands"], item_mask=_mask(w["keep"], len(w["cands"])), candidates=w["cands"])
    ref_seqs, ref_scores = _per_user_reference(m, w["ids"], w["mask"], w["max_length"], w["cands"], w["keep"])
    assert torch.equal(_pad(out["sequences"], w["max_length"]), ref_seqs)
    assert torch.equal(out["sequences_scores"].cpu(), ref_scores)
    assert not torch.equal(ref_scores, w["ref_scores"])  # (it is another arithmetic)


def test_greedy(world):
    w = world
    out = _masked(w, k=1)
    assert out["sequences_scores"] is None
    ref_seqs, _ = _per_user_reference(w["m"], w["ids"], w["mask"], w["max_length"], w["cands"], w["keep"], k=1)
    assert torch.equal(_pad(out["sequences"], w["max_length"]), ref_seqs)
    plain, _ = _gen(w["m"], w["ids"], w["mask"], w["max_length"], w["cands"], 1, fn=w["fn"])
    assert not torch.equal(_pad(plain["sequences"], w["max_length"]), ref_seqs)


def test_mask_dtypes_devices_and_strides(world):
    """bool on the CPU (the default of these tests), uint8 on the device, int64 with other non-zero values, and a non-contiguous
    view (a transposed tensor; every other column of a wider one): the same results"""
    w = world
    m = _mask(w["keep"], len(w["cands"]))
    want = _masked(w, m)
    wide = torch.zeros(B, 2 * m.shape[1], dtype=torch.int32)
    wide[:, ::2] = m.to(torch.int32) * -3
    for other in (m.to(torch.uint8).to(DEV), m.to(torch.int64) * 1000, m.t().contiguous().t(), wide[:, ::2].to(DEV)):
        assert other.shape == m.shape
        got = _masked(w, other)
        assert torch.equal(got["sequences"], want["sequences"]) and torch.equal(got["sequences_scores"], want["sequences_scores"])
    assert not m.t().contiguous().t().is_contiguous() and not wide[:, ::2].is_contiguous()


def test_duplicate_candidate_kept_by_its_second_spelling(gpu, world):
    """A candidate list with a duplicated sequence where the mask keeps only the second spelling: the item is reachable, and the
    result is the one of the de-duplicated set"""
    w = world
    cands = w["cands"] + [list(w["cands"][7])]  # candidate 60 spells candidate 7 again
    n = len(cands)
    keep = [{60, 3}, {7, 3}, {60}, {5, 60, 9}, {3, 9}, {60, 7}]
    out, fn = _gen(w["m"], w["ids"], w["mask"], w["max_length"], cands, item_mask=_mask(keep, n), candidates=cands)
    dedup = [{7 if i == 60 else i for i in kp} for kp in keep]
    ref_seqs, ref_scores = _per_user_reference(w["m"], w["ids"], w["mask"], w["max_length"], w["cands"], dedup)
    assert torch.equal(_pad(out["sequences"], w["max_length"]), ref_seqs) and torch.equal(out["sequences_scores"].cpu(), ref_scores)
    seven = list(w["cands"][7])
    for b in (0, 2, 3, 5):  # the sequence of candidates 7 / 60 is among the rows of the users that kept only spelling 60
        rows = _pad(out["sequences"], w["max_length"])[b * K:(b + 1) * K].tolist()
        assert any(r[: len(seven)] == seven and not any(r[len(seven):]) for r in rows), b
    assert not any(r[: len(seven)] == seven and not any(r[len(seven):])
                   for r in _pad(out["sequences"], w["max_length"])[4 * K:5 * K].tolist())


def test_empty_row_is_a_value_error_naming_the_user(world):
    w = world
    m = _mask(w["keep"], len(w["cands"]))
    m[4] = False
    with pytest.raises(ValueError, match="item_mask leaves user 4 without any item"):
        _masked(w, m)
    m[2] = False
    with pytest.raises(ValueError, match="item_mask leaves user 2 without any item"):
        _masked(w, m.to(torch.uint8).to(DEV))


def test_sets_that_no_list_can_say(gpu):
    """About 9 000 items, two users; each keeps a random half of the catalogue from which its own unfiltered top-3 have been
    removed: more than 4096 kept AND more than 4096 dropped, so neither allowed_items nor exclude_items could express the set.  The
    result differs from the unfiltered one and equals the per-user-Trie reference."""
    from gram_amd import _lib
    oc, sd, m = _model(gpu, "tiny", 11)
    g = torch.Generator().manual_seed(9)
    b_ = 2
    ids, mask = _inputs(g, b_, N, L, min(oc.vocab_size, 32100))
    cands = _random_items(g, 9000, 3, 4, 40)
    n = len(cands)
    max_length = max(len(c) for c in cands)
    plain, fn = _gen(m, ids, mask, max_length, cands)
    top = m.sequence_items(plain["sequences"], fn, cands).cpu().view(b_, K)
    keep = []
    for b in range(b_):
        half = set(torch.randperm(n, generator=g)[: n // 2].tolist()) - set(top[b][:3].tolist())
        assert len(half) > _lib.GRAM_MAX_USER_ITEMS and n - len(half) > _lib.GRAM_MAX_USER_ITEMS
        keep.append(half)
    for form, sets in (("allowed_items", keep), ("exclude_items", [set(range(n)) - k for k in keep])):
        with pytest.raises(ValueError, match="at most 4096"):  # (what the issue is about)
            _gen(m, ids, mask, max_length, cands, fn=fn, candidates=cands, **{form: [sorted(s) for s in sets]})
    out, _ = _gen(m, ids, mask, max_length, cands, fn=fn, item_mask=_mask(keep, n), candidates=cands)
    seqs = _pad(out["sequences"], max_length)
    pseqs = _pad(plain["sequences"], max_length)
    for b in range(b_):
        assert not torch.equal(seqs[b * K:(b + 1) * K], pseqs[b * K:(b + 1) * K]), b
    ref_seqs, ref_scores = _per_user_reference(m, ids, mask, max_length, cands, keep)
    assert torch.equal(seqs, ref_seqs)
    assert torch.equal(out["sequences_scores"].cpu(), ref_scores)
    items = m.sequence_items(out["sequences"], fn, cands).cpu().view(b_, K)
    for b in range(b_):
        assert set(items[b].tolist()) <= keep[b]
