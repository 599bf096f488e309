"""-m gpu: per-user item filters of GRAM.generate (exclude_items / allowed_items): every user searches its own view of the one shared
device Trie.

The definition every test rests on: user b with remaining candidates A_b gets exactly what ``generate`` returns for that user ALONE
with ``prefix_allowed_tokens_fn(Trie(A_b))`` and the same ``max_length`` -- HF 4.26 PrefixConstrainedLogitsProcessor semantics,
-inf fillers included.  The reference of the bit-exactness tests is therefore the unmodified fast path on one-user batches with
per-user Tries, and equality is ``torch.equal`` on sequences and scores: the path is batch-invariant bit for bit, and a dead
candidate only removes a key from a selection whose keys are unique and totally ordered.  One test goes to the CPU oracle instead
(``O.generate`` with a per-user callback) at the project's tolerance for generate against the oracle."""
import pytest
import torch

from oracle import gram_oracle as O
from tests.test_gpu_path import DEV, SCORE_TOL, _check_generate, _inputs, _model, _random_items

pytestmark = pytest.mark.gpu

B, N, L, K = 6, 2, 32, 5
N_ITEMS = 60


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gram_amd
    return gram_amd


def _gen(m, ids, mask, max_length, cands, k=K, **kw):
    from gram_amd.utils import generation_trie as gt
    fn = kw.pop("fn", None) or gt.prefix_allowed_tokens_fn(gt.Trie(cands))
    out = m.generate(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), max_length=max_length, prefix_allowed_tokens_fn=fn,
                     num_beams=k, num_return_sequences=k, output_scores=True, return_dict_in_generate=True, length_penalty=1.0, **kw)
    return out, fn


def _pad(seqs, width):
    seqs = seqs.cpu()
    assert seqs.shape[1] <= width
    return torch.nn.functional.pad(seqs, (0, width - seqs.shape[1]))


def _per_user_reference(m, ids, mask, max_length, cands, keep_sets, k=K):
    """One one-user generate per user on the unmodified fast path with Trie(A_b); sequences padded to max_length, scores or None"""
    seqs, scores = [], []
    for b, keep in enumerate(keep_sets):
        sub = [cands[i] for i in sorted(keep)]
        out, _ = _gen(m, ids[b:b + 1], mask[b:b + 1], max_length, sub, k)
        seqs.append(_pad(out["sequences"], max_length))
        if k > 1:
            scores.append(out["sequences_scores"].cpu())
    return torch.cat(seqs), (torch.cat(scores) if k > 1 else None)


def _tensor(lists):
    """B lists -> the (B, M) tensor form, padded with -1"""
    t = torch.full((len(lists), max(1, max(map(len, lists)))), -1, dtype=torch.int64)
    for b, r in enumerate(lists):
        t[b, : len(r)] = torch.tensor(r, dtype=torch.int64)
    return t


def _exclude_lists(cands, top_items, g):
    """The six users of the exclude-mode test, from each user's unfiltered top-K item indices"""
    n = len(cands)
    first = cands[top_items[2][0]][1]  # user 2: every item under the first token of its best item -- an inner node dies
    keep3 = {4, 17, 33}
    return [
        [],                                                                   # 0: all padding
        list(top_items[1][:3]),                                               # 1: the top 3 of its own unfiltered result
        [i for i, c in enumerate(cands) if c[1] == first],                    # 2
        [i for i in range(n) if i not in keep3],                              # 3: fewer than K left
        [top_items[4][0], -1, top_items[4][0], 9, -1, 9, -1, top_items[4][1]],  # 4: duplicates interleaved with padding
        torch.randperm(n, generator=g)[:20].tolist(),                         # 5: 20 random items
    ]


@pytest.fixture(scope="module")
def world(gpu):
    """Model, inputs, candidates, the unfiltered result, the exclude lists and their per-user reference: computed once"""
    oc, sd, m = _model(gpu, "tiny", 11)
    g = torch.Generator().manual_seed(2024)
    ids, mask = _inputs(g, B, N, L, min(oc.vocab_size, 32100))
    cands = _random_items(g, N_ITEMS, 2, 4, 40)
    max_length = max(len(c) for c in cands)
    plain, fn = _gen(m, ids, mask, max_length, cands)
    plain_items = m.sequence_items(plain["sequences"], fn, cands).cpu().view(B, K)
    assert bool((plain_items >= 0).all())
    lists = _exclude_lists(cands, plain_items.tolist(), g)
    keep = [set(range(len(cands))) - {i for i in r if i >= 0} for r in lists]
    ref_seqs, ref_scores = _per_user_reference(m, ids, mask, max_length, cands, keep)
    return dict(oc=oc, sd=sd, m=m, ids=ids, mask=mask, cands=cands, max_length=max_length, plain=plain, plain_items=plain_items, fn=fn,
                lists=lists, keep=keep, ref_seqs=ref_seqs, ref_scores=ref_scores)


def _assert_equals_reference(w, out, tag):
    seqs, scores = _pad(out["sequences"], w["max_length"]), out["sequences_scores"].cpu()
    for b in range(B):
        rows = slice(b * K, (b + 1) * K)
        assert torch.equal(seqs[rows], w["ref_seqs"][rows]), (tag, "sequences of user", b, seqs[rows], w["ref_seqs"][rows])
        assert torch.equal(scores[rows], w["ref_scores"][rows]), (tag, "scores of user", b, scores[rows], w["ref_scores"][rows])


def _exclude(w):
    out, _ = _gen(w["m"], w["ids"], w["mask"], w["max_length"], w["cands"], fn=w["fn"], exclude_items=_tensor(w["lists"]),
                  candidates=w["cands"])
    return out


def test_exclude_mode_equals_per_user_tries(world):
    w = world
    out = _exclude(w)  # (a non-finite candidate or an impossible beam state raises here: GRAM_E_NONFINITE / GRAM_E_BEAM)
    _assert_equals_reference(w, out, "exclude")
    seqs, scores = _pad(out["sequences"], w["max_length"]), out["sequences_scores"].cpu()
    pseqs, pscores = _pad(w["plain"]["sequences"], w["max_length"]), w["plain"]["sequences_scores"].cpu()
    # user 0 excludes nothing: its unfiltered rows; users 1, 2, 3 and 5 lose items of their unfiltered top-K: different rows
    assert torch.equal(seqs[:K], pseqs[:K]) and torch.equal(scores[:K], pscores[:K])
    for b in (1, 2, 3, 5):
        assert set(w["plain_items"][b].tolist()) - w["keep"][b], f"user {b}'s list misses its unfiltered top-{K}: the test is vacuous"
        assert not torch.equal(seqs[b * K:(b + 1) * K], pseqs[b * K:(b + 1) * K]), b
    # what comes back is never excluded, and sequence_items works on the result unchanged
    items = w["m"].sequence_items(out["sequences"], w["fn"], w["cands"]).cpu().view(B, K)
    for b in range(B):
        got = [i for i in items[b].tolist() if i >= 0]
        assert set(got) <= w["keep"][b], (b, got)
    # user 3 keeps 3 items < K: they come first with ordinary scores.  Its other rows hold no further item: what HF 4.26 returns for
    # Trie(A_3) there (the reference above) is either a -inf filler beam -- no candidate: sequence_items gives -1 -- or a copy of a
    # kept item from one of the beams that HF starts at -1e9 (beam_scores[1:] = -1e9), whose score stays below -1e8
    assert sorted(items[3].tolist()[:3]) == sorted(w["keep"][3])
    assert bool((scores[3 * K:3 * K + 3] > -100).all())
    for i, sc in zip(items[3].tolist()[3:], scores[3 * K + 3:4 * K].tolist()):
        assert (i == -1 and sc == float("-inf")) or (i in w["keep"][3] and sc < -1e8), (i, sc)


def test_allow_mode(world):
    w = world
    allowed = [sorted(k) for k in w["keep"]]  # the complements of the exclude lists, as Python lists
    out, _ = _gen(w["m"], w["ids"], w["mask"], w["max_length"], w["cands"], fn=w["fn"], allowed_items=allowed, candidates=w["cands"])
    _assert_equals_reference(w, out, "allow")
    # a user allowing every item: its unfiltered rows; a user allowing one item: that item first
    every = list(range(len(w["cands"])))
    one = 23
    out, _ = _gen(w["m"], w["ids"], w["mask"], w["max_length"], w["cands"], fn=w["fn"],
                  allowed_items=[every, [one], every, [one, one, -1], every, every], candidates=w["cands"])
    seqs, scores = _pad(out["sequences"], w["max_length"]), out["sequences_scores"].cpu()
    pseqs, pscores = _pad(w["plain"]["sequences"], w["max_length"]), w["plain"]["sequences_scores"].cpu()
    for b in (0, 2, 4, 5):
        assert torch.equal(seqs[b * K:(b + 1) * K], pseqs[b * K:(b + 1) * K]) and torch.equal(scores[b * K:(b + 1) * K], pscores[b * K:(b + 1) * K])
    items = w["m"].sequence_items(out["sequences"], w["fn"], w["cands"]).cpu().view(B, K)
    for b in (1, 3):
        assert items[b, 0] == one and set(items[b].tolist()) <= {one, -1}, items[b]
        assert seqs[b * K].tolist()[: len(w["cands"][one])] == w["cands"][one]


@pytest.mark.parametrize("variant", ["chunked_cap7", "live_rows_off"])
def test_exclude_mode_chunked_and_without_live_rows(world, variant):
    """The chunked search step (7 fresh candidates per round: chunk boundaries inside every user's list) and the step without the
    live-row compaction return the bits of the default path."""
    from gram_amd import _lib
    lib = _lib.load()
    try:
        if variant == "chunked_cap7":
            assert lib.gram_debug_set_beam_chunked(1) == 0 and lib.gram_debug_set_beam_chunk_capacity(7) == 0
        else:
            assert lib.gram_debug_set_live_rows(0) == 0
        out = _exclude(world)
    finally:
        lib.gram_debug_set_beam_chunked(-1)
        lib.gram_debug_set_beam_chunk_capacity(0)
        lib.gram_debug_set_live_rows(-1)
    _assert_equals_reference(world, out, variant)


def test_exclude_mode_one_piece(gpu, world):
    """The one-piece arithmetic (gram_beam_step_sparse_items) against per-user Tries in the same mode"""
    from gram_amd import _lib
    w = world
    _, _, m = _model(gpu, "tiny", 11)
    m.set_precision("f16" if _lib.piece_dtype() == torch.float16 else "bf16")
    out, _ = _gen(m, w["ids"], w["mask"], w["max_length"], w["cands"], exclude_items=_tensor(w["lists"]), candidates=w["cands"])
    ref_seqs, ref_scores = _per_user_reference(m, w["ids"], w["mask"], w["max_length"], w["cands"], w["keep"])
    assert torch.equal(_pad(out["sequences"], w["max_length"]), ref_seqs)
    assert torch.equal(out["sequences_scores"].cpu(), ref_scores)
    assert not torch.equal(ref_scores, w["ref_scores"])  # (it is another arithmetic)


def test_greedy_with_exclude_lists(world):
    w = world
    out, _ = _gen(w["m"], w["ids"], w["mask"], w["max_length"], w["cands"], 1, fn=w["fn"], exclude_items=_tensor(w["lists"]),
                  candidates=w["cands"])
    assert out["sequences_scores"] is None
    ref_seqs, _ = _per_user_reference(w["m"], w["ids"], w["mask"], w["max_length"], w["cands"], w["keep"], k=1)
    assert torch.equal(_pad(out["sequences"], w["max_length"]), ref_seqs)
    plain, _ = _gen(w["m"], w["ids"], w["mask"], w["max_length"], w["cands"], 1, fn=w["fn"])
    assert not torch.equal(_pad(plain["sequences"], w["max_length"]), ref_seqs)  # (users 1 and 2 exclude their best item)


def test_exclude_mode_vs_oracle(gpu):
    """O.generate on the CPU with a per-user callback over O.Trie(A_b), at the tolerance of generate against the oracle"""
    oc, sd, m = _model(gpu, "tiny", 11)
    g = torch.Generator().manual_seed(7)
    b_, k_ = 3, 4
    ids, mask = _inputs(g, b_, N, L, min(oc.vocab_size, 32100))
    cands = _random_items(g, N_ITEMS, 2, 4, 40)
    max_length = max(len(c) for c in cands)
    lists = [torch.randperm(N_ITEMS, generator=g)[:n].tolist() for n in (20, 40, N_ITEMS - 2 * k_)]  # every user keeps >= K items
    keep = [sorted(set(range(N_ITEMS)) - set(r)) for r in lists]
    fns = [O.prefix_allowed_tokens_fn(O.Trie([cands[i] for i in kp])) for kp in keep]
    ref = O.generate(sd, oc, ids, mask, max_length, lambda b, sent: fns[b](b, sent), k_, k_, 1.0)
    out, fn = _gen(m, ids, mask, max_length, cands, k_, exclude_items=lists, candidates=cands)
    assert out["sequences"].shape[1] == ref["sequences"].shape[1]
    _check_generate(oc, sd, out, ref, ids, mask, cands, k_, tol=SCORE_TOL)
    items = m.sequence_items(out["sequences"], fn, cands).cpu().view(b_, k_)
    for b in range(b_):
        assert set(items[b].tolist()) <= set(keep[b])


def test_wide_step0_mixes_dead_and_alive_children(gpu):
    """100 first tokens under the start token (> 64: several wavefronts of step 0's shared-row keys), dead and alive ones mixed"""
    oc, sd, m = _model(gpu, "tiny", 11)
    g = torch.Generator().manual_seed(31)
    b_ = 3
    ids, mask = _inputs(g, b_, N, L, min(oc.vocab_size, 32100))
    cands = [[0, a, c, 1] for a in range(2, 102) for c in (110 + a % 7, 120 + a % 5)]
    n = len(cands)
    plain, fn = _gen(m, ids, mask, 4, cands)
    top = m.sequence_items(plain["sequences"], fn, cands).cpu().view(b_, K).tolist()
    lists = [
        [i for i in range(n) if cands[i][1] % 2 == 0] + top[0][:1],               # every other first token dies, and the best item
        sorted(set(torch.randperm(n, generator=g)[:120].tolist()) | set(top[1][:2])),  # random: some first tokens die, some lose one leaf
        [i for i in range(n) if cands[i][1] > 8 and i not in top[2][2:]],          # a handful of first tokens left
    ]
    keep = [set(range(n)) - set(r) for r in lists]
    assert all(len(k) >= 1 for k in keep)
    out, _ = _gen(m, ids, mask, 4, cands, fn=fn, exclude_items=lists, candidates=cands)
    ref_seqs, ref_scores = _per_user_reference(m, ids, mask, 4, cands, keep)
    assert torch.equal(_pad(out["sequences"], 4), ref_seqs)
    assert torch.equal(out["sequences_scores"].cpu(), ref_scores)
    assert not torch.equal(_pad(out["sequences"], 4), _pad(plain["sequences"], 4))


def test_value_errors(world):
    from gram_amd import _lib
    w = world
    n = len(w["cands"])

    def call(**kw):
        fn = kw.pop("fn", w["fn"])
        return _gen(w["m"], w["ids"], w["mask"], w["max_length"], w["cands"], fn=fn, **kw)

    some = [[1]] * B
    with pytest.raises(ValueError, match="mutually exclusive"):
        call(exclude_items=some, allowed_items=some, candidates=w["cands"])
    with pytest.raises(ValueError, match="candidates"):
        call(exclude_items=some)
    for bad in (n, -2):
        with pytest.raises(ValueError, match="outside"):
            call(exclude_items=[[bad]] + [[1]] * (B - 1), candidates=w["cands"])
    too_many = [[i % n for i in range(_lib.GRAM_MAX_USER_ITEMS + 1)]] + [[1]] * (B - 1)
    with pytest.raises(ValueError, match="at most"):
        call(allowed_items=too_many, candidates=w["cands"])
    with pytest.raises(ValueError, match="without any item"):
        call(exclude_items=[list(range(n))] + [[1]] * (B - 1), candidates=w["cands"])
    with pytest.raises(ValueError, match="without any item"):
        call(allowed_items=[[1]] * (B - 1) + [[-1, -1]], candidates=w["cands"])
    with pytest.raises(ValueError, match="one list per user"):
        call(exclude_items=[[1]] * (B - 1), candidates=w["cands"])
    def callback(batch_id, sent):  # (any callable that is no Trie closure)
        return [2, 3, 1]

    with pytest.raises(ValueError, match="closure"):
        call(fn=callback, exclude_items=some, candidates=w["cands"])
    # exactly the limit is accepted
    full = [[i % n for i in range(_lib.GRAM_MAX_USER_ITEMS)]] + [list(range(n))] * (B - 1)
    out, _ = call(allowed_items=full, candidates=w["cands"])
    assert torch.equal(_pad(out["sequences"], w["max_length"]), _pad(w["plain"]["sequences"], w["max_length"]))
