"""-m gpu: beam search with per-item score biases through the whole path -- GRAM.generate(item_bias=, bias_lookahead=) ->
torch.ops.gram.item_bias_table + torch.ops.gram.generate_bias -> gram_generate_bias -- against the restatement (tests/bias_oracle.py)
on the tiny model of tests/test_gpu_path.py.  The inputs are bias_oracle.whole_path_cases(): their decision margin on the oracle
model is at least 5e-4 with and without lookahead (tests/test_item_bias_host.py), far above the device's score deviation, so the
device must return the restatement's sequences exactly."""
import pytest
import torch

from gram_amd import _lib
from gram_amd.utils import generation_trie as gt
from tests import bias_oracle as BO
from tests.test_gpu_path import DEV, SCORE_TOL, _model

pytestmark = pytest.mark.gpu
N_CASES = len(BO.WHOLE_PATH_SEEDS)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gram_amd
    return gram_amd


@pytest.fixture(scope="module")
def world(gpu):
    """every case with its model on the device and the restatement's answers, computed once"""
    out = []
    for c in BO.whole_path_cases():
        _oc, _sd, m = _model(gpu, c["cfg"], c["model_seed"])
        out.append(dict(c, m=m, fn=gt.prefix_allowed_tokens_fn(gt.Trie(c["cands"])), ref=BO.run_case(c, lookahead=True),
                        ref_leaf=BO.run_case(c, lookahead=False), index={tuple(s): i for i, s in enumerate(c["cands"])}))
    return out


def _gen(w, **kw):
    args = dict(input_ids=w["input_ids"].to(DEV), attention_mask=w["attention_mask"].to(DEV), max_length=w["max_length"],
                prefix_allowed_tokens_fn=w["fn"], num_beams=w["K"], length_penalty=w["length_penalty"], candidates=w["cands"],
                item_bias=w["bias"])
    args.update(kw)
    return w["m"].generate(**args)


def _equals(out, ref, what):
    ref_seqs, ref_scores = ref
    seqs, scores = out["sequences"].cpu(), out["sequences_scores"].cpu()
    same = scores.shape == ref_scores.shape
    dev = float((scores - ref_scores)[torch.isfinite(ref_scores)].abs().max()) if same else float("nan")  # (-inf: filler rows)
    print(f"[{what}] max |score - restatement| {dev:.2e}")
    assert seqs.shape[1] == ref_seqs.shape[1]  # the width
    assert seqs.tolist() == ref_seqs.tolist()
    assert torch.allclose(scores, ref_scores, atol=SCORE_TOL, rtol=0)


@pytest.mark.parametrize("i", range(N_CASES))
def test_generate_equals_the_restatement(world, i):
    """Fails without the feature: the keyword is ignored there and the plain list comes back (every case's bias changes a list)."""
    w = world[i]
    tag = f"item bias B={w['B']} K={w['K']} per_user={w['per_user']}"
    _equals(_gen(w), w["ref"], tag + " lookahead")
    _equals(_gen(w, bias_lookahead=False), w["ref_leaf"], tag + " leaf-only")
    assert _gen(w, item_bias=w["bias"].to(DEV))["sequences"].cpu().tolist() == w["ref"][0].tolist()  # a bias on the device


@pytest.mark.parametrize("i", range(N_CASES))
def test_a_zero_bias_is_the_plain_search_bit_for_bit(world, i):
    w = world[i]
    plain = _gen(w, item_bias=None)
    for look in (True, False):
        zero = _gen(w, item_bias=torch.zeros_like(w["bias"]), bias_lookahead=look)
        assert torch.equal(zero["sequences"], plain["sequences"]) and torch.equal(zero["sequences_scores"], plain["sequences_scores"])


@pytest.mark.parametrize("i", range(N_CASES))
def test_scores_are_the_log_probability_plus_the_items_bias(world, i):
    """every returned row: sequences_scores = (score_sequences of the row + T[item]) / len^length_penalty -- the edge terms along a
    path telescope.  +-4 biases over at most six steps add about 5e-6 of fp32 rounding to the 1.9e-6 observed for plain scores.
    Fails without the feature."""
    w = world[i]
    B, K, lp = w["B"], w["K"], 0.6
    worst = 0.0
    for look in (True, False):
        out = _gen(w, length_penalty=lp, bias_lookahead=look)
        seqs, scores = out["sequences"].cpu(), out["sequences_scores"].cpu()
        assert torch.isfinite(scores).all()
        labels = torch.full((B, K, seqs.shape[1] - 1), -100, dtype=torch.long)
        lens = torch.zeros(B, K)
        bias = torch.zeros(B, K)
        for r, row in enumerate(seqs.tolist()):
            b, k = divmod(r, K)
            seq = row[: row.index(1) + 1]
            labels[b, k, : len(seq) - 1] = torch.tensor(seq[1:])
            lens[b, k] = len(seq) - 1  # (HF's length: the hypothesis without the EOS it ends on)
            item = w["index"][tuple(seq)]
            bias[b, k] = w["bias"][b, item] if w["per_user"] else w["bias"][item]
        logp = w["m"].score_sequences(w["input_ids"].to(DEV), w["attention_mask"].to(DEV), labels.to(DEV)).cpu()
        want = (logp + bias) / lens ** lp
        worst = max(worst, float((scores.view(B, K) - want).abs().max()))
    print(f"[item bias B={B} K={K} per_user={w['per_user']}] max |sequences_scores - (score_sequences + T) / len^lp| {worst:.2e}")
    assert worst <= SCORE_TOL


@pytest.mark.parametrize("i", [1, 2, 7])
def test_exclude_items_compose_with_the_bias(world, i):
    w = world[i]
    cands, B, K = w["cands"], w["B"], w["K"]
    top = _gen(w)["sequences"].cpu()
    lists = []
    for b in range(B):  # every user loses the items its biased list starts with, and a few more
        mine = {w["index"][tuple(row[: row.index(1) + 1])] for row in top[b * K:b * K + 3].tolist()}
        lists.append(sorted(mine | {(7 * b + j) % len(cands) for j in range(5)}))
    keep = BO.keep_masks(BO.flat_trie(cands), cands, lists, allow=False)
    m = BO.Margin()
    ref = BO.run_case(w, keep=keep, margin=m, early_exit=False)
    out = _gen(w, exclude_items=lists)
    rows = out["sequences"].cpu().tolist()
    for b in range(B):
        got = {w["index"].get(tuple(r[: r.index(1) + 1])) for r in rows[b * K:(b + 1) * K] if 1 in r}
        assert got and not (got & set(lists[b]))  # none of the excluded items
    assert m.value >= 10 * SCORE_TOL, ("the filtered case is not decidable", m.value, m.where)  # (a property of the input)
    _equals(out, ref, f"item bias + exclude_items B={B} K={K}")


@pytest.mark.parametrize("i", range(N_CASES))
def test_live_row_compaction_is_result_neutral(world, i):
    w = world[i]
    lib = _lib.load()
    a = _gen(w)
    try:
        assert lib.gram_debug_set_live_rows(0) == 0
        b = _gen(w)
    finally:
        lib.gram_debug_set_live_rows(-1)
    assert torch.equal(a["sequences"], b["sequences"]) and torch.equal(a["sequences_scores"], b["sequences_scores"])


@pytest.mark.parametrize("i", [0, 3])
def test_the_ops_called_directly_equal_generate(world, i):
    w = world[i]
    m = w["m"]
    ref = _gen(w)
    dev = torch.device(DEV)
    ids = w["input_ids"].to(dev).contiguous()
    mask = w["attention_mask"].to(dev).view(torch.uint8).contiguous()
    B, N, L = ids.shape
    handle = m._pack()
    flat = m._flat_trie(w["fn"])
    comp, _harvest = m._plan(ids, mask, B, N, L)
    _ctrie, (t_off, t_tok, t_node) = flat.to_device(dev)
    ws = m._get_workspace(handle, B, N, L, w["K"], w["max_length"])
    lo, hi = flat.leaf_ranges_on(dev)
    trie = (t_off, t_tok, t_node, int(flat.max_fanout), int(flat.min_seq_len))
    phi = torch.ops.gram.item_bias_table(w["bias"].reshape(-1, len(w["cands"])).to(dev), flat.leaf_items_on(dev, w["cands"]), lo, hi,
                                         *trie, 0, True)
    assert tuple(phi.shape) == (B if w["per_user"] else 1, flat.n_nodes)
    seqs, scores, width = torch.ops.gram.generate_bias(ids, mask, int(handle), ws, *trie, w["K"], w["K"], w["max_length"], 1.0, phi,
                                                       *m._comp_args(comp))
    assert torch.equal(seqs[:, : int(width[0])], ref["sequences"]) and torch.equal(scores, ref["sequences_scores"])
    with pytest.raises(ValueError, match="phi"):
        torch.ops.gram.generate_bias(ids, mask, int(handle), ws, *trie, w["K"], w["K"], w["max_length"], 1.0, phi[:, :-1].contiguous(),
                                     *m._comp_args(comp))
    with pytest.raises(ValueError, match="num_beams"):
        torch.ops.gram.generate_bias(ids, mask, int(handle), ws, *trie, 1, 1, w["max_length"], 1.0, phi, *m._comp_args(comp))


def test_plain_beam_search_is_unchanged_by_a_biased_one(world):
    w = world[5]
    before = _gen(w, item_bias=None)
    _gen(w)
    after = _gen(w, item_bias=None)
    assert torch.equal(before["sequences"], after["sequences"]) and torch.equal(before["sequences_scores"], after["sequences_scores"])
    assert before["sequences"].cpu().tolist() != w["ref"][0].tolist()  # (the bias changes this case's lists)


def test_fewer_return_sequences_and_two_beams(world):
    """num_return_sequences < num_beams returns the head of the full list; the greedy refusal's advice (num_beams=2,
    num_return_sequences=1) runs"""
    w = world[4]
    K, nret = w["K"], 7
    full, part = _gen(w), _gen(w, num_return_sequences=nret)
    fs = full["sequences"].view(w["B"], K, -1)[:, :nret]
    wp = part["sequences"].shape[1]
    assert torch.equal(part["sequences"].view(w["B"], nret, -1), fs[:, :, :wp]) and not fs[:, :, wp:].any()
    assert torch.equal(part["sequences_scores"].view(w["B"], nret), full["sequences_scores"].view(w["B"], K)[:, :nret])
    one = _gen(w, num_beams=2, num_return_sequences=1)
    assert tuple(one["sequences_scores"].shape) == (w["B"],) and torch.isfinite(one["sequences_scores"]).all()
