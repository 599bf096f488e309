"""-m gpu: group (diverse) beam search through the whole path -- GRAM.generate(num_beam_groups=, diversity_penalty=) ->
torch.ops.gram.generate_groups -> gram_generate_groups -- against the restatement (tests/group_oracle.py) on the tiny model of
tests/test_gpu_path.py.  The inputs are group_oracle.whole_path_cases(): their decision margin on the oracle model is at least
10 x SCORE_TOL (tests/test_group_search_host.py), so the device, whose scores deviate from the oracle's by fp32 rounding, must
return the restatement's sequences exactly."""
import pytest
import torch

from gram_amd import _lib
from gram_amd.utils import generation_trie as gt
from oracle import gram_oracle as O
from tests import group_oracle as GO
from tests.test_gpu_path import DEV, SCORE_TOL, _model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gram_amd
    return gram_amd


@pytest.fixture(scope="module")
def world(gpu):
    """every case with its model on the device and the restatement's answer, computed once"""
    out = []
    for c in GO.whole_path_cases():
        _oc, _sd, m = _model(gpu, c["cfg"], c["model_seed"])
        ref_seqs, ref_scores = GO.run_case(c)
        out.append(dict(c, m=m, fn=gt.prefix_allowed_tokens_fn(gt.Trie(c["cands"])), ref_seqs=ref_seqs, ref_scores=ref_scores))
    return out


def _gen(w, **kw):
    args = dict(input_ids=w["input_ids"].to(DEV), attention_mask=w["attention_mask"].to(DEV), max_length=w["max_length"],
                prefix_allowed_tokens_fn=w["fn"], num_beams=w["K"], num_beam_groups=w["G"], diversity_penalty=w["lam"],
                length_penalty=w["length_penalty"])
    args.update(kw)
    return w["m"].generate(**args)


@pytest.mark.parametrize("i", range(4))
def test_generate_equals_the_restatement(world, i):
    w = world[i]
    out = _gen(w)
    seqs, scores = out["sequences"].cpu(), out["sequences_scores"].cpu()
    same = scores.shape == w["ref_scores"].shape
    dev = float((scores - w["ref_scores"])[torch.isfinite(w["ref_scores"])].abs().max()) if same else float("nan")  # (-inf: filler rows)
    print(f"[group search B={w['B']} K={w['K']} G={w['G']} lambda={w['lam']}] max |score - restatement| {dev:.2e}")
    assert seqs.shape[1] == w["ref_seqs"].shape[1]  # the width
    assert seqs.tolist() == w["ref_seqs"].tolist()
    assert torch.allclose(scores, w["ref_scores"], atol=SCORE_TOL, rtol=0)


@pytest.mark.parametrize("i", range(4))
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


def test_exclude_items_equal_the_users_own_trie(world):
    w = world[1]
    cands, B, K = w["cands"], w["B"], w["K"]
    top = _gen(w)["sequences"].cpu()
    index = {tuple(c): i for i, c in enumerate(cands)}
    lists = []
    for b in range(B):  # every user loses the items its unfiltered list starts with, and a few more
        mine = {index[tuple(x for x in [0] + [t for t in row.tolist()[1:] if t != 0])] for row in top[b * K:b * K + 3]}
        lists.append(sorted(mine | {(7 * b + j) % len(cands) for j in range(5)}))
    out = _gen(w, exclude_items=lists, candidates=cands)
    for b in range(B):
        own = [c for i, c in enumerate(cands) if i not in set(lists[b])]
        alone = w["m"].generate(input_ids=w["input_ids"][b:b + 1].to(DEV), attention_mask=w["attention_mask"][b:b + 1].to(DEV),
                                max_length=w["max_length"], prefix_allowed_tokens_fn=gt.prefix_allowed_tokens_fn(gt.Trie(own)),
                                num_beams=K, num_beam_groups=w["G"], diversity_penalty=w["lam"], length_penalty=w["length_penalty"])
        wa = alone["sequences"].shape[1]
        rows = out["sequences"][b * K:(b + 1) * K]
        assert torch.equal(rows[:, :wa], alone["sequences"]) and not rows[:, wa:].any()
        assert torch.equal(out["sequences_scores"][b * K:(b + 1) * K], alone["sequences_scores"])
        assert not any(tuple(c) in {tuple(x[: len(c)]) for x in rows.tolist()} for c in (cands[i] for i in lists[b]))


def test_fewer_return_sequences(world):
    w = world[2]
    K, nret = w["K"], 7
    full, part = _gen(w), _gen(w, num_return_sequences=nret)
    fs = full["sequences"].view(w["B"], K, -1)[:, :nret]
    wp = part["sequences"].shape[1]
    assert torch.equal(part["sequences"].view(w["B"], nret, -1), fs[:, :, :wp]) and not fs[:, :, wp:].any()
    assert torch.equal(part["sequences_scores"].view(w["B"], nret), full["sequences_scores"].view(w["B"], K)[:, :nret])


def test_the_op_called_directly_equals_generate(world):
    w = world[0]
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
    seqs, scores, width = torch.ops.gram.generate_groups(ids, mask, int(handle), ws, t_off, t_tok, t_node, int(flat.max_fanout),
                                                         int(flat.min_seq_len), w["K"], w["K"], w["max_length"], 1.0, w["G"], w["lam"],
                                                         *m._comp_args(comp))
    assert torch.equal(seqs[:, : int(width[0])], ref["sequences"]) and torch.equal(scores, ref["sequences_scores"])
    with pytest.raises(ValueError, match="num_beam_groups"):
        torch.ops.gram.generate_groups(ids, mask, int(handle), ws, t_off, t_tok, t_node, int(flat.max_fanout), int(flat.min_seq_len),
                                       w["K"], w["K"], w["max_length"], 1.0, 3, w["lam"], *m._comp_args(comp))


def test_plain_beam_search_is_unchanged_by_a_group_search(world):
    w = world[3]
    plain = dict(num_beam_groups=1, diversity_penalty=0.0)
    before = _gen(w, **plain)
    _gen(w)
    after = _gen(w, **plain)
    assert torch.equal(before["sequences"], after["sequences"]) and torch.equal(before["sequences_scores"], after["sequences_scores"])
    ref = O.generate(O.init_state_dict(w["cfg"], w["model_seed"]), w["cfg"], w["input_ids"], w["attention_mask"], w["max_length"],
                     O.prefix_allowed_tokens_fn(O.Trie(w["cands"])), num_beams=w["K"])
    assert torch.allclose(before["sequences_scores"].cpu(), ref["sequences_scores"], atol=SCORE_TOL, rtol=0)
