"""CPU: the host side of group (diverse) beam search (generate(num_beam_groups=, diversity_penalty=)) -- the
restatement the GPU tests compare with (tests/group_oracle.py) on a hand-worked example, against O.beam_search at one group and
with / without HF's early exit; the inputs of the whole-path GPU test (their decision margin and that the penalty acts in them);
every refusal of ``GRAM.generate`` on a CPU model, i.e. before anything touches a device; the new C entry points' argument errors;
the op's schema and meta implementation."""
import ctypes as C
import math

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import gram_amd
from gram_amd import _lib, ops  # noqa: F401
from gram_amd.utils import generation_trie as gt
from oracle import gram_oracle as O
from tests import group_oracle as GO

# 10 x SCORE_TOL of tests/test_gpu_path.py (the device's observed score deviation there is 1.9e-6): a condition on the INPUTS of
# tests/test_gpu_group_search.py, met by the seeds in group_oracle.WHOLE_PATH_SHAPES
MIN_MARGIN = 2e-4

TRIES = {
    "uniform": [[0, a, b, 1] for a in range(2, 9) for b in range(10, 14)],
    "ragged": [[0, 2, 3, 1], [0, 2, 4, 5, 1], [0, 2, 4, 6, 7, 1], [0, 3, 1], [0, 3, 8, 1], [0, 4, 9, 9, 9, 1], [0, 5, 1],
               [0, 6, 2, 1], [0, 6, 3, 1], [0, 7, 7, 1], [0, 8, 1], [0, 9, 2, 2, 1]],
    "narrow_root": [[0, 2, b, c, 1] for b in range(3, 9) for c in range(3, 7)] + [[0, 9, b, c, 1] for b in range(3, 6) for c in range(3, 5)],
}


def _logits(cands, B, K, V, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B * K, V, generator=g) * 2.0 for _ in range(max(len(c) for c in cands) - 1)]


def test_hand_worked_two_groups():
    """B = 1, K = 2, G = 2 (gs = 1), lambda = 1, items 2 3 4 5 (one piece each), normaliser 0 so that a score is a logit.
    Step 0: group 0 takes token 2 (-1.0 against -1.5); for group 1 token 2 now costs -1.0 - 1 = -2.0, so it takes token 3 (-1.5).
    Step 1: group 0's only real candidate is EOS (-1.0 - 0.5): it goes to the heap as -1.5 / 2 and the slot gets the -inf filler
    token 0; group 1's EOS (-1.5 - 0.25) is stored as -0.875, the heap is full and its worst equals the group's best: done."""
    cands = [[0, 2, 1], [0, 3, 1], [0, 4, 1], [0, 5, 1]]
    V = 8
    step0 = torch.full((2, V), -10.0)
    step0[:, 2], step0[:, 3], step0[:, 4], step0[:, 5] = -1.0, -1.5, -3.0, -4.0
    step1 = torch.full((2, V), -10.0)
    step1[0, 1], step1[1, 1] = -0.5, -0.25
    zero = [torch.zeros(2), torch.zeros(2)]
    trace = []
    seqs, scores = GO.logits_search([step0, step1], zero, cands, 1, 2, 2, 1.0, trace=trace)
    assert trace[0]["tokens"].tolist() == [[2, 3]] and trace[0]["beam_scores"].tolist() == [[-1.0, -1.5]]
    assert trace[1]["tokens"].tolist() == [[0, 0]] and trace[1]["beam_scores"].tolist() == [[-math.inf, -math.inf]]
    assert trace[0]["done"] == [False] and trace[1]["done"] == [True]
    assert seqs.tolist() == [[0, 2, 1], [0, 3, 1]] and scores.tolist() == [-0.75, -0.875]
    # without the penalty both groups walk the same branch and the list holds one item twice (the documented consequence)
    seqs0, scores0 = GO.logits_search([step0, step1], zero, cands, 1, 2, 2, 0.0)
    assert seqs0.tolist() == [[0, 2, 1], [0, 2, 1]] and scores0.tolist() == [-0.625, -0.75]


@pytest.mark.parametrize("name,K,lp", [("uniform", 4, 1.0), ("uniform", 20, 1.0), ("ragged", 5, 0.7), ("ragged", 12, 1.0),
                                        ("narrow_root", 6, 1.0), ("narrow_root", 16, 2.0)])
def test_one_group_is_plain_beam_search(name, K, lp):
    cands = TRIES[name]
    B, V = 3, 128
    logits = _logits(cands, B, K, V, 7 + K)
    it = iter(logits)
    ref = O.beam_search(lambda tok: next(it), lambda idx: None, B, K, max(len(c) for c in cands), O.prefix_allowed_tokens_fn(O.Trie(cands)),
                        lp, early_exit=False)
    got = GO.logits_search(logits, None, cands, B, K, 1, 0.0, lp)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


@pytest.mark.parametrize("name,K,G,lam", [("uniform", 4, 2, 1.0), ("ragged", 6, 3, 0.5), ("ragged", 12, 4, 1.5), ("ragged", 8, 8, 2.0),
                                           ("narrow_root", 6, 2, 1.0), ("narrow_root", 16, 4, 1.0), ("uniform", 20, 5, 0.5),
                                           ("ragged", 4, 2, 0.0)])
def test_early_exit_is_result_neutral(name, K, G, lam):
    """HF leaves the loop once every user is done; the device runs the fixed max_length - 1 steps.  A done user's groups are padded
    and its heap is never touched again, and finalize skips it: the same sequences and the same scores either way."""
    cands = TRIES[name]
    B, V = 3, 128
    logits = _logits(cands, B, K, V, 31 + K + G)
    t_all, t_exit = [], []
    full = GO.logits_search(logits, None, cands, B, K, G, lam, early_exit=False, trace=t_all)
    early = GO.logits_search(logits, None, cands, B, K, G, lam, early_exit=True, trace=t_exit)
    assert torch.equal(full[0], early[0]) and torch.equal(full[1], early[1])
    assert len(t_exit) <= len(t_all) == max(len(c) for c in cands) - 1


def test_whole_path_cases_are_decidable_and_exercise_the_penalty():
    cases = GO.whole_path_cases()
    assert [(c["B"], c["N"], c["L"], c["K"], c["G"], c["lam"]) for c in cases] == [
        (3, 2, 32, 4, 2, 0.5), (2, 3, 32, 6, 3, 1.0), (2, 1, 32, 20, 5, 0.5), (2, 2, 32, 8, 8, 1.0)]
    for c in cases:
        assert 40 <= len(c["cands"]) <= 200 and all(4 <= len(s) <= 6 for s in c["cands"])
        m = GO.Margin()
        seqs, _ = GO.run_case(c, margin=m, early_exit=False)
        print(f"[whole-path case K={c['K']} G={c['G']}] margin {m.value:.2e} at {m.where}")
        assert m.value >= MIN_MARGIN, (c["K"], c["G"], m.value, m.where)
        half, _ = GO.run_case(c, lam=c["lam"] / 2)
        assert half.shape != seqs.shape or not torch.equal(half, seqs)  # the penalty decides something in this case


@pytest.fixture(scope="module")
def cpu_model():
    cfg = gram_amd.T5Config(vocab_size=256, d_model=128, d_ff=256, num_layers=1, num_decoder_layers=1, num_heads=2, max_item_num=3)
    return gram_amd.create_model("gram", cfg).eval()


def test_refusals_fire_before_the_device(cpu_model):
    fn = gt.prefix_allowed_tokens_fn(gt.Trie([[0, 5, 1], [0, 6, 7, 1], [0, 6, 8, 1], [0, 9, 1]]))
    ids = torch.randint(2, 200, (2, 2, 32))
    mask = torch.ones(2, 2, 32, dtype=torch.bool)

    def call(**kw):
        args = dict(input_ids=ids, attention_mask=mask, max_length=4, prefix_allowed_tokens_fn=fn, num_beams=4, num_beam_groups=2,
                    diversity_penalty=1.0)
        args.update(kw)
        return cpu_model.generate(**args)

    for kw in (dict(num_beam_groups=8), dict(num_beam_groups=3), dict(num_beams=6, num_beam_groups=4)):
        with pytest.raises(ValueError, match="num_beam_groups"):
            call(**kw)
    with pytest.raises(ValueError, match="do_sample"):
        call(do_sample=True, num_beams=1, num_beam_groups=2)
    with pytest.raises(ValueError, match="do_sample"):
        call(do_sample=True)
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="diversity_penalty"):
            call(diversity_penalty=bad)
    with pytest.raises(NotImplementedError, match="closure"):
        call(prefix_allowed_tokens_fn=lambda b, s: [1])
    with pytest.raises(ValueError, match="num_return_sequences"):
        call(num_return_sequences=5)
    # one group is today's path: a non-zero penalty is refused by name, as it always was
    with pytest.raises(NotImplementedError, match="diversity_penalty"):
        call(num_beam_groups=1)
    # a legal group search (lambda = 0.0 included) passes every host check: a CPU model gets as far as the device and fails there
    for kw in (dict(), dict(diversity_penalty=0.0), dict(num_beam_groups=4), dict(num_beam_groups=1, diversity_penalty=0.0)):
        with pytest.raises(Exception) as e:
            call(**kw)
        assert not isinstance(e.value, (ValueError, NotImplementedError)), e.value


def test_argument_errors_without_gpu():
    """(K, G, lambda) are judged on the host before any launch: callable without a GPU, the pointers are never dereferenced"""
    lib = _lib.load()
    fake = C.c_void_p(0x1000)
    trie = _lib.Trie(0x1000, 0x1000, 0x1000, 4, 3, 3, 2)
    nan, inf = float("nan"), float("inf")
    bad = [(4, 0, 1.0), (4, -1, 1.0), (4, 8, 1.0), (4, 3, 1.0), (6, 4, 1.0), (4, 2, -1.0), (4, 2, nan), (4, 2, inf), (4, 2, -inf)]
    for K, G, lam in bad:
        st = _lib.BeamState(B=2, K=K, Tmax=6, length_penalty=1.0, eos=1, pad=0)
        assert lib.gram_beam_step_groups(C.byref(st), C.byref(trie), fake, fake, 128, 1, K, G, lam, None) == _lib.E_ARG, (K, G, lam)
        assert lib.gram_beam_step_groups_sparse(C.byref(st), C.byref(trie), fake, fake, None, 128, fake, 128, 1, K, None, 1, G, lam, None,
                                                None) == _lib.E_ARG, (K, G, lam)
        assert lib.gram_generate_groups(fake, fake, fake, 2, 2, 32, K, K, 6, 1.0, C.byref(trie), None, G, lam, None, fake, 1 << 30, fake,
                                        fake, None, None) == _lib.E_ARG, (K, G, lam)
        if lam == 1.0:
            assert lib.gram_beam_init_groups(C.byref(st), C.byref(trie), 0, G, None) == _lib.E_ARG, (K, G)
    # the whole-path entry needs a beam search: K < 2 is refused whatever the groups
    assert lib.gram_generate_groups(fake, fake, fake, 2, 2, 32, 1, 1, 6, 1.0, C.byref(trie), None, 1, 0.0, None, fake, 1 << 30, fake, fake,
                                    None, None) == _lib.E_ARG
    st = _lib.BeamState(B=2, K=4, Tmax=6, length_penalty=1.0, eos=1, pad=0)
    assert lib.gram_beam_step_groups(C.byref(st), C.byref(trie), None, fake, 128, 1, 4, 2, 1.0, None) == _lib.E_ARG  # no logits
    assert lib.gram_beam_step_groups(None, C.byref(trie), fake, fake, 128, 1, 4, 2, 1.0, None) == _lib.E_ARG
    assert lib.gram_beam_init_groups(None, C.byref(trie), 0, 2, None) == _lib.E_ARG


def test_op_schema_fake_and_all():
    assert "generate_groups" not in ops.__all__ and len(ops.__all__) == 12
    schema = str(torch.ops.gram.generate_groups.default._schema)
    assert schema.startswith("gram::generate_groups(Tensor input_ids, Tensor attention_mask, SymInt handle, Tensor(a3!) workspace, ")
    assert "float length_penalty, SymInt num_beam_groups, float diversity_penalty, Tensor? comp_map" in schema
    assert schema.endswith("Tensor? leaf_lo=None, Tensor? leaf_hi=None, Tensor? item_rank=None, Tensor? items=None, bool allow=False)"
                           " -> (Tensor, Tensor, Tensor)")
    I32, I64, U8 = torch.int32, torch.int64, torch.uint8
    with FakeTensorMode():
        def e(*shape, dtype=I32):
            return torch.empty(*shape, dtype=dtype, device="cuda")
        B, K, nret, T = 3, 6, 4, 7
        ids, ws, t = e(B, 2, 32, dtype=I64), e(1024, dtype=U8), e(8)
        head = (ids, ids.to(U8), 0, ws, t, t, t, 4, 3, K, nret, T, 1.0, 3, 0.5, None, None, None, None, None, 0, 0)
        for got in (torch.ops.gram.generate_groups(*head), torch.ops.gram.generate_groups(*head, t, t, t, e(B, 6), True)):
            s, sc, wd = got
            assert tuple(s.shape) == (B * nret, T) and s.dtype == I64 and s.device.type == "cuda"
            assert tuple(sc.shape) == (B * nret,) and sc.dtype == torch.float32
            assert tuple(wd.shape) == (1,) and wd.dtype == I32 and wd.device.type == "cpu"
