"""CPU: the host side of sampling without replacement (``generate(do_sample=True, replacement=False)``): the
C ABI's symbols, the refusals of ``generate`` on a CPU model, the ops' schemas and meta implementations, Philox's known answers, the
restatement (tests/sbs_oracle.py) against the Plackett-Luce law and its nested property, and the decidability of the inputs of the GPU
tests (tests/test_gpu_sbs.py, tests/test_gpu_sbs_step.py)."""
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import gram_amd
from gram_amd import _lib, ops  # noqa: F401
from gram_amd.utils import generation_trie as gt
from oracle import gram_oracle as O
from tests import sample_oracle as S
from tests import sbs_oracle as X
from tests.test_gpu_teacher_forced import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gram_sbs_init", "gram_sbs_step", "gram_sbs_step_items", "gram_sbs_finalize", "gram_sbs_capacity", "gram_debug_set_sbs_capacity",
       "gram_workspace_bytes_sbs", "gram_generate_sbs", "gram_generate_sbs_items")


def test_header_symbols_are_bound():
    header = open(os.path.join(ROOT, "include", "gram_hip.h")).read()
    declared = set(re.findall(r"\b(gram_\w*sbs\w*)\s*\(", header))
    assert declared == set(NEW), declared
    assert "#define GRAM_ABI_VERSION 7" in header  # (additive: the version stays)
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    stub = open(os.path.join(ROOT, "tools", "launch_trace", "stub.cpp")).read()
    for name in ("gram_sbs_init", "gram_sbs_step", "gram_sbs_step_items", "gram_sbs_finalize", "gram_sbs_capacity"):
        assert re.search(r"\b" + name + r"\(", stub), name  # (the launch-trace tool links against generate.o)


def test_capacity_hook():
    lib = _lib.load()
    assert lib.gram_sbs_capacity() == 4096
    try:
        assert lib.gram_debug_set_sbs_capacity(8) == 0 and lib.gram_sbs_capacity() == 8
        assert lib.gram_debug_set_sbs_capacity(1 << 20) == 0 and lib.gram_sbs_capacity() == 4096
        assert lib.gram_debug_set_sbs_capacity(-1) == _lib.E_ARG
    finally:
        lib.gram_debug_set_sbs_capacity(0)
    assert lib.gram_sbs_capacity() == 4096


@pytest.fixture(scope="module")
def cpu_model():
    cfg = gram_amd.T5Config(vocab_size=256, d_model=128, d_ff=256, num_layers=1, num_decoder_layers=1, num_heads=2, max_item_num=3)
    return gram_amd.create_model("gram", cfg).eval()


def test_refusals_fire_before_the_device(cpu_model):
    fn = gt.prefix_allowed_tokens_fn(gt.Trie([[0, 5, 1], [0, 6, 7, 1]]))
    ids = torch.randint(2, 200, (2, 2, 32))
    mask = torch.ones(2, 2, 32, dtype=torch.bool)

    def call(**kw):
        args = dict(input_ids=ids, attention_mask=mask, max_length=4, prefix_allowed_tokens_fn=fn, do_sample=True, num_beams=1,
                    num_return_sequences=3, replacement=False, seed=1)
        args.update(kw)
        return cpu_model.generate(**args)

    with pytest.raises(ValueError, match="uniforms"):
        call(uniforms=torch.rand(2, 3, 3))
    for bad in (1, 3, 49):
        with pytest.raises(NotImplementedError, match="top_k"):
            call(top_k=bad)
    with pytest.raises(NotImplementedError, match="top_p"):
        call(top_p=0.9)
    for bad in (1.5, "7", True):
        with pytest.raises(ValueError, match="seed"):
            call(seed=bad)
    for bad in (torch.arange(3), torch.arange(2, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int64), [0, 1]):
        with pytest.raises(ValueError, match="user_keys"):
            call(user_keys=bad)
    with pytest.raises(NotImplementedError, match="beam-sample"):
        call(num_beams=4)
    with pytest.raises(ValueError, match="temperature"):
        call(temperature=0.0)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="num_return_sequences"):
            call(num_return_sequences=bad)
    # what is accepted gets as far as the device and fails there: top_k None / 0 / the default 50, no seed (one is drawn), keys given
    for kw in (dict(top_k=None), dict(top_k=0), dict(top_k=50, seed=None), dict(seed=-5, user_keys=torch.tensor([9, 2 ** 62])),
               dict(seed=None, generator=torch.Generator().manual_seed(3))):
        with pytest.raises(Exception) as e:
            call(**kw)
        assert not isinstance(e.value, (ValueError, NotImplementedError)), (kw, e.value)
    # replacement=True is today's path, untouched: uniforms are taken, seed / user_keys are not its arguments
    with pytest.raises(ValueError, match="uniforms"):
        call(replacement=True, seed=None, uniforms=torch.rand(2, 3, 4))


def test_the_drawn_seed_follows_the_generator():
    f = gram_amd.GRAM._distinct_args
    a = f(2, 50, 1.0, None, None, None, torch.Generator().manual_seed(11))
    b = f(2, 50, 1.0, None, None, None, torch.Generator().manual_seed(11))
    c = f(2, 50, 1.0, None, None, None, torch.Generator().manual_seed(12))
    assert a[0] == b[0] != c[0] and -2 ** 63 <= a[0] < 2 ** 63
    assert a[1].tolist() == [0, 1] and a[1].dtype == torch.int64
    assert f(2, 0, 1.0, None, 2 ** 64 + 5, None, None)[0] == 5 and f(2, None, 1.0, None, 2 ** 63, None, None)[0] == -2 ** 63


SCHEMA_HEAD = ("Tensor input_ids, Tensor attention_mask, SymInt handle, Tensor(a3!) workspace, Tensor trie_child_off, Tensor trie_child_tok, "
               "Tensor trie_child_node, SymInt trie_max_fanout, SymInt trie_min_seq_len, SymInt num_return_sequences, SymInt max_length, "
               "float temperature, SymInt seed, Tensor user_keys, Tensor? comp_map, Tensor? comp_ids, Tensor? comp_mask, "
               "Tensor? cache_slot, Tensor? cache_x, SymInt n_cached, SymInt cache_L")


def test_op_schemas_and_fakes():
    out = " -> (Tensor, Tensor, Tensor, Tensor, Tensor)"
    assert str(torch.ops.gram.sample_distinct.default._schema) == "gram::sample_distinct(" + SCHEMA_HEAD + ")" + out
    assert str(torch.ops.gram.sample_distinct_items.default._schema) == (
        "gram::sample_distinct_items(" + SCHEMA_HEAD + ", Tensor leaf_lo, Tensor leaf_hi, Tensor item_rank, Tensor items, bool allow)" + out)
    I32, I64, U8, F32 = torch.int32, torch.int64, torch.uint8, torch.float32
    with FakeTensorMode():
        def e(*shape, dtype=I32):
            return torch.empty(*shape, dtype=dtype, device="cuda")
        B, R, T = 3, 5, 7
        ids, ws, t = e(B, 2, 32, dtype=I64), e(1024, dtype=U8), e(8)
        head = (ids, ids.to(U8), 0, ws, t, t, t, 4, 3, R, T, 0.7, -12345, e(B, dtype=I64))
        nocomp = (None, None, None, None, None, 0, 0)
        comp = (e(4), e(4, 32, dtype=I64), e(4, 32, dtype=U8), e(2), e(9, 128, 64, dtype=F32), 2, 128)
        for got in (torch.ops.gram.sample_distinct(*head, *nocomp), torch.ops.gram.sample_distinct(*head, *comp),
                    torch.ops.gram.sample_distinct_items(*head, *nocomp, t, t, t, e(B, 6), True)):
            s, mlp, slp, g, wd = got
            assert tuple(s.shape) == (B * R, T) and s.dtype == I64 and s.device.type == "cuda"
            assert tuple(mlp.shape) == tuple(slp.shape) == tuple(g.shape) == (B * R,) and mlp.dtype == slp.dtype == g.dtype == F32
            assert tuple(wd.shape) == (1,) and wd.dtype == I32 and wd.device.type == "cpu"


def test_philox_known_answers():
    for counter, key, want in (
            ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
            ((X.M32,) * 4, (X.M32,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
            ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")):
        assert " ".join(f"{w:08x}" for w in X.philox(counter, key)) == want
    assert X.seed_key(-1) == (X.M32, X.M32) and X.seed_key(2 ** 32 + 7) == (7, 1)
    assert 0.0 < X.uniform(0) < X.uniform(X.M32) < 1.0


# ---------------------------------------------------------------------------------------------- the restatement against Plackett-Luce
# 7 items of depth 1 to 3 behind the start token; [0, 5, 1] is a prefix of [0, 5, 6, 1] and [0, 5, 7, 8, 1]
ITEMS = [[0, 5, 1], [0, 5, 6, 1], [0, 5, 7, 8, 1], [0, 5, 7, 9, 1], [0, 11, 1], [0, 12, 3, 1], [0, 12, 4, 1]]


def _small_case():
    trie = O.Trie(ITEMS)
    rng = np.random.default_rng(4)
    logits, prob = {}, {}

    def fill(prefix, lp):
        toks = sorted(trie.get(list(prefix)))
        if not toks:
            return
        z = rng.normal(0.0, 1.5, len(toks))
        logits[prefix] = dict(zip(toks, z))
        lse = np.log(np.exp(z).sum())
        for t, zi in zip(toks, z):
            if t == 1:
                prob[prefix + (1,)] = lp + zi - lse
            fill(prefix + (t,), lp + zi - lse)
    fill((0,), 0.0)
    return trie, logits, prob


def test_restatement_is_plackett_luce_and_nested():
    """20 000 user keys at one seed, R = 3 over the 7-item Trie: every ordered pair of the first two rows within 4.5 sigma of its
    Plackett-Luce probability p_i p_j / (1 - p_i); every row's phi is the item's exact log-probability; the rows of R' = 2 are the
    first two rows of R = 3, identical in every float"""
    trie, logits, prob = _small_case()
    assert len(prob) == 7 and abs(sum(math.exp(v) for v in prob.values()) - 1) < 1e-12
    kids = X.table_kids(trie, logits)
    n, pairs = 20000, {}
    for key in range(n):
        rows, _ = X.run(kids, 3, 5, 7, key)
        assert len(rows) == 3 and len({r["prefix"] for r in rows}) == 3
        assert rows[0]["G"] > rows[1]["G"] > rows[2]["G"] and all(r["fin"] for r in rows)
        for r in rows:
            assert abs(r["phi"] - prob[r["prefix"]]) < 1e-12
        if key < 500:
            two, _ = X.run(kids, 2, 5, 7, key)
            assert [(r["prefix"], r["phi"], r["G"], r["path"]) for r in two] == [(r["prefix"], r["phi"], r["G"], r["path"]) for r in rows[:2]]
        pair = (rows[0]["prefix"], rows[1]["prefix"])
        pairs[pair] = pairs.get(pair, 0) + 1
    worst = 0.0
    for i, j in itertools.permutations(prob, 2):
        p = math.exp(prob[i]) * math.exp(prob[j]) / (1 - math.exp(prob[i]))
        worst = max(worst, abs(pairs.get((i, j), 0) - n * p) / math.sqrt(n * p * (1 - p)))
    print(f"worst |z| over 42 ordered pairs: {worst:.2f}")
    assert worst < 4.5


def test_first_row_follows_the_softmax_on_the_restatement():
    """the device's distribution check (tests/test_gpu_sbs_step.py) on the restatement, with the same seed, keys, tokens and logits"""
    counts = np.zeros(len(X.DIST_LOGITS))
    toks = list(X.DIST_TOKENS)

    def kids(prefix):
        return toks, np.asarray(X.DIST_LOGITS), 3.0
    for key in X.dist_keys():
        r = X.root(X.DIST_SEED, key)
        ranked, _ = X.expand([r], kids, 1.0, X.DIST_SEED, 3)
        assert ranked[0]["G"] == r["G"]
        counts[toks.index(ranked[0]["tok"])] += 1
    assert float(np.abs(X.dist_z(counts)).max()) < 4.5


# ---------------------------------------------------------------------------------------------- the GPU test's inputs are decidable
@pytest.fixture(scope="module")
def case():
    c = S.whole_path_case()
    return c, [O.Trie(c["cands"])] * S.B


def test_delta_constants_cover_the_measurement(case):
    """DELTA[mode] >= 4 x the largest |dG| under logit moves of TOL[mode]['logit'] and under float32, and with it at most 10 % of the
    (user, step) pairs of the restatement's own run are left out; the one-piece tolerance is NOT decidable, which is why
    tests/test_gpu_sbs.py runs the selection test in the two-piece modes only"""
    c, tries = case
    assert TOL["f16x3"]["logit"] in (1e-4, 16e-4)  # (the default build's and the PIECE=bf16 build's two-piece tolerance)
    for mode, tol in (("f16x3", 1e-4), ("bf16x3", 16e-4)):
        worst, exact = X.measure_delta(c, tries, S.R, S.MAX_LENGTH, tol)
        gaps = [h["gap"] for hb in exact for h in hb]
        print(f"[{mode}] logit tolerance {tol:.1e}: largest |dG| {worst:.3e}, 4 x = {4 * worst:.3e}, constant {X.DELTA[mode]:.1e}; "
              f"smallest gap {min(gaps):.3e}")
        assert 4 * worst <= X.DELTA[mode]
        assert sum(g <= X.DELTA[mode] for g in gaps) <= 0.10 * len(gaps)
    worst, exact = X.measure_delta(c, tries, S.R, S.MAX_LENGTH, TOL["f16"]["logit"])
    gaps = [h["gap"] for hb in exact for h in hb]
    assert sum(g <= 4 * worst for g in gaps) > 0.10 * len(gaps) and "f16" not in X.DELTA and "bf16" not in X.DELTA


def test_whole_path_case_on_the_restatement(case):
    """the GPU test's case on the restatement alone: 8 distinct candidates per user in descending order of G, nested in R and in the
    length, phi the exact log-probability of the item under the Trie-renormalised distribution"""
    c, tries = case
    a = (c["sd"], c["oc"], c["ids"], c["mask"], tries)
    full = X.walk(*a, S.R, S.MAX_LENGTH, X.SEED, X.USER_KEYS)
    three = X.walk(*a, 3, S.MAX_LENGTH, X.SEED, X.USER_KEYS)
    short = X.walk(*a, S.R, 3, X.SEED, X.USER_KEYS)
    cands = {tuple(s) for s in c["cands"]}
    for b, rows in enumerate(X.final_rows(full, S.R)):
        assert len(rows) == S.R and {r["prefix"] for r in rows} <= cands and len({r["prefix"] for r in rows}) == S.R
        assert all(r["fin"] for r in rows) and all(x["G"] > y["G"] for x, y in zip(rows, rows[1:]))
        got3 = X.final_rows(three, 3)[b]
        # (the same rows; the oracle's fp32 decoder over 9 rows instead of 24 moves a logit by ~1e-7, so not the same floats here --
        # the table-driven test above shows those identical)
        assert [r["prefix"] for r in got3] == [r["prefix"] for r in rows[:3]]
        assert all(abs(x["G"] - y["G"]) < 1e-5 and abs(x["phi"] - y["phi"]) < 1e-5 for x, y in zip(got3, rows))
        assert [r["prefix"] for r in short[b][1]["ranked"][:S.R]] == [r["prefix"] for r in full[b][1]["ranked"][:S.R]]
