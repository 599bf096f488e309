"""CPU: the host side of Trie-constrained sampling (generate(do_sample=True)) -- the new C entry points are
declared, bound and exported; every refusal of ``GRAM.generate(do_sample=True)`` fires on a CPU model, i.e. before anything touches
a device; the two ops' schemas and meta implementations; the float64 restatement the GPU tests compare with (tests/sample_oracle.py)
against HF's own warpers; and the inputs of the capped whole-path test (tests/test_gpu_sample.py): the restatement alone, on those
inputs, must leave fewer than 10 % of the steps undecidable, so the cap is known to be reachable before the GPU is asked."""
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
from tests.test_gpu_teacher_forced import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gram_sample_step", "gram_sample_step_items", "gram_sample_finalize", "gram_sample_capacity", "gram_debug_set_sample_capacity",
       "gram_workspace_bytes_sample", "gram_sample", "gram_sample_items")


def test_header_symbols_are_bound():
    header = open(os.path.join(ROOT, "include", "gram_hip.h")).read()
    declared = set(re.findall(r"\b(gram_(?:debug_set_)?(?:sample|workspace_bytes_sample)\w*)\s*\(", header))
    assert declared == set(NEW), declared
    assert "gram_sample_params_t" in header and "#define GRAM_ABI_VERSION 7" in header
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert lib.gram_abi_version() == 7 and _lib.ABI_VERSION == 7
    assert [f[0] for f in _lib.SampleParams._fields_] == ["temperature", "top_k", "top_p"]


def test_sample_params_layout(tmp_path):
    """gram_sample_params_t against its ctypes mirror: size and every field's offset from a C program compiled against the header"""
    import ctypes
    import subprocess
    fields = [f[0] for f in _lib.SampleParams._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gram_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(gram_sample_params_t));\n'
                   + "".join(f'  printf(" %zu", offsetof(gram_sample_params_t, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.SampleParams)] + [getattr(_lib.SampleParams, f).offset for f in fields]


def test_capacity_hook():
    lib = _lib.load()
    # the capacity hook: lowers, never raises above the default, 0 restores
    assert lib.gram_sample_capacity() == 8192
    try:
        assert lib.gram_debug_set_sample_capacity(64) == 0 and lib.gram_sample_capacity() == 64
        assert lib.gram_debug_set_sample_capacity(1 << 20) == 0 and lib.gram_sample_capacity() == 8192
        assert lib.gram_debug_set_sample_capacity(-1) == _lib.E_ARG
    finally:
        lib.gram_debug_set_sample_capacity(0)
    assert lib.gram_sample_capacity() == 8192


@pytest.fixture(scope="module")
def cpu_model():
    oc = O.OracleConfig(vocab_size=256, d_model=128, d_kv=64, d_ff=256, num_layers=1, num_decoder_layers=1, num_heads=2, max_item_num=3)
    cfg = gram_amd.T5Config(vocab_size=oc.vocab_size, d_model=oc.d_model, d_ff=oc.d_ff, num_layers=1, num_decoder_layers=1, num_heads=2,
                            max_item_num=3)
    return gram_amd.create_model("gram", cfg).eval()


def test_refusals_fire_before_the_device(cpu_model):
    fn = gt.prefix_allowed_tokens_fn(gt.Trie([[0, 5, 1], [0, 6, 7, 1]]))
    ids = torch.randint(2, 200, (2, 2, 32))
    mask = torch.ones(2, 2, 32, dtype=torch.bool)

    def call(**kw):
        args = dict(input_ids=ids, attention_mask=mask, max_length=4, prefix_allowed_tokens_fn=fn, do_sample=True, num_beams=1,
                    num_return_sequences=3)
        args.update(kw)
        return cpu_model.generate(**args)

    with pytest.raises(NotImplementedError, match="beam-sample"):
        call(num_beams=4)
    with pytest.raises(NotImplementedError, match="closure"):
        call(prefix_allowed_tokens_fn=lambda b, s: [1])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            call(temperature=bad)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="top_p"):
            call(top_p=bad)
    with pytest.raises(ValueError, match="top_k"):
        call(top_k=-1)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="num_return_sequences"):
            call(num_return_sequences=bad)
    for bad in (torch.rand(2, 3, 4), torch.rand(3, 2, 3), torch.rand(2, 3, 3, dtype=torch.float64), torch.zeros(2, 3, 3, dtype=torch.int64),
                [[0.5] * 3] * 6):
        with pytest.raises(ValueError, match="uniforms"):
            call(uniforms=bad)
    # without do_sample the sampling arguments are ignored as before, and the refusals above are not reached: a CPU model gets as far
    # as the device and fails there, for greedy and for beam search alike
    for kw in (dict(do_sample=False, temperature=-1.0, top_p=7.0, top_k=-3), dict(do_sample=False, num_beams=4, temperature=0.0)):
        with pytest.raises(Exception) as e:
            call(**kw)
        assert not isinstance(e.value, ValueError), e.value


SCHEMA_HEAD = ("Tensor input_ids, Tensor attention_mask, SymInt handle, Tensor(a3!) workspace, Tensor trie_child_off, Tensor trie_child_tok, "
               "Tensor trie_child_node, SymInt trie_max_fanout, SymInt trie_min_seq_len, SymInt num_return_sequences, SymInt max_length, "
               "float temperature, SymInt top_k, float top_p, Tensor uniforms, Tensor? comp_map, Tensor? comp_ids, Tensor? comp_mask, "
               "Tensor? cache_slot, Tensor? cache_x, SymInt n_cached, SymInt cache_L")


def test_op_schemas_and_fakes():
    out = " -> (Tensor, Tensor, Tensor, Tensor)"
    assert str(torch.ops.gram.sample.default._schema) == "gram::sample(" + SCHEMA_HEAD + ")" + out
    assert str(torch.ops.gram.sample_items.default._schema) == (
        "gram::sample_items(" + SCHEMA_HEAD + ", Tensor leaf_lo, Tensor leaf_hi, Tensor item_rank, Tensor items, bool allow)" + out)
    I32, I64, U8, F32 = torch.int32, torch.int64, torch.uint8, torch.float32
    with FakeTensorMode():
        def e(*shape, dtype=I32):
            return torch.empty(*shape, dtype=dtype, device="cuda")
        B, R, T = 3, 5, 7
        ids, ws, t = e(B, 2, 32, dtype=I64), e(1024, dtype=U8), e(8)
        head = (ids, ids.to(U8), 0, ws, t, t, t, 4, 3, R, T, 0.7, 50, 0.9, e(B, R, T - 1, dtype=F32))
        nocomp = (None, None, None, None, None, 0, 0)
        comp = (e(4), e(4, 32, dtype=I64), e(4, 32, dtype=U8), e(2), e(9, 128, 64, dtype=F32), 2, 128)
        for got in (torch.ops.gram.sample(*head, *nocomp), torch.ops.gram.sample(*head, *comp),
                    torch.ops.gram.sample_items(*head, *nocomp, t, t, t, e(B, 6), True)):
            s, mlp, slp, wd = got
            assert tuple(s.shape) == (B * R, T) and s.dtype == I64 and s.device.type == "cuda"
            assert tuple(mlp.shape) == tuple(slp.shape) == (B * R,) and mlp.dtype == slp.dtype == F32
            assert tuple(wd.shape) == (1,) and wd.dtype == I32 and wd.device.type == "cpu"


def test_restatement_keeps_what_hf_warpers_keep():
    """1 000 random rows without ties through HF's installed TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper (the
    order of ``_get_logits_warper``): the kept sets are the restatement's.  Rows whose top_p cut falls within 1e-6 of a cumulative
    sum are redrawn (HF cuts in float32)."""
    from transformers import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    rng = np.random.default_rng(2025)
    done = 0
    while done < 1000:
        F = int(rng.integers(1, 40))
        z = rng.normal(0.0, 3.0, F)
        tau = float(rng.choice([0.5, 1.0, 2.0]))
        k = int(rng.choice([0, 1, 2, 5, F, F + 5]))
        p = float(rng.choice([1.0, 0.9, 0.5, 1e-6]))
        y, kept, cum = S.warp(z, tau, k, p)
        if len(np.unique(y)) < F or (p < 1 and np.nanmin(np.abs(cum - (1 - p))) < 1e-6):
            continue
        scores = torch.from_numpy(z).float()[None]
        scores = TemperatureLogitsWarper(tau)(None, scores)
        if k > 0:
            scores = TopKLogitsWarper(top_k=k)(None, scores)
        if p < 1:
            scores = TopPLogitsWarper(top_p=p)(None, scores)
        hf = torch.isfinite(scores[0]).numpy()
        assert np.array_equal(hf, kept), (z, tau, k, p, hf, kept)
        done += 1


def test_restatement_draw_and_ties():
    z = np.array([1.0, 3.0, 3.0, -2.0, 0.5])
    # ties at the top_k threshold and at the top_p boundary stay together
    assert S.warp(z, 1.0, 1, 1.0)[1].tolist() == [False, True, True, False, False]
    assert S.warp(z, 1.0, 0, 1e-6)[1].tolist() == [False, True, True, False, False]
    y, kept, _ = S.warp(z, 2.0, 4, 1.0)
    lo, hi, logq = S.cdf(y, kept)
    assert kept.tolist() == [True, True, True, False, True] and abs(np.nansum(np.exp(logq)) - 1) < 1e-12
    assert S.pick(z, 0.0, 2.0, 4) == 0 and S.pick(z, np.nextafter(np.float32(1), np.float32(0)), 2.0, 4) == 4
    for i in np.nonzero(kept)[0]:
        assert S.pick(z, 0.5 * (lo[i] + hi[i]), 2.0, 4) == i


@pytest.mark.parametrize("mode", ["f16x3", "f16"])
def test_capped_case_is_decidable_by_the_oracle_alone(mode):
    """The inputs of test_gpu_sample.py's capped test, with delta = 4 * TOL[mode]['logit'] / temperature: the restatement's own run
    skips fewer than 10 % of the steps, and the constructed trajectories of the first test exist (every step has an interval wider
    than 4 delta)."""
    c = S.whole_path_case()
    cands = S.case_candidates(c, mode)
    assert len(cands) <= 30 and gt.FlatTrie(gt.Trie(cands)).max_fanout <= 4
    delta = 4 * TOL[mode]["logit"] / 1.0
    tries = [O.Trie(cands)] * S.B
    res = S.walk(c["sd"], c["oc"], c["ids"], c["mask"], tries, S.R, S.MAX_LENGTH, top_k=50, uniforms=c["uniforms"])
    share = S.skipped_share(res, delta)
    print(f"[{mode}] delta {delta:.3g}: the oracle alone skips {share:.3f} of {(res['want'] >= 0).sum()} steps")
    assert share < 0.10
    built = S.walk(c["sd"], c["oc"], c["ids"], c["mask"], tries, S.R, S.MAX_LENGTH, top_k=50, delta=delta, rng=np.random.default_rng(S.SEED))
    assert len({tuple(r) for r in built["seq"].tolist()}) >= 2  # (more than one trajectory: the uniforms matter)
