"""CPU: the host side of the per-user item masks (include/gram_hip.h ``gram_user_mask_t``): the layout of
the new struct against the header, the argument errors of the new entry points (returned before any launch: no GPU needed),
gram_user_mask_words, every refusal of ``GRAM.generate(item_mask=)`` that needs no device, the folding of duplicate candidates, the
op's fake implementation, and the launch train of gram_generate_mask against gram_generate_items' at the same shape."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import gram_amd
from gram_amd import _lib
from gram_amd.utils import generation_trie as gt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_user_mask_struct_matches_the_header(tmp_path):
    """gram_user_mask_t against its ctypes mirror: total size and every field's offset from a C program compiled against the real
    header (gcc; no GPU); the ABI version and gram_user_items_t's size stay what they were"""
    st, cname = _lib.UserMask, "gram_user_mask_t"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gram_hip.h"', "int main(void) {",
             f'  printf("size %zu\\n", sizeof({cname}));', '  printf("items %zu\\n", sizeof(gram_user_items_t));',
             '  printf("abi %d\\n", GRAM_ABI_VERSION);']
    lines += [f'  printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in st._fields_]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    got = {k: int(v) for k, v in got.items()}
    assert got["size"] == C.sizeof(st) == 40
    want = {"leaf_lo": 0, "leaf_hi": 8, "words": 16, "stride": 24, "n_leaves": 32}
    assert [f for f, _ in st._fields_] == list(want)
    for f, _ in st._fields_:
        assert got[f] == getattr(st, f).offset == want[f], f
    assert got["items"] == C.sizeof(_lib.UserItems) == 40
    assert got["abi"] == _lib.ABI_VERSION == 7 == _lib.load().gram_abi_version()


def test_user_mask_words():
    lib = _lib.load()
    assert [lib.gram_user_mask_words(n) for n in (1, 31, 32, 33, 64)] == [1, 1, 2, 2, 3]
    assert lib.gram_user_mask_words(12101) == 12101 // 32 + 1 and lib.gram_user_mask_words(1 << 24) == (1 << 19) + 1
    assert lib.gram_user_mask_words(0) == _lib.E_ARG and lib.gram_user_mask_words(-4) == _lib.E_ARG


def test_argument_errors_without_gpu():
    """A null struct or array, n_leaves < 1, a stride below gram_user_mask_words(n_leaves), rowpos with rows_per_user != K: GRAM_E_ARG
    before any launch (the pointers are never dereferenced)"""
    lib = _lib.load()
    p = 0x1000  # (never dereferenced)
    good = dict(leaf_lo=p, leaf_hi=p, words=p, stride=3, n_leaves=64)
    bad = [dict(good, **{k: None}) for k in ("leaf_lo", "leaf_hi", "words")]
    bad += [dict(good, n_leaves=0), dict(good, n_leaves=-1), dict(good, stride=2), dict(good, stride=0), dict(good, n_leaves=65, stride=2)]
    st = _lib.BeamState(B=2, K=4, Tmax=5, length_penalty=1.0, eos=1, pad=0, tokens=p, node=p, beam_scores=p, seq=p, anc=p, done=p,
                        n_hyps=p, hyp_score=p, worst=p, hyp_len=p, hyp_tok=p, error=p)
    st1 = _lib.BeamState(B=2, K=1, Tmax=5, length_penalty=1.0, eos=1, pad=0, tokens=p, node=p, beam_scores=p, seq=p, anc=p, done=p,
                         n_hyps=p, hyp_score=p, worst=p, hyp_len=p, hyp_tok=p, error=p)
    trie = _lib.Trie(p, p, p, 10, 9, 3, 2)
    width = C.c_int32(0)

    def step(um, rpu=4, rowpos=None, pieces=2, st_=st):
        return lib.gram_beam_step_sparse_mask(C.byref(st_), C.byref(trie), p, p, p, 128, p, 256, 1, rpu, rowpos, pieces, um, None)

    def calls(um):
        u = C.byref(um) if um is not None else None
        return [
            lib.gram_generate_mask(None, p, p, 2, 1, 32, 4, 4, 5, 1.0, C.byref(trie), None, u, p, 1 << 20, p, p, C.byref(width), None),
            step(u), step(u, pieces=1),
            lib.gram_greedy_step_mask(C.byref(st1), C.byref(trie), p, 256, 1, u, None),
        ]

    assert calls(None) == [_lib.E_ARG] * 4
    for kw in bad:
        assert calls(_lib.UserMask(**kw)) == [_lib.E_ARG] * 4, kw
    ok = _lib.UserMask(**good)
    # good masks, other arguments wrong: still refused before any launch
    assert lib.gram_generate_mask(None, p, p, 2, 1, 32, 4, 4, 5, 1.0, C.byref(trie), None, C.byref(ok), p, 1 << 20, p, p, C.byref(width),
                                  None) == _lib.E_ARG  # (no model)
    assert step(C.byref(ok), rpu=1, rowpos=p) == _lib.E_ARG  # live rows: K rows per user
    assert step(C.byref(ok), rpu=2, rowpos=p) == _lib.E_ARG
    assert step(C.byref(ok), rpu=0) == _lib.E_ARG
    assert lib.gram_greedy_step_mask(C.byref(st), C.byref(trie), p, 256, 1, C.byref(ok), None) == _lib.E_ARG  # K != 1
    # the preparation: null arrays, sizes below 1, a mask row shorter than n_items, too many leaves, a record row too short
    prep = lib.gram_user_mask_prepare
    g = dict(mask=p, mask_stride=10, B=2, n_items=10, leaf_item=p, n_leaves=64, words=p, stride=3, count=p)
    order = ("mask", "mask_stride", "B", "n_items", "leaf_item", "n_leaves", "words", "stride", "count")
    for kw in (dict(mask=None), dict(leaf_item=None), dict(words=None), dict(count=None), dict(B=0), dict(n_items=0), dict(mask_stride=9),
               dict(n_leaves=0), dict(n_leaves=(1 << 24) + 1, stride=1 << 20), dict(stride=2), dict(words=p + 4)):
        a = dict(g, **kw)
        assert prep(*[a[k] for k in order], None) == _lib.E_ARG, kw


@pytest.fixture(scope="module")
def cpu_model():
    cfg = gram_amd.T5Config(vocab_size=256, d_model=128, d_ff=256, num_layers=1, num_decoder_layers=1, num_heads=2, max_item_num=3)
    return gram_amd.create_model("gram", cfg).eval()


CANDS = [[0, 5, 1], [0, 6, 7, 1], [0, 6, 8, 1], [0, 9, 1]]


def _call(model, **kw):
    args = dict(input_ids=torch.randint(2, 200, (2, 2, 32), generator=torch.Generator().manual_seed(3)),
                attention_mask=torch.ones(2, 2, 32, dtype=torch.bool), max_length=4,
                prefix_allowed_tokens_fn=gt.prefix_allowed_tokens_fn(gt.Trie(CANDS)), num_beams=4, candidates=CANDS,
                item_mask=torch.ones(2, 4, dtype=torch.bool))
    args.update(kw)
    return model.generate(**args)


def test_refusals_fire_before_the_device(cpu_model):
    """Every ValueError / NotImplementedError of generate(item_mask=) that does not read the mask's values, on a CPU-only model"""
    import numpy as np
    for bad in (torch.ones(4, dtype=torch.bool), torch.ones(2, 3, dtype=torch.bool), torch.ones(3, 4, dtype=torch.bool),
                torch.ones(2, 4, 1, dtype=torch.bool), torch.ones(4, 2, dtype=torch.uint8), torch.ones(2, 4), torch.ones(2, 4, dtype=torch.float16),
                [[1, 1, 1, 1], [1, 1, 1, 1]], np.ones((2, 4), dtype=np.uint8)):
        with pytest.raises(ValueError, match="item_mask must be a bool, uint8 or integer tensor of shape"):
            _call(cpu_model, item_mask=bad)
    with pytest.raises(ValueError, match="candidates"):
        _call(cpu_model, candidates=None)
    with pytest.raises(ValueError, match="closure"):
        _call(cpu_model, prefix_allowed_tokens_fn=lambda b, s: [1])
    for kw in (dict(exclude_items=[[0], [1]]), dict(allowed_items=[[0], [1]])):
        with pytest.raises(ValueError, match="fold those into the mask"):
            _call(cpu_model, **kw)
    with pytest.raises(NotImplementedError, match="do_sample"):
        _call(cpu_model, do_sample=True, num_beams=1, num_return_sequences=2)
    with pytest.raises(NotImplementedError, match="do_sample"):
        _call(cpu_model, do_sample=True, replacement=False, num_beams=1, num_return_sequences=2)
    with pytest.raises(NotImplementedError, match="num_beam_groups"):
        _call(cpu_model, num_beam_groups=2, diversity_penalty=0.5)
    with pytest.raises(NotImplementedError, match="item_bias"):
        _call(cpu_model, item_bias=torch.zeros(4))
    # a legal masked call passes every host check: a CPU model gets as far as the device and fails there
    for kw in (dict(), dict(item_mask=torch.ones(2, 4, dtype=torch.uint8)), dict(item_mask=torch.ones(2, 4, dtype=torch.int64)),
               dict(num_beams=1, num_return_sequences=1), dict(item_mask=torch.ones(4, 2, dtype=torch.int32).t())):
        with pytest.raises(Exception) as e:
            _call(cpu_model, **kw)
        assert not isinstance(e.value, (ValueError, NotImplementedError)), e.value


def test_mask_on_the_host_folds_duplicates_and_names_the_empty_user():
    """GRAM._user_item_mask on the CPU: non-zero -> 1; two spellings of one sequence are folded onto the candidate FlatTrie.leaf_items
    names (only where the Trie has fewer leaves than the list has entries); a row that keeps nothing is a ValueError with its index"""
    from gram_amd.model.gram import GRAM
    f = GRAM._user_item_mask
    flat = gt.FlatTrie(gt.Trie(CANDS))
    m = torch.tensor([[0, 7, 0, -1], [1, 0, 0, 0]], dtype=torch.int64)
    out = f(m, flat, CANDS, "cpu")
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.tolist() == [[0, 1, 0, 1], [1, 0, 0, 0]]
    assert f(m.to(torch.int32).t().contiguous().t(), flat, CANDS, "cpu").tolist() == out.tolist()  # (any strides)
    dup = CANDS + [list(CANDS[1]), list(CANDS[0])]  # candidates 4 and 5 spell 1 and 0 again
    flat2 = gt.FlatTrie(gt.Trie(dup))
    assert int(flat2.leaf_ranges()[1][0]) == 4 and flat2.leaf_items(dup).tolist() == [0, 1, 2, 3]
    only_second = torch.tensor([[0, 0, 0, 0, 1, 0], [0, 0, 1, 0, 0, 1]], dtype=torch.bool)
    assert f(only_second, flat2, dup, "cpu").tolist() == [[0, 1, 0, 0, 0, 0], [1, 0, 1, 0, 0, 0]]
    with pytest.raises(ValueError, match="item_mask leaves user 1 without any item"):
        f(torch.tensor([[1, 0, 0, 0], [0, 0, 0, 0]]), flat, CANDS, "cpu")
    with pytest.raises(ValueError, match="item_mask leaves user 0 without any item"):
        f(torch.zeros(2, 6, dtype=torch.uint8), flat2, dup, "cpu")


def test_without_item_mask_nothing_changes(cpu_model, monkeypatch):
    """item_mask=None reaches the plain op and never the new one; a mask reaches generate_mask with the folded uint8 tensor.  The
    ops are replaced: nothing touches a device."""
    import warnings
    from gram_amd import ops  # noqa: F401  (registered before torch.ops.gram is replaced)
    calls = []

    class Stop(Exception):
        pass

    def record(name):
        def op(*a, **k):
            calls.append((name, a))
            raise Stop(name)
        return op

    fake_ns = type("ns", (), {n: staticmethod(record(n)) for n in ("generate", "generate_items", "generate_mask")})
    monkeypatch.setattr(torch.ops, "gram", fake_ns, raising=False)
    m = cpu_model
    monkeypatch.setattr(type(m), "_pack", lambda self: 1)
    monkeypatch.setattr(type(m), "_device", lambda self: torch.device("cpu"))
    monkeypatch.setattr(type(m), "_plan", lambda self, ids, mask, B, N, Lp: (None, None))
    monkeypatch.setattr(type(m), "_get_workspace", lambda self, *a: torch.zeros(16, dtype=torch.uint8))
    monkeypatch.setattr(type(m), "_tail_plan", lambda self, *a, **k: (0, 0))
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the name is a parameter now: no "ignores the keyword argument"
        with pytest.raises(Stop, match="^generate$"):
            _call(m, item_mask=None)
    assert [c[0] for c in calls] == ["generate"]
    calls.clear()
    with pytest.raises(Stop, match="^generate_mask$"):
        _call(m, item_mask=torch.tensor([[0, 2, 0, 1], [1, 0, 0, 0]]))
    assert [c[0] for c in calls] == ["generate_mask"]
    mask = calls[0][1][-1]
    assert mask.dtype == torch.uint8 and mask.tolist() == [[0, 1, 0, 1], [1, 0, 0, 0]]
    assert calls[0][1][-2].tolist() == gt.FlatTrie(gt.Trie(CANDS)).leaf_items(CANDS).tolist()
    calls.clear()
    with pytest.raises(ValueError, match="item_mask leaves user 1 without any item"):  # (before the workspace, before any op)
        _call(m, item_mask=torch.tensor([[0, 2, 0, 1], [0, 0, 0, 0]]))
    assert calls == []


def test_generate_mask_op_traces_with_fake_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from gram_amd import ops
    assert "generate_mask" not in ops.__all__ and len(ops.__all__) == 12  # (reached as torch.ops.gram.generate_mask, like generate_groups)
    schema = str(torch.ops.gram.generate_mask.default._schema)
    assert schema.endswith("Tensor leaf_lo, Tensor leaf_hi, Tensor leaf_item, Tensor item_mask) -> (Tensor, Tensor, Tensor, Tensor)")
    with FakeTensorMode():
        ids = torch.zeros(3, 2, 32, dtype=torch.int64, device="cuda")
        t = torch.zeros(8, dtype=torch.int32, device="cuda")
        ws = torch.zeros(1024, dtype=torch.uint8, device="cuda")
        m = torch.zeros(3, 6, dtype=torch.uint8, device="cuda")
        s, sc, wd, cnt = torch.ops.gram.generate_mask(ids, ids.to(torch.uint8), 0, ws, t, t, t, 4, 3, 5, 5, 7, 1.0, None, None, None, None, None,
                                                      0, 0, t, t, t, m)
        assert s.shape == (15, 7) and s.dtype == torch.int64 and sc.shape == (15,) and sc.dtype == torch.float32 and wd.shape == (1,)
        assert cnt.shape == (3,) and cnt.dtype == torch.int32
        s, sc, wd, cnt = torch.ops.gram.generate_mask(ids, ids.to(torch.uint8), 0, ws, t, t, t, 4, 3, 1, 1, 7, 1.0, None, None, None, None, None,
                                                      0, 0, t, t, t, m)
        assert s.shape == (3, 7) and sc.shape == (0,)


# ------------------------------------------------------------------------------------ the launch train
STEP_NAMES = {"gram_beam_step_sparse_mask": "step", "gram_beam_step_sparse_items": "step", "gram_beam_step_sparse_split_items": "step",
              "gram_greedy_step_mask": "greedy", "gram_greedy_step_items": "greedy"}


def _normalised(lines):
    """A trace with the step functions' names mapped to one name and their filter operand (the last struct in braces) dropped; the
    mask step always carries both lm_head tables and the piece count, the list steps one table (and the piece count with two
    pieces): those operands are dropped from both sides too, so that what is left is the state, the Trie, the hidden rows, d, lse,
    V, cur_len, rows_per_user, rowpos and the stream."""
    out = []
    for ln in lines:
        name = ln.split(" ", 1)[0]
        if name not in STEP_NAMES:
            out.append(ln)
            continue
        structs = re.findall(r"\{[^}]*\}", ln)
        flat = re.sub(r"\{[^}]*\}", "@", ln).split()
        assert flat[1] == flat[2] == "@" and flat[-2] == "@" and len(structs) == 3, ln
        args = flat[3:-2] + flat[-1:]  # between the Trie and the filter, then the stream
        if STEP_NAMES[name] == "step":
            if name.endswith("_mask"):  # hidden lm16 lm32 d lse V cur_len rpu rowpos pieces
                args = args[:1] + args[3:9] + args[10:]
            elif "split" in name:  # hidden lm32 d lse V cur_len rpu rowpos pieces
                args = args[:1] + args[2:8] + args[9:]
            else:  # hidden lm16 d lse V cur_len rpu rowpos
                args = args[:1] + args[2:]
            assert len(args) == 8, ln
        out.append(" ".join([STEP_NAMES[name], structs[0], structs[1]] + args))
    return out


@pytest.mark.parametrize("pair", [("generate_p2_mask", "generate_p2_items"), ("generate_p1_mask", "generate_p1_items"),
                                  ("generate_greedy_mask", "generate_greedy_items")])
def test_launch_train_of_generate_mask_is_generate_items(pair):
    """gram_generate_mask's train equals gram_generate_items' at the same shape call for call -- encoder, bank, the shared step-0 row,
    the live-row compaction, the workspace offsets -- once the step functions' names are mapped and the filter operand is dropped"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "launch_trace")], check=True, capture_output=True, text=True)
    tool = os.path.join(ROOT, "gram_amd", "csrc", "build_trace", "launch_trace")
    a, b = (subprocess.run([tool, c], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines() for c in pair)
    assert a[-1] == b[-1] == "return 0"
    assert sum(ln.split(" ", 1)[0] in STEP_NAMES for ln in a) == 3 and any("_mask " in ln for ln in a) and not any("_mask " in ln for ln in b)
    assert _normalised(a) == _normalised(b)
