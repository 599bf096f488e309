"""CPU: the host side of beam search with per-item score biases (generate(item_bias=, bias_lookahead=)) --
the inputs of the whole-path GPU test (their decision margins, and that the bias and the lookahead act in them); the restatement's
potentials against a brute-force walk of the nested-dict Trie; the telescoping identity on the oracle; the zero bias against
O.beam_search; every refusal of ``GRAM.generate`` on a CPU model, i.e. before anything touches a device; that ``item_bias=None``
goes down the unchanged path; the new C entry points' argument errors; the ops' schemas and meta implementations."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import gram_amd
from gram_amd import _lib, ops  # noqa: F401
from gram_amd.utils import generation_trie as gt
from oracle import gram_oracle as O
from tests import bias_oracle as BO

RAGGED = [[0, 2, 3, 1], [0, 2, 4, 5, 1], [0, 2, 4, 6, 7, 1], [0, 3, 1], [0, 3, 8, 1], [0, 4, 9, 9, 9, 1], [0, 5, 1],
          [0, 6, 2, 1], [0, 6, 3, 1], [0, 7, 7, 1], [0, 8, 1], [0, 9, 2, 2, 1]]


def test_whole_path_cases_have_their_three_properties():
    cases = BO.whole_path_cases()
    assert [(c["B"], c["N"], c["L"], c["K"], c["per_user"]) for c in cases] == [
        (B, N, L, K, pu) for (B, N, L, K) in ((3, 2, 32, 4), (2, 3, 32, 6), (2, 1, 32, 20), (2, 2, 32, 8)) for pu in (False, True)]
    for c in cases:
        n = len(c["cands"])
        assert 40 <= n <= 200 and tuple(c["bias"].shape) == ((c["B"], n) if c["per_user"] else (n,))
        assert c["bias"].dtype == torch.float32 and float(c["bias"].abs().max()) <= 4.0
        m1, m0, bias_acts, look_acts = BO.case_properties(c)
        print(f"[whole-path case K={c['K']} per_user={c['per_user']} seed={c['seed']}] margin {m1:.2e} with lookahead, {m0:.2e} without")
        assert m1 >= BO.MIN_MARGIN and m0 >= BO.MIN_MARGIN, (c["K"], c["per_user"], m1, m0)  # (a)
        assert bias_acts, "the bias changes no user's list against the plain search"  # (b)
        assert look_acts, "the lookahead changes no user's list against leaf-only"  # (c)


@pytest.mark.parametrize("key", list(BO.WHOLE_PATH_SEEDS))
def test_a_cases_seed_is_the_first_that_qualifies(key):
    """the table is find_seed's answer: no earlier seed of 0, 1, 2, ... meets (a)-(c) (about 20 oracle runs over the eight cases)"""
    assert BO.WHOLE_PATH_SEEDS[key] == BO.find_seed(*key, limit=BO.WHOLE_PATH_SEEDS[key] + 1)


def _brute_force(cands, T, lookahead):
    """phi by walking the nested dict: a node's leaves are the sequences below it; the first candidate that spells one names it"""
    first = {}
    for i, c in enumerate(cands):
        first.setdefault(tuple(c), i)
    flat = BO.flat_trie(cands)
    T = np.asarray(T, dtype=np.float32).reshape(-1, len(cands))
    phi = np.zeros((T.shape[0], flat.n_nodes), dtype=np.float32)

    def walk(d, prefix):
        """-> the biases [rows][leaves below] of the node that `prefix` ends on"""
        node = flat.leaf_of(prefix)
        if not d:
            vals = T[:, [first[tuple(prefix)]]]
        else:
            vals = np.concatenate([walk(d[t], prefix + [t]) for t in sorted(d)], axis=1)
        if node > 0 and len(prefix) > 1 and (not d or lookahead):
            phi[:, node] = vals.max(axis=1)
        return vals

    walk(gt.Trie(cands).trie_dict, [])
    return phi


@pytest.mark.parametrize("lookahead", [True, False])
@pytest.mark.parametrize("rows", [1, 3])
def test_potentials_against_a_brute_force_walk(lookahead, rows):
    """ids of different depth (RAGGED), duplicate candidates (the first one's bias counts) and a random Trie"""
    g = torch.Generator().manual_seed(5 + rows)
    rand = BO.GO.random_cands(g, 60, 2, 4, 256)
    dup = RAGGED + [RAGGED[4], RAGGED[0], RAGGED[4]]
    for cands in (RAGGED, dup, rand, rand + rand[:7]):
        T = (torch.randn(rows, len(cands), generator=g) * 1.5).clamp_(-4, 4).numpy()
        phi = BO.potentials(cands, T if rows > 1 else T[0], lookahead)
        want = _brute_force(cands, T, lookahead)
        assert phi.dtype == np.float32 and phi.shape == want.shape
        assert np.array_equal(phi.view(np.uint32), want.view(np.uint32))
        flat = BO.flat_trie(cands)
        assert not phi[:, 0].any() and not phi[:, flat.leaf_of([0])].any()  # the root and the start node
        for i, c in enumerate(cands):  # a leaf carries the bias of the FIRST candidate that spells it
            j = min(k for k, o in enumerate(cands) if o == c)
            assert np.array_equal(phi[:, flat.leaf_of(c)], T[:, j]), (i, j)
        if lookahead:  # phi never rises along a path below the start node
            for c in cands:
                p = [phi[:, flat.leaf_of(c[:k])] for k in range(2, len(c) + 1)]
                assert all((a >= b).all() for a, b in zip(p, p[1:]))


def test_leaf_items_table():
    """FlatTrie.leaf_items: the candidate of every leaf rank, the first one among duplicates"""
    dup = RAGGED + [RAGGED[4], RAGGED[0]]
    flat = BO.flat_trie(dup)
    li = flat.leaf_items(dup)
    ranks = flat.item_ranks(dup)
    assert li.dtype == np.int32 and li.shape == (len(RAGGED),) and sorted(li.tolist()) == list(range(len(RAGGED)))
    assert all(li[ranks[i]] == min(i, dup.index(c)) for i, c in enumerate(dup))
    # a candidate list that leaves a leaf unnamed: -1 there
    part = flat.leaf_items(RAGGED[:5])
    assert sorted(part.tolist()) == [-1] * (len(RAGGED) - 5) + list(range(5))


@pytest.mark.parametrize("i", [1, 2, 5])
def test_telescoping_identity_on_the_oracle(i):
    """every returned score equals (sum of log p + T[item]) / len^lp: the edge terms along a path cancel"""
    c = BO.whole_path_cases()[i]
    sd = O.init_state_dict(c["cfg"], c["model_seed"])
    index = {tuple(s): k for k, s in enumerate(c["cands"])}
    for lookahead in (True, False):
        for lp in (1.0, 0.5):
            T = c["bias"].numpy()
            seqs, scores = BO.generate(sd, c["cfg"], c["input_ids"], c["attention_mask"], c["max_length"], c["cands"], c["K"], T,
                                       lookahead, lp, num_return_sequences=3)
            worst = 0.0
            for r, (row, sc) in enumerate(zip(seqs.tolist(), scores.tolist())):
                b = r // 3
                seq = row[: row.index(1) + 1]
                item = index[tuple(seq)]
                logp = O.sequence_logprob(sd, c["cfg"], c["input_ids"][b:b + 1], c["attention_mask"][b:b + 1], seq)
                t = float(T[b, item] if c["per_user"] else T[item])
                want = (logp + t) / (len(seq) - 1) ** lp  # (HF's length is the hypothesis without the EOS it ends on)
                worst = max(worst, abs(sc - want))
            assert worst <= 1e-5, (lookahead, lp, worst)


@pytest.mark.parametrize("K,lp", [(4, 1.0), (12, 0.7)])
def test_zero_bias_is_plain_beam_search(K, lp):
    B, V = 3, 128
    g = torch.Generator().manual_seed(7 + K)
    logits = [torch.randn(B * K, V, generator=g) * 2.0 for _ in range(max(len(c) for c in RAGGED) - 1)]
    it = iter(logits)
    ref = O.beam_search(lambda tok: next(it), lambda idx: None, B, K, max(len(c) for c in RAGGED), O.prefix_allowed_tokens_fn(O.Trie(RAGGED)),
                        lp, early_exit=False)
    for T in (None, np.zeros(len(RAGGED), dtype=np.float32)):
        got = BO.logits_search(logits, None, RAGGED, B, K, T, True, lp)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


@pytest.fixture(scope="module")
def cpu_model():
    cfg = gram_amd.T5Config(vocab_size=256, d_model=128, d_ff=256, num_layers=1, num_decoder_layers=1, num_heads=2, max_item_num=3)
    return gram_amd.create_model("gram", cfg).eval()


CANDS = [[0, 5, 1], [0, 6, 7, 1], [0, 6, 8, 1], [0, 9, 1]]


def _call(model, **kw):
    args = dict(input_ids=torch.randint(2, 200, (2, 2, 32), generator=torch.Generator().manual_seed(3)), attention_mask=torch.ones(2, 2, 32, dtype=torch.bool), max_length=4,
                prefix_allowed_tokens_fn=gt.prefix_allowed_tokens_fn(gt.Trie(CANDS)), num_beams=4, candidates=CANDS,
                item_bias=torch.zeros(4))
    args.update(kw)
    return model.generate(**args)


def test_refusals_fire_before_the_device(cpu_model):
    nan, inf = float("nan"), float("inf")
    # wrong shape or dtype
    for bad in (torch.zeros(3), torch.zeros(5), torch.zeros(3, 4), torch.zeros(1, 4), torch.zeros(2, 4, 1), torch.zeros(4, 2),
                torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float16), torch.zeros(4, dtype=torch.int32),
                [0.0, 0.0, 0.0, 0.0], np.zeros(4, dtype=np.float32)):
        with pytest.raises(ValueError, match="item_bias must be a float32 tensor of shape"):
            _call(cpu_model, item_bias=bad)
    # non-finite values
    for v in (nan, inf, -inf):
        with pytest.raises(ValueError, match="finite"):
            _call(cpu_model, item_bias=torch.tensor([0.0, v, 0.0, 0.0]))
        with pytest.raises(ValueError, match="finite"):
            _call(cpu_model, item_bias=torch.tensor([[0.0] * 4, [0.0, 0.0, 0.0, v]]))
    # a missing candidates
    with pytest.raises(ValueError, match="candidates"):
        _call(cpu_model, candidates=None)
    with pytest.raises(NotImplementedError, match="do_sample"):
        _call(cpu_model, do_sample=True, num_beams=1, num_return_sequences=2)
    with pytest.raises(NotImplementedError, match="do_sample"):
        _call(cpu_model, do_sample=True, replacement=False, num_beams=1, num_return_sequences=2)
    with pytest.raises(NotImplementedError, match="num_beam_groups"):
        _call(cpu_model, num_beam_groups=2, diversity_penalty=0.5)
    with pytest.raises(NotImplementedError, match="num_beams=2, num_return_sequences=1"):
        _call(cpu_model, num_beams=1)
    with pytest.raises(NotImplementedError, match="closure"):
        _call(cpu_model, prefix_allowed_tokens_fn=lambda b, s: [1])
    # a legal biased call passes every host check: a CPU model gets as far as the device and fails there
    for kw in (dict(), dict(item_bias=torch.zeros(2, 4)), dict(bias_lookahead=False), dict(num_beams=2, num_return_sequences=1),
               dict(exclude_items=[[0], [1]]), dict(item_bias=torch.full((4,), 3.5))):
        with pytest.raises(Exception) as e:
            _call(cpu_model, **kw)
        assert not isinstance(e.value, (ValueError, NotImplementedError)), e.value


def test_item_bias_none_is_the_unchanged_path(cpu_model, monkeypatch):
    """item_bias=None (with or without bias_lookahead) reaches the plain op with the plain arguments and never the new ones; a
    bias reaches item_bias_table and generate_bias.  The ops are replaced: nothing touches a device."""
    calls = []

    class Stop(Exception):
        pass

    def record(name):
        def op(*a, **k):
            calls.append((name, a))
            raise Stop(name)
        return op

    fake_ns = type("ns", (), {n: staticmethod(record(n)) for n in
                              ("generate", "generate_items", "generate_groups", "generate_bias", "item_bias_table")})
    monkeypatch.setattr(torch.ops, "gram", fake_ns, raising=False)
    m = cpu_model
    monkeypatch.setattr(type(m), "_pack", lambda self: 1)
    monkeypatch.setattr(type(m), "_device", lambda self: torch.device("cpu"))
    monkeypatch.setattr(type(m), "_plan", lambda self, ids, mask, B, N, Lp: (None, None))
    monkeypatch.setattr(type(m), "_get_workspace", lambda self, *a: torch.zeros(16, dtype=torch.uint8))
    monkeypatch.setattr(type(m), "_tail_plan", lambda self, *a, **k: (0, 0))
    import warnings
    plain_args = []
    for kw in (dict(), dict(bias_lookahead=False), dict(bias_lookahead=True)):
        calls.clear()
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # the two names are parameters now: no "ignores the keyword argument"
            with pytest.raises(Stop, match="^generate$"):
                _call(m, item_bias=None, **kw)
        assert [c[0] for c in calls] == ["generate"]
        plain_args.append(calls[0][1])
    for a in plain_args[1:]:
        assert len(a) == len(plain_args[0]) and all((x is y) or (not isinstance(x, torch.Tensor) and x == y) or
                                                    (isinstance(x, torch.Tensor) and torch.equal(x, y)) for x, y in zip(a, plain_args[0]))
    calls.clear()
    with pytest.raises(Stop, match="item_bias_table"):
        _call(m, item_bias=torch.ones(4))
    name, a = calls[0]
    assert name == "item_bias_table" and tuple(a[0].shape) == (1, 4) and a[0].dtype == torch.float32 and a[-1] is True and a[-2] == 0
    assert a[1].tolist() == gt.FlatTrie(gt.Trie(CANDS)).leaf_items(CANDS).tolist()


def test_argument_errors_without_gpu():
    """judged on the host before any launch: callable without a GPU, the pointers are never dereferenced"""
    lib = _lib.load()
    fake = C.c_void_p(0x1000)
    trie = _lib.Trie(0x1000, 0x1000, 0x1000, 40, 39, 3, 2)
    st = _lib.BeamState(B=2, K=4, Tmax=6, length_penalty=1.0, eos=1, pad=0)
    E = _lib.E_ARG
    # no potentials; a per-user stride shorter than a row
    assert lib.gram_beam_step_bias(C.byref(st), C.byref(trie), fake, fake, 128, 1, 4, None, 0, None, None) == E
    assert lib.gram_beam_step_bias(C.byref(st), C.byref(trie), fake, fake, 128, 1, 4, fake, 39, None, None) == E
    assert lib.gram_beam_step_bias(C.byref(st), C.byref(trie), fake, fake, 128, 1, 4, fake, -1, None, None) == E
    assert lib.gram_beam_step_bias(C.byref(st), C.byref(trie), None, fake, 128, 1, 4, fake, 0, None, None) == E  # no logits
    assert lib.gram_beam_step_bias(C.byref(st), None, fake, fake, 128, 1, 4, fake, 0, None, None) == E
    assert lib.gram_beam_step_bias(None, C.byref(trie), fake, fake, 128, 1, 4, fake, 0, None, None) == E
    sparse = lambda phi, stride, hidden=fake, state=st: lib.gram_beam_step_bias_sparse(  # noqa: E731
        C.byref(state) if state is not None else None, C.byref(trie), hidden, fake, None, 128, fake, 128, 1, 4, None, 1, phi, stride, None, None)
    assert sparse(None, 0) == E and sparse(fake, 39) == E and sparse(fake, 0, hidden=None) == E and sparse(fake, 0, state=None) == E
    bad_items = _lib.UserItems(0x1000, 0x1000, 0x1000, 0x1000, 0, _lib.ITEMS_EXCLUDE)  # stride 0
    assert lib.gram_beam_step_bias(C.byref(st), C.byref(trie), fake, fake, 128, 1, 4, fake, 0, C.byref(bad_items), None) == E
    gen = lambda K, phi, stride, items=None: lib.gram_generate_bias(  # noqa: E731
        fake, fake, fake, 2, 2, 32, K, K, 6, 1.0, C.byref(trie), None, phi, stride, items, fake, 1 << 30, fake, fake, None, None)
    assert gen(1, fake, 0) == E and gen(4, None, 0) == E and gen(4, fake, 39) == E and gen(4, fake, 0, C.byref(bad_items)) == E
    good = dict(bias=fake, stride=12, rows=1, n_items=12, leaf_item=fake, n_leaves=12, lo=fake, hi=fake, trie=C.byref(trie), start=0,
                look=1, phi=fake, stream=None)  # (in the entry's argument order)
    tab = lambda **k: lib.gram_item_bias_table(*dict(good, **k).values())  # noqa: E731
    for k in (dict(bias=None), dict(leaf_item=None), dict(lo=None), dict(hi=None), dict(trie=None), dict(phi=None), dict(rows=0),
              dict(rows=65536), dict(n_items=0), dict(n_leaves=0), dict(rows=2, stride=11), dict(stride=-1)):
        assert tab(**k) == E, k


def test_op_schemas_and_fakes():
    assert "generate_bias" not in ops.__all__ and "item_bias_table" not in ops.__all__
    schema = str(torch.ops.gram.generate_bias.default._schema)
    assert schema.startswith("gram::generate_bias(Tensor input_ids, Tensor attention_mask, SymInt handle, Tensor(a3!) workspace, ")
    assert "float length_penalty, Tensor phi, Tensor? comp_map" in schema
    assert schema.endswith("Tensor? leaf_lo=None, Tensor? leaf_hi=None, Tensor? item_rank=None, Tensor? items=None, bool allow=False)"
                           " -> (Tensor, Tensor, Tensor)")
    assert str(torch.ops.gram.item_bias_table.default._schema).endswith("SymInt start_token, bool lookahead) -> Tensor")
    I32, I64, U8, F32 = torch.int32, torch.int64, torch.uint8, torch.float32
    with FakeTensorMode():
        def e(*shape, dtype=I32):
            return torch.empty(*shape, dtype=dtype, device="cuda")
        B, K, nret, T = 3, 6, 4, 7
        ids, ws, t = e(B, 2, 32, dtype=I64), e(1024, dtype=U8), e(8)
        phi = torch.ops.gram.item_bias_table(e(B, 11, dtype=F32), e(5), e(7), e(7), t, t, t, 4, 3, 0, True)
        assert tuple(phi.shape) == (B, 7) and phi.dtype == F32 and phi.device.type == "cuda"
        head = (ids, ids.to(U8), 0, ws, t, t, t, 4, 3, K, nret, T, 1.0, phi, None, None, None, None, None, 0, 0)
        for got in (torch.ops.gram.generate_bias(*head), torch.ops.gram.generate_bias(*head, t, t, t, e(B, 6), True)):
            s, sc, wd = got
            assert tuple(s.shape) == (B * nret, T) and s.dtype == I64 and s.device.type == "cuda"
            assert tuple(sc.shape) == (B * nret,) and sc.dtype == F32
            assert tuple(wd.shape) == (1,) and wd.dtype == I32 and wd.device.type == "cpu"
