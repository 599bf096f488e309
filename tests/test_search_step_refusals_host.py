"""CPU: every refusal of the eleven ``gram_beam_step*`` entry points, side by side (beam.hip: the entry points' own checks and the
one launcher's behind them).  Each entry point has one well-formed call; every case below changes it in one respect and must get
GRAM_E_ARG back before anything is launched -- the pointers are never dereferenced, so no GPU is needed.

The table states what is refused TODAY, entry point by entry point, the differences included:
  * ``rowpos`` with ``rows_per_user != K`` is refused wherever both exist except by gram_beam_step_sparse_split, which has never
    judged it (not listed there);
  * the group step refuses ``K * V > INT32_MAX`` and ``max_fanout > V`` always, the plain step only where the shape takes the
    streamed kernel (``K * max_fanout > 16 384``).

Everything here rests on the well-formed call (BASE with STATE, TRIE, ITEMS, MASK and each entry point's own changes) being one
that NO check refuses: were it refusable, every case would pass vacuously.  It cannot be shown here, because a call that passes the
checks launches, and these pointers must never reach a kernel (for the same reason there is no GPU companion that calls it: it would
need a whole step's real operands, which is what tests/test_gpu_kernels.py and its siblings do).  So it was read against every
check of the entry points and the launcher; whoever adds a check adds to BASE what satisfies it.  What the test does hold is that
each case is BASE changed in keys it names, at least one, and in no other.
"""
import ctypes as C

import pytest

from gram_amd import _lib

P = 0x1000  # (never dereferenced)
NAN, INF = float("nan"), float("inf")

STATE = dict(B=2, K=4, Tmax=6, length_penalty=1.0, eos=1, pad=0, tokens=P, node=P, beam_scores=P, seq=P, anc=P, done=P, n_hyps=P,
             hyp_score=P, worst=P, hyp_len=P, hyp_tok=P, error=P)
TRIE = dict(child_off=P, child_tok=P, child_node=P, n_nodes=10, n_edges=9, max_fanout=3, min_seq_len=2)
ITEMS = dict(leaf_lo=P, leaf_hi=P, ranks=P, count=P, stride=8, mode=0)
MASK = dict(leaf_lo=P, leaf_hi=P, words=P, stride=3, n_leaves=64)
STRUCTS = {"st": _lib.BeamState, "tr": _lib.Trie, "items": _lib.UserItems, "mask": _lib.UserMask}

# the well-formed call: every entry point reads its arguments from here, by name
BASE = dict(st=STATE, tr=TRIE, logits=P, hidden=P, lm16=P, lm32=P, d=128, lse=P, V=256, cur_len=1, rpu=4, rowpos=None, pieces=1, G=2,
            lam=0.5, phi=P, phi_stride=10, items=None, mask=MASK, stream=None)

# entry point -> (its parameters in order, what its well-formed call changes in BASE)
ENTRIES = {
    "gram_beam_step": ("st tr logits lse V cur_len rpu stream", {}),
    "gram_beam_step_sparse": ("st tr hidden lm16 d lse V cur_len rpu stream", {}),
    "gram_beam_step_sparse_live": ("st tr hidden lm16 d lse V cur_len rowpos stream", dict(rowpos=P)),
    "gram_beam_step_sparse_split": ("st tr hidden lm32 d lse V cur_len rpu rowpos pieces stream", dict(pieces=2)),
    "gram_beam_step_sparse_items": ("st tr hidden lm16 d lse V cur_len rpu rowpos items stream", dict(items=ITEMS)),
    "gram_beam_step_sparse_split_items": ("st tr hidden lm32 d lse V cur_len rpu rowpos pieces items stream",
                                          dict(pieces=2, items=ITEMS)),
    "gram_beam_step_sparse_mask": ("st tr hidden lm16 lm32 d lse V cur_len rpu rowpos pieces mask stream", {}),
    "gram_beam_step_groups": ("st tr logits lse V cur_len rpu G lam stream", {}),
    "gram_beam_step_groups_sparse": ("st tr hidden lm16 lm32 d lse V cur_len rpu rowpos pieces G lam items stream", {}),
    "gram_beam_step_bias": ("st tr logits lse V cur_len rpu phi phi_stride items stream", {}),
    "gram_beam_step_bias_sparse": ("st tr hidden lm16 lm32 d lse V cur_len rpu rowpos pieces phi phi_stride items stream", {}),
}


def _beams(K, **kw):
    """a state of K beams and the K rows per user that go with it"""
    return dict(st=dict(STATE, K=K), rpu=K, **kw)


def _cases(name):
    """the malformed calls of one entry point: (what is wrong, what it changes in the well-formed call)"""
    keys, own = ENTRIES[name]
    keys = keys.split()
    good = dict(BASE, **own)
    has = lambda *ks: all(k in keys for k in ks)  # noqa: E731
    c = []
    # null operands
    c += [(f"{k} = NULL", {k: None}) for k in ("st", "tr", "logits", "hidden", "lse", "phi", "mask") if has(k)]
    if has("items") and good["items"] is not None:
        c.append(("items = NULL", dict(items=None)))
    if name == "gram_beam_step_sparse_live":
        c.append(("rowpos = NULL", dict(rowpos=None)))
    if has("lm16", "lm32"):
        c.append(("no lm_head at all", dict(lm16=None, lm32=None)))
        c.append(("two pieces without lm_head_f32", dict(pieces=2, lm32=None)))
    elif has("lm16"):
        c.append(("lm_head_bf16 = NULL", dict(lm16=None)))
    else:
        c += [("lm_head_f32 = NULL", dict(lm32=None))] if has("lm32") else []
    # the state and the shape
    c += [(f"state {kw}", dict(st=dict(STATE, **kw))) for kw in (dict(B=0), dict(K=0), dict(K=65), dict(Tmax=1), dict(Tmax=65))]
    c += [(f"cur_len = {v}", dict(cur_len=v)) for v in (0, -1, 6, 7)]
    c += [(f"V = {v}", dict(V=v)) for v in (1, 0, -256)]
    c.append(("max_fanout < 0", dict(tr=dict(TRIE, max_fanout=-1))))
    if has("rpu"):
        c += [(f"rows_per_user = {v} (K = 4)", dict(rpu=v)) for v in (0, 2, 3, 5, -4)]
    if has("rpu", "rowpos") and name != "gram_beam_step_sparse_split":
        c += [(f"rowpos with rows_per_user = {v}", dict(rowpos=P, rpu=v)) for v in (1, 2)]
    if has("pieces"):
        c += [(f"pieces = {v}", dict(pieces=v)) for v in (0, -1, 3)]
    if has("d"):
        c += [(f"d = {v}", dict(d=v)) for v in (0, 32, 96, 100, 127, 129, -64)]
        if has("pieces", "lm32"):
            c.append(("two pieces, d = 96", dict(pieces=2, d=96)))
    # the group search: (K, G, penalty), and the limits of the kernel's 32-bit state at every shape
    if has("G"):
        for K, G, lam in [(4, 0, 1.0), (4, -1, 1.0), (4, 8, 1.0), (4, 3, 1.0), (6, 4, 1.0), (4, 2, -1.0), (4, 2, NAN), (4, 2, INF), (4, 2, -INF)]:
            c.append((f"(K, G, penalty) = ({K}, {G}, {lam})", _beams(K, G=G, lam=lam)))
        c.append(("K * V > INT32_MAX", _beams(64, V=1 << 26)))
        c.append(("K * V > INT32_MAX, one group", _beams(64, V=1 << 26, G=1)))
        c.append(("max_fanout > V", dict(V=2)))
    else:
        # the plain step judges them where the candidates stream: K * max_fanout = 19 200 > 16 384
        c.append(("streamed, K * V > INT32_MAX", _beams(64, V=1 << 26, tr=dict(TRIE, max_fanout=300))))
        c.append(("streamed, max_fanout > V", _beams(64, tr=dict(TRIE, max_fanout=300))))
    if has("phi_stride"):
        c += [(f"phi_stride = {v} (n_nodes = 10)", dict(phi_stride=v)) for v in (9, 1, -1)]
    if has("items"):
        c += [(f"items.{k} = NULL", dict(items=dict(ITEMS, **{k: None}))) for k in ("leaf_lo", "leaf_hi", "ranks", "count")]
        c += [(f"items {kw}", dict(items=dict(ITEMS, **kw))) for kw in (dict(stride=0), dict(stride=-1), dict(stride=4097), dict(mode=2),
                                                                         dict(mode=-1))]
    if has("mask"):
        c += [(f"mask.{k} = NULL", dict(mask=dict(MASK, **{k: None}))) for k in ("leaf_lo", "leaf_hi", "words")]
        c += [(f"mask {kw}", dict(mask=dict(MASK, **kw))) for kw in (dict(n_leaves=0), dict(n_leaves=-1), dict(stride=2), dict(stride=0),
                                                                     dict(n_leaves=65, stride=2), dict(words=P + 4))]
    if not has("rpu"):  # (gram_beam_step_sparse_live: always K rows per user)
        c = [(what, {k: v for k, v in change.items() if k != "rpu"}) for what, change in c]
    return keys, good, c


def _differs(a, b):
    return not (a == b or (a != a and b != b))  # (NaN is no change of NaN)


def call(lib, name, keys, args):
    """one call of an entry point from named arguments; the structs are built here and outlive the call"""
    keep = {k: STRUCTS[k](**args[k]) for k in STRUCTS if k in keys and args[k] is not None}
    return getattr(lib, name)(*[(C.byref(keep[k]) if k in keep else None) if k in STRUCTS else args[k] for k in keys])


@pytest.mark.parametrize("name", list(ENTRIES))
def test_malformed_calls_are_refused_before_any_launch(name):
    lib = _lib.load()
    keys, good, cases = _cases(name)
    assert len(cases) >= 20 and len({what for what, _ in cases}) == len(cases), name
    for what, change in cases:
        assert set(change) <= set(keys), (name, what)  # (a case changes only what the entry point takes)
        args = dict(good, **change)
        # the case is the well-formed call in every key but the ones it names, and differs from it in at least one of those
        changed = {k for k in good if _differs(args[k], good[k])}
        assert changed and changed <= set(change), (name, what)
        assert call(lib, name, keys, args) == _lib.E_ARG, (name, what)


def test_the_table_covers_the_eleven_entry_points():
    steps = sorted(n for n in _lib.SIGNATURES if n.startswith("gram_beam_step"))
    assert steps == sorted(ENTRIES) and len(steps) == 11
    for name, (keys, _) in ENTRIES.items():
        assert len(keys.split()) == len(_lib.SIGNATURES[name][1]), name
