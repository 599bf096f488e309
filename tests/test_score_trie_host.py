"""CPU: the host side of scoring every catalogue item in one decoder pass over the Trie (gram_score_trie, GRAM.score_all_items) --
FlatTrie.decoder_rows against a brute-force walk, its refusals, the C ABI's argument checks (no GPU needed: refused before any
launch), the launch train against the teacher-forced pass's for the same row count, and full_ranking against a NumPy restatement."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest
import torch

from gram_amd import _lib
from gram_amd.utils import generation_trie as gt
from gram_amd.utils.evaluate import full_ranking, ndcg_at_k
from tests.test_teacher_forced_host import _fake_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_train")
TOOL = os.path.join(ROOT, "gram_amd", "csrc", "build_trace", "launch_trace")


# ---------------------------------------------------------------------------------------------------------- decoder_rows
def _brute(cands, start=0):
    """The row tables by a plain Python walk: prefixes of length 1..len-1 are the rows, ordered by (depth, tokens) -- the flat Trie's
    breadth-first numbering with children in token order."""
    cands = [tuple(c) for c in cands]
    assert all(c[0] == start for c in cands)
    internal = sorted({c[:n] for c in cands for n in range(1, len(c))}, key=lambda p: (len(p), p))
    row = {p: i for i, p in enumerate(internal)}
    leaves = sorted(set(cands))
    return internal, row, leaves


def _check_rows(cands, flat):
    r = flat.decoder_rows()
    internal, row, leaves = _brute(cands)
    assert r.Q == len(internal) == len(r.tokens) == len(r.pos) == len(r.row_node) and r.anc.shape == (r.Q, r.Tq)
    assert r.n_leaves == len(leaves) and r.n_nodes == flat.n_nodes == 1 + len(internal) + len(leaves)
    fan = np.diff(flat.child_off)
    assert r.Q == int(((fan > 0) & (np.arange(flat.n_nodes) > 0)).sum())  # the internal nodes below the root
    assert r.Tq == max(len(p) for p in internal)
    assert [int(t) for t in r.tokens] == [p[-1] for p in internal]
    assert [int(t) for t in r.pos] == [len(p) - 1 for p in internal]
    assert (np.diff(r.pos) >= 0).all()  # every depth contiguous
    assert (r.anc[np.arange(r.Q), r.pos] == np.arange(r.Q)).all()
    for i, p in enumerate(internal):
        assert [int(a) for a in r.anc[i, : len(p)]] == [row[p[: j + 1]] for j in range(len(p))]
        assert flat.leaf_of(p) == int(r.row_node[i])
    assert ((r.anc >= 0) & (r.anc < r.Q)).all()
    # node tables: every non-root node hangs below the row of its parent with its own token; leaves carry their lexicographic rank
    assert int(r.node_row[0]) == -1 and int(r.node_row[r.row_node[0]]) == -1 and int(r.node_leaf[0]) == -1
    for i, p in enumerate(internal[1:], 1):
        n = int(r.row_node[i])
        assert int(r.node_row[n]) == row[p[:-1]] and int(r.node_tok[n]) == p[-1] and int(r.node_leaf[n]) == -1
    for k, c in enumerate(leaves):
        n = flat.leaf_of(c)
        assert int(r.node_leaf[n]) == k and int(r.node_row[n]) == row[c[:-1]] and int(r.node_tok[n]) == c[-1]
    assert sorted(int(x) for x in r.node_leaf if x >= 0) == list(range(len(leaves)))
    assert flat.decoder_rows() is r  # cached


def _random_cands(rng, n, lo, hi, vocab, fan1=False):
    """n candidates [0, ..., 1] of lo..hi tokens over `vocab` body tokens (EOS = 1 only at the end: no candidate is another's prefix)"""
    out = []
    for _ in range(n):
        ln = rng.randint(lo, hi)
        body = [rng.randint(2, 2 + vocab - 1) for _ in range(ln - 2)]
        out.append([0] + body + [1])
    return out


@pytest.mark.parametrize("seed,n,lo,hi,vocab", [(0, 40, 3, 9, 3), (1, 300, 3, 6, 400), (2, 25, 2, 64, 2), (3, 1, 64, 64, 5),
                                                 (4, 500, 3, 4, 300), (5, 60, 2, 12, 1)])
def test_decoder_rows_equal_a_brute_force_walk(seed, n, lo, hi, vocab):
    """vocab 1: chains, fan-out 1 everywhere; vocab 300-400 with short ids: fan-outs of hundreds below the start token"""
    rng = random.Random(seed)
    cands = _random_cands(rng, n, lo, hi, vocab)
    cands += cands[: max(1, n // 5)]  # duplicate candidates
    by_seq = gt.FlatTrie(gt.Trie(cands))
    _check_rows(cands, by_seq)
    by_dict = gt.FlatTrie(gt.Trie.load_from_dict(gt.Trie(cands).trie_dict))
    _check_rows(cands, by_dict)
    a, b = by_seq.decoder_rows(), by_dict.decoder_rows()
    for f in gt.DecoderRows.ARRAYS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    if vocab >= 300:
        assert by_seq.max_fanout >= 100


def test_decoder_rows_of_a_single_candidate():
    r = gt.FlatTrie(gt.Trie([[0, 1]])).decoder_rows()
    assert (r.Q, r.Tq, r.n_nodes, r.n_leaves) == (1, 1, 3, 1)
    assert r.tokens.tolist() == [0] and r.pos.tolist() == [0] and r.anc.tolist() == [[0]] and r.row_node.tolist() == [1]
    assert r.node_row.tolist() == [-1, -1, 0] and r.node_tok.tolist()[1:] == [0, 1] and r.node_leaf.tolist() == [-1, -1, 0]
    for a in gt.DecoderRows.ARRAYS:
        assert getattr(r, a).dtype == np.int32


def test_decoder_rows_refusals():
    with pytest.raises(ValueError, match="start token"):
        gt.FlatTrie(gt.Trie([[5, 6, 1]])).decoder_rows()  # no start child under the root
    with pytest.raises(ValueError, match="other than"):
        gt.FlatTrie(gt.Trie([[0, 6, 1], [5, 6, 1]])).decoder_rows()  # a second child under the root
    with pytest.raises(ValueError, match="start token"):
        gt.FlatTrie(gt.Trie([[0, 6, 1]])).decoder_rows(start_token=3)
    ok = [0] + [2] * (_lib.GRAM_MAX_DEC_LEN - 1) + [1]  # GRAM_MAX_DEC_LEN labels: the deepest row sits at the last position
    assert gt.FlatTrie(gt.Trie([ok])).decoder_rows().Tq == _lib.GRAM_MAX_DEC_LEN
    with pytest.raises(ValueError, match="GRAM_MAX_DEC_LEN"):
        gt.FlatTrie(gt.Trie([[0] + [2] * _lib.GRAM_MAX_DEC_LEN + [1]])).decoder_rows()


# ---------------------------------------------------------------------------------------------------------- the C ABI's refusals
def test_score_trie_argument_errors_without_gpu():
    lib, h = _fake_model()
    f = 0x1000
    E = _lib.E_ARG

    def rows(**kw):
        d = dict(tokens=f, pos=f, anc=f, row_node=f, node_row=f, node_tok=f, node_leaf=f, Q=12, Tq=4, n_nodes=40, n_leaves=27)
        d.update(kw)
        return _lib.TrieRows(**d)

    try:
        good = [lib.gram_workspace_bytes_trie(h, b, 3, 32, 200) for b in (1, 2, 3, 8)]
        assert good[0] > 0 and all(x < y for x, y in zip(good, good[1:]))  # monotone in B
        # and in Q: never smaller, and growing once the decoder's rows outweigh the encoder's, whose bytes they share
        by_q = [lib.gram_workspace_bytes_trie(h, 2, 3, 32, q) for q in (1, 12, 64, 65, 1000, 5000, 20000)]
        assert by_q[0] > 0 and all(x <= y for x, y in zip(by_q, by_q[1:])) and by_q[-3] < by_q[-2] < by_q[-1]
        assert lib.gram_workspace_bytes_trie(h, 2, 3, 32, 12) > lib.gram_workspace_bytes_tf(h, 2, 3, 32, 12, 1)  # + the two row tables
        assert lib.gram_workspace_bytes_trie(None, 2, 3, 32, 12) == E
        assert lib.gram_workspace_bytes_trie(h, 0, 3, 32, 12) == E
        assert lib.gram_workspace_bytes_trie(h, 2, 3, 32, 0) == E  # Q < 1
        assert lib.gram_workspace_bytes_trie(h, 2, 3, 48, 12) == E  # L % 32
        assert lib.gram_workspace_bytes_trie(h, 2, 9, 32, 12) == E  # N > max_passages
        assert lib.gram_workspace_bytes_trie(h, 1 << 16, 1, 32, 1 << 16) == E  # more rows than one call indexes
        trie = _lib.Trie(f, f, f, 40, 39, 3, 2)
        ws = 1 << 40

        def call(r, t=trie, ids=f, mask=f, leaf=f, B=2, wsb=ws, m=h):
            return lib.gram_score_trie(m, ids, mask, B, 3, 32, None, C.byref(t) if t else None, C.byref(r) if r else None, f, wsb, leaf,
                                       None, None)

        assert call(None) == E and call(rows(), t=None) == E and call(rows(), m=None) == E
        assert call(rows(), mask=None) == E and call(rows(), leaf=None) == E and call(rows(), ids=None) == E
        for field in gt.DecoderRows.ARRAYS:
            assert call(rows(**{field: None})) == E, field
        assert call(rows(Q=0)) == E and call(rows(Tq=0)) == E and call(rows(Tq=_lib.GRAM_MAX_DEC_LEN + 1)) == E
        assert call(rows(n_nodes=41)) == E  # not the Trie's node count
        assert call(rows(n_leaves=0)) == E and call(rows(n_leaves=40)) == E
        assert call(rows(), B=0) == E
        assert call(rows(), wsb=1024) == _lib.E_WORKSPACE  # too small a workspace: also before any launch
    finally:
        lib.gram_model_destroy(h)
    # the kernels' own entry points
    tree = lambda **kw: lib.gram_dec_self_attn_tree_split(*[{**dict(qkv=f, pos=f, anc=f, bias=f, out=f, B=2, Q=12, Tq=4, H=2, pieces=1,  # noqa: E731
                                                                    ps=0, st=None), **kw}[k]
                                                            for k in ("qkv", "pos", "anc", "bias", "out", "B", "Q", "Tq", "H", "pieces", "ps", "st")])
    for p in ("qkv", "pos", "anc", "bias", "out"):
        assert tree(**{p: None}) == E, p
    assert tree(Tq=0) == E and tree(Tq=_lib.GRAM_MAX_DEC_LEN + 1) == E
    assert tree(H=0) == E and tree(H=17) == E and tree(pieces=0) == E and tree(pieces=3) == E
    assert tree(B=0) == E and tree(Q=0) == E
    assert tree(pieces=2, ps=2 * 12 * 3 * 2 * 64 - 1) == E  # a piece stride shorter than the rows
    assert lib.gram_trie_repeat_tokens(None, f, 2, 12, None) == E and lib.gram_trie_repeat_tokens(f, None, 2, 12, None) == E
    assert lib.gram_trie_repeat_tokens(f, f, 0, 12, None) == E and lib.gram_trie_repeat_tokens(f, f, 2, 0, None) == E
    leaf = lambda r, **kw: lib.gram_trie_leaf_logprob_split(*[{**dict(h=f, e16=f, e32=None, d=128, lse=f, r=C.byref(r) if r else None, B=2,  # noqa: E731
                                                                      V=256, pieces=1, edge=f, leaf=f, node=None, st=None), **kw}[k]
                                                              for k in ("h", "e16", "e32", "d", "lse", "r", "B", "V", "pieces", "edge", "leaf",
                                                                        "node", "st")])
    assert leaf(None) == E
    for p in ("h", "lse", "edge", "leaf", "e16"):
        assert leaf(rows(), **{p: None}) == E, p
    assert leaf(rows(), pieces=2) == E  # two pieces need the fp32 table
    assert leaf(rows(), d=100) == E and leaf(rows(), B=0) == E and leaf(rows(), V=0) == E and leaf(rows(), pieces=3) == E
    assert leaf(rows(Tq=65)) == E and leaf(rows(Q=0)) == E and leaf(rows(node_leaf=None)) == E and leaf(rows(n_leaves=0)) == E


def test_trie_rows_struct_matches_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gram_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(gram_trie_rows_t));']
    lines += [f'  printf("{n} %zu\\n", offsetof(gram_trie_rows_t, {n}));' for n, _ in _lib.TrieRows._fields_]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.TrieRows)
    for n, _ in _lib.TrieRows._fields_:
        assert int(got[n]) == getattr(_lib.TrieRows, n).offset, n


# ---------------------------------------------------------------------------------------------------------- launch train
@pytest.mark.parametrize("trie_case,tf_case", [("score_trie_folded", "tf_folded"), ("score_trie_p2", "tf_p2")])
def test_launch_train_is_the_teacher_forced_one_with_the_tree_kernels(trie_case, tf_case):
    """gram_score_trie over Q = 12 rows per user against gram_teacher_forced over C * T = 3 * 4: the same 24 rows, the same workspace
    offsets.  Line for line the same train, except: the tokens are repeated per user first (and the embedding reads that copy), every
    self-attention line is the tree kernel's on the same operands, and the Trie reduction stands where the label log-probs stood."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "launch_trace")], check=True, capture_output=True, text=True)
    run = lambda c: subprocess.run([TOOL, c], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()  # noqa: E731
    got, ref = run(trie_case), run(tf_case)
    assert got[-1] == ref[-1] == "return 0"
    assert got[3].startswith("gram_workspace_bytes_trie ") and int(got[3].split()[1]) > int(ref[1].split()[1])
    got = got[:3] + got[4:]
    rep = [i for i, ln in enumerate(got) if ln.startswith("gram_trie_repeat_tokens ")]
    assert len(rep) == 1
    _, src, dst, B, Q, st = got[rep[0]].split()
    assert (B, Q) == ("2", "12") and dst.startswith("ws+") and int(dst[3:]) >= int(ref[1].split()[1])  # behind carve_tf's layout
    del got[rep[0]]
    assert len(got) == len(ref)
    n_self = 0
    for g, r in zip(got, ref):
        gw, rw = g.split(), r.split()
        if rw[0] == "gram_dec_self_attn_tf_split":
            # (qkv, bias, out, n_seq, T, H, pieces, ps, st) -> (qkv, pos, anc, bias, out, B, Q, Tq, H, pieces, ps, st)
            assert gw[0] == "gram_dec_self_attn_tree_split"
            assert [gw[1], gw[4], gw[5]] == rw[1:4] and gw[6:9] == ["2", "12", "4"] and gw[9:] == rw[6:]
            n_self += 1
        elif rw[0] == "gram_label_logprob_split":
            assert gw[0] == "gram_trie_leaf_logprob_split"
            assert gw[1:6] == rw[1:6]  # hidden, both lm_heads, d, lse
            assert gw[gw.index("}") + 1:gw.index("}") + 4] == ["2", rw[9], rw[10]]  # B, V, pieces
        elif rw[0] == "gram_embed_ex_xs" and rw[2] != gw[2]:
            assert gw[2] == dst and gw[1] == rw[1] and gw[3:] == rw[3:]  # the decoder's embedding: ids = the repeated tokens
        else:
            assert g == r
    assert n_self == 2  # one per decoder layer of the tiny model


# ---------------------------------------------------------------------------------------------------------- full_ranking
def _np_ranking(scores, tgt, ks, sid):
    B, M = scores.shape
    out = {"rank": [], "mrr": [], **{f"hit@{k}": [] for k in ks}, **{f"ndcg@{k}": [] for k in ks}}
    for b in range(B):
        best = {}
        for j in range(M):  # one score per distinct sequence
            best.setdefault(int(sid[j]), scores[b, j])
        t = scores[b, tgt[b]]
        rank = 1 + sum(1 for s in best.values() if s > t)
        out["rank"].append(rank)
        out["mrr"].append(1.0 / rank)
        for k in ks:
            rel = [[1 if i == rank - 1 else 0 for i in range(k)]]
            out[f"hit@{k}"].append(1.0 if rank <= k else 0.0)
            out[f"ndcg@{k}"].append(ndcg_at_k(rel, k))
    return out


def test_full_ranking_equals_a_numpy_restatement():
    rng = np.random.RandomState(0)
    B, M, ks = 7, 40, (1, 5, 10, 40)
    sid = rng.randint(0, 25, size=M)  # duplicates: columns that spell one sequence...
    per_seq = np.round(rng.randn(B, 25), 1).astype(np.float32)  # ...and ties between different sequences (one decimal)
    scores = per_seq[:, sid]
    tgt = rng.randint(0, M, size=B)
    want = _np_ranking(scores, tgt, ks, sid)
    got = full_ranking(torch.from_numpy(scores), torch.from_numpy(tgt), ks, sequence_ids=torch.from_numpy(sid))
    assert got["rank"].tolist() == want["rank"] and got["rank"].dtype == torch.int64
    for k in ("mrr",) + tuple(f"{m}@{c}" for m in ("hit", "ndcg") for c in ks):
        assert np.allclose(got[k].numpy(), np.asarray(want[k]), rtol=0, atol=1e-12), k
    # by leaf: no duplicate columns, no identities needed
    present = np.unique(sid)  # (sorted: the sequences that have a column at all)
    leaf = full_ranking(torch.from_numpy(per_seq[:, present]), torch.from_numpy(np.searchsorted(present, sid[tgt])), ks)
    assert leaf["rank"].tolist() == want["rank"]
    # counting duplicates twice would differ on this data: the identities matter
    naive = full_ranking(torch.from_numpy(scores), torch.from_numpy(tgt), ks)
    assert naive["rank"].tolist() != want["rank"]
    with pytest.raises(ValueError):
        full_ranking(torch.from_numpy(scores), torch.tensor([M] * B), ks)
    with pytest.raises(ValueError):
        full_ranking(torch.from_numpy(scores), torch.from_numpy(tgt), ks, sequence_ids=sid[:-1])


def test_score_all_items_refuses_cpu_and_bad_calls():
    import gram_amd
    cfg = gram_amd.T5Config(vocab_size=256, d_model=128, d_ff=256, num_layers=1, num_decoder_layers=1, num_heads=2, max_item_num=3)
    m = gram_amd.create_model("gram", cfg)
    ids = torch.zeros(1, 1, 32, dtype=torch.long)
    mask = torch.ones(1, 1, 32, dtype=torch.bool)
    cands = [[0, 5, 1]]
    with pytest.raises(NotImplementedError, match="no CPU path"):
        m.score_all_items(ids, mask, gt.prefix_allowed_tokens_fn(gt.Trie(cands)), cands)
