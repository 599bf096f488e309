"""-m gpu: the Trie-constrained search step on Tries of any fan-out (beam_step_chunked_kernel, gram_amd/csrc/beam.hip).

1. wide Tries (K * max_fanout > 16 384, or an LDS sum the one-shot kernel cannot hold) through the C ABI against the oracle's search;
2. the chunked kernel forced onto shapes the one-shot kernel accepts (gram_debug_set_beam_chunked), the whole beam state bit for bit
   after every step, for every operand form and for chunk capacities that put the candidate count on and around a chunk boundary
   (gram_debug_set_beam_chunk_capacity);
3. a non-finite candidate in a late chunk is still flagged;
4. GRAM.generate on a Trie with a root fan-out of 900+ against O.generate."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import gram_oracle as O
from tests.test_wide_trie_host import golden_cands, is_wide, make_logits, oracle_search, wide_tries

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    return gpu_util


# ------------------------------------------------------------------------------------ 1. wide Tries against the oracle
def _wide_case(name):
    if name == "yelp":
        cands = golden_cands("Yelp")
        return cands, 1, 64, 32128, max(len(c) for c in cands)
    cands, B, K, V, max_length, _fan = wide_tries()[name]
    return cands, B, K, V, max_length


@pytest.mark.parametrize("kind", ["randn", "int"])
@pytest.mark.parametrize("name,lp", [("root900", 1.0), ("second300", 1.0), ("second300", 0.7), ("advice", 1.0), ("vocab_root", 1.0),
                                     ("yelp", 1.0)])
def test_wide_trie_search_vs_oracle(G, name, lp, kind):
    """Same logits into the oracle's restated HF-4.26 search and into gram_beam_*: identical sequences, scores within the real-Trie
    tolerance of test_beam_search_real_trie_shapes (2e-5), error flag clear.  'int' logits (-3..3) tie dozens of candidates at the
    2K cut and across chunk boundaries: the oracle's tie rule (lower flat index) keeps the comparison exact."""
    from gram_amd.utils import generation_trie as gt
    cands, B, K, V, max_length = _wide_case(name)
    flat = gt.FlatTrie(gt.Trie(cands))
    assert is_wide(K, flat.max_fanout, max_length)
    logits = make_logits(kind, max_length - 1, B * K, V, seed=len(name) * 100 + K)
    seqs, scores = oracle_search(cands, logits, B, K, max_length, lp)
    assert torch.isfinite(scores).all()
    dseq, dscore, err, _ = G.device_beam_search([l.to(G.DEV) for l in logits], flat, B, K, max_length, lp)
    assert err == 0
    assert dseq.tolist() == seqs.tolist()
    assert torch.allclose(dscore, scores, atol=2e-5, rtol=0)


# ------------------------------------------------------------------------------------ 2. chunked against one-shot, bit for bit
STATE = ("tokens", "node", "beam_scores", "seq", "anc", "done", "n_hyps", "hyp_score", "worst", "hyp_len", "hyp_tok", "error")
MODES = ("dense", "sparse", "live", "split1", "split2")


def _raw(t):
    """a state array as integers of its element size (floats compared by their bits)"""
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


def _small_tries():
    """the three Tries of tests/test_gpu_kernels.py::_tries"""
    uniform = [[0, a, b, 1] for a in range(2, 9) for b in range(10, 14)]
    ragged = [[0, 2, 3, 1], [0, 2, 4, 5, 1], [0, 2, 4, 6, 7, 1], [0, 3, 1], [0, 3, 8, 1], [0, 4, 9, 9, 9, 1], [0, 5, 1],
              [0, 6, 2, 1], [0, 6, 3, 1], [0, 7, 7, 1], [0, 8, 1], [0, 9, 2, 2, 1]]
    narrow_root = [[0, 2, b, c, 1] for b in range(3, 9) for c in range(3, 7)] + [[0, 9, b, c, 1] for b in range(3, 6) for c in range(3, 5)]
    return {"uniform": uniform, "ragged": ragged, "narrow_root": narrow_root}


class _Search:
    """One search problem (Trie, B, K, lp, operands of one entry-point form); run() steps it with the one-shot or the chunked kernel
    and returns the state after every step plus the final sequences and scores."""

    def __init__(self, G, cands, B, K, V, lp, mode, seed):
        from gram_amd import _lib
        from gram_amd.utils import generation_trie as gt
        self.G, self.B, self.K, self.V, self.lp, self.mode = G, B, K, V, lp, mode
        self.flat = gt.FlatTrie(gt.Trie(cands))
        self.ctrie, self._keep_trie = self.flat.to_device(torch.device(G.DEV))
        self.max_length = max(len(c) for c in cands)
        self.d = d = 128
        R, steps = B * K, self.max_length - 1
        g = torch.Generator().manual_seed(seed)
        L_ = G.lib()
        if mode == "dense":  # step 0: one shared row per user
            self.logits = [(torch.randn(B if t == 0 else R, V, generator=g) * 2.0).to(G.DEV) for t in range(steps)]
            self.lse = []
            for lg in self.logits:
                lse = torch.empty(lg.shape[0], dtype=torch.float32, device=G.DEV)
                _lib.check(L_.gram_row_lse(G.p(lg), G.p(lse), lg.shape[0], V, G.stream()), "row_lse")
                self.lse.append(lse)
            return
        self.pieces = pieces = 2 if mode == "split2" else 1
        self.E32 = torch.randn(V, d, generator=g).to(G.DEV)
        hidden32 = [(torch.randn(B if t == 0 else R, d, generator=g) * d ** -0.5 * 3).to(G.DEV) for t in range(steps)]
        if pieces == 2:
            self.W, self.hidden = G.inter(self.E32), [G.inter(h) for h in hidden32]
        else:
            self.W, self.hidden = G.bf(self.E32), [G.bf(h) for h in hidden32]
        sp = _lib.Split(pieces, 0, 0, 0, 1.0)
        self.lse = []
        for h in self.hidden:
            rows = h.shape[0]
            part = torch.empty(rows, V // 64, 2, dtype=torch.float32, device=G.DEV)
            lse = torch.empty(rows, dtype=torch.float32, device=G.DEV)
            _lib.check(L_.gram_gemm_bf16_lse_split(G.p(h), G.p(self.W), None, G.p(part), rows, V, d, pieces * d, V, C.byref(sp), G.stream()),
                       "gemm")
            _lib.check(L_.gram_lse_combine(G.p(part), G.p(lse), rows, V // 64, G.stream()), "lse")
            self.lse.append(lse)

    def run(self, chunked, cap=0):
        from gram_amd import _lib
        G, B, K, V, d, mode = self.G, self.B, self.K, self.V, self.d, self.mode
        L_ = G.lib()
        R = B * K
        st, keep = G.make_beam_state(B, K, self.max_length, self.lp, cand_scratch=mode != "dense")
        ct = C.byref(self.ctrie)
        snaps, counts = [], []
        try:
            assert L_.gram_debug_set_beam_chunked(1 if chunked else -1) == 0
            assert L_.gram_debug_set_beam_chunk_capacity(cap) == 0
            _lib.check(L_.gram_beam_init(C.byref(st), ct, 0, G.stream()), "init")
            for t in range(self.max_length - 1):
                rpu = 1 if t == 0 else K
                lse = self.lse[t]
                if mode == "dense":
                    rc = L_.gram_beam_step(C.byref(st), ct, G.p(self.logits[t]), G.p(lse), V, t + 1, rpu, G.stream())
                else:
                    h, rowpos = self.hidden[t], None
                    if t > 0 and mode in ("live", "split2"):
                        rows, rowpos, _users = G.device_live_rows(st, self.ctrie)
                        n = rows.numel()
                        h_live, lse_live = torch.full_like(h, float("nan")), torch.full_like(lse, float("nan"))
                        h_live[:n], lse_live[:n] = h[rows.long()], lse[rows.long()]
                        h, lse = h_live, lse_live
                    if mode in ("split1", "split2"):
                        rc = L_.gram_beam_step_sparse_split(C.byref(st), ct, G.p(h), G.p(self.E32), d, G.p(lse), V, t + 1, rpu, G.p(rowpos),
                                                            self.pieces, G.stream())
                    elif rowpos is not None:
                        rc = L_.gram_beam_step_sparse_live(C.byref(st), ct, G.p(h), G.p(self.W), d, G.p(lse), V, t + 1, G.p(rowpos), G.stream())
                    else:
                        rc = L_.gram_beam_step_sparse(C.byref(st), ct, G.p(h), G.p(self.W), d, G.p(lse), V, t + 1, rpu, G.stream())
                _lib.check(rc, f"step {mode}")
                torch.cuda.synchronize()
                snaps.append({k: keep[k].clone() for k in STATE})
            seqs = torch.empty(R, self.max_length, dtype=torch.int64, device=G.DEV)
            scores = torch.empty(R, dtype=torch.float32, device=G.DEV)
            width = torch.zeros(4, dtype=torch.int32, device=G.DEV)
            _lib.check(L_.gram_beam_finalize(C.byref(st), K, self.max_length, G.p(seqs), G.p(scores), G.p(width), G.stream()), "fin")
            torch.cuda.synchronize()
        finally:
            L_.gram_debug_set_beam_chunked(-1)
            L_.gram_debug_set_beam_chunk_capacity(0)
        return snaps, seqs.cpu(), scores.cpu(), int(keep["error"][0])

    def candidate_counts(self, snaps):
        """candidates per user of every step (step 0: K beams on the start token's node), from the states the steps left"""
        fan = np.diff(self.flat.child_off)
        start = int(self.flat.child_node[0])  # the root's only child in these Tries: the start token
        out = [self.K * int(fan[start])]
        for s in snaps[:-1]:
            node = s["node"].cpu().numpy().reshape(self.B, self.K)
            done = s["done"].cpu().numpy().astype(bool)
            per = np.where(node >= 0, fan[np.maximum(node, 0)], 0).sum(1)
            out.append(int(np.where(done, 0, per).max()))
        return out


def _boundary_caps(counts):
    """chunk capacities that put a step's candidate count C on capacity - 1, on it, + 1, and on 2 x + 1 (an odd C; an even one gives
    2 x capacity, the boundary itself), plus the kernel's own capacity (0) and one candidate per round's neighbour, 2"""
    big = max(counts)
    later = max(counts[1:]) if len(counts) > 1 and max(counts[1:]) > 2 else big
    odd = [c for c in counts if c % 2 and c >= 3]
    half = (max(odd) - 1) // 2 if odd else later // 2
    return sorted({0, 2, big - 1, later + 1, later, later - 1, max(1, half)})


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,B,K,lp", [("uniform", 3, 4, 1.0), ("uniform", 2, 20, 1.0), ("ragged", 3, 5, 0.7), ("ragged", 2, 12, 1.0),
                                        ("narrow_root", 3, 6, 1.0), ("narrow_root", 2, 64, 2.0), ("beauty", 2, 20, 1.0)])
def test_chunked_step_matches_one_shot_bit_for_bit(G, name, B, K, lp, mode):
    """Every state array after EVERY step, the error flag, the final sequences and scores: the chunked kernel's bits are the
    one-shot kernel's, for the dense, sparse, live-row and split (1 and 2 pieces; the latter with rowpos) entry points, step 0's
    shared row included, at capacities around the candidate counts of the search itself."""
    if name == "beauty":
        cands, V = golden_cands("Beauty"), 32128
    else:
        cands, V = _small_tries()[name], 256
    s = _Search(G, cands, B, K, V, lp, mode, seed=1000 * B + 10 * K + MODES.index(mode))
    assert not is_wide(K, s.flat.max_fanout, s.max_length)
    ref_snaps, ref_seqs, ref_scores, ref_err = s.run(chunked=False)
    counts = s.candidate_counts(ref_snaps)
    caps = _boundary_caps(counts)
    print(f"\n[chunked vs one-shot] {name} K={K} {mode}: candidates per step {counts}, capacities {caps}")
    assert max(counts) > 2
    for cap in caps:
        snaps, seqs, scores, err = s.run(chunked=True, cap=cap)
        for t, (a, b) in enumerate(zip(ref_snaps, snaps)):
            for k in STATE:
                assert torch.equal(_raw(a[k]), _raw(b[k])), (cap, t, k)
        assert err == ref_err
        assert torch.equal(seqs, ref_seqs) and torch.equal(_raw(scores), _raw(ref_scores)), cap


# ------------------------------------------------------------------------------------ 3. non-finite candidates in a late chunk
@pytest.mark.parametrize("bad", [float("nan"), -float("nan"), float("inf")])
def test_nonfinite_candidate_in_a_late_chunk_is_flagged(G, bad):
    """Root fan-out 900, K = 20: step 0 has 18 000 candidates, five rounds of the chunked kernel.  The LAST beam's LAST token (flat
    candidate 17 999, the last round) gets a NaN / -NaN / +inf logit while the row's normaliser is the clean row's, so only the check
    on the candidate keys can see it; a negative NaN sorts below every other key, so that candidate is dropped by the selection of
    its own round.  error[0] == 4, and 0 without the bad value."""
    from gram_amd import _lib
    from gram_amd.utils import generation_trie as gt
    cands, B, K, V, max_length, _fan = wide_tries()["root900"]
    flat = gt.FlatTrie(gt.Trie(cands))
    ctrie, _keep_trie = flat.to_device(torch.device(G.DEV))
    L_ = G.lib()
    lg = make_logits("randn", 1, B * K, V, seed=3)[0].to(G.DEV)
    lse = torch.empty(B * K, dtype=torch.float32, device=G.DEV)
    _lib.check(L_.gram_row_lse(G.p(lg), G.p(lse), B * K, V, G.stream()), "row_lse")
    for poison, want in ((False, 0), (True, 4)):
        st, keep = G.make_beam_state(B, K, max_length)
        _lib.check(L_.gram_beam_init(C.byref(st), C.byref(ctrie), 0, G.stream()), "init")
        if poison:
            lg[1 * K + K - 1, 901] = bad  # user 1, beam K - 1, the root's last child
        _lib.check(L_.gram_beam_step(C.byref(st), C.byref(ctrie), G.p(lg), G.p(lse), V, 1, K, G.stream()), "step")
        torch.cuda.synchronize()
        assert int(keep["error"][0]) == want


# ------------------------------------------------------------------------------------ 4. the whole path
def _check_generate(oc, sd, out, ref, ids, mask, cands, K, tol, lp=1.0):
    """Tolerance-aware comparison of device vs oracle top-K lists (tests/test_gpu_path.py::_check_generate, restated): a returned
    sequence is a Trie member, its score matches the oracle's score of that same sequence, and any disagreement in membership or order
    is between candidates whose oracle scores are closer than the tolerance."""
    cand_set = {tuple(c) for c in cands}
    B = ids.shape[0]
    seqs, scores = out["sequences"].cpu(), out["sequences_scores"].cpu()
    rseqs, rscores = ref["sequences"], ref["sequences_scores"]

    def strip(row):
        row = [int(x) for x in row]
        while row and row[-1] == 0:
            row.pop()
        return tuple(row)

    max_dev = 0.0
    for b in range(B):
        dev = [strip(r) for r in seqs[b * K:(b + 1) * K]]
        orc = [strip(r) for r in rseqs[b * K:(b + 1) * K]]
        osc = {s: float(v) for s, v in zip(orc, rscores[b * K:(b + 1) * K])}
        assert len(set(dev)) == K, "duplicate hypotheses"
        kth = float(rscores[(b + 1) * K - 1])
        dsc = scores[b * K:(b + 1) * K]
        assert all(dsc[i] >= dsc[i + 1] for i in range(K - 1)), "scores not descending"
        for i, s in enumerate(dev):
            assert s in cand_set, f"user {b}: {s} is not a Trie member"
            if s in osc:
                exact = osc[s]
            else:  # not in the oracle's top-K: must be a near-miss of the K-th score
                exact = O.sequence_logprob(sd, oc, ids[b:b + 1], mask[b:b + 1], list(s)) / (len(s) - 1) ** lp
                assert exact > kth - 2 * tol, (b, s, exact, kth)
            assert abs(float(dsc[i]) - exact) < tol, (b, s, float(dsc[i]), exact)
            max_dev = max(max_dev, abs(float(dsc[i]) - exact))
        ex = [osc.get(s) for s in dev]
        for i in range(K - 1):
            if ex[i] is not None and ex[i + 1] is not None and ex[i] < ex[i + 1]:
                assert ex[i + 1] - ex[i] < 2 * tol
    print(f"\n[wide generate parity] max |score - oracle score of the same sequence| = {max_dev:.2e} (tol {tol})")


@pytest.fixture(scope="module")
def wide_path(G):
    """tiny config with a 2 048-token vocabulary, a random-item Trie whose root has 960 children, the oracle's beam result"""
    import gram_amd
    from gram_amd import _lib
    oc = O.OracleConfig(vocab_size=2048, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2, max_item_num=5)
    gc = gram_amd.T5Config(vocab_size=2048, d_model=128, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2, max_item_num=5)
    sd = O.init_state_dict(oc, 11)
    m = gram_amd.create_model("gram", gc)
    m.load_state_dict(sd)
    m = m.to(G.DEV).eval()
    g = torch.Generator().manual_seed(21)
    items = set()
    for a in range(2, 962):  # every first token 2..961 leads somewhere: root fan-out 960
        for _ in range(int(torch.randint(1, 3, (1,), generator=g))):
            tail = torch.randint(2, 2048, (int(torch.randint(1, 4, (1,), generator=g)),), generator=g)
            items.add((a,) + tuple(int(x) for x in tail))
    cands = [[0] + list(it) + [1] for it in sorted(items)]
    B, N, L, K = 2, 2, 32, 20
    ids = torch.randint(2, 2048, (B, N, L), generator=g)
    mask = torch.ones(B, N, L, dtype=torch.bool)
    mask[0, 1, 20:] = False
    ids[0, 1, 20:] = 0
    max_length = max(len(c) for c in cands)
    ref = O.generate(sd, oc, ids, mask, max_length, O.prefix_allowed_tokens_fn(O.Trie(cands)), K, K, 1.0)
    tol = 2e-5 * (1.0 if _lib.piece_dtype() == torch.float16 else 16.0)  # tests/test_gpu_path.py SCORE_TOL
    return dict(oc=oc, sd=sd, m=m, cands=cands, ids=ids, mask=mask, max_length=max_length, ref=ref, K=K, tol=tol)


def _generate(G, w, fn, K):
    return w["m"].generate(input_ids=w["ids"].to(G.DEV), attention_mask=w["mask"].to(G.DEV), max_length=w["max_length"],
                           prefix_allowed_tokens_fn=fn, num_beams=K, num_return_sequences=K, output_scores=True,
                           return_dict_in_generate=True, length_penalty=1.0)


def test_generate_on_a_wide_trie_vs_oracle(G, wide_path):
    """GRAM.generate at K = 20 on a root fan-out of 960 (K * fan-out = 19 200) against O.generate; live-row compaction on and off
    return the same bits."""
    from gram_amd.utils import generation_trie as gt
    w = wide_path
    trie = gt.Trie(w["cands"])
    assert gt.FlatTrie(trie).max_fanout >= 900 and is_wide(w["K"], gt.FlatTrie(trie).max_fanout, w["max_length"])
    fn = gt.prefix_allowed_tokens_fn(trie)
    L_ = G.lib()
    outs = []
    try:
        for live in (1, 0):
            L_.gram_debug_set_live_rows(live)
            outs.append(_generate(G, w, fn, w["K"]))
    finally:
        L_.gram_debug_set_live_rows(-1)
    assert outs[0]["sequences"].shape[1] == w["ref"]["sequences"].shape[1]
    _check_generate(w["oc"], w["sd"], outs[0], w["ref"], w["ids"], w["mask"], w["cands"], w["K"], w["tol"])
    assert torch.equal(outs[0]["sequences"], outs[1]["sequences"])
    assert torch.equal(_raw(outs[0]["sequences_scores"]), _raw(outs[1]["sequences_scores"]))


def test_greedy_on_a_wide_trie_vs_oracle(G, wide_path):
    """num_beams = 1 (HF greedy_search) on the same Trie: the oracle's sequences, or a first difference at a step where the oracle's
    own two logits are closer than the logit tolerance of tests/test_gpu_path.py (5e-5)."""
    from gram_amd.utils import generation_trie as gt
    w = wide_path
    oc, sd, ids, mask = w["oc"], w["sd"], w["ids"], w["mask"]
    ref = O.generate(sd, oc, ids, mask, w["max_length"], O.prefix_allowed_tokens_fn(O.Trie(w["cands"])), 1, 1)
    out = w["m"].generate(input_ids=ids.to(G.DEV), attention_mask=mask.to(G.DEV), max_length=w["max_length"],
                          prefix_allowed_tokens_fn=gt.prefix_allowed_tokens_fn(gt.Trie(w["cands"])), num_beams=1, num_return_sequences=1)
    assert out["sequences_scores"] is None
    cand_set = {tuple(c) for c in w["cands"]}
    logit_tol = 5e-5 * w["tol"] / 2e-5
    for b in range(ids.shape[0]):
        d = [int(x) for x in out["sequences"][b].cpu()]
        r = [int(x) for x in ref["sequences"][b]]
        while d and d[-1] == 0:
            d.pop()
        while r and r[-1] == 0:
            r.pop()
        assert tuple(d) in cand_set
        if d == r:
            continue
        t = next(i for i in range(min(len(d), len(r))) if d[i] != r[i])
        ext = ((1.0 - mask[b:b + 1].reshape(1, -1).float()) * O.FMIN)[:, None, None, :]
        st = O.DecodeState(O.cross_kv(sd, oc, O.encode_fused(sd, oc, ids[b:b + 1], mask[b:b + 1])), ext, 1)
        for i in range(t):
            lg = O.decoder_step(sd, oc, torch.tensor([r[i]]), st)
        assert abs(float(lg[0, d[t]] - lg[0, r[t]])) < logit_tol, (b, t, d, r)


def test_generic_callback_on_a_wide_trie_matches_fast_path(G, wide_path):
    """A plain Python prefix_allowed_tokens_fn (no Trie in its closure) answers 960 tokens per beam at the first step: the step-wise
    path returns the fast path's sequences (scores within the tolerance: its logits are the dense ones)."""
    from gram_amd.utils import generation_trie as gt
    w = wide_path
    fast = _generate(G, w, gt.prefix_allowed_tokens_fn(gt.Trie(w["cands"])), w["K"])
    table = {}
    for c in w["cands"]:
        for i in range(1, len(c)):
            table.setdefault(tuple(c[:i]), set()).add(c[i])

    def plain(batch_id, sent):
        return sorted(table.get(tuple(int(x) for x in sent), ()))

    assert w["m"]._closure_trie(plain) is None
    slow = _generate(G, w, plain, w["K"])
    assert slow["sequences"].cpu().tolist() == fast["sequences"].cpu().tolist()
    assert torch.allclose(slow["sequences_scores"].cpu(), fast["sequences_scores"].cpu(), atol=w["tol"], rtol=0)
