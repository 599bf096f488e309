"""-m gpu: the stochastic-beam-search step kernel (gram_sbs_init / gram_sbs_step / gram_sbs_step_items, gram_amd/csrc/sbs.hip) through
the C ABI against the float64 restatement of DESIGN.md section 4.10 (tests/sbs_oracle.py): hidden rows, an lm_head and a hand-built
state, no model; d = 128, three users.

Every case is DECIDABLE by construction.  delta -- derived, not guessed: the device differs from float64 in the logits and in the
fp32 arithmetic behind them, and the conditioning amplifies both where a row's best child lies far below the row's own G.  A logit
is d products (exact in fp32 for one piece, rounded once for two) added in fp32: a lane adds d / 8 of them and three butterfly
additions follow, so at most d / 8 + 3 roundings lie on any path, one more for a rounded product and one for the division by the
temperature: |dy| <= (d / 8 + 5) 2^-24 sum_j |h_j E_ij| / temperature (``logit_bound``).  The restatement is rerun with every logit
moved by a random amount up to that bound (three draws) and once in numpy float32; delta = 4 x the largest |dG| seen + 1e-5 for the
device's logf / expf / log1pf (a few ulp of values below 32).  Candidates whose G lie within delta of a neighbour's form a cluster
that the device may order either way; the test scans Philox seeds, on the host, for the first one at which at most 10 % of every
user's first R positions lie in such a cluster (none up to R = 9).  The device must then put at every position the restatement's
candidate, or one of its cluster, with G within delta and both log-probabilities within TOL's logp.  The rows' path words are
integers and must be equal."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from gram_amd import _lib
from gram_amd.utils import generation_trie as gt
from tests import gpu_util as U
from tests import sbs_oracle as X
from tests.test_gpu_teacher_forced import TOL

pytestmark = pytest.mark.gpu
DEV = U.DEV
D = 128
TMAX = 6
FANOUTS = (1, 1, 2, 5, 33, 70)  # node 1's only child and one of node 3's five are EOS
EOS_NODES = (1, 3)
NEG = float("-inf")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gram_amd
    return gram_amd


class World:
    """A Trie root -> one node per fan-out -> leaves over disjoint token sets (EOS = 1 among the children of ``eos_nodes``), random
    hidden rows (one per node) and lm_head rows with logits of standard deviation ~2, as the operands the device reads and their
    float64 values."""

    def __init__(self, pieces, fanouts=FANOUTS, eos_nodes=EOS_NODES, seed=0, planted=None):
        rng = np.random.default_rng(77 + 10 * pieces + seed)
        self.d, self.pieces, self.fanouts = D, pieces, tuple(fanouts)
        M = len(fanouts)
        V = (M + sum(fanouts) + 127) // 128 * 128 + 128
        perm = rng.permutation(np.arange(2 if planted is None else 1 + max(X.DIST_TOKENS), V))
        self.node_tok = sorted(perm[:M].tolist())
        rest, self.children, o = perm[M:], [], 0
        for m, F in enumerate(fanouts):
            n = F - (1 if m in eos_nodes else 0)
            self.children.append(np.sort(np.concatenate([rest[o:o + n], [1] if m in eos_nodes else []]).astype(np.int64)))
            o += n
        if planted is not None:
            self.children = [np.asarray(X.DIST_TOKENS, dtype=np.int64) for _ in range(M)]
        self.V = V
        self.cands = [[int(self.node_tok[m]), int(t)] for m in range(M) for t in self.children[m]]
        self.flat = gt.FlatTrie(gt.Trie(self.cands))
        self.node_id = [self.flat.leaf_of([self.node_tok[m]]) for m in range(M)]
        h = rng.normal(0.0, 1.0, (M, D)).astype(np.float32)
        E = rng.normal(0.0, 2.0 / math.sqrt(D), (V, D)).astype(np.float32)
        if planted is not None:  # logits that are exact in every format: h = e_0, E[tok] = a_tok e_0
            h[:] = 0.0
            h[:, 0] = 1.0
            for m in range(M):
                E[self.children[m]] = 0.0
                E[self.children[m], 0] = np.asarray(planted, dtype=np.float32)
        self.h32, self.E32 = torch.from_numpy(h), torch.from_numpy(E)
        if pieces == 2:
            self.E_dev = self.E32.to(DEV).contiguous()
            self.E64 = self.E32.double()
            self.h64 = U.join(U.pieces_of(self.h32.to(DEV), 2)).cpu()
        else:
            self.E_dev = U.bf(self.E32)
            self.E64 = self.E_dev.double().cpu()
            self.h64 = U.bf(self.h32).double().cpu()

    def hidden(self, nodes):
        h = self.h32[torch.as_tensor(nodes)]
        return U.inter(h.to(DEV)) if self.pieces == 2 else U.bf(h)

    def logits(self, m, alive=None):
        toks = self.children[m] if alive is None else self.children[m][alive]
        prod = self.E64[torch.as_tensor(toks)] * self.h64[m]
        return [int(t) for t in toks], prod.sum(-1).numpy(), float(prod.abs().sum(-1).max()) if len(toks) else 0.0


@pytest.fixture(scope="module")
def worlds(gpu):
    return {p: World(p) for p in (1, 2)}


# ---------------------------------------------------------------------------------------------- a state, one launch, its expectation
def make_rows(B, R, kinds, rng, cur_len):
    """rows[b][k] = dict(node m or None, G, phi, model, path, fin) from kinds[b][k]: an int m (live on node m), 'fin' or 'dead'"""
    rows = []
    for b in range(B):
        user = []
        for k in range(R):
            kind = kinds[b][k]
            r = dict(m=None, G=NEG, phi=NEG, model=NEG, path=0, fin=0)
            if kind != "dead":
                r.update(G=float(np.float32(rng.normal(-1.0, 1.5))), phi=float(np.float32(-rng.uniform(0.5, 4.0))),
                         model=float(np.float32(-rng.uniform(5.0, 9.0))), path=int(rng.integers(0, 2 ** 63)))
                if kind == "fin":
                    r["fin"] = int(rng.integers(2, cur_len + 1))
                else:
                    r["m"] = int(kind)
            user.append(r)
        rows.append(user)
    return rows


def launch(w, rows, seed, cur_len=3, rpu=None, items=None, tau=1.0, cand=True, hidden_nodes=None):
    B, R = len(rows), len(rows[0])
    n = B * R
    flat_rows = [r for u in rows for r in u]
    st, keep = U.make_beam_state(B, R, TMAX)
    keep["node"].copy_(torch.tensor([w.node_id[r["m"]] if r["m"] is not None else -1 for r in flat_rows], dtype=torch.int32))
    keep["beam_scores"].copy_(torch.tensor([r["G"] for r in flat_rows], dtype=torch.float32))
    keep["hyp_len"].view(-1)[:n].copy_(torch.tensor([r["fin"] for r in flat_rows], dtype=torch.int32))
    keep["anc"].copy_(torch.arange(n, dtype=torch.int32).repeat(TMAX, 1))
    seq0 = (1000 * torch.arange(n, dtype=torch.int32)[:, None] + torch.arange(TMAX, dtype=torch.int32)[None, :]) + 5
    keep["seq"].copy_(seq0)
    if cand:
        stride = 2 * max(w.fanouts)
        keep["cand"] = torch.full((n, stride), float("nan"), dtype=torch.float32, device=DEV)
        st.cand_logits, st.cand_logits_users, st.cand_logits_stride = keep["cand"].data_ptr(), n, stride
    if hidden_nodes is None:
        hidden_nodes = [r["m"] if r["m"] is not None else 0 for r in flat_rows]
    hid = w.hidden(hidden_nodes)
    g = torch.Generator().manual_seed(n + cur_len)
    lse = (torch.rand(hid.shape[0], generator=g) * 4 + 6)
    phi = torch.tensor([r["phi"] for r in flat_rows], dtype=torch.float32).to(DEV)
    model = torch.tensor([r["model"] for r in flat_rows], dtype=torch.float32).to(DEV)
    path = torch.tensor([r["path"] for r in flat_rows], dtype=torch.int64).to(DEV)
    lse_d = lse.to(DEV)
    ctrie, keep2 = w.flat.to_device(torch.device(DEV))
    lm16 = w.E_dev.data_ptr() if w.pieces == 1 else None
    lm32 = w.E_dev.data_ptr() if w.pieces == 2 else None
    head = (C.byref(st), C.byref(ctrie), hid.data_ptr(), lm16, lm32, w.d, lse_d.data_ptr(), w.V, cur_len, R if rpu is None else rpu,
            w.pieces, tau, seed, phi.data_ptr(), model.data_ptr(), path.data_ptr())
    if items is None:
        rc = U.lib().gram_sbs_step(*head, U.stream())
    else:
        rc = U.lib().gram_sbs_step_items(*head, C.byref(items), U.stream())
    _lib.check(rc, "gram_sbs_step")
    torch.cuda.synchronize()
    out = {k: keep[k].cpu() for k in ("tokens", "node", "seq", "anc", "hyp_len", "error", "beam_scores")}
    out.update(phi=phi.cpu(), model=model.cpu(), path=path.cpu(), lse=lse, seq0=seq0)
    return out


def expectation(w, rows, b, seed, cur_len, R, lse, lr_of, tau=1.0, alive=None, dtype=np.float64, shift=None):
    """the restatement's ranked candidates of user b (X.expand): a row's prefix is (its slot,) * cur_len"""
    urows, info = [], {}
    for k, r in enumerate(rows[b]):
        if r["G"] == NEG:
            continue
        urows.append(dict(prefix=(k,) * cur_len, phi=r["phi"], G=r["G"], model=r["model"], path=(r["path"] & X.M32, r["path"] >> 32),
                          fin=r["fin"] > 0))
        if r["m"] is not None:
            toks, z, absmax = w.logits(r["m"], None if alive is None else alive(b, r["m"]))
            info[k] = (toks, z if shift is None else z + shift(len(z), absmax), float(lse[lr_of(b, k)]), absmax)

    def kids(prefix):
        return info[prefix[0]][:3]
    ranked, gap = X.expand(urows, kids, tau, seed, R, dtype)
    return ranked, gap, max([i[3] for i in info.values()], default=0.0)


def logit_bound(absmax, tau):
    return (D / 8 + 5) * 2.0 ** -24 * absmax / tau


def clusters(ranked, delta):
    """cluster number of every ranked candidate: neighbours whose G differ by delta or less share one (they may come in any order)"""
    cid = [0] * len(ranked)
    for i in range(1, len(ranked)):
        cid[i] = cid[i - 1] + (1 if ranked[i - 1]["G"] - ranked[i]["G"] > delta else 0)
    return cid


def undecided(ranked, delta, R):
    """how many of the first R positions share their cluster with another candidate"""
    cid = clusters(ranked, delta)
    return sum(1 for j in range(min(R, len(ranked))) if cid.count(cid[j]) > 1)


def decidable_seed(w, rows, cur_len, R, lse, lr_of, tau=1.0, alive=None):
    """the first Philox seed at which, for every user, at most 10 % of the first R positions lie within delta of a neighbour (none
    up to R = 9); returns (seed, per user (ranked, delta))"""
    for seed in range(1, 200):
        per_user = []
        for b in range(len(rows)):
            a = (w, rows, b, seed, cur_len, R, lse, lr_of, tau, alive)
            ranked, gap, absmax = expectation(*a)
            bound = logit_bound(absmax, tau)
            worst = 0.0
            runs = [expectation(*a, dtype=np.float32)[0]]
            for dr in range(3):
                rng = np.random.default_rng(dr)
                runs.append(expectation(*a, shift=lambda n, am, rng=rng: rng.uniform(-1, 1, n) * logit_bound(am, 1.0))[0])
            for other in runs:
                got = {c["prefix"]: c["G"] for c in other}
                worst = max([worst] + [abs(c["G"] - got[c["prefix"]]) for c in ranked[:R + 1]])
            delta = 4 * worst + 1e-5
            if 10 * undecided(ranked, delta, R) > min(R, len(ranked)):
                break
            per_user.append((ranked, delta, bound))
        else:
            return seed, per_user
    raise AssertionError("no decidable seed among 200: re-plant the case")


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


def check(w, rows, out, per_user, cur_len, R, rpu_one=False):
    tol = TOL["f16x3" if w.pieces == 2 else "f16"]["logp"]
    assert int(out["error"][0]) == 0
    worst = 0.0
    for b, (ranked, delta, _) in enumerate(per_user):
        row0 = b * R
        cid = clusters(ranked, delta)
        where = {(c["prefix"][0], c["tok"]): i for i, c in enumerate(ranked)}
        seen = set()
        for j in range(R):
            r = row0 + j
            if j >= len(ranked):  # a dead row
                assert out["beam_scores"][r] == NEG and out["phi"][r] == NEG and out["model"][r] == NEG, (b, j)
                assert int(out["tokens"][r]) == 0 and int(out["node"][r]) == -1 and int(out["hyp_len"].view(-1)[r]) == 0
                continue
            # which candidate the device put here (its parent shows in the sequence that moved along): the restatement's at this
            # position, or one within delta of it
            ident = ((int(out["seq"][r, 0]) - 5) // 1000 - row0, int(out["tokens"][r]))
            assert ident in where and ident not in seen, (b, j, ident)
            seen.add(ident)
            i = where[ident]
            assert cid[i] == cid[j], (b, j, i, ranked[j]["G"], ranked[i]["G"], delta)
            c = ranked[i]
            k = c["prefix"][0]
            old = rows[b][k]
            assert torch.equal(out["seq"][r, :cur_len], out["seq0"][row0 + k, :cur_len]), (b, j, "sequence moved with the selection")
            assert bool((out["anc"][: cur_len - 1, r] == row0 + k).all()) and int(out["anc"][cur_len - 1, r]) == (b if rpu_one else row0 + k)
            assert bool((out["anc"][cur_len:, r] == r).all())
            if c["fin"] and old["fin"] > 0:  # a finished row, carried unchanged
                assert int(out["tokens"][r]) == 0 and int(out["node"][r]) == -1 and int(out["seq"][r, cur_len]) == 0
                assert int(out["hyp_len"].view(-1)[r]) == old["fin"]
                assert bits(out["beam_scores"][r]) == bits(old["G"]) and bits(out["phi"][r]) == bits(old["phi"])
                assert bits(out["model"][r]) == bits(old["model"]) and int(out["path"][r]) == old["path"]
                continue
            tok = c["tok"]
            assert int(out["tokens"][r]) == tok and int(out["seq"][r, cur_len]) == tok, (b, j, int(out["tokens"][r]), tok)
            assert int(out["node"][r]) == (-1 if tok == 1 else w.flat.leaf_of([w.node_tok[old["m"]], tok]))
            assert int(out["hyp_len"].view(-1)[r]) == (cur_len + 1 if tok == 1 else 0)
            assert int(out["path"][r]) & (2 ** 64 - 1) == (c["path"][1] << 32 | c["path"][0])
            dG = abs(float(out["beam_scores"][r]) - c["G"])
            dp, dm = abs(float(out["phi"][r]) - c["phi"]), abs(float(out["model"][r]) - c["model"])
            worst = max(worst, dG, dp, dm)
            assert dG <= delta and dp < tol and dm < tol, (b, j, dG, delta, dp, dm)
            if w.fanouts[old["m"]] == 1:  # a chain: G and phi are carried bit for bit
                assert bits(out["beam_scores"][r]) == bits(old["G"]) and bits(out["phi"][r]) == bits(old["phi"]), (b, j)
    return worst


def kinds_for(R, rng):
    """three users: live rows over every node (chain, single EOS child, EOS among others, wide) mixed with finished and dead rows;
    a user with a single live row on the two-child node (fewer candidates than R from R = 3 on); a user of live rows only"""
    if R == 1:
        return [[4], [3], [0]]
    a = [int(rng.integers(len(FANOUTS))) for _ in range(R)]
    a[:6] = [0, 4, 1, 3, 5, 2][:R]
    for k in range(1, R, 3):
        a[k] = "fin" if k % 2 else "dead"
    a[1 % R] = "fin"
    # (R = 64: every row of the last user on the 70-child node -- 4 480 candidates, more than the 4 096 held on chip and three
    # rounds of the 2 048-word key array)
    return [a, [2] + ["dead"] * (R - 1), [5] * R if R == 64 else [int(rng.integers(2, len(FANOUTS))) for _ in range(R)]]


@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("R", [1, 3, 8, 64])
def test_step_matches_the_restatement(worlds, R, pieces):
    """R = 1, 3, 8, 64; at R = 64 the last user's 4 480 candidates lie in the state's scratch and stream through the key array in
    three rounds"""
    w = worlds[pieces]
    rng = np.random.default_rng(R)
    cur_len = 3
    rows = make_rows(3, R, kinds_for(R, rng), rng, cur_len)
    lse = launch(w, rows, 0, cur_len)["lse"]  # (the launch's lse is a function of the shape: take it from a first launch)
    seed, per_user = decidable_seed(w, rows, cur_len, R, lse, lambda b, k: b * R + k)
    out = launch(w, rows, seed, cur_len)
    worst = check(w, rows, out, per_user, cur_len, R)
    assert len(per_user[1][0]) == (5 if R == 1 else 2)  # user 1 at R >= 3: fewer candidates than R, the rest are dead rows
    assert R < 64 or len(per_user[2][0]) == 64 * 70 > U.lib().gram_sbs_capacity()
    print(f"R={R} pieces={pieces}: seed {seed}, worst |d| {worst:.2e}, delta {max(p[1] for p in per_user):.2e}")


@pytest.mark.parametrize("R", [1, 3, 8])
def test_compact_step0(worlds, R):
    """the step on one hidden row per user (rows_per_user == 1): only row 0 of a user is live, as after gram_sbs_init"""
    w = worlds[2]
    cur_len, nodes = 1, [4, 3, 5]
    rng = np.random.default_rng(70 + R)
    rows = make_rows(3, R, [[m] + ["dead"] * (R - 1) for m in nodes], rng, cur_len)
    lse = launch(w, rows, 0, cur_len, rpu=1, hidden_nodes=nodes)["lse"]
    seed, per_user = decidable_seed(w, rows, cur_len, R, lse, lambda b, k: b)
    out = launch(w, rows, seed, cur_len, rpu=1, hidden_nodes=nodes)
    check(w, rows, out, per_user, cur_len, R, rpu_one=True)


def test_init_writes_the_root_words(worlds):
    """gram_sbs_init: row 0 of a user carries the restatement's root (path words equal, G within fp32 of -log(-log u)), phi = model
    = 0, not finished; the other rows are dead"""
    w = worlds[1]
    B, R, seed = 3, 4, 2 ** 63 + 12345
    keys = [5, 2 ** 40 + 3, -7]
    roots = [X.root(seed, k) for k in keys]
    st, keep = U.make_beam_state(B, R, TMAX)
    keep["hyp_len"].fill_(9)
    ctrie, _k = w.flat.to_device(torch.device(DEV))
    f = dict(dtype=torch.float32, device=DEV)
    phi, model, path = torch.full((B * R,), 7.0, **f), torch.full((B * R,), 7.0, **f), torch.full((B * R,), 7, dtype=torch.int64, device=DEV)
    uk = torch.tensor(keys, dtype=torch.int64, device=DEV)
    _lib.check(U.lib().gram_sbs_init(C.byref(st), C.byref(ctrie), 0, seed, uk.data_ptr(), phi.data_ptr(), model.data_ptr(),
                                     path.data_ptr(), U.stream()), "gram_sbs_init")
    torch.cuda.synchronize()
    G, phi, model, path = keep["beam_scores"].cpu(), phi.cpu(), model.cpu(), path.cpu()
    for b in range(B):
        assert abs(float(G[b * R]) - roots[b]["G"]) < 1e-5 and float(phi[b * R]) == 0.0 and float(model[b * R]) == 0.0
        assert int(path[b * R]) & (2 ** 64 - 1) == roots[b]["path"][1] << 32 | roots[b]["path"][0]
        for t in (G, phi, model):
            assert bool((t[b * R + 1:(b + 1) * R] == NEG).all())
    assert int(keep["hyp_len"].cpu().view(-1)[: B * R].abs().sum()) == 0


@pytest.mark.parametrize("pieces", [1, 2])
def test_item_filters(gpu, pieces, worlds):
    """User 0 excludes children of every node (and ALL of node 2's); user 1 is allowed three items; user 2 excludes nothing.
    Expected: the restatement over the alive children only."""
    w = worlds[pieces]
    R, cur_len = 8, 3
    idx = {tuple(c): i for i, c in enumerate(w.cands)}
    dead0 = {m: sorted({0, F // 3, *range(5, 5 + F // 4)} & set(range(F))) if m != 2 else [0, 1] for m, F in enumerate(w.fanouts)}
    dead0[0], dead0[1] = [], []
    ex0 = [idx[(w.node_tok[m], int(w.children[m][i]))] for m in dead0 for i in dead0[m]]
    only = [idx[(w.node_tok[4], int(w.children[4][i]))] for i in (3, 20)] + [idx[(w.node_tok[5], int(w.children[5][69]))]]
    rng = np.random.default_rng(5)
    kinds = [[4, 2, 5, 3, "fin", 0, 4, 1], [4, 5, 5, 4, "dead", "fin", 4, 5], [5, 4, 3, 2, 1, 0, 5, 4]]
    rows = make_rows(3, R, kinds, rng, cur_len)
    for mode, lists, alive in (
            (_lib.ITEMS_EXCLUDE, [ex0, [], []],
             lambda b, m: np.setdiff1d(np.arange(w.fanouts[m]), dead0[m]).astype(np.int64) if b == 0 else None),
            (_lib.ITEMS_ALLOW, [list(range(len(w.cands))), only, list(range(len(w.cands)))],
             lambda b, m: (np.array([3, 20]) if m == 4 else np.array([69] if m == 5 else [], dtype=np.int64)) if b == 1 else None)):
        ui, keep = U.user_items(w.flat, w.cands, lists, mode)
        lse = launch(w, rows, 0, cur_len, items=ui)["lse"]
        seed, per_user = decidable_seed(w, rows, cur_len, R, lse, lambda b, k: b * R + k, alive=alive)
        out = launch(w, rows, seed, cur_len, items=ui)
        check(w, rows, out, per_user, cur_len, R)
        if mode == _lib.ITEMS_ALLOW:
            assert len(per_user[1][0]) == 1 + 2 * 3 + 3  # the finished row, 3 x two items under node 4, 3 x one under node 5


def test_streamed_equals_resident(worlds):
    """The debug capacity lowered to 8 candidates: the same cases run from the state's scratch, bit-identical to the on-chip run --
    unfiltered and filtered; without the scratch the streamed launch is refused before it runs."""
    lib = U.lib()
    assert lib.gram_sbs_capacity() == 4096
    for pieces in (1, 2):
        w = worlds[pieces]
        idx = {tuple(c): i for i, c in enumerate(w.cands)}
        ex = [idx[(w.node_tok[m], int(w.children[m][i]))] for m in (3, 4, 5) for i in range(0, w.fanouts[m], 3)]
        for R in (3, 8):
            rng = np.random.default_rng(40 + R)
            rows = make_rows(3, R, kinds_for(R, rng), rng, 3)
            for items in (None, "exclude"):
                ui = U.user_items(w.flat, w.cands, [ex, [], ex[::2]], _lib.ITEMS_EXCLUDE) if items else (None, None)
                a = launch(w, rows, 11, items=ui[0])
                try:
                    assert lib.gram_debug_set_sbs_capacity(8) == 0 and lib.gram_sbs_capacity() == 8
                    b = launch(w, rows, 11, items=ui[0])
                    with pytest.raises(_lib.GramHipError):
                        launch(w, rows, 11, items=ui[0], cand=False)
                finally:
                    lib.gram_debug_set_sbs_capacity(0)
                for k in ("tokens", "node", "seq", "anc", "hyp_len", "error", "path"):
                    assert torch.equal(a[k], b[k]), (pieces, R, items, k)
                for k in ("beam_scores", "phi", "model"):
                    assert np.array_equal(bits(a[k]), bits(b[k])), (pieces, R, items, k)


def test_bad_arguments_are_refused(worlds):
    w = worlds[1]
    rows = make_rows(1, 3, [[4, 4, 4]], np.random.default_rng(0), 3)
    for kw in (dict(tau=0.0), dict(tau=-1.0), dict(tau=float("inf")), dict(cur_len=0), dict(cur_len=TMAX), dict(rpu=2)):
        with pytest.raises(_lib.GramHipError):
            launch(w, rows, 1, **kw)


def test_first_row_follows_the_softmax(gpu):
    """4 096 users share one hidden row over a 5-child node and differ in their user keys: the token of a user's FIRST row is the
    argmax of its children's perturbed scores -- the Gumbel-max trick -- so its counts follow softmax(y).  Within 4.5 sigma per child,
    seed and keys fixed (tests/test_sbs_host.py shows the restatement passing with the same ones)."""
    w = World(2, fanouts=(5,), eos_nodes=(), planted=X.DIST_LOGITS)
    B, R, cur_len = X.DIST_USERS, 3, 1
    st, keep = U.make_beam_state(B, R, TMAX)
    ctrie, _k = w.flat.to_device(torch.device(DEV))
    f = dict(dtype=torch.float32, device=DEV)
    phi, model = torch.empty(B * R, **f), torch.empty(B * R, **f)
    path = torch.empty(B * R, dtype=torch.int64, device=DEV)
    uk = torch.tensor(X.dist_keys(), dtype=torch.int64, device=DEV)
    lib = U.lib()
    _lib.check(lib.gram_sbs_init(C.byref(st), C.byref(ctrie), 0, X.DIST_SEED, uk.data_ptr(), phi.data_ptr(), model.data_ptr(),
                                 path.data_ptr(), U.stream()), "gram_sbs_init")
    keep["node"].fill_(w.node_id[0])
    root_G = keep["beam_scores"].cpu().view(B, R)[:, 0].clone()
    hid = w.hidden([0] * B)
    lse = torch.full((B,), 3.0, **f)
    _lib.check(lib.gram_sbs_step(C.byref(st), C.byref(ctrie), hid.data_ptr(), None, w.E_dev.data_ptr(), D, lse.data_ptr(), w.V, cur_len, 1,
                                 2, 1.0, X.DIST_SEED, phi.data_ptr(), model.data_ptr(), path.data_ptr(), U.stream()), "gram_sbs_step")
    torch.cuda.synchronize()
    assert int(keep["error"][0]) == 0
    toks = keep["tokens"].cpu().view(B, R)
    assert bool((toks[:, 0] != toks[:, 1]).all()) and bool((toks[:, 1] != toks[:, 2]).all()) and bool((toks[:, 0] != toks[:, 2]).all())
    counts = np.array([int((toks[:, 0] == int(t)).sum()) for t in w.children[0]])
    zs = X.dist_z(counts)
    print("counts", counts.tolist(), "z", np.round(zs, 2).tolist())
    assert counts.sum() == B and float(np.abs(zs).max()) < 4.5
    G = keep["beam_scores"].cpu().view(B, R)
    assert bool((G[:, 0] >= G[:, 1]).all()) and bool((G[:, 1] >= G[:, 2]).all())
    assert np.array_equal(bits(G[:, 0]), bits(root_G))  # the best child carries the root's G exactly
