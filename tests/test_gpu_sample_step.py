"""-m gpu: the sampling step kernel (gram_sample_step / gram_sample_step_items, gram_amd/csrc/sample.hip) through the C ABI against
the float64 restatement of DESIGN.md section 4.8 (tests/sample_oracle.py): hidden rows, an lm_head and a hand-built state, no model.

Every case is DECIDABLE by construction, so nothing is skipped and nothing is capped.  The uniforms are constructed: for every row
the test picks a target among the kept children and sets u to the midpoint of that child's float64 CDF interval, using only
intervals wider than 4 delta; the device's token and next node must then equal the target exactly.

delta -- a bound, not a measurement.  The device differs from float64 in three places:
  * the logit z_i = sum_j h_j E_ij: d products (exact in fp32 for one piece, rounded once for two) added in fp32, so
    |dz_i| <= 2 d 2^-24 sum_j |h_j E_ij|, and y = z / temperature scales it (the division adds one rounding of y, inside the factor 2);
  * the weights w_i = exp(y_i - y_max): a relative error |dy_i| + |dy_max| + 2^-23 (expf and the subtraction) each, <= 1 in value;
  * the running sums: F fp32 additions of values <= W, a relative F 2^-24 of W.
A CDF boundary c_i = sum_{j<=i} w_j / W therefore moves by at most 2 * (2 d 2^-24 max_i sum_j |h_j E_ij| / temperature) (numerator
and denominator) + F 2^-24 + 2^-20 (the constant covers expf, the product u * W and the conversions); the test uses twice that sum
again: delta = 4 * (2 d 2^-24 max_i sum_j |h_j E_ij| / temperature + F 2^-24 + 2^-20).  A uniform further than delta from every
boundary is decided alike by both; targets use intervals wider than 4 delta and sit in their middle.
The filter thresholds are placed mid-gap the same way (``_decidable``): the k'-th and (k'+1)-th largest y differ by more than twice
the logit bound, and no cumulative mass of the top_p rule lies within delta of 1 - top_p.

Log-probabilities are compared with float64 at ``TOL[...]['logp']`` of tests/test_gpu_teacher_forced.py (two pieces: the f16x3
entry; one piece: the f16 entry)."""
import ctypes as C

import numpy as np
import pytest
import torch

from gram_amd import _lib
from gram_amd.utils import generation_trie as gt
from tests import gpu_util as U
from tests import sample_oracle as S
from tests.test_gpu_teacher_forced import TOL

pytestmark = pytest.mark.gpu
DEV = U.DEV
FANOUTS = (1, 2, 32, 33, 63, 64, 65, 255, 256, 257)  # (63 / 64 / 65: the lowered capacity of 64, -1 / +-0 / +1)
U_MAX = float(np.nextafter(np.float32(1), np.float32(0)))


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gram_amd
    return gram_amd


def _logp_tol(pieces):
    return TOL["f16x3" if pieces == 2 else "f16"]["logp"]


# ---------------------------------------------------------------------------------------------- the world of one (d, pieces)
class World:
    """A Trie root -> one node per fan-out -> leaves, over disjoint token sets; one hidden direction h_m per node and lm_head rows
    E_tok = a_tok * h_m / |h_m|^2, so that the logit of child tok at node m is a_tok (up to the operands' 16-bit rounding, which the
    float64 reference shares) and sum_j |h_j E_tok,j| = |a_tok|: the error bound stays small at every d.  Planted logits per node:
    first child 5.0, last 4.7, two inner ones 4.4 and 1.0, the rest evenly spaced over [-16, -10] in random order."""

    def __init__(self, d, pieces, fanouts=FANOUTS, seed=0, full_vocab=False):
        rng = np.random.default_rng(1000 * d + 10 * pieces + seed)
        self.d, self.pieces, self.fanouts = d, pieces, tuple(fanouts)
        M = len(fanouts)
        if full_vocab:  # ONE node whose children are the whole vocabulary (the node tokens double as children of the node)
            assert M == 1
            V = fanouts[0]
            self.node_tok, child_toks = [7], [np.arange(V)]
        else:
            V = (M + sum(fanouts) + 127) // 128 * 128 + 128
            perm = rng.permutation(np.arange(2, V))
            self.node_tok = sorted(perm[:M].tolist())
            rest, child_toks, o = perm[M:], [], 0
            for F in fanouts:
                child_toks.append(np.sort(rest[o:o + F]))
                o += F
        self.V = V
        self.children = child_toks
        self.cands = [[int(self.node_tok[m]), int(t)] for m in range(M) for t in child_toks[m]]
        self.flat = gt.FlatTrie(gt.Trie(self.cands))
        self.node_id = [self.flat.leaf_of([self.node_tok[m]]) for m in range(M)]
        h = rng.normal(0.0, 1.0, (M, d)).astype(np.float32)
        E = rng.normal(0.0, 0.01, (V, d)).astype(np.float32)
        self.planted = []
        for m, F in enumerate(fanouts):
            a = -10.0 - 6.0 * rng.permutation(F) / F  # (evenly spaced: a top_k threshold inside the tail is mid-gap too)
            a[0] = 5.0
            if F > 1:
                a[F - 1] = 4.7
            if F > 3:
                a[F // 3], a[2 * F // 3] = 4.4, 1.0
            self.planted.append(a)
            E[child_toks[m]] = (a[:, None] * h[m][None, :] / float((h[m].astype(np.float64) ** 2).sum())).astype(np.float32)
        self.h32, self.E32 = torch.from_numpy(h), torch.from_numpy(E)
        # the operands the device reads, and their float64 values
        if pieces == 2:
            self.E_dev = self.E32.to(DEV).contiguous()
            self.E64 = self.E32.double()
            self.h64 = U.join(U.pieces_of(self.h32.to(DEV), 2)).cpu()
        else:
            self.E_dev = U.bf(self.E32)
            self.E64 = self.E_dev.double().cpu()
            self.h64 = U.bf(self.h32).double().cpu()

    def hidden(self, node_of_row):
        h = self.h32[torch.as_tensor(node_of_row)]
        return U.inter(h.to(DEV)) if self.pieces == 2 else U.bf(h)

    def logits(self, m, alive=None):
        """float64 logits of node m's (alive) children in token order, and the bound's sum_j |h_j E_ij| maximum"""
        toks = self.children[m] if alive is None else self.children[m][alive]
        Em = self.E64[torch.as_tensor(toks)]
        z = (Em * self.h64[m]).sum(-1).numpy()
        absmax = float((Em * self.h64[m]).abs().sum(-1).max())
        return toks, z, absmax


def _delta(d, absmax, tau, F):
    return 4 * (2 * d * 2.0 ** -24 * absmax / tau + F * 2.0 ** -24 + 2.0 ** -20)


def _decidable(z, tau, top_k, top_p, d, absmax):
    """are both filter thresholds mid-gap for this row?"""
    y, kept, cum = S.warp(z, tau, top_k, top_p)
    F = len(z)
    bound = 2 * d * 2.0 ** -24 * absmax / tau
    if top_k > 0 and min(max(top_k, 1), F) < F:
        ys = np.sort(y)[::-1]
        kk = min(max(top_k, 1), F)
        if ys[kk - 1] != ys[kk] and ys[kk - 1] - ys[kk] <= 2 * bound:
            return False
    if top_p < 1:
        c = cum[~np.isnan(cum) & (y < y.max())]
        if c.size and np.abs(c - (1 - top_p)).min() <= _delta(d, absmax, tau, F):
            return False
    return True


def _targets(z, tau, top_k, top_p, d, absmax):
    """[(child index, u)]: the first and the last child where they are kept and wide, the first and last wide kept child, one inner
    wide child, and u = 0 / u = the largest float below 1 (which pick the first / last kept child, their intervals wide or not: 0 and
    1 are further than delta from every interior boundary when those intervals are)"""
    assert _decidable(z, tau, top_k, top_p, d, absmax), "the case is not decidable: re-plant the logits"
    y, kept, _ = S.warp(z, tau, top_k, top_p)
    lo, hi, logq = S.cdf(y, kept)
    dl = _delta(d, absmax, tau, len(z))
    idx = np.nonzero(kept)[0]
    wide = [int(i) for i in idx if hi[i] - lo[i] > 4 * dl]
    assert wide, "no interval wider than 4 delta"
    out = [(i, float(np.float32(0.5 * (lo[i] + hi[i])))) for i in dict.fromkeys([wide[0], wide[-1], wide[len(wide) // 2]])]
    if int(idx[0]) in wide:
        out.append((int(idx[0]), 0.0))
    if int(idx[-1]) in wide:
        out.append((int(idx[-1]), U_MAX))
    for i, u in out:
        assert S.pick(z, u, tau, top_k, top_p) == i
    return out, logq, y


# ---------------------------------------------------------------------------------------------- one launch
def _launch(w, node_of_row, u, prm, B, R, rows_per_user=None, cur_len=2, fin=None, items=None, cand_stride=0, lse=None, acc0=None,
            hidden_rows=None):
    """One gram_sample_step[_items] on a hand-built state: row r stands on node node_of_row[r].  Returns the state tensors after
    the step and the two accumulators (all on the host)."""
    rows = B * R
    rpu = R if rows_per_user is None else rows_per_user
    st, keep = U.make_beam_state(B, R, 6)
    keep["node"].copy_(torch.tensor([w.node_id[m] for m in node_of_row], dtype=torch.int32))
    keep["anc"].copy_(torch.arange(rows, dtype=torch.int32).repeat(6, 1))
    keep["seq"].fill_(-7)
    if fin is not None:
        keep["hyp_len"].view(-1)[:rows].copy_(torch.tensor(fin, dtype=torch.int32))
    if cand_stride:
        keep["cand"] = torch.full((rows, cand_stride), float("nan"), dtype=torch.float32, device=DEV)
        st.cand_logits, st.cand_logits_users, st.cand_logits_stride = keep["cand"].data_ptr(), rows, cand_stride
    hid = w.hidden(node_of_row if hidden_rows is None else hidden_rows)
    g = torch.Generator().manual_seed(rows)
    lse_t = (torch.rand(hid.shape[0], generator=g) * 4 + 6).to(DEV) if lse is None else lse.to(DEV)
    a0 = torch.randn(2, rows, generator=g) if acc0 is None else acc0
    acc_s, acc_m = a0[0].to(DEV).contiguous(), a0[1].to(DEV).contiguous()
    ut = torch.tensor(u, dtype=torch.float32).to(DEV)
    ctrie, keep2 = w.flat.to_device(torch.device(DEV))
    p = _lib.SampleParams(*prm)
    lm16 = w.E_dev.data_ptr() if w.pieces == 1 else None
    lm32 = w.E_dev.data_ptr() if w.pieces == 2 else None
    head = (C.byref(st), C.byref(ctrie), hid.data_ptr(), lm16, lm32, w.d, lse_t.data_ptr(), w.V, cur_len, rpu, w.pieces, C.byref(p),
            ut.data_ptr(), 1, acc_s.data_ptr(), acc_m.data_ptr())
    if items is None:
        rc = U.lib().gram_sample_step(*head, U.stream())
    else:
        rc = U.lib().gram_sample_step_items(*head, C.byref(items), U.stream())
    _lib.check(rc, "gram_sample_step")
    torch.cuda.synchronize()
    out = {k: keep[k].cpu() for k in ("tokens", "node", "seq", "anc", "hyp_len", "error")}
    out.update(acc_s=acc_s.cpu(), acc_m=acc_m.cpu(), acc0=a0, lse=lse_t.cpu())
    return out


def _expect_rows(w, prm, B, R, nodes):
    """rows of a launch: every (node, target) of ``nodes`` in turn until B * R rows are filled"""
    tau, top_k, top_p = prm
    combos = []
    for m in nodes:
        toks, z, absmax = w.logits(m)
        tg, logq, y = _targets(z, tau, top_k, top_p, w.d, absmax)
        combos += [(m, i, u, int(toks[i]), float(logq[i]), float(z[i])) for i, u in tg]
    return [combos[r % len(combos)] for r in range(B * R)], combos


def _check(w, out, rows, pieces, cur_len=2, lr=None):
    tol = _logp_tol(pieces)
    assert int(out["error"][0]) == 0
    worst = 0.0
    for r, (m, i, u, tok, logq, z) in enumerate(rows):
        assert int(out["tokens"][r]) == tok, (r, m, i, u, int(out["tokens"][r]), tok)
        assert int(out["seq"][r, cur_len]) == tok
        assert int(out["node"][r]) == w.flat.leaf_of([w.node_tok[m], tok])
        assert int(out["hyp_len"].view(-1)[r]) == (cur_len + 1 if tok == 1 else 0)
        ds = abs(float(out["acc_s"][r].double() - out["acc0"][0][r].double()) - logq)
        dm = abs(float(out["acc_m"][r].double() - out["acc0"][1][r].double()) - (z - float(out["lse"][r if lr is None else lr[r]])))
        worst = max(worst, ds, dm)
        assert ds < tol and dm < tol, (r, m, i, ds, dm)
    return worst


PARAMS = [(1.0, 0, 1.0), (0.5, 0, 1.0), (2.0, 0, 1.0), (1.0, 1, 1.0), (1.0, 2, 1.0), (1.0, 32, 1.0), (1.0, 37, 1.0), (1.0, 257, 1.0),
          (1.0, 262, 1.0), (1.0, 0, 0.9), (1.0, 0, 1e-6), (0.5, 2, 0.9), (2.0, 5, 0.9), (2.0, 50, 1e-6), (0.5, 33, 0.9)]


@pytest.fixture(scope="module")
def worlds(gpu):
    return {(d, p): World(d, p) for d, p in ((64, 1), (512, 2), (768, 1), (1024, 2))}


@pytest.mark.parametrize("d,pieces", [(64, 1), (512, 2), (768, 1), (1024, 2)])
def test_draws_match_the_restatement(worlds, d, pieces):
    """Every fan-out x every parameter set x every kind of target, B = 3 users of R = 64 rows"""
    w = worlds[(d, pieces)]
    worst, kinds = 0.0, set()
    for prm in PARAMS:
        rows, combos = _expect_rows(w, prm, 3, 64, range(len(w.fanouts)))
        assert len(combos) <= 192
        for m, i, u, *_ in combos:
            F = w.fanouts[m]
            kinds |= {("first", i == 0), ("last", i == F - 1), ("inner", 0 < i < F - 1), ("u0", u == 0.0), ("u1", u == U_MAX)}
        out = _launch(w, [c[0] for c in rows], [c[2] for c in rows], prm, 3, 64)
        worst = max(worst, _check(w, out, rows, pieces))
        # a row writes its own slots only: the identity ancestors and the other sequence positions are untouched
        assert torch.equal(out["anc"], torch.arange(192, dtype=torch.int32).repeat(6, 1))
        assert bool((out["seq"][:, [0, 1, 3, 4, 5]] == -7).all())
    assert {(k, True) for k in ("first", "last", "inner", "u0", "u1")} <= kinds
    print(f"d={d} pieces={pieces}: worst |log-prob - fp64| {worst:.2e} (tolerance {_logp_tol(pieces):.0e})")


@pytest.mark.parametrize("B,R,rpu", [(1, 1, 1), (1, 20, 20), (3, 20, 20), (3, 20, 1), (1, 64, 1), (3, 64, 64)])
def test_row_counts_and_the_compact_step(worlds, B, R, rpu):
    """R = 1, 20, 64 and B = 1, 3; rows_per_user = 1: hidden and lse hold one row per user, every row of user b reads row b, and the
    step points slot cur_len - 1 of the ancestor table at it"""
    w = worlds[(512, 2)]
    prm = (1.0, 50, 1.0)
    user_node = [4, 7, 2][:B]  # fan-outs 63, 255, 32
    if rpu == 1 and R > 1:
        per_user = [_expect_rows(w, prm, 1, R, [m])[0] for m in user_node]
        rows = [c for u_rows in per_user for c in u_rows]
        out = _launch(w, [c[0] for c in rows], [c[2] for c in rows], prm, B, R, rows_per_user=1, cur_len=1, hidden_rows=user_node)
        _check(w, out, rows, 2, cur_len=1, lr=[r // R for r in range(B * R)])
        want = torch.arange(B * R, dtype=torch.int32).repeat(6, 1)
        want[0] = torch.arange(B * R, dtype=torch.int32) // R
        assert torch.equal(out["anc"], want)
    else:
        rows, _ = _expect_rows(w, prm, B, R, user_node)
        out = _launch(w, [c[0] for c in rows], [c[2] for c in rows], prm, B, R, rows_per_user=rpu)
        _check(w, out, rows, 2)


def test_full_vocabulary_node(gpu):
    """One node whose children are all V = 512 tokens (EOS among them)"""
    w = World(64, 1, fanouts=(512,), full_vocab=True)
    for prm in ((1.0, 0, 1.0), (1.0, 50, 0.9)):
        rows, combos = _expect_rows(w, prm, 1, 8, [0])
        out = _launch(w, [c[0] for c in rows], [c[2] for c in rows], prm, 1, 8)
        _check(w, out, rows, 1)
        assert any(c[3] == 511 for c in combos) and any(c[3] == 0 for c in combos)


def test_ties_stay_together(gpu):
    """Two children with identical lm_head rows (bit-equal logits) at the top_k threshold and at the top_p boundary: both are kept.
    top_k = 2 over logits (5, 4, 4, ...) keeps three; top_p = 0.97 over (5, 1, 1, ...) keeps the tied pair, whose JOINT mass 0.035
    exceeds 0.03 where either alone (0.018) would not."""
    for a_tie, prm, n_kept in ((4.0, (1.0, 2, 1.0), 3), (1.0, (1.0, 0, 0.97), 3)):
        w = World(64, 1, fanouts=(33,))
        toks = w.children[0]
        hn = w.h32[0].double()
        row = (a_tie * hn / float((hn ** 2).sum())).float()
        w.E32[toks[10]] = row
        w.E32[toks[20]] = row
        for i in (11, 22, 32):  # (the other planted children join the tail: only the first child lies above the tied pair)
            w.E32[toks[i]] = w.E32[toks[12]]
        w.E_dev = U.bf(w.E32)
        w.E64 = w.E_dev.double().cpu()
        _, z, absmax = w.logits(0)
        assert z[10] == z[20]
        y, kept, _ = S.warp(z, *prm)
        assert int(kept.sum()) == n_kept and kept[10] and kept[20]
        rows, combos = _expect_rows(w, prm, 1, 8, [0])
        lo, hi, logq = S.cdf(y, kept)
        for i in (10, 20):  # both tied children are drawn from the middle of their own intervals
            assert hi[i] - lo[i] > 4 * _delta(64, absmax, prm[0], 33)
            combos.append((0, i, float(np.float32(0.5 * (lo[i] + hi[i]))), int(toks[i]), float(logq[i]), float(z[i])))
        rows = [combos[r % len(combos)] for r in range(8)]
        assert {c[1] for c in rows} >= {10, 20}
        out = _launch(w, [c[0] for c in rows], [c[2] for c in rows], prm, 1, 8)
        _check(w, out, rows, 1)


def test_finished_rows_emit_pad(worlds):
    w = worlds[(64, 1)]
    prm = (1.0, 0, 1.0)
    rows, _ = _expect_rows(w, prm, 2, 4, [3, 5])
    fin = [0, 3, 0, 0, 2, 0, 5, 0]
    out = _launch(w, [c[0] for c in rows], [c[2] for c in rows], prm, 2, 4, cur_len=4, fin=fin)
    live = [r for r in range(8) if not fin[r]]
    sub = {k: (v[live] if k in ("tokens", "node", "seq", "acc_s", "acc_m") else v) for k, v in out.items()}
    sub["acc0"] = out["acc0"][:, live]
    sub["hyp_len"] = out["hyp_len"].view(-1)[:8][live]
    sub["lse"] = out["lse"][live]
    _check(w, sub, [rows[r] for r in live], 1, cur_len=4)
    for r in range(8):
        if fin[r]:
            assert int(out["tokens"][r]) == 0 and int(out["node"][r]) == -1 and int(out["seq"][r, 4]) == 0
            assert int(out["hyp_len"].view(-1)[r]) == fin[r]
            assert out["acc_s"][r] == out["acc0"][0][r] and out["acc_m"][r] == out["acc0"][1][r]  # bit for bit


def test_eos_finishes_a_row(gpu):
    """a node whose children include token 1: the row that draws it records cur_len + 1"""
    w = World(64, 1, fanouts=(512,), full_vocab=True, seed=3)
    toks, z, absmax = w.logits(0)
    y, kept, _ = S.warp(z, 1.0, 0, 1.0)
    lo, hi, logq = S.cdf(y, kept)
    i = 511  # (planted 4.7) -- and child 1 = EOS is drawn through a second launch with its own interval, if wide
    rows = [(0, i, float(np.float32(0.5 * (lo[i] + hi[i]))), int(toks[i]), float(logq[i]), float(z[i]))]
    out = _launch(w, [0], [rows[0][2]], (1.0, 0, 1.0), 1, 1)
    _check(w, out, rows, 1)
    # plant EOS as the dominant child and draw it
    hn = w.h32[0].double()
    w.E32[1] = (9.0 * hn / float((hn ** 2).sum())).float()
    w.E_dev = U.bf(w.E32)
    w.E64 = w.E_dev.double().cpu()
    toks, z, absmax = w.logits(0)
    rows = [(0, 1, 0.5, 1, float(S.cdf(*S.warp(z, 1.0, 0, 1.0)[:2])[2][1]), float(z[1]))]
    assert S.pick(z, 0.5) == 1
    out = _launch(w, [0], [0.5], (1.0, 0, 1.0), 1, 1, cur_len=3)
    _check(w, out, rows, 1, cur_len=3)
    assert int(out["hyp_len"].view(-1)[0]) == 4


@pytest.mark.parametrize("pieces", [1, 2])
def test_item_filters(gpu, pieces):
    """User 0 excludes the first child, a planted inner child and a block of the tail of every node (dead children); user 1 is
    allowed a single item (one alive child, at one node); user 2 excludes nothing.  Expected: the restatement over the alive
    children only."""
    w = World(64, pieces, fanouts=(33, 65, 257))
    idx = {tuple(c): i for i, c in enumerate(w.cands)}
    dead0 = {m: sorted({0, w.fanouts[m] // 3, *range(5, 5 + w.fanouts[m] // 4)}) for m in range(3)}
    ex0 = [idx[(w.node_tok[m], int(w.children[m][i]))] for m in range(3) for i in dead0[m]]
    only = idx[(w.node_tok[1], int(w.children[1][40]))]
    prm = (1.0, 50, 0.9)
    R = 6
    for mode, lists, alive_of in (
            (_lib.ITEMS_EXCLUDE, [ex0, [], []], lambda b, m: np.setdiff1d(np.arange(w.fanouts[m]), dead0[m]) if b == 0 else None),
            (_lib.ITEMS_ALLOW, [list(range(len(w.cands))), [only], list(range(len(w.cands)))],
             lambda b, m: np.array([40]) if b == 1 else None)):
        ui, keep = U.user_items(w.flat, w.cands, lists, mode)
        rows = []
        for b in range(3):
            nodes = [1] if (mode == _lib.ITEMS_ALLOW and b == 1) else [0, 1, 2]
            combos = []
            for m in nodes:
                alive = alive_of(b, m)
                toks, z, absmax = w.logits(m, alive)
                tg, logq, y = _targets(z, *prm, w.d, absmax)
                combos += [(m, i, u, int(toks[i]), float(logq[i]), float(z[i])) for i, u in tg]
            rows += [combos[r % len(combos)] for r in range(R)]
        out = _launch(w, [c[0] for c in rows], [c[2] for c in rows], prm, 3, R, items=ui)
        _check(w, out, rows, pieces)
        if mode == _lib.ITEMS_EXCLUDE:
            assert not {int(t) for t in out["tokens"][:R]} & {int(w.children[m][i]) for m in range(3) for i in dead0[m]}
        else:
            assert {int(t) for t in out["tokens"][R:2 * R]} == {int(w.children[1][40])}


def test_streamed_equals_resident(worlds):
    """The debug capacity lowered to 64: fan-outs 65, 255, 256, 257 stream through the state's scratch, 63 and 64 stay on chip;
    tokens, nodes and accumulators equal the resident form's bit for bit -- unfiltered and filtered."""
    lib = U.lib()
    for d, pieces in ((64, 1), (1024, 2)):
        w = worlds[(d, pieces)]
        idx = {tuple(c): i for i, c in enumerate(w.cands)}
        ex = [idx[(w.node_tok[m], int(w.children[m][i]))] for m in range(len(w.fanouts)) for i in range(0, w.fanouts[m], 3) if i]
        for prm in ((1.0, 0, 1.0), (0.5, 40, 0.9)):
            rows, _ = _expect_rows(w, prm, 3, 20, range(len(w.fanouts)))
            g = torch.Generator().manual_seed(5)
            us = torch.rand(60, generator=g).tolist()  # (any uniforms: the two forms are compared with each other)
            for items in (None, "exclude"):
                ui = U.user_items(w.flat, w.cands, [ex, [], ex[::2]], _lib.ITEMS_EXCLUDE) if items else (None, None)
                acc0 = torch.randn(2, 60, generator=g)
                args = dict(lse=torch.rand(60, generator=g) + 7, acc0=acc0, items=ui[0], cand_stride=257)
                a = _launch(w, [c[0] for c in rows], us, prm, 3, 20, **args)
                try:
                    assert lib.gram_debug_set_sample_capacity(64) == 0
                    b = _launch(w, [c[0] for c in rows], us, prm, 3, 20, **args)
                    # (without the scratch a streamed launch is refused before it runs)
                    with pytest.raises(_lib.GramHipError):
                        _launch(w, [c[0] for c in rows], us, prm, 3, 20, **dict(args, cand_stride=0))
                finally:
                    lib.gram_debug_set_sample_capacity(0)
                for k in ("tokens", "node", "seq", "hyp_len", "acc_s", "acc_m", "error"):
                    assert torch.equal(a[k], b[k]), (d, pieces, prm, items, k)


def test_a_row_alone_equals_the_row_among_191(worlds):
    w = worlds[(768, 1)]
    prm = (2.0, 5, 0.9)
    rows, combos = _expect_rows(w, prm, 3, 64, range(len(w.fanouts)))
    g = torch.Generator().manual_seed(9)
    us = torch.rand(192, generator=g)
    lse = torch.rand(192, generator=g) + 7
    acc0 = torch.randn(2, 192, generator=g)
    full = _launch(w, [c[0] for c in rows], us.tolist(), prm, 3, 64, lse=lse, acc0=acc0)
    for r in (0, 77, 191):
        one = _launch(w, [rows[r][0]], [float(us[r])], prm, 1, 1, lse=lse[r:r + 1], acc0=acc0[:, r:r + 1].contiguous())
        for k in ("tokens", "node", "acc_s", "acc_m"):
            assert torch.equal(one[k][:1], full[k][r:r + 1]), (r, k)
        assert int(one["seq"][0, 2]) == int(full["seq"][r, 2])


def test_bad_arguments_are_refused(worlds):
    w = worlds[(64, 1)]
    for prm in ((0.0, 0, 1.0), (-1.0, 0, 1.0), (1.0, -1, 1.0), (1.0, 0, 0.0), (1.0, 0, 1.5)):
        with pytest.raises(_lib.GramHipError):
            _launch(w, [0], [0.5], prm, 1, 1)
