"""-m gpu: the forest kernels of the tail pass (gram_amd/csrc/beam.hip: tail_count_kernel, tail_fill_kernel, tail_anc_kernel,
tail_rowpos_kernel) through gram_tail_forest and gram_tail_rowpos, against the plain enumeration of tests/tail_oracle.py.

Integers only: every cell of every array of gram_forest_t is compared, and every array has a guard band behind it (what the header
does not say is written still holds the fill value afterwards).  The beam states are hand-made over a comb Trie -- prefixes of length
3 that own subtrees of 1 to 40 forest rows -- at the user counts where the kernels take another turn: the 1024-user rounds of the
count kernel's scan, the 64-user blocks of the fill kernel, users with 0 to 5 cross-attention entries, forests at and over
capacity, levels the cache has no rows for."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import tail_oracle as T

pytestmark = pytest.mark.gpu
T_POS = T.Comb.d_tail - 1  # position of the beams' rows


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    return gpu_util


@pytest.fixture(scope="module")
def comb():
    return T.Comb(list(range(1, 41)), 6)  # subtrees of 1 .. 40 rows, at most 6 levels deep


class Run:
    """One gram_tail_forest (and gram_tail_rowpos) on a state over a comb: the device buffers and the enumeration."""

    def __init__(self, G, comb, state, B, K, Tmax, n_levels, cap_rows=None, cap_entries=None, sub=None, spare=37):
        from gram_amd import _lib
        self.G, self.comb, self.B, self.K, self.Tmax, self.state = G, comb, B, K, Tmax, state
        sub = comb.sub if sub is None else sub
        if cap_rows is None:
            cap_rows = int(T.promised_rows(comb.flat, sub, state, B, K).sum()) + spare
        self.E = T.enumerate_forest(comb.flat, sub, state, B, K, T_POS, cap_rows, cap_rows // T.ENTRY + B if cap_entries is None else cap_entries,
                                    n_levels)
        self._device(torch.device(G.DEV), sub, cap_rows, n_levels, cap_entries)

    def _device(self, dev, sub, cap_rows, n_levels, cap_entries):
        from gram_amd import _lib
        G, comb, B, K, Tmax, state = self.G, self.comb, self.B, self.K, self.Tmax, self.state
        self.ctrie, _keep = comb.flat.to_device(dev)
        self.sub_d = torch.from_numpy(np.ascontiguousarray(sub)).to(dev)
        self.tail = _lib.TrieTail(self.sub_d.data_ptr(), comb.d_tail, n_levels)
        self.st, self.keep = G.make_beam_state(B, K, Tmax)
        self.upload(state)
        self.keep["anc"].copy_(torch.from_numpy(state["anc"]))
        self.f, self.views, self.whole, self.layout = T.forest_buffers(dev, B, K, Tmax, cap_rows, n_levels, cap_entries)

    def upload(self, state):
        for name in ("node", "tokens", "done"):
            self.keep[name].copy_(torch.from_numpy(state[name]))

    def forest(self):
        from gram_amd import _lib
        _lib.check(self.G.lib().gram_tail_forest(C.byref(self.st), C.byref(self.ctrie), C.byref(self.tail), C.byref(self.f), T_POS,
                                                 self.G.stream()), "gram_tail_forest")
        return self

    def rowpos(self):
        from gram_amd import _lib
        _lib.check(self.G.lib().gram_tail_rowpos(C.byref(self.st), C.byref(self.ctrie), C.byref(self.f), self.G.stream()), "gram_tail_rowpos")
        return self

    def check(self, rowpos=None, error=None):
        torch.cuda.synchronize()
        slot = T.check_forest(self.E, self.whole, self.layout, self.state["anc"], self.Tmax, rowpos)
        assert int(self.keep["error"][0]) == (self.E.error if error is None else error)
        return slot


# ------------------------------------------------------------------------------------ user counts
@pytest.mark.parametrize("B,K", [(1, 4), (2, 4), (63, 4), (64, 4), (65, 4), (1023, 4), (1024, 4), (1025, 4), (2049, 4), (4100, 4), (65, 64)])
def test_every_table_for_every_user_at_the_scan_rounds_and_the_fill_blocks(G, comb, B, K):
    """1024 users per round of tail_count_kernel's scan, 64 per block of tail_fill_kernel, 256 beams per block of
    tail_rowpos_kernel: user counts on both sides of each.  Finished users, beams with node -1, with a node >= n_nodes and on a
    leaf stand at the first and the last slot of the users at those boundaries (tail_oracle.random_state)."""
    Tmax = 12
    state = T.random_state(comb, B, K, Tmax, seed=1000 * B + K)
    r = Run(G, comb, state, B, K, Tmax, n_levels=comb.steps)
    E = r.E
    live = T.live_beams(comb.flat, state["node"], state["done"], B, K)
    assert E.fits and E.error == 0 and E.n == int(E.per_user.sum()) >= 1
    assert not live[0].all() and not live[B - 1].all() and live[0].any() == (E.per_user[0] > 0)
    if B >= 63:
        node = state["node"].reshape(B, K)
        assert state["done"].any() and (node == -1).any() and (node >= comb.flat.n_nodes).any() and np.isin(node, comb.leaves).any()
        assert (E.level_rows > 0).all()  # both groups, every level
    for b in (63, 64, 1023, 1024):  # an odd and an even user on both sides of a block's and of a round's end
        if b < B - 1:
            assert E.per_user[b] > 0 and not live[b].all()
    r.forest().rowpos()
    want, err = T.expected_rowpos(comb.flat, E, state)
    assert err == 0 and (want[~live.reshape(-1)] == -1).all() and (want[live.reshape(-1)] >= 0).all()
    r.check(rowpos=want)


# ------------------------------------------------------------------------------------ entries
def test_users_with_0_to_5_entries_at_every_edge_of_the_64_rows(G, comb):
    K, Tmax = 8, 12
    targets = [0, 1, 63, 64, 65, 127, 128, 129, 130, 200, 320, 0, 64, 1]
    B = len(targets)
    rng = np.random.default_rng(7)
    node = np.zeros((B, K), dtype=np.int32)
    dead = [-1, int(comb.leaves[3]), comb.flat.n_nodes + 1]
    for b, n in enumerate(targets):
        sizes = [40] * (n // 40) + ([n % 40] if n % 40 else [])
        beams = [int(comb.prefix_node[s - 1]) for s in sizes] + [dead[(b + i) % 3] for i in range(K - len(sizes))]
        node[b] = rng.permutation(beams)
    node[11] = comb.prefix_node[39]  # (a finished user's beams stay where they are: it owns no row)
    tok_of = dict(zip(comb.prefix_node.tolist(), comb.prefix_tok.tolist()))
    tokens = np.array([tok_of.get(int(n), 0) for n in node.reshape(-1)], dtype=np.int32)
    state = dict(node=node.reshape(-1), tokens=tokens, done=np.zeros(B, dtype=np.int32),
                 anc=rng.integers(0, B * K, size=(Tmax, B * K)).astype(np.int32))
    state["done"][11] = 1
    r = Run(G, comb, state, B, K, Tmax, n_levels=comb.steps)
    E = r.E
    assert E.per_user.tolist() == targets and E.fits
    assert np.diff(E.ent_off).tolist() == [0, 1, 1, 1, 2, 2, 2, 3, 3, 4, 5, 0, 1, 1] and E.counts[1] == 26 and E.counts[2] == 320
    assert (E.ent_rows[E.ent_off[4] + 1] >= 0).sum() == 1 and (E.ent_rows[E.ent_off[7] + 2] >= 0).sum() == 1  # (65 and 129 rows)
    r.forest().check()
    got = r.views["ent_rows"].cpu().numpy()
    for b, n in enumerate(targets):  # every cell once more, spelled out: a user's rows in order, -1 behind its last row
        cells = got[E.ent_off[b]: E.ent_off[b + 1]].reshape(-1)
        assert cells.tolist() == list(range(int(E.user_off[b]), int(E.user_off[b]) + n)) + [-1] * (len(cells) - n)
        assert r.views["ent_users"][int(E.ent_off[b]): int(E.ent_off[b + 1])].cpu().tolist() == [b] * ((n + 63) // 64)


# ------------------------------------------------------------------------------------ capacity
@pytest.mark.parametrize("case", ["rows-full", "rows-one-over", "entries-full", "entries-one-over", "one-user-over-everything"])
def test_a_forest_at_capacity_fits_and_one_over_it_writes_its_counts_only(G, comb, case):
    B, K, Tmax = 67, 4, 12
    state = T.random_state(comb, B, K, Tmax, seed=5)
    per_user = T.promised_rows(comb.flat, comb.sub, state, B, K)
    n, n_ent = int(per_user.sum()), int(((per_user + 63) // 64).sum())
    cap_rows, cap_entries = dict([("rows-full", (n, None)), ("rows-one-over", (n - 1, None)), ("entries-full", (n + 5, n_ent)),
                                  ("entries-one-over", (n + 5, n_ent - 1)), ("one-user-over-everything", (int(per_user.max()) - 2, None))])[case]
    r = Run(G, comb, state, B, K, Tmax, comb.steps, cap_rows=cap_rows, cap_entries=cap_entries)
    E = r.E
    assert E.fits == case.endswith("full")
    if case == "one-user-over-everything":  # its own count saturates at cap_rows + 1: counts[2] and the offsets behind it say so
        assert E.counts[2] == cap_rows + 1 and int(per_user.max()) > cap_rows + 1 and E.n < n
    else:
        assert E.counts[0] == n and E.counts[1] == n_ent
    r.forest().check()


# ------------------------------------------------------------------------------------ levels
@pytest.mark.parametrize("B", [1, 3])
def test_a_chain_forest_of_the_most_steps_a_pass_replaces(G, B):
    """16 levels; with one user every level of its group holds exactly the B * K rows the cache has per position, and the forest
    exactly cap_rows rows"""
    K, Tmax = 4, 24
    chain = T.Comb([T.MAX_STEPS] * 6, T.MAX_STEPS)
    state = T.random_state(chain, B, K, Tmax, seed=B, dead=0.0, done=0.0, edges=False)
    r = Run(G, chain, state, B, K, Tmax, n_levels=T.MAX_STEPS, spare=0)
    assert r.E.n == r.E.cap_rows == B * K * T.MAX_STEPS and (r.E.level_rows[0] == (B + 1) // 2 * K).all()
    slot = r.forest().check()
    if B == 1:
        assert r.E.level_rows[0].tolist() == [B * K] * T.MAX_STEPS and slot.max() == B * K - 1


@pytest.mark.parametrize("case,n_levels,Tmax", [("fewer-levels-than-the-forest-is-deep", 3, 12), ("one-level", 1, 12),
                                                ("Tmax-inside-the-tail", 6, 5), ("Tmax-right-behind-the-beams", 6, 3)])
def test_rows_below_the_last_level_get_no_slot_and_no_table_row_at_or_beyond_Tmax_is_written(G, comb, case, n_levels, Tmax):
    B, K = 67, 4
    state = T.random_state(comb, B, K, Tmax, seed=11)
    r = Run(G, comb, state, B, K, Tmax, n_levels)
    E = r.E
    assert E.fits and (E.pos - T_POS >= n_levels).any() == (n_levels < comb.steps) and (E.pos >= Tmax).any() == (Tmax < T_POS + comb.steps)
    assert (E.level_rows > 0).all()
    r.forest().check()


# ------------------------------------------------------------------------------------ a subtree table that disagrees with the Trie
def test_rows_the_subtree_table_promises_and_the_trie_does_not_hold_are_copies_of_a_start_row_and_error_3(G, comb):
    B, K, Tmax = 67, 4, 12
    state = T.random_state(comb, B, K, Tmax, seed=13)
    more = comb.sub.copy()
    more[comb.prefix_node[[0, 17, 39]]] += np.array([1, 3, 70], dtype=np.int32)  # (70: the copies alone fill an entry and more)
    r = Run(G, comb, state, B, K, Tmax, comb.steps, sub=more)
    E = r.E
    assert E.error == 3 and E.fits and 0 < (E.node == -1).sum() == E.n - int(T.promised_rows(comb.flat, comb.sub, state, B, K).sum())
    fake = E.node == -1
    assert (E.tokens[fake] == 0).all() and (E.pos[fake] == T_POS).all() and (E.parent[fake] == -1).all() and (E.root[fake] == E.user[fake] * K).all()
    r.forest().check(error=3)


# ------------------------------------------------------------------------------------ gram_tail_rowpos
def _moved(comb, state, B, K, seed):
    """the state some search steps later (the kernel does not ask how many): beams one to three levels down on a node that has
    children, beams on a leaf below them, beams where they were; some users finished; two beams of one user with their nodes swapped"""
    rng = np.random.default_rng(seed)
    flat, fan = comb.flat, np.diff(comb.flat.child_off)
    node, done = state["node"].reshape(B, K).copy(), state["done"].copy()
    live = T.live_beams(flat, node, done, B, K)
    kinds = {"inner": 0, "leaf": 0, "stay": 0}
    for b, k in zip(*np.nonzero(live)):
        pick = ("inner", "leaf", "stay")[int(rng.integers(0, 3))]
        n, steps = int(node[b, k]), int(rng.integers(1, 4)) if pick == "inner" else 99 if pick == "leaf" else 0
        for _ in range(steps):
            kids = flat.child_node[int(flat.child_off[n]): int(flat.child_off[n + 1])]
            kids = kids if pick == "leaf" else kids[fan[kids] > 0]
            if len(kids) == 0:
                break
            n = int(kids[rng.integers(0, len(kids))])
        kinds[pick if n != node[b, k] else "stay"] += 1
        node[b, k] = n
    assert min(kinds.values()) > 10
    now_live = T.live_beams(flat, node, done, B, K)
    finished = [b for b in range(3, B, 9) if now_live[b].any()]
    done[finished] = 1
    swapped = next(b for b in range(B) if not done[b] and now_live[b, 0] and now_live[b, K - 1] and node[b, 0] != node[b, K - 1])
    node[swapped, 0], node[swapped, K - 1] = node[swapped, K - 1], node[swapped, 0]
    assert len(finished) >= 3
    return dict(state, node=node.reshape(-1), done=done), swapped


def test_rowpos_finds_every_beam_its_forest_row_after_a_search_step(G, comb):
    B, K, Tmax = 67, 4, 12
    state = T.random_state(comb, B, K, Tmax, seed=17)
    r = Run(G, comb, state, B, K, Tmax, comb.steps)
    r.forest().check()
    after, swapped = _moved(comb, state, B, K, seed=19)
    want, err = T.expected_rowpos(comb.flat, r.E, after)
    live = T.live_beams(comb.flat, after["node"], after["done"], B, K).reshape(-1)
    assert err == 0 and (want[live] >= 0).all() and (want[~live] == -1).all() and (r.E.pos[want[live]] > T_POS).any()
    assert (r.E.node[want[live]] == after["node"][live]).all() and (r.E.user[want[live]] == np.nonzero(live)[0] // K).all()
    assert want[swapped * K] != want[swapped * K + K - 1]
    r.upload(after)
    r.rowpos().check(rowpos=want, error=0)  # (and gram_tail_rowpos writes nothing else)


def test_rowpos_of_a_live_beam_outside_its_users_forest_is_row_0_and_error_3(G, comb):
    B, K, Tmax = 5, 4, 12
    state = T.random_state(comb, B, K, Tmax, seed=23, dead=0.0, done=0.0, edges=False)
    r = Run(G, comb, state, B, K, Tmax, comb.steps)
    r.forest().check()
    mine = set(state["node"].reshape(B, K)[3].tolist())
    stray = next(int(n) for n in comb.prefix_node if int(n) not in mine)
    after = dict(state, node=state["node"].copy())
    after["node"][3 * K + 1] = stray
    want, err = T.expected_rowpos(comb.flat, r.E, after)
    assert err == 3 and want[3 * K + 1] == 0 and r.E.user_off[3] > 0 and (np.delete(want, 3 * K + 1) >= 0).all()
    r.upload(after)
    r.rowpos().check(rowpos=want, error=3)
