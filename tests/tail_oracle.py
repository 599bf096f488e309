"""The forest of the tail pass (include/gram_hip.h gram_forest_t, gram_tail_forest, gram_tail_rowpos) in plain Python and numpy: what
tests/test_gpu_tail_forest.py and tests/test_gpu_tail_pass.py compare the kernels of gram_amd/csrc/beam.hip with.  Imports without a
GPU (tests/test_tail_pass_host.py checks the enumeration itself against a plain walk).

  Comb                a Trie whose prefixes of length d_tail = 3 own subtrees of exactly the wanted numbers of forest rows
  random_state        a beam state over a Comb: nodes, tokens, done and the ancestor table from a seeded generator
  enumerate_forest    every table gram_tail_forest must write, but for the slots (handed out in arrival order: they differ from run
                      to run)
  forest_buffers      the device arrays of a gram_forest_t, each with a guard band behind it, everything filled with FILL
  check_forest        the device's arrays against the enumeration, every cell of every array: what is not written still holds FILL
  expected_rowpos     what gram_tail_rowpos must write"""
import numpy as np

from gram_amd import _lib
from gram_amd.utils.generation_trie import FlatTrie, Trie

FILL = -7    # what every cell of every buffer holds before the launch
GUARD = 64   # elements behind every array's documented size
ENTRY = _lib.GRAM_TAIL_ENTRY_ROWS
MAX_STEPS = _lib.GRAM_TAIL_MAX_STEPS
ROW_ARRAYS = ("tokens", "pos", "parent", "root", "node")


# ------------------------------------------------------------------------------------ the comb Trie
def comb_candidates(sizes, height):
    """The candidates of a comb Trie: prefix p = (0, 2 + p // 16, 100 + p % 16) owns a subtree of exactly sizes[p] forest rows (nodes
    that have children, the prefix's node included) -- a chain of min(sizes[p], height) nodes below which EOS ends the candidate,
    and for the rest forks: nodes with the one child EOS, hung on the chain's nodes in turn, their tokens on both sides of the chain's
    (500), so that a level's children in token order are fork, chain, fork.  Returns (candidates, prefixes)."""
    cands, prefixes = [], []
    for p, r in enumerate(sizes):
        pre = [0, 2 + p // 16, 100 + p % 16]
        h = min(r, height)
        assert r >= 1 and (r == h or h >= 2), (r, height)
        cands.append(pre + [500] * (h - 1) + [1])
        for i in range(r - h):
            j, q = i % (h - 1), i // (h - 1)  # the chain node the fork hangs on, and which of that node's forks it is
            cands.append(pre + [500] * j + [499 - q // 2 if q % 2 == 0 else 501 + q // 2, 1])
        prefixes.append(tuple(pre))
    return cands, prefixes


def sub_rows_walk(flat):
    """gram_trie_tail_t.sub_rows by a plain recursive walk of the CSR: a node that has children counts itself and what its children
    count, a leaf and the root count 0."""
    sub = np.zeros(flat.n_nodes, dtype=np.int32)

    def rec(n):
        kids = flat.child_node[int(flat.child_off[n]): int(flat.child_off[n + 1])]
        if len(kids) == 0:
            return 0
        sub[n] = 1 + sum(rec(int(c)) for c in kids)
        return int(sub[n])
    for c in flat.child_node[int(flat.child_off[0]): int(flat.child_off[1])]:
        rec(int(c))
    return sub


class Comb:
    """A comb Trie (comb_candidates): .cands, .flat (the CSR), .sub (sub_rows_walk), .d_tail = 3, .sizes, .height, and per prefix its
    node (.prefix_node) and last token (.prefix_tok); .leaves = the nodes without children."""
    d_tail = 3

    def __init__(self, sizes, height):
        self.sizes, self.height = list(sizes), int(height)
        self.cands, prefixes = comb_candidates(self.sizes, self.height)
        self.flat = FlatTrie(Trie(self.cands))
        self.sub = sub_rows_walk(self.flat)
        self.prefix_node = np.array([self.flat.leaf_of(p) for p in prefixes], dtype=np.int64)
        self.prefix_tok = np.array([p[-1] for p in prefixes], dtype=np.int64)
        assert self.sub[self.prefix_node].tolist() == self.sizes
        fan = np.diff(self.flat.child_off)
        self.leaves = np.nonzero(fan == 0)[0]
        sub_flat, d_flat, _steps = self.flat.tail_tables()
        if d_flat == self.d_tail:  # the Trie qualifies under FlatTrie's rule too: the same table
            assert np.array_equal(sub_flat, self.sub)
        self.qualifies = d_flat == self.d_tail

    @property
    def steps(self):
        """decode steps below d_tail: the height of the tallest subtree"""
        return min(max(self.sizes), self.height)


def random_state(comb, B, K, Tmax, seed, dead=0.1, done=0.05, edges=True):
    """A beam state over the comb: every beam on a prefix of length d_tail drawn from a seeded generator; about `dead` of the beams
    not live -- node -1, a node >= n_nodes or a leaf in turn -- and about `done` of the users finished; the ancestor table random.
    edges: the users at the ends of the batch, of tail_fill_kernel's 64-user blocks and of tail_count_kernel's 1024-user rounds
    (0, 63, 64, 1023, 1024, B - 1 ...) are not finished and get a beam that is not live at their first or their last slot (both for
    every third), and their neighbours 62, 65, 1022, 1025 ... are finished.  -> dict of numpy arrays node, tokens [B * K], done [B],
    anc [Tmax][B * K], all int32."""
    rng = np.random.default_rng(seed)
    R, n_nodes = B * K, comb.flat.n_nodes
    p = rng.integers(0, len(comb.sizes), size=(B, K))
    node, tokens = comb.prefix_node[p].copy(), comb.prefix_tok[p].copy()
    kinds = [lambda: -1, lambda: n_nodes + int(rng.integers(0, 5)), lambda: int(comb.leaves[rng.integers(0, len(comb.leaves))])]
    n_kind = 0
    for b, k in zip(*np.nonzero(rng.random((B, K)) < dead)):
        node[b, k] = kinds[n_kind % 3]()
        n_kind += 1
    fin = rng.random(B) < done
    if edges:
        ends = sorted(b for b in {0, 63, 64, B - 1} | {c - d for c in range(1024, B + 1, 1024) for d in (0, 1)} if 0 <= b < B)
        for i, b in enumerate(ends):
            fin[b] = False
            for k in ((0,), (K - 1,), (0, K - 1))[i % 3]:
                node[b, k] = kinds[n_kind % 3]()
                n_kind += 1
        for b in ends:
            for nb in (b - 1, b + 1):
                if 0 <= nb < B and nb not in ends:
                    fin[nb] = True
    return dict(node=node.reshape(R).astype(np.int32), tokens=tokens.reshape(R).astype(np.int32), done=fin.astype(np.int32),
                anc=rng.integers(0, R, size=(Tmax, R)).astype(np.int32))


# ------------------------------------------------------------------------------------ the enumeration
def live_beams(flat, node, done, B, K):
    """[B][K] bool: the user is not finished and the beam stands on a node of the Trie that has children (beam.hip, tail_live)"""
    node = np.asarray(node, dtype=np.int64).reshape(B, K)
    fan = np.diff(flat.child_off)
    inside = (node >= 0) & (node < flat.n_nodes)
    return inside & (np.asarray(done).reshape(B, 1) == 0) & (fan[np.where(inside, node, 0)] > 0)


def promised_rows(flat, sub_rows, state, B, K):
    """[B]: the forest rows sub_rows promises every user -- what its live beams' subtrees hold"""
    live = live_beams(flat, state["node"], state["done"], B, K)
    safe = np.where(live, np.asarray(state["node"], dtype=np.int64).reshape(B, K), 0)
    return np.where(live, np.maximum(np.asarray(sub_rows, dtype=np.int64)[safe], 0), 0).sum(axis=1)


class Forest:
    """What enumerate_forest returns: the arrays of gram_forest_t that do not depend on the order of arrival (numpy), `fits`,
    `error` (what gram_beam_state_t.error[0] must hold), `n` rows, `n_ent` entries, `per_user`, `level_rows` [2][n_levels]."""


def enumerate_forest(flat, sub_rows, state, B, K, t, cap_rows, cap_entries, n_levels, pad=0):
    """The forest of the beam state (random_state's dict) at position t: rows user-major, inside a user depth-major -- the live beams
    in beam order, then level by level the children that have children, parents in row order, children in token order.  A user
    holds the rows sub_rows promises for its live beams, at most cap_rows + 1; rows promised and not found in the Trie are copies
    of a start row (pad token, position t, parent -1, root b * K, node -1) behind the user's real rows, and error is 3.  Level by
    level for all users at once, so that 4100 users cost a few numpy calls per level."""
    fan = np.diff(flat.child_off).astype(np.int64)
    off, ctok, cnode = flat.child_off.astype(np.int64), flat.child_tok.astype(np.int64), flat.child_node.astype(np.int64)
    node = np.asarray(state["node"], dtype=np.int64).reshape(B, K)
    tokens = np.asarray(state["tokens"], dtype=np.int64).reshape(B, K)
    live = live_beams(flat, node, state["done"], B, K)
    per_user = np.minimum(promised_rows(flat, sub_rows, state, B, K), cap_rows + 1)
    ents = (per_user + ENTRY - 1) // ENTRY
    E = Forest()
    E.per_user = per_user
    E.user_off = np.concatenate([[0], np.cumsum(per_user)])
    E.ent_off = np.concatenate([[0], np.cumsum(ents)])
    E.n, E.n_ent = int(E.user_off[B]), int(E.ent_off[B])
    assert E.n < 2 ** 31
    E.counts = np.zeros(4 + 2 * MAX_STEPS, dtype=np.int64)
    E.counts[:3] = E.n, E.n_ent, int(per_user.max())
    E.fits = E.n <= cap_rows and E.n_ent <= cap_entries
    E.error, E.level_rows = 0, np.zeros((2, n_levels), dtype=np.int64)
    E.B, E.K, E.t, E.n_levels, E.cap_rows, E.cap_entries = B, K, t, n_levels, cap_rows, cap_entries
    if not E.fits:
        return E  # (the kernel writes its counts and the two offset tables only)
    # the rows the Trie holds, level by level
    bb, kk = np.nonzero(live)  # (user-major, beam order)
    lv = [dict(user=bb, root=bb * K + kk, node=node[bb, kk], tok=tokens[bb, kk], par=np.full(len(bb), -1, dtype=np.int64))]
    while len(lv[-1]["node"]):
        nd = lv[-1]["node"]
        cnt = fan[nd]
        edges = np.repeat(off[nd] - (np.cumsum(cnt) - cnt), cnt) + np.arange(int(cnt.sum()))
        par = np.repeat(np.arange(len(nd)), cnt)
        keep = fan[cnode[edges]] > 0
        edges, par = edges[keep], par[keep]
        lv.append(dict(user=lv[-1]["user"][par], root=lv[-1]["root"][par], node=cnode[edges], tok=ctok[edges], par=par))
    lv.pop()
    start = np.concatenate([[0], np.cumsum([len(x["node"]) for x in lv])])
    cat = {k: np.concatenate([x[k] for x in lv]) if lv else np.zeros(0, dtype=np.int64) for k in ("user", "root", "node", "tok")}
    level = np.concatenate([np.full(len(x["node"]), l, dtype=np.int64) for l, x in enumerate(lv)]) if lv else np.zeros(0, dtype=np.int64)
    par = np.concatenate([x["par"] + (start[l - 1] if l else 0) for l, x in enumerate(lv)]) if lv else np.zeros(0, dtype=np.int64)
    order = np.lexsort((level, cat["user"]))  # user-major, then the level; stable: a level keeps its order
    found = np.bincount(cat["user"], minlength=B)
    assert (found <= per_user).all(), "a subtree table that promises fewer rows than the Trie holds is not enumerated here"
    first = np.concatenate([[0], np.cumsum(found)])
    u = cat["user"][order]
    dest = np.empty(len(order), dtype=np.int64)  # forest row of every enumerated row
    dest[order] = E.user_off[u] + (np.arange(len(order)) - first[u])
    # every row starts as the copy of a start row that a promised and missing row is
    owner = np.repeat(np.arange(B), per_user)
    E.tokens, E.pos = np.full(E.n, pad, dtype=np.int64), np.full(E.n, t, dtype=np.int64)
    E.parent, E.root, E.node = np.full(E.n, -1, dtype=np.int64), owner * K, np.full(E.n, -1, dtype=np.int64)
    E.tokens[dest], E.pos[dest], E.root[dest], E.node[dest] = cat["tok"], t + level, cat["root"], cat["node"]
    E.parent[dest] = np.where(par >= 0, dest[np.maximum(par, 0)], -1)
    E.user = owner
    if (found < per_user).any():
        E.error = 3
    # entries: one per 64 rows of a user
    E.ent_users = np.repeat(np.arange(B), ents)
    i = ENTRY * (np.arange(E.n_ent) - E.ent_off[E.ent_users])[:, None] + np.arange(ENTRY)[None, :]
    E.ent_rows = np.where(i < per_user[E.ent_users][:, None], E.user_off[E.ent_users][:, None] + i, -1)
    # rows per (group, level): the even and the odd users
    l = E.pos - t
    ok = l < n_levels
    np.add.at(E.level_rows, ((owner & 1)[ok], l[ok]), 1)
    for g in range(2):
        E.counts[4 + g * MAX_STEPS: 4 + g * MAX_STEPS + n_levels] = E.level_rows[g]
    return E


def expected_lvl_anc(E, slot, anc, Tmax):
    """[2][n_levels][Tmax][B * K]: column s of a (group, level) table belongs to the row of that level with slot s (if s < B * K:
    the table has no more columns) and holds, below t, the column of the search's table (anc) of the row's beam, and at the
    position of each of the row's ancestors that ancestor's slot (if the position is < Tmax and the slot < B * K).  Every other
    cell is not written."""
    R = E.B * E.K
    want = np.full((2, E.n_levels, Tmax, R), FILL, dtype=np.int64)
    l, g = E.pos - E.t, E.user & 1
    col = (l < E.n_levels) & (slot >= 0) & (slot < R)
    for j in range(E.t):
        want[g[col], l[col], j, slot[col]] = anc[j, E.root[col]]
    a = E.parent.copy()
    for _ in range(MAX_STEPS):
        up = col & (a >= 0)
        if not up.any():
            break
        aa = np.maximum(a, 0)
        put = up & (E.pos[aa] >= E.t) & (E.pos[aa] < Tmax) & (slot[aa] >= 0) & (slot[aa] < R)
        want[g[put], l[put], E.pos[aa][put], slot[put]] = slot[aa][put]
        a = np.where(up, E.parent[aa], -1)
    return want


# ------------------------------------------------------------------------------------ buffers and the comparison
def forest_sizes(B, K, Tmax, cap_rows, cap_entries, n_levels):
    """documented elements of every array of gram_forest_t, in the struct's order"""
    R = B * K
    return dict(tokens=cap_rows, pos=cap_rows, parent=cap_rows, root=cap_rows, node=cap_rows, user_off=B + 1, ent_off=B + 1,
                ent_users=cap_entries, ent_rows=cap_entries * ENTRY, rowpos=R, counts=4 + 2 * MAX_STEPS, slot=cap_rows,
                lvl_rows=2 * n_levels * cap_rows, lvl_tokens=2 * n_levels * cap_rows, lvl_anc=2 * n_levels * Tmax * R)


SHAPES = dict(ent_rows=lambda s: (-1, ENTRY), lvl_rows=lambda s: (2, s["n_levels"], -1), lvl_tokens=lambda s: (2, s["n_levels"], -1),
              lvl_anc=lambda s: (2, s["n_levels"], s["Tmax"], s["B"] * s["K"]))


def forest_buffers(device, B, K, Tmax, cap_rows, n_levels, cap_entries=None):
    """(gram_forest_t, {name: device tensor of the documented shape}, the allocation, {name: (offset, elements, guard elements)}): one
    int32 allocation filled with FILL, every array followed by at least GUARD elements no kernel may touch.  cap_entries None: one entry per 64
    rows of the capacity and one per user, what gram_generate_tail carves."""
    import torch
    if cap_entries is None:
        cap_entries = cap_rows // ENTRY + B
    sizes = forest_sizes(B, K, Tmax, cap_rows, cap_entries, n_levels)
    def span(n):  # an array and its guard band, rounded up so that the next array starts on 256 bytes as a workspace's arrays do
        return (n + GUARD + 63) // 64 * 64
    whole = torch.full((sum(span(n) for n in sizes.values()),), FILL, dtype=torch.int32, device=device)
    dims = dict(B=B, K=K, Tmax=Tmax, n_levels=n_levels)
    layout, views, at = {}, {}, 0
    for name, n in sizes.items():
        layout[name] = (at, n, span(n) - n)
        views[name] = whole[at: at + n].view(*SHAPES[name](dims)) if name in SHAPES else whole[at: at + n]
        at += span(n)
    f = _lib.Forest(**{k: v.data_ptr() for k, v in views.items()}, cap_rows=cap_rows, cap_entries=cap_entries, n_levels=n_levels, pad_=0)
    return f, views, whole, layout


def _padded(values, n):
    out = np.full(n, FILL, dtype=np.int64)
    v = np.asarray(values, dtype=np.int64).reshape(-1)
    out[: len(v)] = v
    return out


def check_forest(E, whole, layout, anc, Tmax, rowpos=None):
    """The allocation after gram_tail_forest (and gram_tail_rowpos, if rowpos is given) against the enumeration E: every guard band
    and every cell of every array.  Slots: per (group, level) a permutation of 0..n-1, -1 for a row below the last level; lvl_rows
    and lvl_tokens its inverse; lvl_anc what expected_lvl_anc says for these slots.  Over capacity: the counts and the two offset
    tables, nothing else.  Returns the slots."""
    host = whole.cpu().numpy().astype(np.int64)
    got = {}
    for name, (at, n, guard) in layout.items():
        got[name] = host[at: at + n]
        assert guard >= GUARD and (host[at + n: at + n + guard] == FILL).all(), f"the guard band behind {name} was written"
    assert got["counts"].tolist() == E.counts.tolist(), "counts"
    assert got["user_off"].tolist() == E.user_off.tolist(), "user_off"
    assert got["ent_off"].tolist() == E.ent_off.tolist(), "ent_off"
    want_rowpos = _padded([] if rowpos is None else rowpos, layout["rowpos"][1])
    assert np.array_equal(got["rowpos"], want_rowpos), "rowpos"
    if not E.fits:
        for name in layout:
            if name not in ("counts", "user_off", "ent_off", "rowpos"):
                assert (got[name] == FILL).all(), f"{name} was written for a forest over capacity"
        return None
    for name in ROW_ARRAYS:
        assert np.array_equal(got[name], _padded(getattr(E, name), E.cap_rows)), name
    assert np.array_equal(got["ent_users"], _padded(E.ent_users, E.cap_entries)), "ent_users"
    assert np.array_equal(got["ent_rows"], _padded(E.ent_rows, E.cap_entries * ENTRY)), "ent_rows"
    # slots
    slot = got["slot"][: E.n]
    assert (got["slot"][E.n:] == FILL).all(), "slot behind the last row"
    l, g = E.pos - E.t, E.user & 1
    ok = l < E.n_levels
    assert (slot[~ok] == -1).all(), "a row below the last level has a slot"
    key = g[ok] * E.n_levels + l[ok]
    order = np.lexsort((slot[ok], key))
    rows_of = np.concatenate([[0], np.cumsum(E.level_rows.reshape(-1))])
    assert np.array_equal(slot[ok][order], np.arange(len(order)) - rows_of[key[order]]), "slots are no permutation per (group, level)"
    lvl_rows = np.full((2, E.n_levels, E.cap_rows), FILL, dtype=np.int64)
    lvl_tokens = lvl_rows.copy()
    lvl_rows[g[ok], l[ok], slot[ok]] = np.nonzero(ok)[0]
    lvl_tokens[g[ok], l[ok], slot[ok]] = E.tokens[ok]
    assert np.array_equal(got["lvl_rows"], lvl_rows.reshape(-1)), "lvl_rows"
    assert np.array_equal(got["lvl_tokens"], lvl_tokens.reshape(-1)), "lvl_tokens"
    want = expected_lvl_anc(E, slot, np.asarray(anc, dtype=np.int64), Tmax)
    bad = np.argwhere(got["lvl_anc"].reshape(want.shape) != want)
    assert len(bad) == 0, f"lvl_anc differs at {len(bad)} cells, first (group, level, position, slot) = {bad[0].tolist()}"
    return slot


def expected_rowpos(flat, E, state):
    """(rowpos [B * K], error): the first row of the beam's user whose node is the beam's, -1 for a beam that is not live; a live beam
    whose node is not in its user's forest gets row 0 and sets error 3."""
    live = live_beams(flat, state["node"], state["done"], E.B, E.K).reshape(-1)
    node = np.asarray(state["node"]).reshape(-1)
    out, error = np.full(E.B * E.K, -1, dtype=np.int64), 0
    for r in np.nonzero(live)[0]:
        b = r // E.K
        hit = np.nonzero(E.node[E.user_off[b]: E.user_off[b + 1]] == node[r])[0]
        if len(hit):
            out[r] = E.user_off[b] + hit[0]
        else:
            out[r], error = 0, 3
    return out, error
