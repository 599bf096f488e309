"""-m gpu: the entry cross-attention of the tail pass (gram_cross_attn_entries_split) on runs of a user's entries.

One workgroup serves a (head, run of consecutive entries that name one user), two entries at a time, and computes only the 16-slot
tiles that hold a row (dec_attn.hip, cross_attn_runs_kernel).  Every row a table names must come out with exactly the bits
gram_cross_attn_decode_split gives it in a group of K rows of its user (torch.equal on the raw 16-bit patterns), wherever the table
puts it; every row no table names keeps the sentinel.  The step-wise result of a row depends on its query, its user and K alone, so
one reference per (pieces, K, S) serves every table."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SENT = 0x5A5A  # 16-bit sentinel pattern (a finite number in IEEE half and in bfloat16)
B, H = 6, 2
COUNTS = [65, 0, 128, 129, 17, 200]  # rows per user: no entry | runs of 1, 2, 3 and 4 entries | last entries that hold one row
ER = 64  # table slots per entry (GRAM_TAIL_ENTRY_ROWS)
SPARE = 7  # rows of q / out behind the users' that no table names


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests import gpu_util
    return gpu_util


def _bits(t):
    return t.view(torch.int16)


def _rows_of():
    out, base = [], 0
    for c in COUNTS:
        out.append(list(range(base, base + c)))
        base += c
    return out


def _mask(S):
    mask = torch.ones(B, S, dtype=torch.uint8)
    if S >= 160:
        mask[0, 32:64] = 0   # a fully masked 32-key step
        mask[0, 150:] = 0    # a ragged tail
        mask[2, 40:70] = 0
        mask[5, :32] = 0     # the first step fully masked: the second wave of a key split gets step 1's successor
        mask[5, 130:] = 0
    else:
        mask[0, 20:] = 0     # a ragged tail inside the only step
        mask[5, 5:9] = 0
    mask[3, :] = 0           # every key masked: the user keeps all steps (uniform softmax)
    return mask


_REF = {}


def _problem(G, pieces, K, S):
    """q, banks, mask and the step-wise result of every row (computed once per shape, never written again)"""
    key = (pieces, K, S)
    if key in _REF:
        return _REF[key]
    from gram_amd import _lib
    inner = H * 64
    n = sum(COUNTS) + SPARE
    g = torch.Generator().manual_seed(1000 * S + 10 * K + pieces)
    q = G.pieces_of((torch.randn(n, inner, generator=g) * 0.6).to(G.DEV), pieces)
    kb = G.pieces_of((torch.randn(B, H, S, 64, generator=g) * 0.6).to(G.DEV), pieces)
    vt = G.pieces_of(G.vt_blocked((torch.randn(B, H, 64, S, generator=g) * 0.6).to(G.DEV)), pieces)
    mask = _mask(S).to(G.DEV)
    ref = torch.empty(n, pieces * inner, dtype=G.DT, device=G.DEV)
    _bits(ref).fill_(SENT)
    rows_of = _rows_of()
    L_ = G.lib()
    for g0 in range(0, max(COUNTS), K):  # group g0 / K of every user that has one, in one launch (the last group padded with zero queries)
        qg = torch.zeros(pieces, B * K, inner, dtype=G.DT, device=G.DEV)
        take = []
        for b in range(B):
            rs = rows_of[b][g0: g0 + K]
            if rs:
                qg[:, b * K: b * K + len(rs)] = q[:, rs[0]: rs[0] + len(rs)]
                take.append((b, rs))
        og = torch.empty(B * K, pieces * inner, dtype=G.DT, device=G.DEV)
        _lib.check(L_.gram_cross_attn_decode_split(G.p(qg), G.p(kb), G.p(vt), G.p(mask), G.p(og), B, K, H, S, None, None, pieces,
                                                   qg[0].numel(), kb[0].numel(), None, G.stream()), "decode")
        for b, rs in take:
            ref[rs[0]: rs[0] + len(rs)] = og[b * K: b * K + len(rs)]
    torch.cuda.synchronize()
    assert not bool((_bits(ref[: n - SPARE]) == SENT).all(dim=1).any())
    _REF[key] = (q, kb, vt, mask, ref)
    return _REF[key]


def _chunks(user, rows):
    """a user's rows as consecutive entries, the last one padded with -1"""
    return [(user, rows[i: i + ER] + [-1] * (ER - len(rows[i: i + ER]))) for i in range(0, len(rows), ER)]


def _canonical():
    ents = []
    for b, rs in enumerate(_rows_of()):
        ents += _chunks(b, rs)
    return ents


def _non_adjacent():
    r = _rows_of()
    return [(0, r[0][:40] + [-1] * 24), (2, r[2][:64]), (0, r[0][40:] + [-1] * 39), (2, r[2][64:]), (5, r[5][:64]), (0, [-1] * ER),
            (5, r[5][64:128])]


def _holes():
    r = _rows_of()
    none = [-1] * ER
    a = r[2][:10] + [-1] * 3 + r[2][10:13] + [-1] * 16 + r[2][13:29] + r[2][29:34] + [-1] * 11  # holes in a tile | an empty tile between live ones
    assert len(a) == ER
    c = [-1] * 16 + r[2][34:50] + [-1] * 31 + r[2][50:51]
    ents = [(2, a), (2, none), (2, c), (2, none)]                      # an empty entry inside a run and at its end
    ents += [(3, none), (3, r[3][:64]), (3, none)]                     # an empty entry leads a run; the run's second pair is one empty entry
    ents += [(4, none)]                                                # a run that holds nothing
    ents += [(5, [-1] * 63 + r[5][:1]), (5, r[5][1:2] + [-1] * 63), (5, [-1] * 31 + r[5][2:4] + [-1] * 31)]
    return ents


def _shuffled():
    g = torch.Generator().manual_seed(7)
    ents = []
    for b, rs in enumerate(_rows_of()):
        if not rs:
            continue
        pick = [rs[i] for i in torch.randperm(len(rs), generator=g).tolist()][: max(1, (2 * len(rs)) // 3)]  # shuffled, non-contiguous
        slots = pick + [-1] * (len(pick) // 5)
        slots = [slots[i] for i in torch.randperm(len(slots), generator=g).tolist()]
        ents += _chunks(b, slots)
    return ents


# (canonical_key_bits: the canonical tables with the key bits precomputed by gram_mask_key_bits, as generate passes them)
TABLES = {"canonical": _canonical, "canonical_key_bits": _canonical, "non_adjacent": _non_adjacent, "holes": _holes, "shuffled": _shuffled}


def test_the_tables_cover_what_they_claim():
    can = _canonical()
    runs = {}
    for u, _ in can:
        runs[u] = runs.get(u, 0) + 1
    assert runs == {0: 2, 2: 2, 3: 3, 4: 1, 5: 4} and 1 not in runs
    assert sum(s >= 0 for s in can[1][1]) == 1 and sum(s >= 0 for s in can[6][1]) == 1  # last entries with one row
    for name, fn in TABLES.items():
        named = [s for _, e in fn() for s in e if s >= 0]
        assert len(named) == len(set(named)), name  # a row is named once
        assert all(len(e) == ER for _, e in fn()), name
    holes = _holes()
    assert any(all(s < 0 for s in e[16 * t: 16 * t + 16]) and any(s >= 0 for s in e[:16 * t]) and any(s >= 0 for s in e[16 * t + 16:])
               for _, e in holes for t in (1, 2))
    users = [u for u, _ in _non_adjacent()]
    assert users[:3] == [0, 2, 0]


def _entries(G, table, S, K, pieces):
    """what gram_cross_attn_entries_split writes over a sentinel-filled `out`, the reference, and which rows the table names"""
    from gram_amd import _lib
    q, kb, vt, mask, ref = _problem(G, pieces, K, S)
    ents = TABLES[table]()
    i32 = dict(dtype=torch.int32, device=G.DEV)
    ent_users = torch.tensor([u for u, _ in ents], **i32)
    ent_rows = torch.tensor([e for _, e in ents], **i32).contiguous()
    L_ = G.lib()
    key_bits = None
    if table.endswith("key_bits"):
        key_bits = torch.zeros(B * 128, **i32)
        _lib.check(L_.gram_mask_key_bits(G.p(mask), G.p(key_bits), B, S, G.stream()), "key bits")
    out = torch.empty_like(ref)
    _bits(out).fill_(SENT)
    _lib.check(L_.gram_cross_attn_entries_split(G.p(q), G.p(kb), G.p(vt), G.p(mask), G.p(out), len(ents), K, H, S, G.p(ent_users),
                                                G.p(ent_rows), pieces, q[0].numel(), kb[0].numel(), G.p(key_bits), G.stream()), "entries")
    torch.cuda.synchronize()
    named = torch.zeros(ref.shape[0], dtype=torch.bool, device=G.DEV)
    named[ent_rows[ent_rows >= 0].long()] = True
    return out, ref, named


CASES = [(table, S, K, pieces) for table in sorted(TABLES) for S in (32, 160) for K in (4, 20, 40) for pieces in (2, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [2, 1])
@pytest.mark.parametrize("K", [4, 20, 40])  # two waves per key split up to 32 beams, one above: the split is part of a row's bits
@pytest.mark.parametrize("S", [32, 160])    # S = 32: a single key step, the second wave of a split has nothing to do
@pytest.mark.parametrize("table", sorted(TABLES))
def test_entry_runs_equal_the_stepwise_kernel(G, table, S, K, pieces):
    out, ref, named = _entries(G, table, S, K, pieces)
    assert bool(named.any()) and not bool(named.all())
    assert torch.equal(_bits(out)[named], _bits(ref)[named])
    assert bool((_bits(out)[~named] == SENT).all())  # a row no table names is not written


@pytest.mark.gpu
def test_race_screen_of_the_entry_runs_against_the_chaos_build(G, tmp_path):
    """the key loop of cross_attn_runs_kernel has a workgroup barrier per step (two waves share a stage): every case again with
    libgram_hip_chaos.so, whose waves sleep at random behind every barrier, in a child process; the bits must be the product's"""
    lib = os.path.join(ROOT, "gram_amd", "csrc", "libgram_hip_chaos.so")
    if not os.path.exists(lib):
        pytest.skip("libgram_hip_chaos.so not built (make -C gram_amd/csrc CHAOS=1)")
    env = dict(os.environ)
    env["GRAM_LIB"] = lib
    path = str(tmp_path / "chaos.pt")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    chaos = torch.load(path)
    assert len(chaos) == len(CASES)
    for case, got in zip(CASES, chaos):
        out, _, _ = _entries(G, *case)
        assert torch.equal(_bits(out).cpu(), got), case


if __name__ == "__main__":  # --child OUT: every case's `out` with the library GRAM_LIB names
    sys.path.insert(0, ROOT)
    from tests import gpu_util
    assert sys.argv[1] == "--child"
    torch.save([_bits(_entries(gpu_util, *case)[0]).cpu() for case in CASES], sys.argv[2])
