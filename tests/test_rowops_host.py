"""CPU: the argument checks of the row kernels' launchers (gram_amd/csrc/rowops.hip).  Every call below is refused with GRAM_E_ARG
before any launch, so fake pointers do and no GPU is needed; each differs from a legal call in the one argument its comment names."""
from gram_amd import _lib

F = 0x1000  # a non-null, 16-byte aligned address that is never dereferenced
E = _lib.E_ARG


def test_embed_ex_argument_errors_without_gpu():
    lib = _lib.load()

    def xs(rows=8, d=768, ss=F, nblk=12, pieces=1, xs_out=None):
        # (table, ids, ids_are_i64, x, xb, ss, xs_out, nblk, rows, d, pieces, stream)
        return lib.gram_embed_ex_xs(F, F, 1, F, F, ss, xs_out, nblk, rows, d, pieces, None)

    assert xs(rows=0) == E and xs(rows=-3) == E
    assert xs(d=766, nblk=1) == E  # d % 4
    assert xs(d=1028, nblk=1) == E and xs(d=2048, nblk=32) == E  # d > 1024
    assert xs(ss=None) == E
    assert xs(nblk=0) == E and xs(nblk=65) == E
    assert xs(pieces=0) == E and xs(pieces=3) == E
    assert xs(d=784, nblk=1, pieces=2) == E  # two pieces: d % 32
    assert xs(d=96, nblk=1, xs_out=F) == E  # the row factor needs whole 64-column blocks ...
    assert xs(d=160, nblk=2, xs_out=F) == E
    assert xs(d=768, nblk=1, xs_out=F) == E and xs(d=768, nblk=6, xs_out=F) == E  # ... and all of them
    # the two entry points in front of it pass everything on
    assert lib.gram_embed_ex_split(F, F, 1, F, F, F, 12, 0, 768, 1, None) == E
    assert lib.gram_embed_ex_split(F, F, 1, F, F, F, 12, 8, 768, 3, None) == E
    assert lib.gram_embed_ex_split(F, F, 1, F, F, None, 12, 8, 768, 2, None) == E
    assert lib.gram_embed_ex(F, F, 0, F, F, F, 12, 0, 768, None) == E
    assert lib.gram_embed_ex(F, F, 0, F, F, F, 65, 8, 768, None) == E
    assert lib.gram_embed_ex(F, F, 0, F, F, F, 1, 8, 1028, None) == E


def test_embed_plain_argument_errors_without_gpu():
    lib = _lib.load()
    for fn in (lib.gram_embed_i64, lib.gram_embed_i32):
        # (table, ids, x, rows, d, stream)
        assert fn(F, F, F, 0, 768, None) == E and fn(F, F, F, -1, 768, None) == E
        assert fn(F, F, F, 8, 770, None) == E and fn(F, F, F, 8, 3, None) == E  # d % 4


def test_rmsnorm_argument_errors_without_gpu():
    lib = _lib.load()

    def norm(rows=8, d=768, pos=None, N=1, L=1, pieces=1):
        # (x, w, out, rows, d, eps, scale, pos, N, L, passage_map, pieces, stream)
        return lib.gram_rmsnorm_bf16_split(F, F, F, rows, d, 1e-6, 1.0, pos, N, L, None, pieces, None)

    assert norm(rows=0) == E
    assert norm(d=766) == E  # d % 4
    assert norm(d=1028) == E  # d > 1024
    assert norm(pieces=0) == E and norm(pieces=3) == E
    assert norm(d=784, pieces=2) == E  # two pieces: d % 32
    assert norm(pos=F, N=0, L=4) == E and norm(pos=F, N=3, L=0) == E and norm(pos=F, N=-1, L=-1) == E
    # (x, w, out, rows, d, eps, scale, pos, N, L[, passage_map], stream)
    assert lib.gram_rmsnorm_bf16(F, F, F, 0, 768, 1e-6, 1.0, None, 1, 1, None) == E
    assert lib.gram_rmsnorm_bf16(F, F, F, 8, 1028, 1e-6, 1.0, None, 1, 1, None) == E
    assert lib.gram_rmsnorm_bf16(F, F, F, 8, 768, 1e-6, 1.0, F, 0, 4, None) == E
    assert lib.gram_rmsnorm_bf16_map(F, F, F, 8, 766, 1e-6, 1.0, None, 1, 1, None, None) == E
    assert lib.gram_rmsnorm_bf16_map(F, F, F, 8, 768, 1e-6, 1.0, F, 3, 0, F, None) == E


def test_lse_argument_errors_without_gpu():
    lib = _lib.load()
    # (logits, lse, R, V, stream)
    assert lib.gram_row_lse(F, F, 0, 1024, None) == E and lib.gram_row_lse(F, F, -2, 1024, None) == E
    assert lib.gram_row_lse(F, F, 4, 1022, None) == E and lib.gram_row_lse(F, F, 4, 3, None) == E  # V % 4
    # (lse_part, lse, M, nblk, stream)
    assert lib.gram_lse_combine(F, F, 0, 8, None) == E and lib.gram_lse_combine(F, F, 4, 0, None) == E
    assert lib.gram_lse_combine(F, F, -1, 8, None) == E and lib.gram_lse_combine(F, F, 4, -1, None) == E


def test_row_rscale_argument_errors_without_gpu():
    lib = _lib.load()

    def rscale(ss=F, rs=F + 0x100, xs_in=None, xs_out=None, M=8, nblk=12, d=768):
        # (ss, rs, xs_in, xs_out, M, nblk, d, eps, stream)
        return lib.gram_row_rscale_xs(ss, rs, xs_in, xs_out, M, nblk, d, 1e-6, None)

    assert rscale(M=0) == E
    assert rscale(nblk=1, d=64) == E and rscale(nblk=3, d=192) == E  # the partials are read in pairs
    assert rscale(nblk=0) == E
    assert rscale(nblk=2, d=32) == E and rscale(d=0) == E  # d < 64
    assert rscale(ss=None) == E and rscale(rs=None) == E
    assert rscale(xs_in=F + 0x200, xs_out=F + 0x200) == E  # xs_out may not alias xs_in
    # (ss, rs, M, nblk, d, eps, stream)
    assert lib.gram_row_rscale(F, F, 0, 12, 768, 1e-6, None) == E
    assert lib.gram_row_rscale(F, F, 8, 3, 192, 1e-6, None) == E
    assert lib.gram_row_rscale(None, F, 8, 12, 768, 1e-6, None) == E


def test_gather_and_iota_argument_errors_without_gpu():
    lib = _lib.load()

    def gather(cache=F, slot=F, x=F, n=3, L=64, cache_L=64, d=768):
        return lib.gram_gather_passage_x(cache, slot, x, n, L, cache_L, d, None)

    assert gather(cache=None) == E and gather(slot=None) == E and gather(x=None) == E
    assert gather(n=0) == E and gather(L=0) == E and gather(cache_L=0) == E
    assert gather(d=0) == E and gather(d=6) == E
    assert lib.gram_iota_i32(None, 16, None) == E
    assert lib.gram_iota_i32(F, 0, None) == E and lib.gram_iota_i32(F, -5, None) == E
