"""The host references of tests/vec_kernel_refs.py are checked themselves, without a GPU: Philox against published known answers,
the block-cyclic index map as a bijection, the two shard steps of the distributed Hermitian completion against the serial
completion, pack / unpack as inverses, and the generator's host model against the limits the device fill has to meet."""
import itertools
import numpy as np
import pytest
import vec_kernel_refs as R

GRIDS = [(1, 1), (2, 2), (4, 2), (3, 1)]
BLOCKS = [1, 7, 64]
N_SIZES = [149, 331]                    # primes: no multiple of block * p for any p > 1 or block > 1 used here


@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox4x32_10_known_answers(ctr, key, out):
    """Random123 kat_vectors, philox4x32 10 rounds"""
    got = R.philox4x32_10(ctr, key)
    assert tuple(int(w) for w in got) == out
    # the same through arrays (what the fills use), mixed with another counter
    c = [np.array([w, 0], dtype=np.uint64) for w in ctr]
    k = [np.array([w, 0], dtype=np.uint64) for w in key]
    got = R.philox4x32_10(c, k)
    assert tuple(int(w[0]) for w in got) == out
    assert tuple(int(w[1]) for w in got) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)


def test_uniforms_are_53_bit_and_inside_their_intervals():
    u1, u2 = R.uniforms_ref(np.arange(1 << 12, dtype=np.uint64), 99)
    assert np.all(u1 > 0) and np.all(u1 <= 1) and np.all(u2 >= 0) and np.all(u2 < 1)
    assert np.all(u2 * 2.0 ** 53 == np.floor(u2 * 2.0 ** 53))
    # the counter's high word and the seed's high word are used
    a = R.uniforms_ref(np.array([5], dtype=np.uint64), 1)[0]
    assert a != R.uniforms_ref(np.array([5 + (1 << 32)], dtype=np.uint64), 1)[0]
    assert a != R.uniforms_ref(np.array([5], dtype=np.uint64), 1 + (1 << 32))[0]


@pytest.mark.parametrize("N", N_SIZES)
@pytest.mark.parametrize("b", BLOCKS)
@pytest.mark.parametrize("p", sorted({p for g in GRIDS for p in g}))
def test_bc_global_is_a_bijection_over_the_ranks(N, b, p):
    assert N % (b * p) != 0 or b * p == 1
    seen = []
    for q in range(p):
        g = R.bc_rows(N, b, p, q)
        assert np.all(np.diff(g) > 0) and np.all(g < N) and np.all((g // b) % p == q)      # ascending, inside, on their owner
        assert R.bc_global(len(g), b, p, q) >= N                                            # and the next one is outside
        seen.append(g)
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(N))
    assert R.bc_global(3, 5, 2, 1, off=100) == 100 + 5 + 3


def _shards(H, N, b, pr, pc):
    return {(pi, pj): (R.bc_rows(N, b, pr, pi), R.bc_rows(N, b, pc, pj)) for pi in range(pr) for pj in range(pc)}


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("uplo", ["U", "L"])
@pytest.mark.parametrize("b", BLOCKS)
@pytest.mark.parametrize("grid", GRIDS)
def test_distributed_completion_is_the_serial_one(grid, b, uplo, cplx):
    """tri_mask on every shard, then the conjugate transpose of every shard's piece added into the shard that owns the
    transposed positions (the second hop of symOrHermMatrix), reassembled = complete_hermitian of the whole matrix"""
    N = 149
    pr, pc = grid
    rng = np.random.default_rng(1000 * pr + 100 * pc + b)
    H = R.rand(rng, (N, N), cplx)                         # both triangles and the diagonal's imaginary parts are random
    own = _shards(H, N, b, pr, pc)
    masked = {r: R.tri_mask_ref(H[np.ix_(gi, gj)], uplo, b, pr, r[0], b, pc, r[1]) for r, (gi, gj) in own.items()}
    for r, (gi, gj) in own.items():                       # the mask itself: kept triangle by GLOBAL position
        keep = (gi[:, None] < gj[None, :]) if uplo == "U" else (gi[:, None] > gj[None, :])
        want = np.where(keep, H[np.ix_(gi, gj)], 0) + np.where(gi[:, None] == gj[None, :], H[np.ix_(gi, gj)] / 2, 0)
        assert np.array_equal(masked[r], want)
    result = {r: m.copy() for r, m in masked.items()}
    for src, dst in itertools.product(own, own):
        sgi, sgj = own[src]
        dgi, dgj = own[dst]
        la = np.nonzero(np.isin(sgi, dgj))[0]             # src rows whose global index is a column of dst
        lb = np.nonzero(np.isin(sgj, dgi))[0]             # src columns whose global index is a row of dst
        if len(la) == 0 or len(lb) == 0:
            continue
        P = masked[src][np.ix_(la, lb)]
        rowmap = np.searchsorted(dgj, sgi[la])            # dst local column of P's row a
        colmap = np.searchsorted(dgi, sgj[lb])            # dst local row of P's column b
        result[dst] = R.conj_transpose_add_ref(P, rowmap, colmap, result[dst])
    got = np.zeros_like(H)
    for r, (gi, gj) in own.items():
        got[np.ix_(gi, gj)] = result[r]
    want = R.complete_hermitian_ref(H, uplo)
    d = np.arange(N)
    assert np.array_equal(got[d, d].real, H[d, d].real)   # d/2 + conj(d)/2
    if cplx:
        assert np.all(got[d, d].imag == 0) and np.any(want[d, d].imag != 0)      # the serial one leaves the diagonal alone
    got[d, d] = want[d, d]
    assert np.array_equal(got, want)
    assert np.array_equal(want, want.conj().T) or cplx    # and that is Hermitian up to the diagonal's imaginary part
    w0 = want.copy()
    w0[d, d] = w0[d, d].real
    assert np.array_equal(w0, w0.conj().T)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n", [1, 2, 5, 33])
def test_pack_and_unpack_are_inverses(n, cplx):
    rng = np.random.default_rng(n)
    A = R.rand(rng, (n, n), cplx)
    P = R.pack_upper_ref(A)
    assert P.shape == (n * (n + 1) // 2,)
    assert P[-1] == A[n - 1, n - 1] and P[0] == A[0, 0]
    if n >= 2:
        assert P[1] == A[0, 1] and P[2] == A[1, 1]        # column by column
    mark = np.full((n, n), 7.0, dtype=A.dtype, order="F")
    B = R.unpack_upper_ref(P, mark)
    assert np.array_equal(np.triu(B), np.triu(A)) and np.all(np.tril(B, -1) == np.tril(mark, -1))
    assert np.array_equal(R.unpack_upper_ref(P, mark, mirror=1), R.complete_hermitian_ref(A, "U"))
    L = R.complete_hermitian_ref(A, "L")
    assert np.array_equal(np.tril(L), np.tril(A)) and np.array_equal(np.triu(L, 1), np.tril(A, -1).conj().T)


def test_gathers_and_scalings_on_small_known_cases():
    X = np.asfortranarray(np.arange(12, dtype=np.float64).reshape(4, 3))
    out0 = np.full((5, 3), -1.0, order="F")
    assert np.array_equal(R.rows_indexed_ref(X, [2, 0], out0, 0)[:2], X[[2, 0]])
    assert np.array_equal(R.rows_indexed_ref(X, [4, 1], out0, 1)[[4, 1]], X[:2])
    assert np.array_equal(R.cols_indexed_ref(X, [2, 2, 0]), X[:, [2, 2, 0]])
    Z = np.zeros((4, 2), dtype=np.complex128, order="F")
    Z.real, Z.imag = X[:, :2], np.array([[0.0, -0.0]] * 4)
    S = R.scale_rows_bc_ref(Z, 3, 2, 2, 1, -1.0)          # rank 1 of 2, blocks of 2: local rows are global 2, 3, 6, 7
    assert np.array_equal(S[0], Z[0]) and np.array_equal(S[1:], -Z[1:])
    assert np.signbit(S[1, 0].imag) and not np.signbit(S[1, 1].imag)             # parts scaled one by one: signed zeros flip
    assert np.array_equal(R.scale_rows_ref(X, 1, 2.0), np.vstack([X[:1], 2 * X[1:]]))
    assert np.array_equal(R.col_scal_ref(X, [3.0, 3.0, 3.0], 1), X * (1.0 / 3.0))
    assert np.array_equal(R.shift_list_ref(Z, [1], [0], 0.5), Z + 0.5 * (np.arange(8).reshape(2, 4).T == 1))


def test_clement_shards_tile_the_matrix():
    from oracle.chase_oracle import clement
    N, b = 45, 7
    H = clement(N, True, perturb=0)
    got = np.zeros_like(H)
    for pi in range(3):
        for pj in range(2):
            gi, gj = R.bc_rows(N, b, 3, pi), R.bc_rows(N, b, 2, pj)
            got[np.ix_(gi, gj)] = R.clement_shard_ref(N, True, len(gi), len(gj), b, 3, pi, 0, b, 2, pj, 0)
    assert np.array_equal(got, H)
    assert np.array_equal(R.clement_shard_ref(N, False, 5, 4, N, 1, 0, 10, N, 1, 0, 9), clement(N, False, perturb=0)[10:15, 9:13])


@pytest.mark.parametrize("cplx", [False, True])
def test_fill_model_windows_and_block_cyclic_rows_agree_with_the_whole(cplx):
    gld, n, seed = 37, 5, 12345                           # odd: the real pairing g >> 1 crosses columns
    full = R.fill_normal_ref(cplx, gld, n, 0, 0, gld, seed)
    assert np.array_equal(R.fill_normal_ref(cplx, 9, 2, 11, 3, gld, seed), full[11:20, 3:5])
    for pi in range(3):
        g = R.bc_rows(gld, 7, 3, pi)
        assert np.array_equal(R.fill_normal_ref(cplx, len(g), n, 0, 0, gld, seed, mb=7, pr=3, pi=pi), full[g])
    assert not np.array_equal(R.fill_normal_ref(cplx, gld, n, 0, 0, gld, seed + 1), full)
    if not cplx:                                          # the two halves of a pair are neighbours in column-major order
        z0, z1, _ = R.normal_pair_ref(np.arange(4, dtype=np.uint64), seed)
        assert np.array_equal(full.ravel(order="F")[:8], np.stack([z0, z1], axis=-1).ravel().astype(np.float64))


@pytest.mark.parametrize("cplx,shape", [(False, (512, 512)), (True, (512, 256))])
def test_host_model_meets_the_moment_limits_of_the_device_fill(cplx, shape):
    """the same seed, shape and limits as the device test: 6 sigma of a seeded stream is a fixed outcome"""
    Z = R.fill_normal_ref(cplx, shape[0], shape[1], 0, 0, shape[0], 2024)
    n, stats = R.normal_moments(Z)
    assert n == 1 << 18
    for name, val, lim in stats:
        print(f"host fill {'z' if cplx else 'd'} {name}: {val:.3e} (limit {lim:.3e})")
        assert val <= lim, (name, val, lim)


def test_reduction_references_on_exact_data():
    X = np.asfortranarray(np.array([[1 + 2j, 3.0], [0.5j, -1.0]]))
    Y = np.asfortranarray(np.array([[2 - 1j, 1.0], [4.0, 2.0]]))
    d = R.col_dot_ref(X, Y)
    assert complex(d[0]) == (1 - 2j) * (2 - 1j) + (-0.5j) * 4 and complex(d[1]) == 1.0
    assert complex(R.col_dot_ref(Y, X)[0]) == complex(d[0]).conjugate()
    lam = np.array([2.0, -1.0])
    s = R.resid_sumsq_ref(X, Y, lam)
    assert float(s[0]) == (9 + 16) + (64 + 0.25) and float(s[1]) == 16 + 1      # |-3 + 4i|^2 + |-8 + i/2|^2; 4^2 + 1^2
    assert float(R.resid_sumsq_ref(X)[0]) == 5.25
    assert float(R.abs_trace_ref(np.array([[3 + 4j, 1], [1, -2.0]]))) == 7.0
    ref, br, bi = R.col_axpy_ref(np.array([1 + 1j, 5.0]), 0, 0, -1.0, X, Y)
    assert complex(ref[0, 1]) == 1.0 - (1 + 1j) * 3.0 and float(br[0, 1]) == 5 * R.U * (1 + 2 * 3)
