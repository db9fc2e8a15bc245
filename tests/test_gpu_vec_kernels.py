"""The O(N*n) kernels of vec_kernels.hip and gen_kernels.hip (streaming, Lanczos recurrence, shard steps, generators), each called
directly through the C ABI and compared with the plain references of tests/vec_kernel_refs.py.

Every device matrix lives in a window of a larger NaN-filled buffer (odd leading dimension > m, a column in front and one
behind, real windows also one element off the 16-byte boundary where a case asks for it): after a call everything outside the
addressed window is byte-identical to before, and a kernel that reads past its window poisons its result.  Copies and single
IEEE operations are compared bit for bit; sums against long double with bounds derived from the count of roundings (u = 2^-53),
never from what the device gives; every reduction runs twice and must give the same bytes.  Shapes follow the launch geometry:
256-thread blocks, gx = ceil(md / 1024) capped at 64, gy = columns capped at 1024 (generators: 4096), 128 threads per column
in the pack / mirror kernels."""
import ctypes as C
import numpy as np
import pytest
import vec_kernel_refs as R

pytestmark = pytest.mark.gpu

LD, U = R.LD, R.U
EINVAL = -1001
NAN = float("nan")
VEC_SHAPES = [(m, n) for m in (1, 2, 255, 256, 257, 1023, 1025) for n in (1, 3)] + [(65600, 2), (3, 1030)]
GEN_SHAPES = VEC_SHAPES[:-1] + [(3, 4100)]
SQUARE = [1, 2, 127, 128, 129, 300]
GRIDS = [(1, 1), (2, 2), (4, 2), (3, 1)]
BLOCKS = [1, 7, 64]
N_GRID = 149
TYPES = pytest.mark.parametrize("cplx", [False, True], ids=["d", "z"])
_sid = lambda s: "x".join(map(str, s))


def _lib():
    from chase_amd.capi import lib, check
    return lib, check


def _tag(cplx):
    return "z" if cplx else "d"


class Buf:
    """X (m x n) inside a NaN-filled device buffer: leading dimension odd and > row0 + m, `front` columns before the window and
    `back` behind it, the window starting row0 elements below the top of its column"""

    def __init__(self, ctx, X, front=1, back=1, row0=0, pad=3, dtype=None):
        X = np.asarray(X)
        self.dtype = np.dtype(dtype or (np.complex128 if np.iscomplexobj(X) else np.float64))
        self.m, self.n, self.front, self.row0 = X.shape[0], X.shape[1], front, row0
        self.ld = (self.m + row0 + pad) | 1
        fill = complex(NAN, NAN) if self.dtype.kind == "c" else (NAN if self.dtype.kind == "f" else -1)
        self.img = np.full((self.ld, front + self.n + back), fill, dtype=self.dtype, order="F")
        self.img[row0:row0 + self.m, front:front + self.n] = X
        self.d = ctx.empty(self.img.shape, self.dtype).upload(self.img)
        self.ptr = self.d.ptr + (front * self.ld + row0) * self.dtype.itemsize

    def window(self, img):
        return img[self.row0:self.row0 + self.m, self.front:self.front + self.n]

    def get(self, rows=None, cols=None):
        """the window after a call (its first rows x cols part), having checked that nothing else of the buffer changed"""
        got = self.d.download()
        rows, cols = self.m if rows is None else rows, self.n if cols is None else cols
        keep = self.img.copy(order="F")
        keep[self.row0:self.row0 + rows, self.front:self.front + cols] = got[self.row0:self.row0 + rows, self.front:self.front + cols]
        assert got.tobytes() == keep.tobytes(), "the call wrote outside its window"
        return np.asfortranarray(self.window(got)[:rows, :cols])

    def unchanged(self):
        """nothing of the buffer changed (inputs)"""
        self.get(0, 0)
        return True

    def reset(self):
        self.d.upload(self.img)

    def free(self):
        self.d.free()


def _ints(ctx, idx):
    return Buf(ctx, np.asarray(idx, dtype=np.int32).reshape(-1, 1), dtype=np.int32)


def _free(*bufs):
    for b in bufs:
        b.free()


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _parts_err(got, ref):
    """|got - ref| per real component in long double: arrays (re, im) for complex, (re,) for real"""
    if np.iscomplexobj(got):
        return np.abs(got.real.astype(LD) - ref.real), np.abs(got.imag.astype(LD) - ref.imag)
    return (np.abs(got.astype(LD) - ref),)


# ================================================================================================================================
# bit-exact operations
# ================================================================================================================================
@TYPES
@pytest.mark.parametrize("shape", VEC_SHAPES, ids=_sid)
def test_rows_indexed_gather_and_scatter(ctx, cplx, shape):
    lib, check = _lib()
    npk, n = shape
    rng = np.random.default_rng(npk * 31 + n)
    big = npk + 5
    idx = rng.permutation(big)[:npk]                              # a proper subset, out of order
    # gather: out[p, :] = in[idx[p], :]
    src, dst, di = Buf(ctx, R.rand(rng, (big, n), cplx), pad=3), Buf(ctx, R.rand(rng, (npk, n), cplx), pad=12), _ints(ctx, idx)
    assert src.ld != dst.ld
    check(lib.chase_hip_rows_indexed(ctx.h, int(cplx), src.ptr, src.ld, dst.ptr, dst.ld, di.ptr, npk, n, 0), "rows_indexed")
    assert _same(dst.get(), R.rows_indexed_ref(src.window(src.img), idx, dst.window(dst.img), 0))
    assert src.unchanged() and di.unchanged()
    _free(src, dst)
    # scatter: out[idx[p], :] = in[p, :]; the rows of out that idx does not name stay
    src, dst = Buf(ctx, R.rand(rng, (npk, n), cplx), pad=6), Buf(ctx, R.rand(rng, (big, n), cplx), pad=3)
    assert src.ld != dst.ld
    check(lib.chase_hip_rows_indexed(ctx.h, int(cplx), src.ptr, src.ld, dst.ptr, dst.ld, di.ptr, npk, n, 1), "rows_indexed")
    assert _same(dst.get(), R.rows_indexed_ref(src.window(src.img), idx, dst.window(dst.img), 1))
    _free(src, dst, di)


@TYPES
@pytest.mark.parametrize("shape", VEC_SHAPES, ids=_sid)
def test_cols_indexed_with_repeated_sources(ctx, cplx, shape):
    lib, check = _lib()
    m, n = shape
    rng = np.random.default_rng(m * 17 + n)
    nsrc = max(2, n // 2 + 1)
    idx = rng.integers(0, nsrc, n)
    if n >= 3:
        idx[1] = idx[0]                                           # a repeated source column
    src, dst, di = Buf(ctx, R.rand(rng, (m, nsrc), cplx), pad=4), Buf(ctx, R.rand(rng, (m, n), cplx), pad=7), _ints(ctx, idx)
    check(lib.chase_hip_cols_indexed(ctx.h, int(cplx), m, src.ptr, src.ld, dst.ptr, dst.ld, di.ptr, n), "cols_indexed")
    assert _same(dst.get(), R.cols_indexed_ref(src.window(src.img), idx))
    _free(src, dst, di)


@TYPES
@pytest.mark.parametrize("n", SQUARE)
def test_pack_and_unpack_upper(ctx, cplx, n):
    lib, check = _lib()
    rng = np.random.default_rng(n)
    A = R.rand(rng, (n, n), cplx)
    dA = Buf(ctx, A)
    np_ = n * (n + 1) // 2
    dP = Buf(ctx, np.full((np_, 1), 5.0, dtype=R.dt_of(cplx)), row0=1)
    check(lib.chase_hip_pack_upper(ctx.h, int(cplx), n, dA.ptr, dA.ld, dP.ptr), "pack_upper")
    P = dP.get()
    assert _same(P[:, 0], R.pack_upper_ref(A))
    for mirror in (0, 1):
        dB = Buf(ctx, R.rand(rng, (n, n), cplx))
        check(lib.chase_hip_unpack_upper(ctx.h, int(cplx), n, dP.ptr, dB.ptr, dB.ld, mirror), "unpack_upper")
        assert _same(dB.get(), R.unpack_upper_ref(P[:, 0], dB.window(dB.img), mirror))
        dB.free()
    _free(dA, dP)


@TYPES
@pytest.mark.parametrize("uplo", ["U", "L", "u", "l"])
@pytest.mark.parametrize("n", SQUARE)
def test_complete_hermitian(ctx, cplx, uplo, n):
    lib, check = _lib()
    rng = np.random.default_rng(n + ord(uplo))
    A = R.rand(rng, (n, n), cplx)                                 # the diagonal's imaginary part is random too: it stays
    dA = Buf(ctx, A)
    check(lib.chase_hip_complete_hermitian(ctx.h, int(cplx), uplo.encode(), n, dA.ptr, dA.ld), "complete_hermitian")
    got = dA.get()
    assert _same(got, R.complete_hermitian_ref(A, uplo))
    assert _same(np.diagonal(got), np.diagonal(A))
    dA.free()


@TYPES
@pytest.mark.parametrize("n", SQUARE)
def test_set_identity(ctx, cplx, n):
    lib, check = _lib()
    dA = Buf(ctx, np.full((n, n), NAN, dtype=R.dt_of(cplx)), pad=5)
    assert dA.ld > n
    check(lib.chase_hip_set_identity(ctx.h, int(cplx), n, dA.ptr, dA.ld), "set_identity")
    assert _same(dA.get(), np.asfortranarray(np.eye(n, dtype=R.dt_of(cplx))))
    dA.free()


@TYPES
@pytest.mark.parametrize("cnt", [1, 256, 257, 1025])
def test_shift_list_adds_to_the_real_parts_of_the_listed_positions(ctx, cplx, cnt):
    lib, check = _lib()
    rng = np.random.default_rng(cnt)
    m, n = 70, 41
    H = R.rand(rng, (m, n), cplx)
    pos = rng.choice(m * n, cnt, replace=False)                   # unique positions
    rows, cols = pos % m, pos // m
    dH, dr, dc = Buf(ctx, H), _ints(ctx, rows), _ints(ctx, cols)
    check(lib.chase_hip_shift_list(ctx.h, int(cplx), dH.ptr, dH.ld, dr.ptr, dc.ptr, cnt, 0.375), "shift_list")
    got = dH.get()
    assert _same(got, R.shift_list_ref(H, rows, cols, 0.375))
    if cplx:
        assert _same(got.imag, H.imag)
    _free(dH, dr, dc)


@TYPES
@pytest.mark.parametrize("shape", VEC_SHAPES, ids=_sid)
def test_scale_rows(ctx, cplx, shape):
    lib, check = _lib()
    m, n = shape
    rng = np.random.default_rng(m + 7 * n)
    X = R.rand(rng, (m, n), cplx)
    for row0 in sorted({0, m // 2, m - 1, m}):
        dX = Buf(ctx, X, row0=0 if cplx else 1)
        check(lib.chase_hip_scale_rows(ctx.h, int(cplx), m, n, dX.ptr, dX.ld, row0, -1.7), "scale_rows")
        assert _same(dX.get(), R.scale_rows_ref(X, row0, -1.7)), row0
        dX.free()


@TYPES
@pytest.mark.parametrize("nb", BLOCKS)
@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", [(257, 3), (1025, 1), (3, 1030)], ids=_sid)
def test_scale_rows_bc(ctx, cplx, nb, p, shape):
    lib, check = _lib()
    m, n = shape
    rng = np.random.default_rng(m + nb + p)
    X = R.rand(rng, (m, n), cplx)
    g0 = ((m * p // 2) // nb) * nb + nb // 2                      # in the middle of a block (nb = 1: on it)
    for q in range(p):
        dX = Buf(ctx, X)
        check(lib.chase_hip_scale_rows_bc(ctx.h, int(cplx), m, n, dX.ptr, dX.ld, g0, nb, p, q, -1.0), "scale_rows_bc")
        assert _same(dX.get(), R.scale_rows_bc_ref(X, g0, nb, p, q, -1.0)), q
        dX.free()


@TYPES
@pytest.mark.parametrize("shape", VEC_SHAPES, ids=_sid)
def test_col_scal_direct_and_inverse(ctx, cplx, shape):
    lib, check = _lib()
    m, n = shape
    rng = np.random.default_rng(3 * m + n)
    X = R.rand(rng, (m, n), cplx)
    a = rng.uniform(0.5, 3.0, n) * rng.choice([-1.0, 1.0], n)
    da = Buf(ctx, a.reshape(-1, 1), row0=1)
    for inverse in (0, 1):
        dX = Buf(ctx, X, row0=0 if cplx else 1)
        check(lib.chase_hip_col_scal(ctx.h, int(cplx), m, n, da.ptr, inverse, dX.ptr, dX.ld), "col_scal")
        assert _same(dX.get(), R.col_scal_ref(X, a, inverse)), inverse        # inverse: x * (1 / a), two roundings
        dX.free()
    da.free()


def _layout_shards(N, b, pr, pc):
    return [((pi, pj), R.bc_rows(N, b, pr, pi), R.bc_rows(N, b, pc, pj)) for pi in range(pr) for pj in range(pc)]


@TYPES
@pytest.mark.parametrize("uplo", ["U", "L"])
@pytest.mark.parametrize("b", BLOCKS)
@pytest.mark.parametrize("grid", GRIDS, ids=_sid)
def test_tri_mask_bc_on_every_shard(ctx, cplx, uplo, b, grid):
    lib, check = _lib()
    pr, pc = grid
    rng = np.random.default_rng(100 * pr + 10 * pc + b)
    H = R.rand(rng, (N_GRID, N_GRID), cplx)
    for (pi, pj), gi, gj in _layout_shards(N_GRID, b, pr, pc):
        if len(gi) == 0 or len(gj) == 0:
            continue
        loc = np.asfortranarray(H[np.ix_(gi, gj)])
        dH = Buf(ctx, loc)
        check(lib.chase_hip_tri_mask_bc(ctx.h, int(cplx), uplo.encode(), len(gi), len(gj), dH.ptr, dH.ld, b, pr, pi, b, pc, pj),
              "tri_mask_bc")
        got = dH.get()
        want = R.tri_mask_ref(loc, uplo, b, pr, pi, b, pc, pj)
        assert _same(got, want), (pi, pj)                          # bytes: the zeros are +0.0
        dH.free()


@TYPES
@pytest.mark.parametrize("shape", [(1030, 3), (3, 1030)], ids=_sid)
def test_tri_mask_bc_past_one_block_of_rows_and_the_column_cap(ctx, cplx, shape):
    lib, check = _lib()
    mloc, nloc = shape
    rng = np.random.default_rng(mloc)
    mb, pr, pi, nb, pc, pj = (7, 2, 0, 1, 1, 0) if mloc > nloc else (1, 1, 0, 5, 3, 0)     # global (0,0), (1,1), (2,2) are inside
    loc = R.rand(rng, (mloc, nloc), cplx)
    for uplo in ("U", "L"):
        dH = Buf(ctx, loc)
        check(lib.chase_hip_tri_mask_bc(ctx.h, int(cplx), uplo.encode(), mloc, nloc, dH.ptr, dH.ld, mb, pr, pi, nb, pc, pj), "tri_mask_bc")
        want = R.tri_mask_ref(loc, uplo, mb, pr, pi, nb, pc, pj)
        assert _same(dH.get(), want)
        assert not _same(want, loc) and np.any(want != 0)
        dH.free()


@TYPES
@pytest.mark.parametrize("shape", [(1, 1), (257, 3), (1025, 2), (3, 1030)], ids=_sid)
def test_conj_transpose_add(ctx, cplx, shape):
    lib, check = _lib()
    nr, nc = shape
    rng = np.random.default_rng(nr + nc)
    P = R.rand(rng, (nr, nc), cplx)
    H = R.rand(rng, (nc + 3, nr + 2), cplx)
    rowmap, colmap = rng.permutation(nr + 2)[:nr], rng.permutation(nc + 3)[:nc]              # injective
    dP, dH, dr, dc = Buf(ctx, P, pad=5), Buf(ctx, H), _ints(ctx, rowmap), _ints(ctx, colmap)
    check(lib.chase_hip_conj_transpose_add(ctx.h, int(cplx), nr, nc, dP.ptr, dP.ld, dr.ptr, dc.ptr, dH.ptr, dH.ld), "conj_transpose_add")
    assert _same(dH.get(), R.conj_transpose_add_ref(P, rowmap, colmap, H))
    _free(dP, dH, dr, dc)


@pytest.fixture(scope="module")
def sqrt_mismatches(ctx):
    """how many of 4096 device square roots differ from the correctly rounded one (0: the device's sqrt is correctly rounded on
    this sample; the Clement test then asks for identical bits)"""
    lib, check = _lib()
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(0, 4, 2048), 10.0 ** rng.uniform(-300, 300, 2040), [0.0, 1.0, 2.0, 4.0, 1e-310, 5e-324, 0.25, 3.0]])
    dx = Buf(ctx, x.reshape(-1, 1), row0=1)
    check(lib.chase_hip_sqrt_inplace(ctx.h, dx.ptr, x.size), "sqrt_inplace")
    got = dx.get()[:, 0]
    dx.free()
    return int(np.count_nonzero(got != np.sqrt(x)))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_sqrt_inplace_within_one_ulp(ctx, n, sqrt_mismatches):
    lib, check = _lib()
    rng = np.random.default_rng(n)
    x = rng.uniform(0, 1, n) * 10.0 ** rng.integers(-200, 200, n)
    dx = Buf(ctx, x.reshape(-1, 1), row0=1)
    check(lib.chase_hip_sqrt_inplace(ctx.h, dx.ptr, n), "sqrt_inplace")
    got = dx.get()[:, 0]
    dx.free()
    want = np.sqrt(x)
    print(f"sqrt_inplace n={n}: {np.count_nonzero(got != want)} of {n} elements differ from the correctly rounded root "
          f"({sqrt_mismatches} of 4096 on the shared sample)")
    assert np.all(np.abs(got - want) <= np.spacing(want))


@TYPES
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "one-element-off"])
@pytest.mark.parametrize("shape", [(256, 3), (2, 1), (1024, 2), (65600, 2), (4, 1030)], ids=_sid)
def test_lacpy_both_branches_of_the_16_byte_switch(ctx, cplx, shape, shift):
    """even row counts and even leading dimensions on both sides: real data 16-byte aligned takes the two-doubles-per-lane copy,
    the same data one element further down the scalar one; complex data is always 16-byte aligned"""
    lib, check = _lib()
    m, n = shape
    rng = np.random.default_rng(m + n + shift)
    src = Buf(ctx, R.rand(rng, (m, n), cplx), front=2, row0=shift, pad=n + 3)           # two columns in front: an even offset
    dst = Buf(ctx, R.rand(rng, (m, n), cplx), front=2, row0=shift, pad=n + 3)
    lds, ldd = src.ld + 1, dst.ld - 1                             # even, still >= m + shift (views of the same buffers)
    assert lds % 2 == 0 and ldd % 2 == 0 and ldd >= m + shift
    # with a leading dimension that is not the buffer's the window is a different set of elements: compare flat images
    es = src.dtype.itemsize
    simg, dimg = src.img.ravel(order="F"), dst.img.ravel(order="F").copy()
    s0, d0 = (src.ptr - src.d.ptr) // es, (dst.ptr - dst.d.ptr) // es
    assert s0 + (n - 1) * lds + m <= simg.size and d0 + (n - 1) * ldd + m <= dimg.size
    check(lib.chase_hip_lacpy(ctx.h, int(cplx), m, n, src.ptr, lds, dst.ptr, ldd), "lacpy")
    for j in range(n):
        dimg[d0 + j * ldd: d0 + j * ldd + m] = simg[s0 + j * lds: s0 + j * lds + m]
    assert _same(dst.d.download().ravel(order="F"), dimg)
    assert (src.ptr % 16 == 0) == (cplx or shift == 0) and (dst.ptr % 16 == 0) == (cplx or shift == 0)
    _free(src, dst)


# ================================================================================================================================
# bounded operations: long double reference, bounds from the count of roundings
# ================================================================================================================================
@TYPES
@pytest.mark.parametrize("shape", VEC_SHAPES, ids=_sid)
def test_col_axpy_every_scalar_form_the_impls_use(ctx, cplx, shape):
    lib, check = _lib()
    m, n = shape
    rng = np.random.default_rng(5 * m + n)
    X, Y = R.rand(rng, (m, n), cplx), R.rand(rng, (m, n), cplx)
    worst = 0.0
    for a_is_real, a_stride in ((0, 1), (1, 1), (0, 0)):
        a_cplx = cplx and not a_is_real
        a = R.rand(rng, (n if a_stride else 1, 1), a_cplx)
        for sgn in (1.0, -1.0):
            da, dX, dY = Buf(ctx, a, row0=1), Buf(ctx, X, pad=4), Buf(ctx, Y)
            check(lib.chase_hip_col_axpy(ctx.h, int(cplx), m, n, da.ptr, a_is_real, a_stride, sgn, dX.ptr, dX.ld, dY.ptr, dY.ld),
                  "col_axpy")
            got = dY.get()
            ref, br, bi = R.col_axpy_ref(a[:, 0], a_is_real or not cplx, a_stride, sgn, X, Y)
            errs = _parts_err(got, ref)
            for e, b in zip(errs, (br, bi)):
                worst = max(worst, float(np.max(e / b)))
                assert np.all(e <= b), (a_is_real, a_stride, sgn, float(np.max(e / b)))
            _free(da, dX, dY)
    print(f"col_axpy {_tag(cplx)} {m}x{n}: max err / bound = {worst:.3f}")


@TYPES
@pytest.mark.parametrize("shape", VEC_SHAPES + [(0, 3)], ids=_sid)
def test_col_dot(ctx, cplx, shape):
    lib, check = _lib()
    m, n = shape
    e = 2 if cplx else 1
    rng = np.random.default_rng(11 * m + n)
    X, Y = R.rand(rng, (m, n), cplx), R.rand(rng, (m, n), cplx)
    dX, dY = Buf(ctx, X, pad=4), Buf(ctx, Y, row0=0 if cplx else 1)
    dO = Buf(ctx, np.full((n * e, 1), NAN), row0=1)

    def run(a, b):
        outs = []
        for _ in range(2):
            dO.reset()
            check(lib.chase_hip_col_dot(ctx.h, int(cplx), m, n, a.ptr, a.ld, b.ptr, b.ld, dO.ptr), "col_dot")
            outs.append(dO.get()[:, 0])
        assert _same(outs[0], outs[1])                            # fixed summation order
        return (outs[0][0::2] + 1j * outs[0][1::2]) if cplx else outs[0]

    xy, yx = run(dX, dY), run(dY, dX)
    if m == 0:
        assert _same(xy, np.zeros(n, dtype=R.dt_of(cplx))) and _same(yx, xy)                  # exact zeros
    else:
        ref, bound = R.col_dot_ref(X, Y), R.col_dot_bound(X, Y)
        errs = _parts_err(xy, ref)
        print(f"col_dot {_tag(cplx)} {m}x{n}: max err / bound = {max(float(np.max(x / bound)) for x in errs):.3f}")
        for x in errs:
            assert np.all(x <= bound)
        for x in _parts_err(yx, np.conj(ref)):                    # y^H x: the imaginary part flips sign
            assert np.all(x <= bound)
        if cplx:
            assert np.all(np.abs(ref.imag) > bound) and np.all(np.sign(xy.imag) == -np.sign(yx.imag))
    _free(dX, dY, dO)


def _resid_inputs(rng, m, n, cplx, kind):
    V = R.rand(rng, (m, n), cplx)
    lam = rng.uniform(0.5, 3, n) * rng.choice([-1.0, 1.0], n)
    if kind == "random":
        return R.rand(rng, (m, n), cplx), V, lam
    if kind == "cancelling":                                      # W = lam V + 1e-9 noise
        W = np.asfortranarray(V * lam[None, :] + 1e-9 * R.rand(rng, (m, n), cplx))
        return W, V, lam
    return R.rand(rng, (m, n), cplx), None, None                   # V == NULL: plain column norms


@TYPES
@pytest.mark.parametrize("kind", ["random", "cancelling", "null-V"])
@pytest.mark.parametrize("shape", VEC_SHAPES, ids=_sid)
def test_resid_norms_host_and_device_forms(ctx, cplx, kind, shape):
    lib, check = _lib()
    m, n = shape
    rng = np.random.default_rng(13 * m + n)
    W, V, lam = _resid_inputs(rng, m, n, cplx, kind)
    dW = Buf(ctx, W, pad=4)
    dV = Buf(ctx, V, row0=0 if cplx else 1) if V is not None else None
    vptr, vld, lptr = (dV.ptr, dV.ld, lam.ctypes.data) if V is not None else (None, 0, None)
    dO = Buf(ctx, np.full((n, 1), NAN), row0=1)
    res = {}
    for squared in (1, 0):
        outs = []
        for _ in range(2):
            host = np.full(n + 2, NAN)
            check(lib.chase_hip_resid_norms(ctx.h, int(cplx), m, n, dW.ptr, dW.ld, vptr, vld, lptr, host[1:].ctypes.data, squared),
                  "resid_norms")
            assert np.isnan(host[0]) and np.isnan(host[-1])
            dO.reset()
            check(lib.chase_hip_resid_norms_dev(ctx.h, int(cplx), m, n, dW.ptr, dW.ld, vptr, vld, lptr, dO.ptr, squared), "resid_norms_dev")
            dev = dO.get()[:, 0]
            assert _same(dev, host[1:-1])                         # the two forms: the same bytes
            outs.append(dev)
        assert _same(outs[0], outs[1])                            # fixed summation order
        res[squared] = outs[0]
    ref, bound = R.resid_sumsq_ref(W, V, lam), R.resid_sumsq_bound(W, V, lam)
    err = np.abs(res[1].astype(LD) - ref)
    print(f"resid_norms {_tag(cplx)} {kind} {m}x{n}: max err / bound = {float(np.max(err / bound)):.3f}")
    assert np.all(err <= bound)
    if kind == "cancelling":
        assert np.all(ref < 1e-12 * R.resid_sumsq_ref(W))          # the case cancels: a wrong lambda or operand is O(1) off
    root = np.sqrt(res[1])
    assert np.all(np.abs(res[0] - root) <= np.spacing(root))       # the sqrt form: 1 ulp of the root of the squared form's output
    dW.free()
    if dV:
        dV.free()
    dO.free()


@TYPES
@pytest.mark.parametrize("shape", VEC_SHAPES + [(0, 3)], ids=_sid)
def test_col_sumsq_and_col_nrm2(ctx, cplx, shape):
    lib, check = _lib()
    m, n = shape
    rng = np.random.default_rng(17 * m + n)
    X = R.rand(rng, (m, n), cplx)
    dX, dO = Buf(ctx, X, row0=0 if cplx else 1), Buf(ctx, np.full((n, 1), NAN), row0=1)
    res = {}
    for name, fn in (("sumsq", lib.chase_hip_col_sumsq), ("nrm2", lib.chase_hip_col_nrm2)):
        outs = []
        for _ in range(2):
            dO.reset()
            check(fn(ctx.h, int(cplx), m, n, dX.ptr, dX.ld, dO.ptr), "col_" + name)
            outs.append(dO.get()[:, 0])
        assert _same(outs[0], outs[1])
        res[name] = outs[0]
    if m == 0:
        assert _same(res["sumsq"], np.zeros(n)) and _same(res["nrm2"], np.zeros(n))
    else:
        ref, bound = R.resid_sumsq_ref(X), R.resid_sumsq_bound(X)
        err = np.abs(res["sumsq"].astype(LD) - ref)
        print(f"col_sumsq {_tag(cplx)} {m}x{n}: max err / bound = {float(np.max(err / bound)):.3f}")
        assert np.all(err <= bound)
        root = np.sqrt(res["sumsq"])
        assert np.all(np.abs(res["nrm2"] - root) <= np.spacing(root))
    _free(dX, dO)


@TYPES
@pytest.mark.parametrize("n", [1, 257, 600])
def test_abs_trace(ctx, cplx, n):
    lib, check = _lib()
    rng = np.random.default_rng(n)
    A = R.rand(rng, (n, n), cplx)
    dA = Buf(ctx, A)
    outs = []
    for _ in range(2):
        t = C.c_double(NAN)
        check(lib.chase_hip_abs_trace(ctx.h, int(cplx), n, dA.ptr, dA.ld, C.byref(t)), "abs_trace")
        outs.append(t.value)
    assert outs[0] == outs[1]
    ref = R.abs_trace_ref(A)
    bound = (n + 4) * U * ref
    print(f"abs_trace {_tag(cplx)} n={n}: err / bound = {float(abs(LD(outs[0]) - ref) / bound):.3f}")
    assert abs(LD(outs[0]) - ref) <= bound
    assert dA.unchanged()
    dA.free()


# ================================================================================================================================
# generators
# ================================================================================================================================
def _fill(ctx, cplx, m, n, grow0, gcol0, gld, seed, bc=None):
    """one device fill of an m x n window inside a NaN-filled buffer; bc = (mb, pr, pi) for block-cyclic rows"""
    lib, check = _lib()
    dX = Buf(ctx, np.full((m, n), NAN, dtype=R.dt_of(cplx)), row0=0 if cplx else 1)
    if bc is None:
        check(lib.chase_hip_fill_normal(ctx.h, int(cplx), m, n, dX.ptr, dX.ld, grow0, gcol0, gld, seed), "fill_normal")
    else:
        check(lib.chase_hip_fill_normal_bc(ctx.h, int(cplx), m, n, dX.ptr, dX.ld, gld, bc[0], bc[1], bc[2], seed), "fill_normal_bc")
    got = dX.get()
    dX.free()
    return got


@TYPES
@pytest.mark.parametrize("shape", GEN_SHAPES, ids=_sid)
def test_fill_normal_against_the_host_model(ctx, cplx, shape):
    """the uniforms are exact, only the two libms differ: |z - z_ref| <= 2^-48 r, r = sqrt(-2 ln u1) - 32 ulp of margin over the
    few-ulp errors of log / sincospi on one side and log / cos / sin in long double on the other"""
    m, n = shape
    grow0, gcol0, seed = 5, 3, 0x1234567890ABCDEF
    gld = (m + grow0 + 2) | 1                                     # odd: the real pairing g >> 1 crosses columns
    got = _fill(ctx, cplx, m, n, grow0, gcol0, gld, seed)
    parts, r = R.fill_normal_ref(cplx, m, n, grow0, gcol0, gld, seed, full=True)
    G = np.stack([got.real, got.imag], axis=-1) if cplx else got[..., None]
    assert np.all(np.isfinite(G))
    err = np.abs(G.astype(LD) - parts)
    rr = r[..., None]
    ratio = np.max(np.where(rr > 0, err / np.where(rr > 0, U * rr, 1), 0))
    print(f"fill_normal {_tag(cplx)} {m}x{n}: max |z - z_ref| / (u r) = {float(ratio):.3f} (bound 32)")
    assert np.all(err <= 2.0 ** -48 * rr)


@TYPES
def test_fill_normal_shards_are_windows_of_the_whole(ctx, cplx):
    gld, n, seed = 301, 6, 77                                     # odd global row count
    full = _fill(ctx, cplx, gld, n, 0, 0, gld, seed)
    assert _same(full, _fill(ctx, cplx, gld, n, 0, 0, gld, seed))
    for (r0, c0, m, k) in [(0, 0, 1, 1), (300, 5, 1, 1), (17, 1, 255, 3), (44, 2, 257, 4), (1, 0, 300, 6)]:
        assert _same(_fill(ctx, cplx, m, k, r0, c0, gld, seed), full[r0:r0 + m, c0:c0 + k]), (r0, c0, m, k)
    for pr in (2, 3):
        for mb in (1, 7):
            got = np.full_like(full, NAN)
            for pi in range(pr):
                g = R.bc_rows(gld, mb, pr, pi)
                got[g] = _fill(ctx, cplx, len(g), n, 0, 0, gld, seed, bc=(mb, pr, pi))
            assert _same(got, full), (pr, mb)
    other = _fill(ctx, cplx, gld, n, 0, 0, gld, seed + 1)
    assert not np.any(other == full)                              # different seeds differ, everywhere
    hi = _fill(ctx, cplx, gld, n, 0, 0, gld, seed + (1 << 32))
    assert not np.any(hi == full)                                 # the seed's high word counts


@pytest.mark.parametrize("cplx,shape", [(False, (512, 512)), (True, (512, 256))], ids=["d512x512", "z512x256"])
def test_fill_normal_moments(ctx, cplx, shape):
    """2^18 samples of a seeded stream against 6 sigma: a fixed outcome (the host model passes the same limits on the CPU)"""
    Z = _fill(ctx, cplx, shape[0], shape[1], 0, 0, shape[0], 2024)
    n, stats = R.normal_moments(Z)
    assert n == 1 << 18
    for name, val, lim in stats:
        print(f"fill_normal {_tag(cplx)} {name}: {val:.3e} (limit {lim:.3e})")
        assert val <= lim, (name, val, lim)


def _clement(ctx, cplx, mloc, nloc, N, mb, pr, pi, roff, nb, pc, pj, coff, scale, perturb, seed=42):
    lib, check = _lib()
    dH = Buf(ctx, np.full((mloc, nloc), NAN, dtype=R.dt_of(cplx)), row0=0 if cplx else 1)
    check(lib.chase_hip_gen_clement(ctx.h, int(cplx), dH.ptr, dH.ld, mloc, nloc, N, mb, pr, pi, roff, nb, pc, pj, coff, scale, perturb,
                                    seed), "gen_clement")
    got = dH.get()
    dH.free()
    return got


@TYPES
@pytest.mark.parametrize("b", BLOCKS)
@pytest.mark.parametrize("grid", GRIDS, ids=_sid)
def test_gen_clement_unperturbed_shards(ctx, cplx, b, grid, sqrt_mismatches):
    """every shard against the oracle's matrix, with row and column offsets: the entries are square roots of exactly
    representable products - identical bits where the device's square root is correctly rounded, else 1 ulp"""
    pr, pc = grid
    roff, coff = 6, 5
    N = N_GRID + 11
    for (pi, pj), gi, gj in _layout_shards(N_GRID, b, pr, pc):
        if len(gi) == 0 or len(gj) == 0:
            continue
        got = _clement(ctx, cplx, len(gi), len(gj), N, b, pr, pi, roff, b, pc, pj, coff, 1.0, 0.0)
        want = R.clement_shard_ref(N, cplx, len(gi), len(gj), b, pr, pi, roff, b, pc, pj, coff)
        if sqrt_mismatches == 0:
            assert _same(got, want), (pi, pj)
        else:
            assert np.all(np.abs(got.real - want.real) <= np.spacing(want.real)) and _same(got.imag, want.imag), (pi, pj)


@TYPES
def test_gen_clement_past_one_block_of_rows_and_the_column_cap(ctx, cplx):
    """a tall and a wide window across the diagonal, generated whole and in pieces (device alone, bit for bit)"""
    N = 4200
    for perturb in (0.0, 1e-6):
        tall = _clement(ctx, cplx, 1030, 3, N, N, 1, 0, 50, N, 1, 0, 500, 1.0, perturb)
        parts = [_clement(ctx, cplx, k, 3, N, N, 1, 0, 50 + r0, N, 1, 0, 500, 1.0, perturb) for r0, k in ((0, 515), (515, 515))]
        assert _same(tall, np.vstack(parts)) and np.count_nonzero(tall.real > 1.0) == 6
        wide = _clement(ctx, cplx, 3, 4100, N, N, 1, 0, 2000, N, 1, 0, 7, 1.0, perturb)
        parts = [_clement(ctx, cplx, 3, 2050, N, N, 1, 0, 2000, N, 1, 0, 7 + c0, 1.0, perturb) for c0 in (0, 2050)]
        assert _same(wide, np.hstack(parts)) and np.count_nonzero(wide.real > 1.0) == 6
        g = 2000.0                                                # H[2000, 2001] = sqrt(2000 (N + 1 - 2000)), local column 2001 - 7
        if perturb == 0.0:
            assert abs(wide[0, 2001 - 7].real - np.sqrt(g * (N + 1 - g))) <= np.spacing(np.sqrt(g * (N + 1 - g)))


@TYPES
@pytest.mark.parametrize("b", BLOCKS)
@pytest.mark.parametrize("grid", GRIDS, ids=_sid)
def test_gen_clement_perturbed_is_hermitian_and_shard_independent(ctx, cplx, b, grid):
    pr, pc = grid
    N, scale, perturb = N_GRID, 0.75, 1e-6
    got = np.full((N, N), NAN, dtype=R.dt_of(cplx), order="F")
    for (pi, pj), gi, gj in _layout_shards(N, b, pr, pc):
        if len(gi) and len(gj):
            got[np.ix_(gi, gj)] = _clement(ctx, cplx, len(gi), len(gj), N, b, pr, pi, 0, b, pc, pj, 0, scale, perturb)
    whole = _clement(ctx, cplx, N, N, N, N, 1, 0, 0, N, 1, 0, 0, scale, perturb)
    assert _same(got, whole)                                      # any layout generates the same matrix
    assert np.array_equal(whole, whole.conj().T)                  # exactly Hermitian
    plain = _clement(ctx, cplx, N, N, N, N, 1, 0, 0, N, 1, 0, 0, scale, 0.0)
    assert _same(whole[0, :], plain[0, :]) and _same(whole[:, 0], plain[:, 0])               # row and column 0: no perturbation
    assert _same(np.diagonal(whole), np.diagonal(plain))                                      # nor the diagonal
    off = ~np.eye(N, dtype=bool)
    off[0, :] = off[:, 0] = False
    assert np.all(whole[off] != plain[off])                       # everything else is perturbed
    d = (whole - plain)[off] / (scale * perturb)
    assert 0.9 < np.std(d.real) < 1.1 and (not cplx or 0.9 < np.std(d.imag) < 1.1)


# ================================================================================================================================
# argument checks: every call below returns before anything is launched
# ================================================================================================================================
def _bad_calls(h, p, ip):
    """(entry point, arguments) - p: a valid device pointer, ip: a valid device index list; each call has exactly one fault"""
    N_ = None
    return [
        ("col_dot", (h, 0, -1, 2, p, 8, p, 8, p)), ("col_dot", (h, 0, 4, -2, p, 8, p, 8, p)), ("col_dot", (h, 0, 4, 2, p, 3, p, 8, p)),
        ("col_dot", (h, 1, 4, 2, p, 8, p, 3, p)), ("col_dot", (h, 0, 4, 2, N_, 8, p, 8, p)), ("col_dot", (h, 0, 4, 2, p, 8, N_, 8, p)),
        ("col_dot", (h, 0, 4, 2, p, 8, p, 8, N_)),
        ("col_nrm2", (h, 0, -1, 2, p, 8, p)), ("col_nrm2", (h, 0, 4, -2, p, 8, p)), ("col_nrm2", (h, 1, 4, 2, p, 3, p)),
        ("col_nrm2", (h, 0, 4, 2, N_, 8, p)), ("col_nrm2", (h, 0, 4, 2, p, 8, N_)),
        ("col_sumsq", (h, 0, -1, 2, p, 8, p)), ("col_sumsq", (h, 0, 4, -2, p, 8, p)), ("col_sumsq", (h, 1, 4, 2, p, 3, p)),
        ("col_sumsq", (h, 0, 4, 2, N_, 8, p)), ("col_sumsq", (h, 0, 4, 2, p, 8, N_)),
        ("sqrt_inplace", (h, p, -1)), ("sqrt_inplace", (h, N_, 4)),
        ("col_axpy", (h, 0, -1, 2, p, 1, 1, 1.0, p, 8, p, 8)), ("col_axpy", (h, 0, 4, -2, p, 1, 1, 1.0, p, 8, p, 8)),
        ("col_axpy", (h, 0, 4, 2, p, 1, -1, 1.0, p, 8, p, 8)), ("col_axpy", (h, 0, 4, 2, p, 1, 1, 1.0, p, 3, p, 8)),
        ("col_axpy", (h, 1, 4, 2, p, 0, 1, 1.0, p, 8, p, 3)), ("col_axpy", (h, 0, 4, 2, N_, 1, 1, 1.0, p, 8, p, 8)),
        ("col_axpy", (h, 0, 4, 2, p, 1, 1, 1.0, N_, 8, p, 8)), ("col_axpy", (h, 0, 4, 2, p, 1, 1, 1.0, p, 8, N_, 8)),
        ("col_scal", (h, 0, -1, 2, p, 0, p, 8)), ("col_scal", (h, 0, 4, -2, p, 0, p, 8)), ("col_scal", (h, 1, 4, 2, p, 1, p, 3)),
        ("col_scal", (h, 0, 4, 2, N_, 0, p, 8)), ("col_scal", (h, 0, 4, 2, p, 0, N_, 8)),
        ("resid_norms_dev", (h, 0, -1, 2, p, 8, p, 8, p, p, 0)), ("resid_norms_dev", (h, 0, 4, -2, p, 8, p, 8, p, p, 0)),
        ("resid_norms_dev", (h, 0, 4, 2, p, 3, p, 8, p, p, 0)), ("resid_norms_dev", (h, 1, 4, 2, p, 8, p, 3, p, p, 1)),
        ("resid_norms_dev", (h, 0, 4, 2, N_, 8, N_, 0, N_, p, 0)), ("resid_norms_dev", (h, 0, 4, 2, p, 8, p, 8, N_, p, 0)),
        ("resid_norms_dev", (h, 0, 4, 2, p, 8, N_, 0, N_, N_, 0)),
        ("resid_norms", (h, 0, -1, 2, p, 8, p, 8, p, p, 0)), ("resid_norms", (h, 0, 4, -2, p, 8, p, 8, p, p, 0)),
        ("resid_norms", (h, 0, 4, 2, p, 3, p, 8, p, p, 0)), ("resid_norms", (h, 1, 4, 2, p, 8, p, 3, p, p, 1)),
        ("resid_norms", (h, 0, 4, 2, N_, 8, N_, 0, N_, p, 0)), ("resid_norms", (h, 0, 4, 2, p, 8, N_, 0, N_, N_, 0)),
        ("set_identity", (h, 0, -1, p, 8)), ("set_identity", (h, 1, 4, p, 3)), ("set_identity", (h, 0, 4, N_, 8)),
        ("pack_upper", (h, 0, -1, p, 8, p)), ("pack_upper", (h, 0, 4, p, 3, p)), ("pack_upper", (h, 0, 4, N_, 8, p)),
        ("pack_upper", (h, 1, 4, p, 8, N_)),
        ("unpack_upper", (h, 0, -1, p, p, 8, 0)), ("unpack_upper", (h, 0, 4, p, p, 3, 1)), ("unpack_upper", (h, 0, 4, N_, p, 8, 0)),
        ("unpack_upper", (h, 1, 4, p, N_, 8, 1)),
        ("rows_indexed", (h, 0, p, 8, p, 8, ip, -1, 2, 0)), ("rows_indexed", (h, 0, p, 8, p, 8, ip, 4, -2, 1)),
        ("rows_indexed", (h, 0, N_, 8, p, 8, ip, 4, 2, 0)), ("rows_indexed", (h, 1, p, 8, N_, 8, ip, 4, 2, 0)),
        ("rows_indexed", (h, 0, p, 8, p, 8, N_, 4, 2, 1)),
        ("cols_indexed", (h, 0, -1, p, 8, p, 8, ip, 2)), ("cols_indexed", (h, 0, 4, p, 8, p, 8, ip, -2)),
        ("cols_indexed", (h, 0, 4, p, 3, p, 8, ip, 2)), ("cols_indexed", (h, 0, 4, p, 8, p, 8, N_, 2)),
        ("shift_list", (h, 0, p, 8, ip, ip, -1, 1.0)), ("shift_list", (h, 0, N_, 8, ip, ip, 2, 1.0)),
        ("shift_list", (h, 1, p, 8, N_, ip, 2, 1.0)), ("shift_list", (h, 0, p, 8, ip, N_, 2, 1.0)),
        ("scale_rows", (h, 0, -1, 2, p, 8, 0, 2.0)), ("scale_rows", (h, 0, 4, -2, p, 8, 0, 2.0)), ("scale_rows", (h, 0, 4, 2, p, 8, -1, 2.0)),
        ("scale_rows", (h, 1, 4, 2, p, 3, 0, 2.0)), ("scale_rows", (h, 0, 4, 2, N_, 8, 0, 2.0)),
        ("scale_rows_bc", (h, 0, -1, 2, p, 8, 0, 2, 2, 0, 2.0)), ("scale_rows_bc", (h, 0, 4, -2, p, 8, 0, 2, 2, 0, 2.0)),
        ("scale_rows_bc", (h, 0, 4, 2, p, 3, 0, 2, 2, 0, 2.0)), ("scale_rows_bc", (h, 0, 4, 2, p, 8, 0, 2, 2, 2, 2.0)),
        ("scale_rows_bc", (h, 0, 4, 2, N_, 8, 0, 2, 2, 0, 2.0)),
        ("abs_trace", (h, 0, -1, p, 8, C.pointer(C.c_double()))), ("abs_trace", (h, 0, 4, p, 3, C.pointer(C.c_double()))),
        ("abs_trace", (h, 0, 4, N_, 8, C.pointer(C.c_double()))), ("abs_trace", (h, 0, 4, p, 8, None)),
        ("tri_mask_bc", (h, 0, b"U", -1, 2, p, 8, 2, 1, 0, 2, 1, 0)), ("tri_mask_bc", (h, 0, b"X", 4, 2, p, 8, 2, 1, 0, 2, 1, 0)),
        ("tri_mask_bc", (h, 0, b"L", 4, 2, p, 8, 2, 2, 2, 2, 1, 0)), ("tri_mask_bc", (h, 0, b"L", 4, 2, N_, 8, 2, 1, 0, 2, 1, 0)),
        ("conj_transpose_add", (h, 0, -1, 2, p, 8, ip, ip, p, 8)), ("conj_transpose_add", (h, 0, 4, 2, p, 3, ip, ip, p, 8)),
        ("conj_transpose_add", (h, 0, 4, 2, p, 8, N_, ip, p, 8)), ("conj_transpose_add", (h, 1, 4, 2, p, 8, ip, ip, N_, 8)),
        ("complete_hermitian", (h, 0, b"U", -1, p, 8)), ("complete_hermitian", (h, 0, b"U", 4, p, 3)),
        ("complete_hermitian", (h, 0, b"U", 4, N_, 8)), ("complete_hermitian", (h, 0, b"Q", 4, p, 8)),
        ("fill_normal", (h, 0, -1, 2, p, 8, 0, 0, 8, 1)), ("fill_normal", (h, 0, 4, 2, p, 3, 0, 0, 8, 1)), ("fill_normal", (h, 0, 4, 2, N_, 8, 0, 0, 8, 1)),
        ("fill_normal_bc", (h, 0, 4, -2, p, 8, 8, 2, 2, 0, 1)), ("fill_normal_bc", (h, 0, 4, 2, p, 8, 8, 0, 2, 0, 1)),
        ("fill_normal_bc", (h, 0, 4, 2, N_, 8, 8, 2, 2, 0, 1)),
        ("gen_clement", (h, 0, p, 8, -1, 2, 8, 8, 1, 0, 0, 8, 1, 0, 0, 1.0, 0.0, 1)), ("gen_clement", (h, 0, p, 3, 4, 2, 8, 8, 1, 0, 0, 8, 1, 0, 0, 1.0, 0.0, 1)),
        ("gen_clement", (h, 0, N_, 8, 4, 2, 8, 8, 1, 0, 0, 8, 1, 0, 0, 1.0, 0.0, 1)),
    ]


def test_bad_arguments_are_refused_before_any_launch(ctx):
    lib, check = _lib()
    mark = np.full((16, 4), 3.0, order="F")
    d = Buf(ctx, mark)                                            # 16 x 4 doubles: room for every shape named below, were it used
    ip = _ints(ctx, [0, 1, 2, 3])
    calls = _bad_calls(ctx.h, d.ptr, ip.ptr)
    seen = set()
    for name, args in calls:
        rc = getattr(lib, "chase_hip_" + name)(*args)
        msg = lib.chase_hip_last_error().decode()
        assert rc == EINVAL, (name, args[1:], rc)
        assert msg.startswith(name + ":"), (name, msg)
        seen.add(name)
    assert seen >= {"col_dot", "col_nrm2", "col_sumsq", "sqrt_inplace", "col_axpy", "col_scal", "resid_norms", "resid_norms_dev",
                    "set_identity", "pack_upper", "unpack_upper", "rows_indexed", "cols_indexed", "shift_list"}
    ctx.sync()
    assert d.unchanged() and ip.unchanged()                       # and nothing was written
    _free(d, ip)


def test_empty_calls_are_legal_and_write_nothing(ctx):
    """n == 0 returns 0 whatever the pointers; m == 0 with n > 0 (a rank without local rows) is legal and does what it did"""
    lib, check = _lib()
    d = Buf(ctx, np.full((16, 4), 3.0, order="F"))
    h, p, Z = ctx.h, d.ptr, None
    for name, args in [("col_dot", (h, 0, 4, 0, Z, 4, Z, 4, Z)), ("col_nrm2", (h, 1, 4, 0, Z, 4, Z)), ("col_sumsq", (h, 0, 4, 0, Z, 4, Z)),
                       ("sqrt_inplace", (h, Z, 0)), ("col_axpy", (h, 0, 4, 0, Z, 1, 1, 1.0, Z, 4, Z, 4)),
                       ("col_axpy", (h, 1, 0, 3, Z, 0, 1, 1.0, Z, 0, Z, 0)), ("col_scal", (h, 0, 4, 0, Z, 0, Z, 4)),
                       ("col_scal", (h, 0, 0, 3, Z, 1, Z, 0)), ("resid_norms_dev", (h, 0, 4, 0, Z, 4, Z, 4, Z, p, 0)),
                       ("resid_norms", (h, 0, 4, 0, Z, 4, Z, 4, Z, p, 0)), ("set_identity", (h, 0, 0, Z, 0)),
                       ("pack_upper", (h, 0, 0, Z, 0, Z)), ("unpack_upper", (h, 1, 0, Z, Z, 0, 1)),
                       ("rows_indexed", (h, 0, Z, 0, Z, 0, Z, 0, 3, 0)), ("rows_indexed", (h, 0, Z, 4, Z, 4, Z, 4, 0, 1)),
                       ("cols_indexed", (h, 0, 0, Z, 0, Z, 0, Z, 3)), ("shift_list", (h, 0, Z, 4, Z, Z, 0, 1.0)),
                       ("scale_rows", (h, 0, 4, 0, Z, 4, 0, 2.0)), ("scale_rows_bc", (h, 0, 0, 3, Z, 0, 0, 2, 2, 1, 2.0))]:
        assert getattr(lib, "chase_hip_" + name)(*args) == 0, name
    # m == 0, n > 0: the reductions give exact zeros (tested with data in test_col_dot / test_col_sumsq_and_col_nrm2 as well)
    out = Buf(ctx, np.full((6, 1), NAN), row0=1)
    check(lib.chase_hip_col_dot(h, 1, 0, 3, Z, 0, Z, 0, out.ptr), "col_dot")
    assert _same(out.get()[:, 0], np.zeros(6))
    ctx.sync()
    assert d.unchanged()
    _free(d, out)
