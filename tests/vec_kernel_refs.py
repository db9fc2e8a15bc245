"""Plain host references of the streaming, Lanczos, shard and generator kernels (include/chase_hip.h), written from the header's
contracts: numpy only, no GPU, no chase_amd.  What tests/test_gpu_vec_kernels.py compares the device with; checked themselves
by tests/test_vec_kernel_refs_cpu.py.  Reductions are summed in long double."""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble
assert np.finfo(LD).nmant >= 63, "long double is not wider than double here: the references would be no better than the device"
U = 2.0 ** -53                                   # unit roundoff of fp64


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u)"""
    return k * U / (1.0 - k * U)


def dt_of(cplx):
    return np.complex128 if cplx else np.float64


def rand(rng, shape, cplx):
    a = rng.standard_normal(shape)
    if cplx:
        a = a + 1j * rng.standard_normal(shape)
    return np.asfortranarray(a.astype(dt_of(cplx)))


def as_doubles(X):
    """(m, n) fp64 / complex fp64 -> the (m * ept, n) doubles the kernels see (interleaved re, im), a copy"""
    X = np.asarray(X)
    if np.iscomplexobj(X):
        D = np.empty((2 * X.shape[0], X.shape[1]), dtype=np.float64, order="F")
        D[0::2] = X.real
        D[1::2] = X.imag
        return D
    return np.array(X, dtype=np.float64, order="F", copy=True)


def from_doubles(D, cplx):
    """the inverse: parts are copied, never combined arithmetically (signed zeros survive)"""
    D = np.asfortranarray(D, dtype=np.float64)
    if not cplx:
        return D
    out = np.empty((D.shape[0] // 2, D.shape[1]), dtype=np.complex128, order="F")
    out.real = D[0::2]
    out.imag = D[1::2]
    return out


# ---- block-cyclic layouts ------------------------------------------------------------------------------------------------------
def bc_global(l, b, p, q, off=0):
    """global index of local index l on rank q of p, blocks of b"""
    return off + ((l // b) * p + q) * b + l % b


def bc_count(N, b, p, q):
    """local extent of rank q: the number of l with bc_global(l, b, p, q) < N"""
    full, rem = divmod(N, b * p)
    return full * b + min(max(rem - q * b, 0), b)


def bc_rows(N, b, p, q):
    return bc_global(np.arange(bc_count(N, b, p, q)), b, p, q)


# ---- shard steps of the distributed symOrHermMatrix -------------------------------------------------------------------------
def tri_mask_ref(Hloc, uplo, mb, pr, pi, nb, pc, pj):
    """kept triangle (by global position) untouched, the other one +0.0, the diagonal halved"""
    out = np.array(Hloc, order="F", copy=True)
    gi = bc_global(np.arange(out.shape[0]), mb, pr, pi)[:, None]
    gj = bc_global(np.arange(out.shape[1]), nb, pc, pj)[None, :]
    out[(gi > gj) if uplo in "Uu" else (gi < gj)] = 0.0
    d = np.broadcast_to(gi == gj, out.shape)
    out[d] = out[d] * 0.5
    return out


def conj_transpose_add_ref(P, rowmap, colmap, H):
    """H[colmap[b], rowmap[a]] += conj(P[a, b]) (injective maps)"""
    out = np.array(H, order="F", copy=True)
    P = np.asarray(P)
    for b in range(P.shape[1]):
        out[colmap[b], rowmap] = out[colmap[b], rowmap] + np.conj(P[:, b])
    return out


def complete_hermitian_ref(A, uplo):
    """the triangle that is not stored <- conj(stored)^T; the diagonal is left alone, imaginary part included"""
    out = np.array(A, order="F", copy=True)
    n = out.shape[0]
    for j in range(n):
        if uplo in "Uu":
            out[j + 1:, j] = np.conj(out[j, j + 1:])
        else:
            out[j, j + 1:] = np.conj(out[j + 1:, j])
    return out


def pack_upper_ref(A):
    """column-packed upper triangle: P[j (j + 1) / 2 + i] = A[i, j], i <= j"""
    n = A.shape[0]
    P = np.empty(n * (n + 1) // 2, dtype=A.dtype)
    for j in range(n):
        P[j * (j + 1) // 2: j * (j + 1) // 2 + j + 1] = A[:j + 1, j]
    return P


def unpack_upper_ref(P, A0, mirror=0):
    """the upper triangle of A0 <- P; mirror: the strictly lower one <- conj(upper)^T; anything else of A0 stays"""
    out = np.array(A0, order="F", copy=True)
    n = out.shape[0]
    for j in range(n):
        out[:j + 1, j] = P[j * (j + 1) // 2: j * (j + 1) // 2 + j + 1]
    return complete_hermitian_ref(out, "U") if mirror else out


# ---- gathers, scalings ---------------------------------------------------------------------------------------------------------
def rows_indexed_ref(inp, idx, out0, scatter):
    """scatter == 0: out[p, :] = in[idx[p], :]; scatter != 0: out[idx[p], :] = in[p, :]; p < len(idx)"""
    out = np.array(out0, order="F", copy=True)
    idx = np.asarray(idx)
    if scatter:
        out[idx, :] = inp[:len(idx), :]
    else:
        out[:len(idx), :] = inp[idx, :]
    return out


def cols_indexed_ref(inp, idx):
    return np.asfortranarray(inp[:, np.asarray(idx)])


def _scaled_rows(X, rows, s):
    """X with the rows selected by the boolean mask multiplied by the REAL s, part by part (no complex product: signed zeros)"""
    cplx = np.iscomplexobj(X)
    D = as_doubles(X)
    sel = np.repeat(rows, 2) if cplx else rows
    D[sel, :] = D[sel, :] * np.float64(s)
    return from_doubles(D, cplx)


def scale_rows_ref(X, row0, s):
    return _scaled_rows(X, np.arange(X.shape[0]) >= row0, s)


def scale_rows_bc_ref(X, g0, nb, p, q, s):
    return _scaled_rows(X, bc_global(np.arange(X.shape[0]), nb, p, q) >= g0, s)


def col_scal_ref(X, a, inverse):
    """X_j *= a[j], or *= 1 / a[j]: the reciprocal is rounded first, then the product"""
    cplx = np.iscomplexobj(X)
    D = as_doubles(X)
    f = (np.float64(1.0) / np.asarray(a, dtype=np.float64)) if inverse else np.asarray(a, dtype=np.float64)
    D = D * f[None, :]
    return from_doubles(D, cplx)


def shift_list_ref(H, rows, cols, shift):
    out = np.array(H, order="F", copy=True)
    if np.iscomplexobj(out):
        out.real[rows, cols] = out.real[rows, cols] + shift
    else:
        out[rows, cols] = out[rows, cols] + shift
    return out


# ---- reductions in long double --------------------------------------------------------------------------------------------
def _wide(X):
    return np.asarray(X).astype(CLD if np.iscomplexobj(X) else LD)


def col_dot_ref(X, Y):
    """x_j^H y_j per column, long double (complex long double)"""
    return np.sum(np.conj(_wide(X)) * _wide(Y), axis=0)


def col_dot_bound(X, Y):
    """any summation order (Higham (3.5)): real gamma_{m+1} sum |x y|; complex, per component, gamma_{m+3} sum (|xr|+|xi|)(|yr|+|yi|)"""
    m = X.shape[0]
    if np.iscomplexobj(X):
        s = np.sum((np.abs(X.real) + np.abs(X.imag)).astype(LD) * (np.abs(Y.real) + np.abs(Y.imag)).astype(LD), axis=0)
        return gamma(m + 3) * s
    return gamma(m + 1) * np.sum(np.abs(_wide(X) * _wide(Y)), axis=0)


def resid_sumsq_ref(W, V=None, lam=None):
    """sum_i |W[i, j] - lam[j] V[i, j]|^2 in long double (V None: plain sums of squares)"""
    R = _wide(W)
    if V is not None:
        R = R - np.asarray(lam).astype(LD)[None, :] * _wide(V)
    return np.sum(R.real * R.real + (R.imag * R.imag if np.iscomplexobj(R) else 0), axis=0)


def resid_sumsq_bound(W, V=None, lam=None):
    """(md + 8) u sum a_i^2, a_i = |w_i| + |lam| |v_i| over the md doubles of a column"""
    Dw = np.abs(as_doubles(W)).astype(LD)
    if V is not None:
        Dw = Dw + np.abs(np.asarray(lam)).astype(LD)[None, :] * np.abs(as_doubles(V)).astype(LD)
    return (Dw.shape[0] + 8) * U * np.sum(Dw * Dw, axis=0)


def abs_trace_ref(A):
    d = np.diagonal(A)[:min(A.shape)]
    return np.sum(np.abs(_wide(d)))


def col_axpy_ref(a, a_is_real, a_stride, sgn, X, Y):
    """(reference, per-component bound) of Y_j += sgn * a[j * a_stride] * X_j with the unfused count of roundings:
    real 3 u (|y| + |a| |x|), complex 5 u (|y_c| + (|a_r| + |a_i|)(|x_r| + |x_i|)); a: array of reals or of complex"""
    n = X.shape[1]
    aj = np.asarray(a)[np.arange(n) * a_stride]
    if np.iscomplexobj(X):
        aw = aj.astype(CLD)
        ref = _wide(Y) + LD(sgn) * aw[None, :] * _wide(X)
        mag = (np.abs(aw.real) + np.abs(aw.imag))[None, :] * (np.abs(X.real) + np.abs(X.imag)).astype(LD)
        return ref, 5 * U * (np.abs(Y.real).astype(LD) + mag), 5 * U * (np.abs(Y.imag).astype(LD) + mag)
    assert a_is_real
    aw = aj.astype(LD)
    ref = _wide(Y) + LD(sgn) * aw[None, :] * _wide(X)
    b = 3 * U * (np.abs(_wide(Y)) + np.abs(aw)[None, :] * np.abs(_wide(X)))
    return ref, b, None


# ---- the generator's host model -------------------------------------------------------------------------------------------
_M0, _M1, _W0, _W1, _M32 = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF))
_S32 = np.uint64(32)


def philox4x32_10(ctr4, key2):
    """Philox4x32 with 10 rounds (Salmon et al., SC'11) on four 32-bit counter words and two key words, each an integer or an
    array of them; returns the four output words as uint64 arrays holding 32-bit values"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in ctr4)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & _M32 for k in key2)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                              # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _W0) & _M32, (k1 + _W1) & _M32
    return c0, c1, c2, c3


def uniforms_ref(ctr, seed):
    """the two 53-bit uniforms of counter ctr: words (o0, o1) and (o2, o3) give w = o_even * 2^21 + (o_odd >> 11);
    u1 = w 2^-53 + 2^-54 in (0, 1], u2 = w 2^-53 in [0, 1)"""
    ctr = np.asarray(ctr, dtype=np.uint64)
    seed = int(seed)
    o = philox4x32_10((ctr & _M32, ctr >> _S32, 0x5eed, 0), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    w1 = (o[0] << np.uint64(21)) ^ (o[1] >> np.uint64(11))
    w2 = (o[2] << np.uint64(21)) ^ (o[3] >> np.uint64(11))
    u1 = w1.astype(np.float64) * 2.0 ** -53 + 2.0 ** -54
    u2 = w2.astype(np.float64) * 2.0 ** -53
    return u1, u2


def normal_pair_ref(ctr, seed):
    """Box-Muller pair of counter ctr in long double: (z0, z1, r), r = sqrt(-2 ln u1), z0 = r cos 2 pi u2, z1 = r sin 2 pi u2"""
    u1, u2 = uniforms_ref(ctr, seed)
    pi = LD(4) * np.arctan(LD(1))
    r = np.sqrt(LD(-2) * np.log(u1.astype(LD)))
    t = LD(2) * pi * u2.astype(LD)
    return r * np.cos(t), r * np.sin(t), r


def fill_normal_ref(cplx, m, n, grow0, gcol0, gld, seed, mb=0, pr=1, pi=0, full=False):
    """the m x n window of the N(0,1) fill whose element identity is g = (gcol0 + j) * gld + row, row = grow0 + i or, for
    block-cyclic rows (mb > 0), grow0 + bc_global(i, mb, pr, pi).  Complex: (re, im) = pair g.  Real: pair g >> 1, z1 for odd g.
    Returns fp64 / complex fp64; full: (parts in long double of shape (m, n, ept), r of shape (m, n))"""
    i = np.arange(m, dtype=np.int64)
    row = grow0 + (bc_global(i, mb, pr, pi) if mb > 0 else i)
    g = ((gcol0 + np.arange(n, dtype=np.int64))[None, :] * gld + row[:, None]).astype(np.uint64)
    if cplx:
        z0, z1, r = normal_pair_ref(g, seed)
        parts = np.stack([z0, z1], axis=-1)
    else:
        z0, z1, r = normal_pair_ref(g >> np.uint64(1), seed)
        parts = np.where((g & np.uint64(1)) == 1, z1, z0)[..., None]
    if full:
        return parts, r
    D = parts.astype(np.float64)
    return np.asfortranarray(D[..., 0] + 1j * D[..., 1]) if cplx else np.asfortranarray(D[..., 0])


def normal_moments(Z):
    """[(name, |statistic|, limit)] of a fill with 2^18 real samples: mean, variance, and the correlation of the two halves of
    a Box-Muller pair (real: vertically adjacent elements; complex: re with im), each against 6 sigma of n = samples"""
    Z = np.asarray(Z)
    cplx = np.iscomplexobj(Z)
    a, b = (Z.real.ravel(), Z.imag.ravel()) if cplx else (Z[0::2, :].ravel(), Z[1::2, :].ravel())
    x = np.concatenate([a, b]).astype(LD)
    n = x.size
    mean = np.sum(x) / n
    var = np.sum((x - mean) ** 2) / n
    al, bl = a.astype(LD), b.astype(LD)
    corr = np.sum((al - np.mean(al)) * (bl - np.mean(bl))) / np.sqrt(np.sum((al - np.mean(al)) ** 2) * np.sum((bl - np.mean(bl)) ** 2))
    return n, [("mean", float(abs(mean)), 6.0 / np.sqrt(n)), ("var - 1", float(abs(var - 1)), 6.0 * np.sqrt(2.0 / n)),
               ("pair correlation", float(abs(corr)), 6.0 / np.sqrt(n))]


def clement_shard_ref(N, cplx, mloc, nloc, mb, pr, pi, roff, nb, pc, pj, coff):
    """the (mloc x nloc) shard of the unperturbed Clement matrix whose local (i, j) is global
    (bc_global(i, mb, pr, pi, roff), bc_global(j, nb, pc, pj, coff))"""
    from oracle.chase_oracle import clement
    H = clement(N, cplx, perturb=0)
    gi = bc_global(np.arange(mloc), mb, pr, pi, roff)
    gj = bc_global(np.arange(nloc), nb, pc, pj, coff)
    return np.asfortranarray(H[np.ix_(gi, gj)])
