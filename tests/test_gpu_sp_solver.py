"""The single-precision Hermitian solver (capi.SpSolver, chase_hip_solver_create_sp, schase_ / cchase_) on the GPU.

1. every new kernel against numpy: odd shapes, padded leading dimensions whose sentinel rows must keep their bytes, more than one
   block per column, empty extents, bad leading dimensions;
2. the operators one by one on fp32 data: the bracketed filter call equals the fp32 MFMA product bit for bit and leaves H and the
   locked columns as they were, QR gives a rounded fp64-orthonormal block, Rayleigh-Ritz and the residuals agree with fp64 numpy on
   the same fp32 data within the product bound of tests/sp_solver_ref.py;
3. whole solves of the four cases of the emulation (tests/sp_solver_ref.py);
4. the schase_ / cchase_ sequence through ctypes;
5. memory (no fp64 matrix on the device), the refused switches and the ignored environment variables.
u = 2^-24 throughout."""
import ctypes as C

import numpy as np
import pytest

import sp_solver_ref as R
from conftest import read_ref_matrix

pytestmark = pytest.mark.gpu
U = R.U
EINVAL = -1001
SENT = 777.0


def _st(cplx): return np.complex64 if cplx else np.float32


def _rand(rng, shape, cplx):
    a = rng.standard_normal(shape)
    if cplx:
        a = a + 1j * rng.standard_normal(shape)
    return np.asfortranarray(a.astype(_st(cplx)))


def _padded(ctx, A, ld):
    """device copy of A with leading dimension ld, the pad rows set to a sentinel; returns (DeviceArray, host image)"""
    m, n = A.shape
    host = np.full((ld, n), SENT, dtype=A.dtype, order="F")
    host[:m, :] = A
    return ctx.empty((ld, n), A.dtype).upload(host), host


# m, n, ld: one block with an odd ld, a 16-byte-aligned ld, and columns longer than one 1024-float pass with a padded ld
SHAPES = [(133, 5, 133), (133, 5, 136), (2050, 3, 2052)]


# ---- 1. kernels -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-ld%d" % s)
def test_copy_kernels_against_numpy(ctx, shape, cplx):
    from chase_amd.capi import lib
    m, n, ld = shape
    rng = np.random.default_rng(m + n + ld + cplx)
    A = _rand(rng, (m, n), cplx)
    dA, hA = _padded(ctx, A, ld)
    # lacpy_sp into another leading dimension: window copied, destination pads untouched
    dB, hB = _padded(ctx, np.zeros_like(A), ld + 4)
    assert lib.chase_hip_lacpy_sp(ctx.h, int(cplx), m, n, dA.ptr, ld, dB.ptr, ld + 4) == 0
    got = dB.download()
    assert np.array_equal(got[:m], A) and np.array_equal(got[m:], hB[m:])
    # ... and from an element offset that breaks the 16-byte alignment (guarded path)
    es = A.dtype.itemsize
    assert lib.chase_hip_lacpy_sp(ctx.h, int(cplx), m - 1, n, dA.ptr + es, ld, dB.ptr + es, ld + 4) == 0
    got = dB.download()
    assert np.array_equal(got[:m], A) and np.array_equal(got[m:], hB[m:])
    # swap_cols_sp
    assert lib.chase_hip_swap_cols_sp(ctx.h, int(cplx), m, dA.ptr, ld, 0, n - 1) == 0
    exp = hA.copy(); exp[:m, [0, n - 1]] = exp[:m, [n - 1, 0]]
    assert np.array_equal(dA.download(), exp)
    assert lib.chase_hip_swap_cols_sp(ctx.h, int(cplx), m, dA.ptr, ld, 1, 1) == 0
    assert np.array_equal(dA.download(), exp)
    # permute_cols_sp: V[:, dst] <- V[:, src] simultaneously (a rotation of the first three columns)
    src, dst = (C.c_int * 3)(1, 2, 0), (C.c_int * 3)(0, 1, 2)
    dS, hS = _padded(ctx, np.zeros_like(A), ld)
    assert lib.chase_hip_permute_cols_sp(ctx.h, int(cplx), m, dA.ptr, ld, dS.ptr, ld, src, dst, 3) == 0
    exp2 = exp.copy(); exp2[:m, [0, 1, 2]] = exp[:m, [1, 2, 0]]
    assert np.array_equal(dA.download(), exp2)
    assert np.array_equal(dS.download()[m:], hS[m:])
    # upload_matrix_sp / download_matrix_sp between different leading dimensions
    host = np.full((m + 2, n), 5.0, dtype=A.dtype, order="F"); host[:m] = A
    assert lib.chase_hip_upload_matrix_sp(ctx.h, int(cplx), m, n, host.ctypes.data, m + 2, dB.ptr, ld + 4) == 0
    got = dB.download()
    assert np.array_equal(got[:m], A) and np.array_equal(got[m:], hB[m:])
    back = np.full((m + 1, n), 9.0, dtype=A.dtype, order="F")
    assert lib.chase_hip_download_matrix_sp(ctx.h, int(cplx), m, n, dB.ptr, ld + 4, back.ctypes.data, m + 1) == 0
    assert np.array_equal(back[:m], A) and np.all(back[m:] == 9.0)
    for a in (dA, dB, dS):
        a.free()


@pytest.mark.parametrize("cplx", [False, True])
def test_kernel_argument_checks_and_empty_extents(ctx, cplx):
    from chase_amd.capi import lib
    A = _rand(np.random.default_rng(1), (8, 4), cplx)
    dA, hA = _padded(ctx, A, 8)
    dB, _ = _padded(ctx, A, 8)
    lam, out = np.zeros(4), np.zeros(4)
    idx = (C.c_int * 1)(0)
    c = int(cplx)
    bad = [lib.chase_hip_lacpy_sp(ctx.h, c, 8, 4, dA.ptr, 7, dB.ptr, 8), lib.chase_hip_lacpy_sp(ctx.h, c, 8, 4, dA.ptr, 8, dB.ptr, 7),
           lib.chase_hip_lacpy_sp(ctx.h, c, -1, 4, dA.ptr, 8, dB.ptr, 8),
           lib.chase_hip_swap_cols_sp(ctx.h, c, 8, dA.ptr, 7, 0, 1), lib.chase_hip_swap_cols_sp(ctx.h, c, 8, dA.ptr, 8, -1, 1),
           lib.chase_hip_permute_cols_sp(ctx.h, c, 8, dA.ptr, 7, dB.ptr, 8, idx, idx, 1),
           lib.chase_hip_permute_cols_sp(ctx.h, c, 8, dA.ptr, 8, dB.ptr, 7, idx, idx, 1),
           lib.chase_hip_upload_matrix_sp(ctx.h, c, 8, 4, A.ctypes.data, 7, dB.ptr, 8),
           lib.chase_hip_download_matrix_sp(ctx.h, c, 8, 4, dB.ptr, 7, A.ctypes.data, 8),
           lib.chase_hip_shift_diag_sp(ctx.h, c, 4, dA.ptr, 3, dB.ptr, 0.5),
           lib.chase_hip_resid_norms_sp(ctx.h, c, 8, 4, dA.ptr, 7, dB.ptr, 8, lam.ctypes.data, out.ctypes.data),
           lib.chase_hip_resid_norms_sp(ctx.h, c, 8, 4, dA.ptr, 8, dB.ptr, 7, lam.ctypes.data, out.ctypes.data),
           lib.chase_hip_complete_hermitian_sp(ctx.h, c, b"U", 4, dA.ptr, 3),
           lib.chase_hip_complete_hermitian_sp(ctx.h, c, b"X", 4, dA.ptr, 8)]
    assert bad == [EINVAL] * len(bad), bad
    empty = [lib.chase_hip_lacpy_sp(ctx.h, c, 0, 4, None, 8, None, 8), lib.chase_hip_lacpy_sp(ctx.h, c, 8, 0, None, 8, None, 8),
             lib.chase_hip_swap_cols_sp(ctx.h, c, 0, dA.ptr, 8, 0, 1),
             lib.chase_hip_permute_cols_sp(ctx.h, c, 8, dA.ptr, 8, dB.ptr, 8, idx, idx, 0),
             lib.chase_hip_upload_matrix_sp(ctx.h, c, 0, 4, None, 8, None, 8),
             lib.chase_hip_download_matrix_sp(ctx.h, c, 8, 0, None, 8, None, 8),
             lib.chase_hip_shift_diag_sp(ctx.h, c, 0, None, 8, None, 0.5),
             lib.chase_hip_resid_norms_sp(ctx.h, c, 8, 0, None, 8, None, 8, None, None),
             lib.chase_hip_complete_hermitian_sp(ctx.h, c, b"L", 0, None, 8)]
    assert empty == [0] * len(empty), empty
    assert np.array_equal(dA.download(), hA)
    # m == 0 with columns: norms of nothing are 0
    out[:] = 3.0
    assert lib.chase_hip_resid_norms_sp(ctx.h, c, 0, 4, dA.ptr, 8, dB.ptr, 8, lam.ctypes.data, out.ctypes.data) == 0
    assert np.all(out == 0.0)
    dA.free(); dB.free()


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-ld%d" % s)
def test_resid_norms_sp_within_the_derived_bound(ctx, shape, cplx):
    from chase_amd.capi import lib
    m, n, ld = shape
    rng = np.random.default_rng(11 * m + ld + cplx)
    W, V = _rand(rng, (m, n), cplx), _rand(rng, (m, n), cplx)
    lam = rng.standard_normal(n)
    W[:, 0] = (V[:, 0] * np.float32(lam[0])).astype(W.dtype)          # a nearly vanishing residual (heavy cancellation)
    dW, hW = _padded(ctx, W, ld)
    dV, hV = _padded(ctx, V, ld)
    out = np.full(n, -1.0)
    assert lib.chase_hip_resid_norms_sp(ctx.h, int(cplx), m, n, dW.ptr, ld, dV.ptr, ld, lam.ctypes.data, out.ctypes.data) == 0
    exact, bound = R.resid_norms_exact(W, V, lam), R.resid_norms_bound(W, V, lam)
    print("resid_norms_sp", shape, cplx, "worst |err| / bound", float(np.max(np.abs(out - exact) / bound)))
    assert np.all(np.abs(out - exact) <= bound)
    # unaligned operands (guarded path) give the same within the same bound; a repeat gives the same bits
    es = W.dtype.itemsize
    out2, out3 = np.zeros(n), np.zeros(n)
    assert lib.chase_hip_resid_norms_sp(ctx.h, int(cplx), m - 1, n, dW.ptr + es, ld, dV.ptr + es, ld, lam.ctypes.data,
                                        out2.ctypes.data) == 0
    assert np.all(np.abs(out2 - R.resid_norms_exact(W[1:], V[1:], lam)) <= R.resid_norms_bound(W[1:], V[1:], lam))
    assert lib.chase_hip_resid_norms_sp(ctx.h, int(cplx), m, n, dW.ptr, ld, dV.ptr, ld, lam.ctypes.data, out3.ctypes.data) == 0
    assert np.array_equal(out, out3)
    assert np.array_equal(dW.download(), hW) and np.array_equal(dV.download(), hV)
    dW.free(); dV.free()


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n,ld", [(133, 133), (133, 136), (2050, 2052)])
def test_shift_diag_sp_bit_for_bit(ctx, n, ld, cplx):
    from chase_amd.capi import lib
    rng = np.random.default_rng(n + ld + cplx)
    A = _rand(rng, (n, n), cplx)
    dA, hA = _padded(ctx, A, ld)
    idx = np.arange(n)
    d0 = np.ascontiguousarray(A[idx, idx])
    dD = ctx.empty((n, 1), A.dtype).upload(d0.reshape(-1, 1))
    # the saved diagonal is what lacpy_sp reads as a 1 x n matrix of leading dimension ld + 1 (how the Impl saves it)
    dD2 = ctx.empty((n, 1), A.dtype)
    assert lib.chase_hip_lacpy_sp(ctx.h, int(cplx), 1, n, dA.ptr, ld + 1, dD2.ptr, 1) == 0
    assert np.array_equal(dD2.download().ravel(), d0)
    acc = 0.0
    for c in (-0.3712345, 1.25e-3, 0.3699845):                     # the accumulated shift, never (h + c) - c
        acc += c
        assert lib.chase_hip_shift_diag_sp(ctx.h, int(cplx), n, dA.ptr, ld, dD.ptr, acc) == 0
        exp = hA.copy()
        re = (d0.real.astype(np.float64) + acc).astype(np.float32)
        exp[idx, idx] = (re + 1j * d0.imag).astype(A.dtype) if cplx else re
        assert np.array_equal(dA.download(), exp)
    assert lib.chase_hip_shift_diag_sp(ctx.h, int(cplx), n, dA.ptr, ld, dD.ptr, 0.0) == 0       # the unshift
    assert np.array_equal(dA.download(), hA)
    for a in (dA, dD, dD2):
        a.free()


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("uplo", ["U", "L"])
def test_complete_hermitian_sp(ctx, uplo, cplx):
    from chase_amd.capi import lib
    n, ld = 133, 136
    A = _rand(np.random.default_rng(3), (n, n), cplx)
    dA, hA = _padded(ctx, A, ld)
    assert lib.chase_hip_complete_hermitian_sp(ctx.h, int(cplx), uplo.encode(), n, dA.ptr, ld) == 0
    T = np.triu(A, 1) if uplo == "U" else np.tril(A, -1)
    exp = hA.copy(); exp[:n] = T + T.conj().T + np.diag(np.diag(A))
    assert np.array_equal(dA.download(), exp)
    dA.free()


# ---- 2. operators --------------------------------------------------------------------------------------------------------------

def _operator_matrix(kind, cplx):
    if kind == "fixture":
        # the reference's 200 x 200 fixtures; the solver is for Hermitian matrices: their Hermitian part, scaled to norm ~1
        H = read_ref_matrix("cdouble_random_BSE.bin" if cplx else "double_random_BSE.bin", 200, 200, cplx)
        H = (H + H.conj().T) / 2
        return np.asfortranarray((H / np.linalg.norm(H, 2)).astype(_st(cplx)))
    return R.case_matrix(int(kind), cplx)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("kind", ["202", "301", "fixture"])
def test_operators_on_fp32_data(ctx, kind, cplx):
    from chase_amd.capi import SpSolver
    H = _operator_matrix(kind, cplx)
    N = H.shape[0]
    nev, nex, L = 12, 8, 3
    ne = nev + nex
    ldh = N + 6 if kind == "202" else N                     # the caller's matrix in place at a padded ld
    dH, hH = _padded(ctx, H, ldh)
    rng = np.random.default_rng(N + cplx)
    V0 = _rand(rng, (N, ne), cplx)
    s = SpSolver(ctx, None, nev, nex, V=V0.copy(order="F"), h_on_device_ptr=dH.ptr, N=N, cplx=cplx, ldh=ldh)
    assert (s.get("tol"), s.get("deg"), s.get("maxdeg"), s.get("lanczositer")) == (1e-5, 10, 18, 12)
    s.Start(); s.initVecs(False)
    assert np.array_equal(s.peek_v(), R.widen(V0))
    s.QR(0, 1.0)
    A0 = s.peek_v()
    bound = 2 * U + U * U + 1e-13
    assert np.max(np.abs(A0.conj().T @ A0 - np.eye(ne))) <= bound
    s.Lock(L)
    # one bracketed filter call of two steps, the second on fewer columns (as the driver does for mixed degrees)
    c, (a1, a2, b2) = 0.3712345, (1.7, -2.3, 0.6)
    s.set(reset_counters=1)
    s.FilterPhaseStart(); s.Shift(-c)
    idx = np.arange(N)
    Hs = H.copy()
    re = (H[idx, idx].real.astype(np.float64) - c).astype(np.float32)
    Hs[idx, idx] = (re + 1j * H[idx, idx].imag).astype(H.dtype) if cplx else re
    exp_shifted = hH.copy(); exp_shifted[:N] = Hs
    assert np.array_equal(dH.download(), exp_shifted)
    s.HEMM(ne - L, a1, 0.0, 0)
    s.HEMM(ne - L - 2, a2, b2, 2)
    s.Shift(+c, True); s.FilterPhaseEnd()
    assert np.array_equal(dH.download(), hH)                # H bitwise what it was, pads included
    got = s.peek_v()
    # the same two products through ctx.gemm32 on the same operands
    ldv = (N + 3) & ~3
    dHs, _ = _padded(ctx, Hs, ldh)
    dB, _ = _padded(ctx, R.narrow(A0), ldv)
    dC, _ = _padded(ctx, np.zeros((N, ne), dtype=H.dtype), ldv)
    off = lambda d, col: d.ptr + col * ldv * H.dtype.itemsize
    ctx.gemm32("N", N, ne - L, N, a1, dHs.ptr, ldh, off(dB, L), ldv, 0.0, off(dC, L), ldv, cplx)
    ctx.gemm32("N", N, ne - L - 2, N, a2, dHs.ptr, ldh, off(dC, L + 2), ldv, b2, off(dB, L + 2), ldv, cplx)
    exp = dB.download()[:N]
    assert np.array_equal(got, R.widen(exp))                # bit for bit, locked columns (and the two skipped ones) included
    assert np.array_equal(got[:, :L], A0[:, :L])
    assert s.get("hemm_calls") == 0 and s.get("hemm_sp_calls") == 2 and s.get("hemm_sp_vecs") == 2 * (ne - L) - 2
    assert s.get("sp_filters") == 1
    # QR of the filtered block: rounding of an fp64-orthonormal block; locked columns restored
    s.QR(L, 50.0)
    assert s.get("qr_variant") == 2                          # 1e1 < 50 < 1e4: the single-precision thresholds
    Q = s.peek_v()
    assert np.array_equal(Q[:, :L], A0[:, :L])
    print("QR", kind, cplx, "max |Q^H Q - I| / bound", float(np.max(np.abs(Q.conj().T @ Q - np.eye(ne))) / bound))
    assert np.max(np.abs(Q.conj().T @ Q - np.eye(ne))) <= bound
    # Rayleigh-Ritz against fp64 numpy on the same fp32 data
    s.RR(ne - L, L)
    Qu = Q[:, L:]
    Hw = R.widen(H)
    A = Qu.conj().T @ (Hw @ Qu)
    w = np.linalg.eigvalsh((A + A.conj().T) / 2)
    margin = R.ritz_margin(H, Qu) + 1e-13
    print("RR", kind, cplx, "max |ritz - eigvalsh| / margin", float(np.max(np.abs(s.ritzv[L:] - w)) / margin))
    assert np.max(np.abs(s.ritzv[L:] - w)) <= margin
    V = s.peek_v()
    assert np.array_equal(V[:, :L], A0[:, :L])
    # ... and so do the residuals
    r = s.Resd(L)
    ref = R.host_residuals(H, s.ritzv[L:], V[:, L:])
    rb = R.resid_product_bound(H, V[:, L:]) + 1e-13
    print("Resd", kind, cplx, "max |resd - fp64| / bound", float(np.max(np.abs(r - ref) / rb)))
    assert np.all(np.abs(r - ref) <= rb)
    assert np.array_equal(s.resid()[L:], r)
    assert np.all(np.abs(s.recompute_residuals(ne, s.ritzv)[L:] - ref) <= rb)      # a fresh product of all columns
    # deferred swaps reach the fp32 block; checkSymmetryEasy sees a Hermitian matrix and an asymmetric one
    s.Swap(L, ne - 1); s.Swap(L + 1, L + 2)
    P = s.peek_v()
    order = list(range(ne)); order[L], order[ne - 1] = order[ne - 1], order[L]; order[L + 1], order[L + 2] = order[L + 2], order[L + 1]
    assert np.array_equal(P, V[:, order])
    assert s.checkSymmetryEasy()
    assert np.array_equal(dH.download(), hH)
    bad = hH.copy(); bad[5, 1] += np.float32(0.25)
    dH.upload(bad)
    assert not s.checkSymmetryEasy()
    s.symOrHermMatrix("U")
    fixed = dH.download()[:N]
    assert np.array_equal(fixed, np.triu(H) + np.triu(H, 1).conj().T) and s.checkSymmetryEasy()
    with pytest.raises(Exception):
        s.set(device_rng=1)
    s.End()
    assert np.array_equal(R.widen(s.V), P)
    s.close()
    for a in (dH, dHs, dB, dC):
        a.free()


# ---- 3. whole solves -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "N%d-%d-%d-%s" % (c[0], c[1], c[2], "c" if c[3] else "r"))
def test_whole_solves_of_the_emulated_cases(ctx, case):
    from chase_amd.capi import SpSolver
    N, nev, nex, cplx = case
    emu = R.emulated(*case)["sp"]
    H = R.case_matrix(N, cplx)
    H0 = H.copy()
    s = SpSolver(ctx, H, nev, nex)
    tol = s.get("tol")
    assert tol == 1e-5
    st = s.solve()
    lam = s.ritzv[:nev].copy()
    own = s.resid()[:nev]
    host = R.host_residuals(H, lam, s.V[:, :nev])
    pb = R.resid_product_bound(H, s.V[:, :nev])
    ev = np.linalg.eigvalsh(R.widen(H))[:nev]
    print("solve", case, {k: st[k] for k in ("iterations", "filtered_vecs", "locked")}, "emulation",
          {k: emu[k] for k in ("iterations", "filtered_vecs")}, "max own resid", float(np.max(own)), "max host resid",
          float(np.max(host)), "max product bound", float(np.max(pb)), "max eig err", float(np.max(np.abs(lam - ev))))
    assert np.array_equal(H, H0)                             # the caller's host matrix is read only
    assert st["locked"] >= nev
    assert np.max(own) <= tol
    assert np.all(host <= tol + pb)
    assert np.max(np.abs(lam - ev)) <= np.max(host)
    assert abs(st["iterations"] - emu["iterations"]) <= 1
    assert abs(st["filtered_vecs"] - emu["filtered_vecs"]) <= 0.05 * emu["filtered_vecs"]
    assert s.get("hemm_calls") == 0 and s.get("hemm_sp_vecs") == st["filtered_vecs"]
    st2 = s.solve()                                          # the handle is reusable: same matrix, same counts
    assert (st2["iterations"], st2["filtered_vecs"], st2["locked"]) == (st["iterations"], st["filtered_vecs"], st["locked"])
    s.close()


# ---- 4. the C interface ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cplx", [False, True])
def test_single_precision_c_interface(ctx, cplx):
    from chase_amd.capi import lib
    N, nev, nex = 256, 24, 16
    H = R.case_matrix(N, cplx)
    pre = "c" if cplx else "s"
    fn = lambda name: getattr(lib, pre + name)
    ci = lambda v: C.byref(C.c_int(v))
    solve = lambda mode: fn("chase_")(ci(10), C.byref(C.c_float(1e-5)), C.c_char_p(mode), C.c_char_p(b"S"), C.c_char_p(b"C"))
    V = np.zeros((N, nev + nex), dtype=H.dtype, order="F")
    lam = np.zeros(nev + nex, dtype=np.float32)
    init = C.c_int(0)
    fn("chase_init_")(ci(N), ci(nev), ci(nex), C.c_void_p(H.ctypes.data), ci(N), C.c_void_p(V.ctypes.data), C.c_void_p(lam.ctypes.data),
                      C.byref(init))
    assert init.value == 1
    lib.chase_hip_cshim_seq_solver.restype = C.c_void_p
    h = C.c_void_p(lib.chase_hip_cshim_seq_solver(4 if cplx else 3))
    assert h.value
    def get(key):
        out = C.c_double(0)
        assert lib.chase_hip_solver_get(h, key.encode(), C.byref(out)) == 0
        return out.value
    solve(b"R")
    tol = float(np.float32(1e-5))
    assert get("tol") == tol and get("locked") >= nev
    its = get("iterations")
    bound = tol + R.resid_product_bound(H, V[:, :nev])
    assert np.all(R.host_residuals(H, lam[:nev].astype(np.float64), V[:, :nev]) <= bound + 4 * U * np.abs(lam[:nev]))
    ev = np.linalg.eigvalsh(R.widen(H))[:nev]
    assert np.max(np.abs(lam[:nev] - ev)) <= tol
    # get_eigenpairs into a padded block
    ld = N + 3
    out = np.zeros((ld, nev), dtype=H.dtype, order="F")
    lo = np.zeros(nev, dtype=np.float32)
    fn("chase_get_eigenpairs_")(C.c_void_p(out.ctypes.data), ci(ld), C.c_void_p(lo.ctypes.data))
    assert np.array_equal(out[:N], V[:, :nev]) and np.all(out[N:] == 0) and np.array_equal(lo, lam[:nev])
    # approximate restart from the solution: converges at once
    solve(b"A")
    assert get("locked") >= nev and get("iterations") <= its
    lib.chase_set_max_iter_(ci(1))                          # the unified setters reach the single-precision solver
    assert get("maxiter") == 1
    # init = 1 reuse: a second init replaces the solver, the internal variant owns its storage
    fn("chase_init_internal_")(ci(N), ci(nev), ci(nex), C.c_void_p(H.ctypes.data), ci(N), C.byref(init))
    assert init.value == 1
    solve(b"R")
    out2 = np.zeros((N, nev), dtype=H.dtype, order="F")
    fn("chase_get_eigenpairs_")(C.c_void_p(out2.ctypes.data), ci(N), C.c_void_p(lo.ctypes.data))
    assert np.max(np.abs(lo - ev)) <= tol
    assert np.all(R.host_residuals(H, lo.astype(np.float64), out2) <= tol + R.resid_product_bound(H, out2) + 4 * U * np.abs(lo))
    flag = C.c_int(7)
    fn("chase_finalize_")(C.byref(flag))
    assert flag.value == 0 and not lib.chase_hip_cshim_seq_solver(4 if cplx else 3)
    solve(b"R")                                             # finalised: a no-op


# ---- 5. memory, refusals, environment ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cplx", [False, True])
def test_no_fp64_matrix_refused_switches_ignored_environment(ctx, cplx, monkeypatch):
    from chase_amd.capi import ChaseHipError, Solver, SpSolver, lib, tape_mode
    N, nev, nex = 1024, 8, 8
    H = R.case_matrix(N, cplx)
    for var, val in (("CHASE_HIP_MIXED_PRECISION", "1"), ("CHASE_HIP_SP_PRODUCT", "bf16x3"), ("CHASE_HIP_SP_PREPACK", "1")):
        monkeypatch.setenv(var, val)
    s = SpSolver(ctx, H, nev, nex)
    fp64_matrix = N * N * 8 * (2 if cplx else 1)
    assert 0 < s.get("device_bytes") < fp64_matrix
    assert s.get("device_bytes") >= H.nbytes                 # its own fp32 copy of H is in the figure
    for key in ("mixed_precision", "sp_product", "sp_prepack", "h2_mixed_precision"):
        assert s.get(key) == 0                               # the environment did not reach it
        with pytest.raises(ChaseHipError) as e:
            s.set(**{key: 1})
        assert e.value.code == EINVAL and "single-precision" in str(e.value)
        s.set(**{key: 0})
    for mode in (1, 2):
        with pytest.raises(ChaseHipError) as e:
            tape_mode(s, mode)
        assert e.value.code == EINVAL
    tape_mode(s, 0)
    hv = C.c_ulonglong()
    assert lib.chase_hip_solver_hash_v(s.h, ctx.h, 1, C.byref(hv)) == EINVAL
    st = s.solve()
    assert st["locked"] >= nev and s.get("hemm_calls") == 0 and s.get("hemm_sp_split_calls") == 0
    assert s.get("hemm_sp_vecs") == st["filtered_vecs"]
    assert s.get("device_bytes") < fp64_matrix               # still no fp64 matrix after a solve
    # the fp64 solver under the same settings holds the fp64 matrix (and, with this environment, its fp32 shadow)
    d = Solver(ctx, np.asfortranarray(R.widen(H)), nev, nex)
    assert d.get("mixed_precision") == 1
    assert d.get("device_bytes") >= fp64_matrix
    d.close()
    # a device matrix is used in place: nothing of the size of H is allocated
    dH, _ = _padded(ctx, H, N)
    t = SpSolver(ctx, None, nev, nex, h_on_device_ptr=dH.ptr, N=N, cplx=cplx, ldh=N)
    assert t.get("device_bytes") < H.nbytes
    t.close(); s.close(); dH.free()
