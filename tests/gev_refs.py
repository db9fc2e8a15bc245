"""Inputs, checkers and numpy models for the generalized problem H x = lambda S x (chase_hip_trsm_left_upper,
chase_hip_potrf_upper_blocked, chase_hip_hegst_upper, chase_hip_gev_reduce / _backtransform, GevSolver): numpy / scipy only, no
GPU, no chase_amd.  Imported by tests/test_gpu_gev.py and - the checkers are checked themselves - tests/test_gev_refs_cpu.py.

The conventions are those of tests/dense_chain_refs.py, whose inputs and helpers are used: every checker returns RATIOS, error
over bound, and a result passes at <= 1; residuals are formed in long double.
* derived bounds, factor 1, no margin: the left solve (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 8.5)
  and the Cholesky factor (Thm 10.3, chol_ratio of dense_chain_refs); four-multiplication complex products (factor 2 sqrt 2).
* measured bound: the two-sided reduction.  |U^H C U - A| <= K_HEGST n eps (|A| + |U^H| |C| |U|) componentwise, with
  K_HEGST = MARGIN x what LAPACK's dsygst / zhegst reach on exactly the inputs of the GPU test (LAPACK_HEGST below; the CPU
  test measures again).  The constant is not tightly derivable; the margin of 8 is the project's margin for measured bounds and
  separates a summation order from a dropped term.
* assembled bounds for the whole solve (gev_residual_bound, gev_value_bound): no further constant."""
import math
import numpy as np
import scipy.linalg as sla
from dense_chain_refs import (hpd, rnd, padded, same_padding, ld_matmul, _max_ratio, gamma, chol_ratio, seed_of,  # noqa: F401
                              MARGIN, EPS, LD, CANARY, LAPACK_EIG_VALUE, K_EIG_ORTH, same_bits, model_potrf, model_trsm, _inv_upper)

NB = 64
SOLVE_WB = 256             # the device's block sizes (capi_gev.hip)
TRAP_CB = 256
POTRF_OUTER_NB = 2048

# max |U^H C U - A| / ((|A| + |U^H| |C| |U|) n eps) of scipy.linalg.lapack.dsygst / zhegst (itype 1, upper) over hegst_cases()
# below, real and complex, rounded up to two digits: 0.171 at n = 2 complex, kappa 10 (n eps is smallest at the small sizes; from
# n = 63 on LAPACK stays at or below 0.02; the numpy model of the device's recurrence: 0.214 at n = 2, at most 0.018 from n = 63).
# tests/test_gev_refs_cpu.py measures again and fails if LAPACK exceeds this.
LAPACK_HEGST = 0.18
K_HEGST = MARGIN * LAPACK_HEGST

# ---- the shapes the GPU tests run --------------------------------------------------------------------------------------------
TRSM_N = [1, 2, 63, 64, 65, 129, 200]
TRSM_NRHS = [1, 33, 130]
POTRF_CASES = [(1, 0), (64, 0), (65, 0), (200, 0), (257, 128), (321, 128)]          # (n, outer_nb)
POTRF_KAPPAS = [10.0, 1e10]
HEGS2_SIZES = [1, 2, 63, 64]
HEGST_CASES = [(65, 0), (129, 0), (200, 0), (321, 128)]                               # (n, nb)
HEGST_KAPPAS = [10.0, 1e5]
SOLVE_N, SOLVE_NEV, SOLVE_NEX, SOLVE_KAPPA, SOLVE_TOL = 257, 20, 12, 100.0, 1e-10


def ref_chol(S):
    """the reference upper factor (LAPACK)"""
    return np.asfortranarray(np.linalg.cholesky(S).conj().T)


def herm_full(A):
    """the Hermitian matrix whose upper triangle is A's (the diagonal's imaginary parts dropped)"""
    A = np.asarray(A)
    F = np.triu(A) + np.triu(A, 1).conj().T
    F[np.diag_indices_from(F)] = np.real(np.diag(A))
    return np.asfortranarray(F)


def nan_lower(A):
    return np.asfortranarray(np.triu(A) + np.tril(np.full(A.shape, np.nan), -1))


def trsm_inputs(n, nrhs, cplx):
    """(R, B): R the reference factor of hpd(n, 1e5), B random n x nrhs"""
    rng = np.random.default_rng(seed_of(21, n, nrhs, cplx))
    return ref_chol(hpd(rng, n, cplx, 1e5)), rnd(rng, (n, nrhs), cplx)


def potrf_input(n, cplx, kappa):
    return hpd(np.random.default_rng(seed_of(22, n, cplx, round(math.log10(kappa)))), n, cplx, kappa)


def hegst_inputs(n, cplx, kappa):
    """(A, U): A random Hermitian, U the reference factor of hpd(n, kappa)"""
    rng = np.random.default_rng(seed_of(23, n, cplx, round(math.log10(kappa))))
    U = ref_chol(hpd(rng, n, cplx, kappa))
    x = rnd(rng, (n, n), cplx)
    return np.asfortranarray(x + x.conj().T), U


def hegst_cases():
    """every (n, nb, kappa) the GPU test runs through chase_hip_hegst_upper"""
    return [(n, 0, k) for n in HEGS2_SIZES for k in HEGST_KAPPAS] + [(n, nb, k) for (n, nb) in HEGST_CASES for k in HEGST_KAPPAS]


def solve_inputs(cplx):
    """(H, S) of the whole-solve test: S = hpd(N, 100), H random Hermitian"""
    rng = np.random.default_rng(seed_of(24, SOLVE_N, cplx))
    S = hpd(rng, SOLVE_N, cplx, SOLVE_KAPPA)
    x = rnd(rng, (SOLVE_N, SOLVE_N), cplx)
    return np.asfortranarray(x + x.conj().T), S


# ---- long double helpers on (re, im) planes ---------------------------------------------------------------------------------------
def _pl(a):
    a = np.asarray(a)
    return (a.real.astype(LD), a.imag.astype(LD)) if np.iscomplexobj(a) else (a.astype(LD), np.zeros(a.shape, dtype=LD))


def _mm(a, b):
    return a[0] @ b[0] - a[1] @ b[1], a[0] @ b[1] + a[1] @ b[0]


def _ct(a):
    return a[0].T, -a[1].T


def _two_norm(M):
    M = np.asarray(M)
    M = M.astype(np.complex128 if np.iscomplexobj(M) else np.float64)
    return float(np.linalg.norm(M, 2)) if M.size else 0.0


# ---- checkers ------------------------------------------------------------------------------------------------------------------
def left_solve_ratio(X, R, B, op):
    """max |op(R) X - B|_ij / (gamma(n) (|op(R)| |X|)_ij), R taken as triu, op 'N' or 'C' (Higham Thm 8.5, by columns)"""
    n = R.shape[1]
    cplx = np.iscomplexobj(B) or np.iscomplexobj(R)
    R = np.triu(np.asarray(R)[:n, :n])
    X = np.asarray(X)
    if not np.all(np.isfinite(X)):
        return math.inf
    re, im = ld_matmul(R, X, conj_a=(op == "C"))
    Br, Bi = _pl(B)
    err = np.hypot(re - Br, (0 if im is None else im) - Bi)
    aR = np.abs(R).astype(LD)
    return _max_ratio(err, gamma(n, cplx) * ((aR.T if op == "C" else aR) @ np.abs(X).astype(LD)))


def hegst_raw(A, U, C):
    """max |U^H C U - A|_ij / ((|A| + |U^H| |C| |U|)_ij n eps) in long double; A Hermitian (both triangles), U taken as triu"""
    n = A.shape[0]
    if n == 0:
        return 0.0
    U = np.triu(np.asarray(U)[:n, :n])
    C = np.asarray(C)[:n, :n]
    if not np.all(np.isfinite(C)):
        return math.inf
    u = _pl(U)
    re, im = _mm(_ct(u), _mm(_pl(C), u))
    ar, ai = _pl(A)
    err = np.hypot(re - ar, im - ai)
    aU = np.abs(U).astype(LD)
    bound = (np.abs(A).astype(LD) + aU.T @ (np.abs(C).astype(LD) @ aU)) * (n * EPS)
    return _max_ratio(err, bound)


def hegst_ratio(A, U, C):
    return hegst_raw(A, U, C) / K_HEGST


def exactly_hermitian(C):
    """the lower triangle is the conjugate of the upper one bit for bit and the imaginary diagonal is +0"""
    C = np.asarray(C)
    il = np.tril_indices(C.shape[0], -1)
    ok = same_bits(C[il], np.conj(C.T)[il])
    if np.iscomplexobj(C):
        d = np.ascontiguousarray(np.diag(C).imag)
        ok = ok and d.tobytes() == np.zeros_like(d).tobytes()
    return ok


def gev_resid_ld(H, S, lam, X):
    """|| H x_j - lambda_j S x_j ||_2 per column in long double"""
    x = _pl(X)
    hr, hi = _mm(_pl(H), x)
    sr, si = _mm(_pl(S), x)
    l = np.asarray(lam, dtype=LD)[None, :]
    return np.sqrt(np.sum((hr - l * sr) ** 2 + (hi - l * si) ** 2, axis=0)).astype(np.float64)


def gev_residual_bound(H, S, U, C, lam, x, rho):
    """The a-priori bound on || H x - lambda S x ||_2 for ONE pair, assembled from what is asserted separately, no further
    constant.  U is the computed factor, C the computed reduced matrix, (lambda, y) the solver's pair of C with ||y||_2 = 1 and
    reported residual rho = || C y - lambda y ||_2, x the computed solution of U x = y.
      S = U^H U + E_s,  |E_s| <= gamma(n+1) |U^H| |U|                      (Thm 10.3, asserted by chol_ratio)
      H = U^H C U + E_h,  |E_h| <= K_HEGST n eps (|H| + |U^H| |C| |U|)        (the hegst allowance, asserted by hegst_ratio)
      (U + dU) x = y,  |dU| <= gamma(n) |U|                                  (Thm 8.5, asserted by left_solve_ratio)
    so  H x - lambda S x = U^H (C - lambda) U x + (E_h - lambda E_s) x = U^H (C y - lambda y) - U^H (C - lambda) dU x + (E_h - lambda E_s) x
    and in norms
      <= ||U|| rho + ||x|| [ K_HEGST n eps || |H| + |U^H||C||U| || + |lambda| gamma(n+1) || |U^H||U| || + gamma(n) ||U|| || |U| || (||C|| + |lambda|) ]."""
    n = H.shape[0]
    cplx = np.iscomplexobj(H) or np.iscomplexobj(S)
    U = np.triu(np.asarray(U)[:n, :n])
    aU = np.abs(U)
    nU, naU, nC = _two_norm(U), _two_norm(aU), _two_norm(C)
    t_h = K_HEGST * n * EPS * _two_norm(np.abs(H) + aU.T @ (np.abs(C) @ aU))
    t_s = abs(lam) * gamma(n + 1, cplx) * _two_norm(aU.T @ aU)
    t_x = gamma(n, cplx) * nU * naU * (nC + abs(lam))
    return nU * rho + float(np.linalg.norm(x)) * (t_h + t_s + t_x)


def gev_value_bound(r_norm, lam_min_S, n, norm_C):
    """| lambda_j - nearest eigenvalue of (H, S) | <= || r_j ||_2 / sqrt(lambda_min(S)) for an S-normalised x_j (r_j the long
    double residual against the original matrices: the residual bound of the definite pencil in the S^{-1} norm), plus the
    error of scipy.linalg.eigh(H, S) itself, MARGIN LAPACK_EIG_VALUE n eps ||C||_2"""
    return r_norm / math.sqrt(lam_min_S) + LAPACK_EIG_VALUE * MARGIN * n * EPS * norm_C


def value_errors(lam, wref):
    wref = np.asarray(wref)
    return np.array([np.min(np.abs(wref - l)) for l in lam])


def orth_ratio(X, S, U):
    """max |X^H S X - I| / (K_EIG_ORTH n eps kappa_2(U)) in long double"""
    n = S.shape[0]
    x = _pl(X)
    re, im = _mm(_ct(x), _mm(_pl(S), x))
    err = np.hypot(re - np.eye(X.shape[1], dtype=LD), im)
    kappa = np.linalg.cond(np.triu(np.asarray(U)[:n, :n]))
    return float(np.max(err)) / (K_EIG_ORTH * n * EPS * kappa)


# ---- numpy models of the device's blocked algorithms (capi_gev.hip) -----------------------------------------------------------
def model_trsm_left(R, Bp, n, op, unconjugated=False, zero_inv_col=None, ld_bug=False):
    """chase_hip_trsm_left_upper on the padded buffer Bp (ldb x nrhs, Fortran order; rows >= n are padding).  Returns the buffer.
    Seeded defects: unconjugated - op C takes the plain transpose; zero_inv_col = (block, column) zeroes one column of one
    inverted block; ld_bug - the solved 64-row panel is copied back with the extent n where the leading dimension belongs."""
    Bp = np.array(Bp, order="F", copy=True)
    ldb, nrhs = Bp.shape
    R = np.triu(np.asarray(R)[:n, :n])
    flat = Bp.reshape(-1, order="F")
    assert np.shares_memory(flat, Bp)
    ct = (lambda M: M.T) if unconjugated else (lambda M: M.conj().T)

    def inv(j0, nb):
        T = _inv_upper(R[j0:j0 + nb, j0:j0 + nb])
        if zero_inv_col is not None and zero_inv_col[0] == j0 // NB:
            T[:, zero_inv_col[1]] = 0
        return T

    def put(j0, P):
        ld = n if ld_bug else ldb
        for c in range(nrhs):
            flat[j0 + c * ld: j0 + c * ld + P.shape[0]] = P[:, c]

    if op == "C":
        for J0 in range(0, n, SOLVE_WB):
            Jend = min(n, J0 + SOLVE_WB)
            if J0 > 0:
                Bp[J0:Jend] -= ct(R[:J0, J0:Jend]) @ Bp[:J0]
            for j0 in range(J0, Jend, NB):
                nb = min(NB, Jend - j0)
                P = ct(inv(j0, nb)) @ Bp[j0:j0 + nb]
                put(j0, P)
                if Jend - j0 - nb > 0:
                    Bp[j0 + nb:Jend] -= ct(R[j0:j0 + nb, j0 + nb:Jend]) @ P
    else:
        for J0 in range((n - 1) // SOLVE_WB * SOLVE_WB, -1, -SOLVE_WB):
            Jend = min(n, J0 + SOLVE_WB)
            if Jend < n:
                Bp[J0:Jend] -= R[J0:Jend, Jend:n] @ Bp[Jend:n]
            for j0 in range(J0 + (Jend - J0 - 1) // NB * NB, J0 - 1, -NB):
                nb = min(NB, Jend - j0)
                P = inv(j0, nb) @ Bp[j0:j0 + nb]
                put(j0, P)
                if j0 > J0:
                    Bp[J0:j0] -= R[J0:j0, j0:j0 + nb] @ P
    return Bp


def model_potrf_blocked(A, outer_nb=0, skip_last_update=False):
    """chase_hip_potrf_upper_blocked: U in the upper triangle, the strictly lower triangle as it came.  skip_last_update: seeded
    defect - the last diagonal block's last trailing update is left out."""
    A = np.array(A, order="F", copy=True)
    n = A.shape[0]
    ob = outer_nb or POTRF_OUTER_NB
    for J0 in range(0, n, ob):
        w = min(ob, n - J0)
        jj = slice(J0, J0 + w)
        Ujj = np.triu(model_potrf(herm_full(A[jj, jj])))
        A[jj, jj] = Ujj + np.tril(A[jj, jj], -1)
        T0 = J0 + w
        if T0 >= n:
            break
        A[jj, T0:] = model_trsm_left(Ujj, A[jj, T0:], w, "C")
        for c0 in range(T0, n, TRAP_CB):
            cc = slice(c0, min(n, c0 + TRAP_CB))
            Pc = A[jj, cc]
            A[T0:c0, cc] -= A[jj, T0:c0].conj().T @ Pc
            if skip_last_update and cc.stop == n and T0 + ob >= n:
                continue
            A[cc, cc] += np.triu(-(Pc.conj().T @ Pc))
    return A


def model_hegs2(A, U):
    """hegs2_diag: two triangular solves on the full Hermitian block, the upper triangle kept and mirrored"""
    W = sla.solve_triangular(U, herm_full(A), trans="C", lower=False)
    Cm = sla.solve_triangular(U, W.conj().T, trans="C", lower=False).conj().T
    return herm_full(Cm)


def _hegst_rec(A, U, nb, top, miss_half, skip_last):
    n = A.shape[0]
    for k0 in range(0, n, nb):
        kb = min(nb, n - k0)
        kk = slice(k0, k0 + kb)
        if kb <= NB:
            A[kk, kk] = model_hegs2(A[kk, kk], np.triu(U[kk, kk]))
        else:
            sub = np.array(A[kk, kk], order="F")
            _hegst_rec(sub, U[kk, kk], NB, False, False, False)
            A[kk, kk] = herm_full(sub)
        T0 = k0 + kb
        if T0 >= n:
            break
        rr = slice(T0, n)
        A[kk, rr] = model_trsm_left(np.triu(U[kk, kk]), A[kk, rr], kb, "C")
        A[kk, rr] -= 0.5 * (A[kk, kk] @ U[kk, rr])
        if not (top and skip_last and T0 + nb >= n):
            A[rr, rr] -= A[kk, rr].conj().T @ U[kk, rr] + U[kk, rr].conj().T @ A[kk, rr]
        if not (top and miss_half and k0 == 0):
            A[kk, rr] -= 0.5 * (A[kk, kk] @ U[kk, rr])
        A[kk, rr] = model_trsm(np.triu(U[rr, rr]), A[kk, rr], kb)


def model_hegst(A, U, nb=0, miss_half=False, skip_last_update=False):
    """chase_hip_hegst_upper.  n <= 64: hegs2_diag.  nb > 0: the blocked xHEGST recurrence on the upper triangle, panels of nb
    (diagonal blocks wider than 64 by the same recurrence with nb = 64), mirrored at the end.  Seeded defects: miss_half - the
    second 1/2 A11 U12 of the first panel is left out; skip_last_update - the last panel's trapezoid update is left out.
    nb = 0: two full solves on the completed matrix with the blocked right and left solves, the LOWER triangle of the result kept
    and mirrored, real diagonal."""
    n = A.shape[0]
    U = np.triu(np.asarray(U))
    if n <= NB:
        return model_hegs2(A, U)
    if nb == 0:
        W = model_trsm(U, herm_full(A), n)
        W = model_trsm_left(U, W, n, "C")
        return herm_full(W.conj().T)
    A = herm_full(A)
    _hegst_rec(A, U, nb, True, miss_half, skip_last_update)
    return herm_full(A)


def lapack_hegst(A, U):
    """LAPACK's dsygst / zhegst (itype 1, upper) on the same inputs, mirrored"""
    f = sla.lapack.zhegst if np.iscomplexobj(A) or np.iscomplexobj(U) else sla.lapack.dsygst
    c, info = f(herm_full(A), np.triu(U), itype=1, lower=0)
    assert info == 0
    return herm_full(c)


def model_pipeline(H, S, nev):
    """model reduce -> scipy.linalg.eigh as the solver (rho: its measured residual on the reduced matrix) -> model back-solve.
    Returns (U, C, lam, Y, rho, X)."""
    U = np.triu(model_potrf_blocked(S))
    Cm = model_hegst(H, U)
    w, Y = sla.eigh(Cm)
    lam, Y = w[:nev], np.asfortranarray(Y[:, :nev])
    rho = np.linalg.norm(Cm @ Y - Y * lam[None, :], axis=0)
    X = model_trsm_left(U, Y, H.shape[0], "N")
    return U, Cm, lam, Y, rho, X
