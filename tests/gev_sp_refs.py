"""Inputs, checkers and numpy models for the single-precision generalized problem H x = lambda S x (chase_hip_gemm_s_op / _c_op,
chase_hip_trsm_left_upper_sp, chase_hip_trmm_left_upper_sp, chase_hip_potrf_upper_blocked_sp, chase_hip_hegst_upper_sp,
chase_hip_gev_reduce_sp / _backtransform_sp / _starttransform_sp, SpGevSolver): numpy / scipy only, no GPU, no chase_amd.
Imported by tests/test_gpu_gev_sp.py and - the checkers are checked themselves - tests/test_gev_sp_refs_cpu.py.

The conventions and helpers are those of tests/gev_refs.py and tests/dense_chain_refs.py with EPS32 = 2**-23 in place of
EPS = 2**-52: every checker returns a RATIO, error over bound, and a result passes at <= 1.  Residuals are formed in long double
against the fp32-ROUNDED inputs taken as exact data (a float widens to long double exactly), so nothing of the rounding of the
inputs is charged to or forgiven the code under test.
* derived bounds, factor 1, no margin: the left solve (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 8.5),
  the triangular product (eq. 3.13: |X' - op(U) X| <= gamma(n) |op(U)| |X|), the Cholesky factor (Thm 10.3) and the product
  C' = alpha op(A) B + beta C with |alpha|, |beta| in {0, 1}: k multiply-adds and the one addition of beta C, each rounded with
  unit roundoff u = EPS32 / 2, give |C' - exact| <= (k + 1) u (|op(A)| |B| + |C|) <= gamma32(k) (|op(A)| |B| + |beta C|) for k >= 1.
  Complex data: four-multiplication products, the factor 2 sqrt 2 of gamma(k, cplx).
* measured bound: the two-sided reduction, |U^H C U - A| <= K_HEGST_SP n EPS32 (|A| + |U^H| |C| |U|) with
  K_HEGST_SP = MARGIN x what LAPACK's ssygst / chegst reach on exactly the inputs of the GPU test (LAPACK_HEGST_SP below; the CPU
  test measures again).
* assembled bounds for the whole solve (gev_residual_bound): no further constant.
Because the fp64 checkers of gev_refs.py normalise by gamma(n) / n EPS, a ratio against the fp32 bound is their ratio times
gamma(n) / gamma32(n) (or EPS / EPS32): the long double residual is the same, only the yardstick changes."""
import math
import numpy as np
import scipy.linalg as sla
import gev_refs as G
from dense_chain_refs import (padded, same_padding, same_bits, ld_matmul, _max_ratio, seed_of, MARGIN, EPS, LD, CANARY,  # noqa: F401
                              K_EIG_ORTH)
from gev_refs import (herm_full, exactly_hermitian, gev_resid_ld, gev_value_bound, value_errors, _two_norm,  # noqa: F401
                      TRSM_N, TRSM_NRHS, POTRF_CASES, HEGS2_SIZES, SOLVE_N, SOLVE_NEV, SOLVE_NEX, NB)

EPS32 = 2.0 ** -23

# max |U^H C U - A| / ((|A| + |U^H| |C| |U|) n EPS32) of scipy.linalg.lapack.ssygst / chegst (itype 1, upper) over hegst_cases()
# below, real and complex, rounded up to two digits: 0.1273 at n = 2 real, kappa 1e3 (n EPS32 is smallest at the small sizes).
# tests/test_gev_sp_refs_cpu.py measures again, fails if LAPACK exceeds this and fails if it stays below half of it.
LAPACK_HEGST_SP = 0.13
K_HEGST_SP = MARGIN * LAPACK_HEGST_SP

# ---- the shapes the GPU tests run --------------------------------------------------------------------------------------------
GEMM_SHAPES = [(1, 1, 1), (127, 65, 9), (128, 64, 16), (129, 130, 200), (257, 33, 321)]      # (m, n, k)
TRMM_N = TRSM_N + [257, 321]             # a second 256-row block, a ragged last 64-step
POTRF_KAPPAS_SP = [10.0, 1e4]            # fp32 cannot factor the fp64 tests' 1e10; LAPACK's spotrf / cpotrf pass up to 1e6
HEGST_N = [65, 129, 200, 321]
HEGST_KAPPAS_SP = [10.0, 1e3]
SOLVE_TOL_SP = 1e-5


def gamma32(k, cplx=False):
    g = k * EPS32 / (1.0 - k * EPS32)
    return g * 2.0 * math.sqrt(2.0) if cplx else g


def r32(a):
    """the input rounded to fp32 / complex fp32, Fortran order"""
    a = np.asarray(a)
    return np.asfortranarray(a.astype(np.complex64 if np.iscomplexobj(a) else np.float32))


def nan_lower(A):
    """A with NaN in its strictly lower triangle, type kept"""
    A = np.asarray(A)
    return np.asfortranarray(np.triu(A) + np.tril(np.full(A.shape, np.nan, dtype=A.dtype), -1))


def wide(a):
    """exact fp64 copy of an fp32 array"""
    a = np.asarray(a)
    return np.asfortranarray(a.astype(np.complex128 if np.iscomplexobj(a) else np.float64))


# ---- inputs: those of gev_refs.py, rounded --------------------------------------------------------------------------------------
def gemm_inputs(m, n, k, cplx):
    """(A m x k, B k x n, C m x n) random fp32"""
    rng = np.random.default_rng(seed_of(31, m, n, k, cplx))
    return tuple(r32(G.rnd(rng, s, cplx)) for s in ((m, k), (k, n), (m, n)))


def trsm_inputs(n, nrhs, cplx):
    R, B = G.trsm_inputs(n, nrhs, cplx)
    return r32(R), r32(B)


def potrf_input(n, cplx, kappa):
    return r32(G.potrf_input(n, cplx, kappa))        # rounding keeps it Hermitian; positive definite up to kappa ~ 1e6


def hegst_inputs(n, cplx, kappa):
    A, U = G.hegst_inputs(n, cplx, kappa)
    return r32(A), r32(U)


def hegst_cases():
    """every (n, kappa) the GPU test runs through chase_hip_hegst_upper_sp"""
    return [(n, k) for n in HEGS2_SIZES + HEGST_N for k in HEGST_KAPPAS_SP]


def solve_inputs(cplx, step=0):
    """(H32, S32) of the whole-solve test: gev_refs.solve_inputs with H divided by the largest |lambda| of the pencil, so that
    ||C||_2 ~ 1 (the fp32 floor of the solver's residual is sqrt(N) 2^-24 ||C||), rounded.  step 1: H moved by 1e-3 ||H||; step 2:
    H and S moved (the next pencils of a sequence)."""
    H, S = G.solve_inputs(cplx)
    H = H / np.max(np.abs(sla.eigh(H, S, eigvals_only=True)))
    if step:
        rng = np.random.default_rng(seed_of(32, step, cplx))
        d = G.rnd(rng, H.shape, cplx)
        H = H + 1e-3 * np.linalg.norm(H, 2) / np.linalg.norm(d + d.conj().T, 2) * (d + d.conj().T)
        if step == 2:
            d = G.rnd(rng, H.shape, cplx)
            S = S + 1e-3 * sla.eigvalsh(S)[0] / np.linalg.norm(d + d.conj().T, 2) * (d + d.conj().T)
    return r32(H), r32(S)


# ---- checkers --------------------------------------------------------------------------------------------------------------------
def _cplx(*a):
    return any(np.iscomplexobj(x) for x in a)


def gemm_ratio(Cout, op, alpha, A, B, beta, C0):
    """max |Cout - (alpha op(A) B + beta C0)| / (gamma32(k) (|op(A)| |B| + |beta C0|)), alpha and beta of modulus 0 or 1"""
    k = B.shape[0]
    cplx = _cplx(A, B, C0)
    re, im = ld_matmul(A, B, conj_a=(op == "C"))
    im = np.zeros_like(re) if im is None else im
    c0 = (np.asarray(C0).real.astype(LD), np.asarray(C0).imag.astype(LD))
    re, im = alpha * re + beta * c0[0], alpha * im + beta * c0[1]
    co = np.asarray(Cout)
    if not np.all(np.isfinite(co)):
        return math.inf
    err = np.hypot(co.real.astype(LD) - re, co.imag.astype(LD) - im)
    aA = np.abs(A).astype(LD)
    bound = gamma32(k, cplx) * ((aA.T if op == "C" else aA) @ np.abs(B).astype(LD) + abs(beta) * np.abs(C0).astype(LD))
    return _max_ratio(err, bound)


def left_solve_ratio(X, R, B, op):
    n = R.shape[1]
    cplx = _cplx(R, B)
    return G.left_solve_ratio(X, R, B, op) * (G.gamma(n, cplx) / gamma32(n, cplx))


def trmm_ratio(Xout, U, X, op):
    """max |Xout - op(U) X| / (gamma32(n) (|op(U)| |X|)), U taken as triu"""
    n = U.shape[1]
    cplx = _cplx(U, X)
    U = np.triu(np.asarray(U)[:n, :n])
    xo = np.asarray(Xout)
    if not np.all(np.isfinite(xo)):
        return math.inf
    re, im = ld_matmul(U, X, conj_a=(op == "C"))
    err = np.hypot(xo.real.astype(LD) - re, xo.imag.astype(LD) - (0 if im is None else im))
    aU = np.abs(U).astype(LD)
    return _max_ratio(err, gamma32(n, cplx) * ((aU.T if op == "C" else aU) @ np.abs(X).astype(LD)))


def chol_ratio(A, R):
    n = A.shape[0]
    cplx = np.iscomplexobj(A)
    return G.chol_ratio(A, R) * (G.gamma(n + 1, cplx) / gamma32(n + 1, cplx))


def hegst_raw(A, U, C):
    """gev_refs.hegst_raw normalised with EPS32"""
    return G.hegst_raw(A, U, C) * (EPS / EPS32)


def hegst_ratio(A, U, C):
    return hegst_raw(A, U, C) / K_HEGST_SP


def orth_ratio(X, S, U):
    return G.orth_ratio(X, S, U) * (EPS / EPS32)


def gev_residual_bound(H, S, U, C, lam, x, rho):
    """gev_refs.gev_residual_bound with gamma32, EPS32 and K_HEGST_SP: the same assembly from chol_ratio, hegst_ratio and
    left_solve_ratio of this file, no further constant.  x: the computed (fp32) solution of U x = y, ||y||_2 = 1; rho: the
    solver's residual of (lam, y) on the reduced matrix."""
    n = H.shape[0]
    cplx = _cplx(H, S)
    U = np.triu(wide(U)[:n, :n])
    aU = np.abs(U)
    H, C = wide(H), wide(C)
    nU, naU, nC = _two_norm(U), _two_norm(aU), _two_norm(C)
    t_h = K_HEGST_SP * n * EPS32 * _two_norm(np.abs(H) + aU.T @ (np.abs(C) @ aU))
    t_s = abs(lam) * gamma32(n + 1, cplx) * _two_norm(aU.T @ aU)
    t_x = gamma32(n, cplx) * nU * naU * (nC + abs(lam))
    return nU * rho + float(np.linalg.norm(wide(x))) * (t_h + t_s + t_x)


# ---- numpy models of the device's blocked algorithms in fp32 (capi_gev.hip, float) ---------------------------------------------------
def model_trsm_left(R, Bp, n, op, **defects):
    """gev_refs.model_trsm_left on float32 data: numpy keeps the type, so every product and inverse is rounded to fp32"""
    assert np.asarray(R).dtype in (np.float32, np.complex64) and np.asarray(Bp).dtype in (np.float32, np.complex64)
    return G.model_trsm_left(R, Bp, n, op, **defects)


def model_trmm_left(U, Xp, n, op, unconjugated=False):
    """chase_hip_trmm_left_upper_sp on the padded buffer Xp: blocks of SOLVE_WB rows, 64-row steps inside"""
    Xp = np.array(Xp, order="F", copy=True)
    U = np.triu(np.asarray(U)[:n, :n])
    ct = (lambda M: M.T) if unconjugated else (lambda M: M.conj().T)
    W = G.SOLVE_WB
    if op == "N":
        for J0 in range(0, n, W):
            Jend = min(n, J0 + W)
            for j0 in range(J0, Jend, NB):
                j1 = min(j0 + NB, Jend)
                Xp[j0:j1] = U[j0:j1, j0:j1] @ Xp[j0:j1]
                if j1 < Jend:
                    Xp[j0:j1] += U[j0:j1, j1:Jend] @ Xp[j1:Jend]
            if Jend < n:
                Xp[J0:Jend] += U[J0:Jend, Jend:n] @ Xp[Jend:n]
    else:
        for J0 in range((n - 1) // W * W, -1, -W):
            Jend = min(n, J0 + W)
            for j0 in range(J0 + (Jend - J0 - 1) // NB * NB, J0 - 1, -NB):
                j1 = min(j0 + NB, Jend)
                Xp[j0:j1] = ct(U[j0:j1, j0:j1]) @ Xp[j0:j1]
                if j0 > J0:
                    Xp[j0:j1] += ct(U[J0:j0, j0:j1]) @ Xp[J0:j0]
            if J0 > 0:
                Xp[J0:Jend] += ct(U[:J0, J0:Jend]) @ Xp[:J0]
    return Xp


def model_potrf_blocked(A, outer_nb=0, skip_last_update=False):
    """gev_refs.model_potrf_blocked on float32 data (seeded defect: the last diagonal block's last trailing update left out)"""
    assert np.asarray(A).dtype in (np.float32, np.complex64)
    return G.model_potrf_blocked(A, outer_nb, skip_last_update)


def model_hegst(A, U, unconjugated=False):
    """chase_hip_hegst_upper_sp in fp32.  n <= 64: hegs2_diag (gev_refs.model_hegs2).  Above: W = U^{-H} A on the completed
    matrix, W <- W^H, W <- U^{-H} W, the lower triangle kept and mirrored.  Seeded defect: unconjugated - the transpose between
    the solves is taken without the conjugation."""
    n = A.shape[0]
    U = np.triu(np.asarray(U))
    if n <= NB:
        return r32(G.model_hegs2(A, U))
    W = model_trsm_left(U, herm_full(A), n, "C")
    W = np.asfortranarray(W.T if unconjugated else W.conj().T)
    W = model_trsm_left(U, W, n, "C")
    return herm_full(W.conj().T)


def model_hegst_missed_half(A, U):
    """the blocked xHEGST recurrence of gev_refs.model_hegst (panels of 64) with the second 1/2 A11 U12 of the first panel left
    out: the checker must reject a missed half-term whatever formulation the device runs"""
    return r32(G.model_hegst(wide(A), wide(U), NB, miss_half=True))


def lapack_potrf(A):
    f = sla.lapack.cpotrf if np.iscomplexobj(A) else sla.lapack.spotrf
    c, info = f(np.asfortranarray(A), lower=0)
    assert info == 0 and c.dtype == A.dtype
    return np.triu(c)


def lapack_hegst(A, U):
    """LAPACK's ssygst / chegst (itype 1, upper) on the same fp32 inputs, mirrored"""
    f = sla.lapack.chegst if _cplx(A, U) else sla.lapack.ssygst
    c, info = f(herm_full(A), np.triu(U), itype=1, lower=0)
    assert info == 0 and c.dtype == A.dtype
    return herm_full(c)


def lapack_pipeline(H, S, nev):
    """the whole solve with LAPACK in fp32: spotrf, ssygst, ssyevd, strtrs.  Returns (U, C, lam, Y, rho, X)."""
    U = lapack_potrf(S)
    Cm = lapack_hegst(H, U)
    w, Y = sla.eigh(Cm)
    assert Y.dtype == H.dtype
    lam, Y = w[:nev].astype(np.float64), np.asfortranarray(Y[:, :nev])
    rho = gev_resid_ld(Cm, np.eye(H.shape[0], dtype=np.float32), lam, Y)
    X = sla.solve_triangular(U, Y, lower=False)
    assert X.dtype == H.dtype
    return U, Cm, lam, Y, rho, X
