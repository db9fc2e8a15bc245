"""Inputs, checkers and numpy models for sequences of generalized problems and for itype 2 / 3 (chase_hip_trmm_left_upper,
chase_hip_hegst_product_upper, chase_hip_gev_reduce_itype / _backtransform_itype / _starttransform, GevSolver(itype=...) and
GevSolver.update): numpy / scipy only, no GPU, no chase_amd.  Imported by tests/test_gpu_gev_seq.py and - the checkers are
checked themselves - tests/test_gev_seq_refs_cpu.py.

The conventions are those of tests/gev_refs.py and tests/dense_chain_refs.py, whose inputs and helpers are used: every checker
returns RATIOS, error over bound, and a result passes at <= 1; residuals are formed in long double.  Every bound here is derived,
factor 1, no margin, no measured constant:
* the triangular product.  Every entry of op(U) X is a sum of at most n products in some order, so
  |Y - op(U) X| <= gamma(n) |op(U)| |X| componentwise (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section
  3.1 and eq. 3.13); gamma(n, True) carries the factor 2 sqrt 2 of four-multiplication complex products that left_solve_ratio
  uses.  The blocking (64-row steps, rectangles, one long product per 256 rows) only changes the order of the sum.
* the product reduction C = U A U^H as two successive products, W = fl(A U^H) = A U^H + E1 with |E1| <= gamma |A| |U^H|, then
  C = fl(U W) = U W + E2 with |E2| <= gamma |U| |W| <= gamma (1 + gamma) |U| |A| |U^H|, so
  |C - U A U^H| <= |U| |E1| + |E2| <= (2 gamma + gamma^2) |U| |A| |U^H|.  The device forms U (U A)^H, the same two products
  with the roles of the sides exchanged, and keeps one triangle of the result, mirrored: the kept triangle satisfies the bound
  as computed and the mirrored one is its conjugate against the conjugate of a Hermitian reference, so the bound is not
  enlarged.
* assembled bounds for whole solves with itype 2 and 3 (gev_residual_bound_itype): no further constant."""
import math
import numpy as np
import scipy.linalg as sla
from dense_chain_refs import (rnd, padded, same_padding, ld_matmul, _max_ratio, gamma, seed_of, MARGIN, EPS, LD,  # noqa: F401
                              LAPACK_EIG_VALUE, K_EIG_ORTH, same_bits)
from gev_refs import (NB, SOLVE_WB, ref_chol, herm_full, nan_lower, hegst_inputs, solve_inputs, exactly_hermitian,  # noqa: F401
                      left_solve_ratio, _pl, _mm, _ct, _two_norm, SOLVE_N)
from dense_chain_refs import hpd

# ---- the shapes the GPU tests run --------------------------------------------------------------------------------------------
TRMM_N = [1, 2, 63, 64, 65, 129, 200, 257, 321]      # one block, ragged 64-steps, the 256-row boundary crossed once and ragged
TRMM_NCOLS = [1, 33, 130]
HEGSTP_N = [1, 2, 63, 64, 65, 129, 200, 321]
HEGSTP_KAPPAS = [10.0, 1e5]
ROUNDTRIP_CASES = [(65, 33), (257, 130), (321, 33)]  # (n, ncols) of the product / solve and start / back-transform round trips
PERTURBATION = 1e-3


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def trmm_inputs(n, ncols, cplx):
    """(U, X): U the reference factor of hpd(n, 1e5), X random n x ncols"""
    rng = np.random.default_rng(seed_of(27, n, ncols, cplx))
    return ref_chol(hpd(rng, n, cplx, 1e5)), rnd(rng, (n, ncols), cplx)


def perturbed_pencil(H, S, key, cplx, with_s=True):
    """The next pencil of a sequence: H + 1e-3 ||H||_2 (e + e^H) / ||e + e^H||_2 and, with_s, S + 1e-3 lambda_min(S)
    (f + f^H) / ||f + f^H||_2, which stays positive definite by construction (Weyl: lambda_min moves by at most 1e-3 of itself).
    e, then f, are drawn from default_rng(seed_of(key, n, cplx)); f is drawn whether it is used or not."""
    n = H.shape[0]
    rng = np.random.default_rng(seed_of(key, n, cplx))
    e = rnd(rng, (n, n), cplx)
    f = rnd(rng, (n, n), cplx)
    e, f = e + e.conj().T, f + f.conj().T
    H1 = np.asfortranarray(H + PERTURBATION * np.linalg.norm(H, 2) * e / np.linalg.norm(e, 2))
    if not with_s:
        return H1, S
    S1 = S + PERTURBATION * sla.eigvalsh(S)[0] * f / np.linalg.norm(f, 2)
    return H1, np.asfortranarray((S1 + S1.conj().T) / 2)


# ---- checkers ------------------------------------------------------------------------------------------------------------------
def tri_product_bound(U, X, op):
    """gamma(n) |op(U)| |X| in long double, U taken as triu"""
    n = U.shape[1]
    cplx = np.iscomplexobj(X) or np.iscomplexobj(U)
    aU = np.abs(np.triu(np.asarray(U)[:n, :n])).astype(LD)
    return gamma(n, cplx) * ((aU.T if op == "C" else aU) @ np.abs(np.asarray(X)).astype(LD))


def tri_product_ratio(Y, U, X, op):
    """max |Y - op(U) X|_ij / (gamma(n) (|op(U)| |X|)_ij), U taken as triu, op 'N' or 'C'"""
    n = U.shape[1]
    U = np.triu(np.asarray(U)[:n, :n])
    Y = np.asarray(Y)
    if not np.all(np.isfinite(Y)):
        return math.inf
    re, im = ld_matmul(U, X, conj_a=(op == "C"))
    yr, yi = _pl(Y)
    err = np.hypot(re - yr, (0 if im is None else im) - yi)
    return _max_ratio(err, tri_product_bound(U, X, op))


def roundtrip_ratio(Z, X, U, Y, op):
    """Z = fl(op(U)^{-1} Y) with Y = fl(op(U) X) against X.  The solve gives op(U) Z = Y + r with |r| <= gamma |op(U)| |Z| (Thm
    8.5), the product Y = op(U) X + p with |p| <= gamma |op(U)| |X|, so op(U) (Z - X) = r + p and
    |Z - X| <= |op(U)^{-1}| gamma |op(U)| (|Z| + |X|): the sum of the two derived bounds, carried through the inverse.
    The inverse comes from LAPACK in double: its relative error, of order n eps kappa, scales a bound, not an error."""
    n = U.shape[1]
    cplx = np.iscomplexobj(X) or np.iscomplexobj(U)
    U = np.triu(np.asarray(U)[:n, :n])
    Z = np.asarray(Z)
    if not np.all(np.isfinite(Z)):
        return math.inf
    aU = np.abs(U).astype(LD)
    aI = np.abs(sla.solve_triangular(U, np.eye(n, dtype=U.dtype), lower=False)).astype(LD)
    if op == "C":
        aU, aI = aU.T, aI.T
    bound = aI @ (gamma(n, cplx) * (aU @ (np.abs(Z).astype(LD) + np.abs(np.asarray(X)).astype(LD))))
    zr, zi = _pl(Z)
    xr, xi = _pl(X)
    return _max_ratio(np.hypot(zr - xr, zi - xi), bound)


def solve_then_product_ratio(Z, X, U, Y, op):
    """Z = fl(op(U) Y) with Y = fl(op(U)^{-1} X) against X - the other order.  (op(U) + dT) Y = X with |dT| <= gamma |op(U)|
    (Thm 8.5) and Z = op(U) Y + p with |p| <= gamma |op(U)| |Y|, so Z - X = p - dT Y and |Z - X| <= 2 gamma |op(U)| |Y|: the
    sum of the two derived bounds, no inverse needed."""
    Z = np.asarray(Z)
    if not np.all(np.isfinite(Z)):
        return math.inf
    zr, zi = _pl(Z)
    xr, xi = _pl(X)
    return _max_ratio(np.hypot(zr - xr, zi - xi), 2 * tri_product_bound(U, Y, op))


def product_reduction_ratio(A, U, C):
    """max |C - U A U^H|_ij / ((2 gamma + gamma^2) (|U| |A| |U^H|)_ij) in long double, gamma = gamma(n, cplx); A Hermitian (both
    triangles), U taken as triu"""
    n = A.shape[0]
    if n == 0:
        return 0.0
    cplx = np.iscomplexobj(A) or np.iscomplexobj(U)
    U = np.triu(np.asarray(U)[:n, :n])
    C = np.asarray(C)[:n, :n]
    if not np.all(np.isfinite(C)):
        return math.inf
    u = _pl(U)
    re, im = _mm(u, _mm(_pl(A), _ct(u)))
    cr, ci = _pl(C)
    err = np.hypot(re - cr, im - ci)
    aU = np.abs(U).astype(LD)
    g = gamma(n, cplx)
    return _max_ratio(err, (2 * g + g * g) * (aU @ (np.abs(A).astype(LD) @ aU.T)))


def pencil_resid_ld(itype, H, S, lam, X):
    """per column in long double: || H x - lambda S x ||_2 (itype 1), || H S x - lambda x ||_2 (2), || S H x - lambda x ||_2 (3)"""
    x, h, s = _pl(X), _pl(H), _pl(S)
    if itype == 1:
        (wr, wi), (vr, vi) = _mm(h, x), _mm(s, x)
    else:
        wr, wi = _mm(h, _mm(s, x)) if itype == 2 else _mm(s, _mm(h, x))
        vr, vi = x
    l = np.asarray(lam, dtype=LD)[None, :]
    return np.sqrt(np.sum((wr - l * vr) ** 2 + (wi - l * vi) ** 2, axis=0)).astype(np.float64)


def gev_residual_bound_itype(itype, H, S, U, C, lam, x, rho):
    """The a-priori bound on the residual of ONE pair of an itype 2 or 3 pencil, assembled from what is asserted separately, no
    further constant.  U is the computed factor, C the computed reduced matrix, (lambda, y) the solver's pair of C with
    ||y||_2 = 1 and reported residual rho = || C y - lambda y ||_2, x the back-transformed vector.  With g = gamma(n):
      S = U^H U + E_s,  |E_s| <= gamma(n+1) |U^H| |U|                          (Thm 10.3, asserted by chol_ratio)
      C = U H U^H + E_c,  |E_c| <= (2 g + g^2) |U| |H| |U^H|                    (asserted by product_reduction_ratio)
    itype 2, H S x = lambda x, x the computed solution of U x = y:  (U + dU) x = y, |dU| <= g |U| (Thm 8.5, left_solve_ratio).
      H S x = H U^H U x + H E_s x,  H U^H = U^{-1} (C - E_c),  U x = y - dU x,  lambda x = U^{-1} lambda (y - dU x), so
      H S x - lambda x = U^{-1} [ (C y - lambda y) - (C - lambda) dU x - E_c U x ] + H E_s x
      and in norms
      <= ||U^{-1}|| rho + ||x|| { ||U^{-1}|| [ g || |U| || (||C|| + |lambda|) + (2 g + g^2) || |U||H||U^H| || ||U|| ]
                                  + ||H|| gamma(n+1) || |U^H||U| || }.
      The factor ||U^{-1}||_2 is real: the residual of the reduced problem is carried back through U^{-1}.
    itype 3, S H x = lambda x, x the computed product U^H y:  x = U^H y + e, |e| <= g |U^H| |y| (asserted by tri_product_ratio).
      S H x = U^H U H x + E_s H x,  U H x = U H U^H y + U H e = (C - E_c) y + U H e,  lambda x = lambda U^H y + lambda e, so
      S H x - lambda x = U^H (C y - lambda y) - U^H E_c y + U^H U H e - lambda e + E_s H x
      and in norms, with ||y|| = 1 and ||e|| <= g || |U| ||,
      <= ||U|| rho + ||U|| (2 g + g^2) || |U||H||U^H| || + g || |U| || (||U||^2 ||H|| + |lambda|) + gamma(n+1) || |U^H||U| || ||H|| ||x||."""
    assert itype in (2, 3)
    n = H.shape[0]
    cplx = np.iscomplexobj(H) or np.iscomplexobj(S)
    U = np.triu(np.asarray(U)[:n, :n])
    aU = np.abs(U)
    g = gamma(n, cplx)
    nU, naU, nC, nH = _two_norm(U), _two_norm(aU), _two_norm(C), _two_norm(H)
    t_c = (2 * g + g * g) * _two_norm(aU @ (np.abs(H) @ aU.T))
    t_s = gamma(n + 1, cplx) * _two_norm(aU.T @ aU) * nH
    nx = float(np.linalg.norm(x))
    if itype == 2:
        ninv = 1.0 / float(np.linalg.svd(U, compute_uv=False)[-1])
        return ninv * rho + nx * (ninv * (g * naU * (nC + abs(lam)) + t_c * nU) + t_s)
    return nU * rho + nU * t_c + g * naU * (nU * nU * nH + abs(lam)) + t_s * nx


def _s_inverse_times(S, X):
    """S^{-1} X to long double accuracy: LAPACK's Cholesky solve, refined twice with long double residuals against S itself"""
    cf = sla.cho_factor(np.asarray(S))
    cplx = np.iscomplexobj(S) or np.iscomplexobj(X)
    zr, zi = _pl(sla.cho_solve(cf, np.asarray(X)))
    xr, xi = _pl(X)
    s = _pl(S)
    for _ in range(2):
        sr, si = _mm(s, (zr, zi))
        rr, ri = (xr - sr).astype(np.float64), (xi - si).astype(np.float64)
        d = sla.cho_solve(cf, rr + 1j * ri if cplx else rr)
        dr, di = _pl(d)
        zr, zi = zr + dr, zi + di
    return zr, zi


def gev_value_bound_itype(itype, r_norm, x, S, n, norm_C):
    """| lambda - nearest eigenvalue of the pencil | for a pair with long double residual norm r_norm.  With S = L L^H exactly and
    C = L^H H L (the pencil's exact reduced matrix, any factor gives the same spectrum):
      itype 2, r = H S x - lambda x, y = L^H x:  L^H r = C y - lambda y, so the distance is <= ||L^H r|| / ||y|| <=
               sqrt(lambda_max(S)) ||r||_2 / ||x||_S;
      itype 3, r = S H x - lambda x, y = L^{-1} x:  L^{-1} r = C y - lambda y, so it is <= ||r||_2 / (sqrt(lambda_min(S)) ||x||_{S^{-1}}).
    ||x||_S, ||x||_{S^{-1}} (1 up to the asserted normalisation) are formed here.  Plus the error of scipy.linalg.eigh(H, S,
    type=itype) itself, MARGIN LAPACK_EIG_VALUE n eps ||C||_2, as gev_value_bound has it."""
    assert itype in (2, 3)
    w = sla.eigvalsh(np.asarray(S))
    x = np.asarray(x).reshape(-1, 1)
    xr, xi = _pl(x)
    if itype == 2:
        sr, si = _mm(_pl(S), (xr, xi))
        scale = math.sqrt(w[-1])
    else:
        sr, si = _s_inverse_times(S, x)
        scale = 1.0 / math.sqrt(w[0])
    nrm = math.sqrt(float(np.sum(xr * sr + xi * si)))
    return scale * r_norm / nrm + LAPACK_EIG_VALUE * MARGIN * n * EPS * norm_C


def orth_ratio_itype(itype, X, S, U):
    """max |X^H S X - I| (itype 1, 2) or max |X^H S^{-1} X - I| (itype 3) over K_EIG_ORTH n eps kappa_2(U), in long double"""
    n = S.shape[0]
    x = _pl(X)
    sx = _mm(_pl(S), x) if itype != 3 else _s_inverse_times(S, X)
    re, im = _mm(_ct(x), sx)
    err = np.hypot(re - np.eye(X.shape[1], dtype=LD), im)
    kappa = np.linalg.cond(np.triu(np.asarray(U)[:n, :n]))
    return float(np.max(err)) / (K_EIG_ORTH * n * EPS * kappa)


# ---- numpy models of the device's algorithms (capi_gev.hip, gev_kernels.hip) -------------------------------------------------
def model_trmm_left(U, Xp, n, op, unconjugated=False, diag_full=False, skip_last_long=False, ld_bug=False):
    """chase_hip_trmm_left_upper on the padded buffer Xp (ldx x ncols, Fortran order; rows >= n are padding).  U is used as it
    comes: whatever lies below its diagonal must not matter.  Returns the buffer.  Seeded defects: unconjugated - op C takes
    the plain transpose; diag_full - a 64-row diagonal block is used as a full square where its upper triangle belongs;
    skip_last_long - the long product of the last block the loop visits is left out; ld_bug - the tile of a 64-row step is
    written back with the extent n where the leading dimension belongs."""
    Xp = np.array(Xp, order="F", copy=True)
    ldx, ncols = Xp.shape
    U = np.asarray(U)[:n, :n]
    flat = Xp.reshape(-1, order="F")
    assert np.shares_memory(flat, Xp)
    ct = (lambda M: M.T) if unconjugated else (lambda M: M.conj().T)

    def diag(j0, nb):
        D = U[j0:j0 + nb, j0:j0 + nb]
        return D if diag_full else np.triu(D)

    def put(j0, P):
        ld = n if ld_bug else ldx
        for c in range(ncols):
            flat[j0 + c * ld: j0 + c * ld + P.shape[0]] = P[:, c]

    blocks = list(range(0, n, SOLVE_WB))
    if op == "N":
        for J0 in blocks:
            Jend = min(n, J0 + SOLVE_WB)
            for j0 in range(J0, Jend, NB):
                nb = min(NB, Jend - j0)
                put(j0, diag(j0, nb) @ Xp[j0:j0 + nb])
                if Jend - j0 - nb > 0:
                    Xp[j0:j0 + nb] += U[j0:j0 + nb, j0 + nb:Jend] @ Xp[j0 + nb:Jend]
            if Jend < n and not (skip_last_long and Jend + SOLVE_WB >= n):
                Xp[J0:Jend] += U[J0:Jend, Jend:n] @ Xp[Jend:n]
    else:
        for J0 in reversed(blocks):
            Jend = min(n, J0 + SOLVE_WB)
            for j0 in range(J0 + (Jend - J0 - 1) // NB * NB, J0 - 1, -NB):
                nb = min(NB, Jend - j0)
                put(j0, ct(diag(j0, nb)) @ Xp[j0:j0 + nb])
                if j0 > J0:
                    Xp[j0:j0 + nb] += ct(U[J0:j0, j0:j0 + nb]) @ Xp[J0:j0]
            if J0 > 0 and not (skip_last_long and J0 == SOLVE_WB):
                Xp[J0:Jend] += ct(U[:J0, J0:Jend]) @ Xp[:J0]
    return Xp


def model_hegst_product(A, U, wrong_mirror=False):
    """chase_hip_hegst_product_upper: the matrix completed from its UPPER triangle, W = U A, W <- W^H, W <- U W, the lower
    triangle of the result kept and mirrored, real diagonal.  Seeded defect: wrong_mirror - the completion takes the lower
    triangle, which the contract says is never read."""
    n = A.shape[0]
    F = herm_full(np.asarray(A).conj().T) if wrong_mirror else herm_full(A)
    W = model_trmm_left(U, F, n, "N")
    W = model_trmm_left(U, np.asfortranarray(W.conj().T), n, "N")
    return herm_full(W.conj().T)


def lapack_hegst_product(itype, A, U):
    """LAPACK's dsygst / zhegst (itype 2 or 3, upper) on the same inputs, mirrored"""
    f = sla.lapack.zhegst if np.iscomplexobj(A) or np.iscomplexobj(U) else sla.lapack.dsygst
    c, info = f(herm_full(A), np.triu(U), itype=itype, lower=0)
    assert info == 0
    return herm_full(c)


def model_pipeline_itype(itype, H, S, nev):
    """model reduce -> scipy.linalg.eigh as the solver (rho: its measured residual on the reduced matrix) -> model
    back-transformation.  Returns (U, C, lam, Y, rho, X)."""
    from gev_refs import model_potrf_blocked, model_trsm_left
    U = np.triu(model_potrf_blocked(S))
    Cm = model_hegst_product(H, U)
    w, Y = sla.eigh(Cm)
    lam, Y = w[:nev], np.asfortranarray(Y[:, :nev])
    rho = np.linalg.norm(Cm @ Y - Y * lam[None, :], axis=0)
    X = model_trsm_left(U, Y, H.shape[0], "N") if itype == 2 else model_trmm_left(U, Y, H.shape[0], "C")
    return U, Cm, lam, Y, rho, X
