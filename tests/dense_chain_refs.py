"""Inputs and checkers for the dense chain between the filter and the Ritz pairs (herk / herkx, potrf_upper, trsm_right_upper,
cholqr, houseqr, heevd / heevd_gpu, stedc, pseudo_rr_small): numpy / scipy only, no GPU, no chase_amd.  Imported by
tests/test_gpu_dense_chain.py, tests/dense_chain_worker.py and - the checkers are checked themselves -
tests/test_dense_chain_refs_cpu.py.

Every checker returns RATIOS, measured error / bound: a result passes when every ratio is <= 1, and a failing assertion shows how
far off it was.  Two kinds of bound:
* derived (Cholesky, right solve, Hermitian product): the componentwise backward-error bounds of Higham, Accuracy and
  Stability of Numerical Algorithms, 2nd ed. (Thm 10.3, Thm 8.5, eq. 3.13), with eps = 2^-52, gamma(k) = k eps / (1 - k eps)
  and the factor 2 sqrt(2) of section 3.6 for complex data (four-multiplication complex products: the context's phase is 0
  around these calls).  They hold for ANY summation order (MFMA, split-K) and are used with factor 1, no margin.  The
  residuals are formed in long double so that the check's own rounding is 2^-11 of the bound.
* measured (QR, eigensolvers): the constants are not derivable tightly; LAPACK (scipy.linalg.qr / eigh / eigh_tridiagonal)
  was measured on exactly the inputs the GPU tests use and the kernels get MARGIN = 8 times its largest ratio - the
  compact-WY products and the merge products sum in MFMA / split-K order, and an order of magnitude is what separates that
  from a dropped or doubled reflector.  The older normwise assertions of tests/test_gpu_kernels.py are part of the same
  checkers, so no result may be looser than what the suite asked before.

Not covered: under- and overflow scaling in house_gen_kernel.  LAPACK's xLARFG rescales columns of norm below about 1e-154;
ours does not, and no input here goes near that."""
import math
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "long double is not wider than double here: the residuals would be no better than the device's"
EPS = 2.0 ** -52
CANARY = 7.25
MARGIN = 8.0

# ---- measured on the CPU (scipy's LAPACK on x86-64; the seeds, shapes and input kinds of the GPU tests - QR_SHAPES,
# HEEVD_GPU_SIZES, HEEVD_HOST_SIZES, the children's 200 / 600 / 700, STEDC_SIZES below - real and complex): the largest ratio
# LAPACK itself reaches, normalised as the checkers normalise, rounded up to two digits.  The maxima sit at the smallest sizes
# (n eps is small there).  tests/test_dense_chain_refs_cpu.py measures again and fails if LAPACK exceeds what is written;
# tests/test_dist_qr_refs_cpu.py does the same for the QR constants on the shapes of the distributed QR (dist_qr_refs.SHAPES).
LAPACK_QR_ORTH = 2.0           # max |Q^H Q - I| / (n eps)                        scipy.linalg.qr(mode="economic"); (1, 1) complex
LAPACK_QR_SPAN = 1.6           # ||V - Q Q^H V||_F / (||V||_F n eps)              1.57 at (1, 1) complex
LAPACK_QR_TRIL = 0.12          # ||tril(Q^H V, -1)||_F / (||V||_F n eps)          0.118 at (9, 4) complex, zero column - a shape of
#                                tests/dist_qr_refs.py (raised from 0.045 = 0.0445 at (33, 32) complex, duplicate column, the largest over QR_SHAPES)
LAPACK_QR_G = 2.0              # G = Q_scipy^H Q_numpy: off-diagonal 0.0058, | |G_jj| - 1 | 2.0, over kappa_2(V) n eps
LAPACK_EIG_RESID = 1.2         # max_j ||A z_j - w_j z_j||_2 / (n eps ||A||_2)    scipy.linalg.eigh(driver="evd"); 1.17 at n = 3 complex
LAPACK_EIG_ORTH = 1.6          # max |Z^H Z - I| / (n eps)                        1.50 at n = 2 complex
LAPACK_EIG_VALUE = 0.36        # max |w - eigvalsh(A)| / (n eps ||A||_2)          evd against eigvalsh's evr, n = 33 real tridiagonal
LAPACK_MRRR_ORTH = 12.3        # the same with LAPACK's MRRR (dstemr on dsytrd / zhetrd of the inputs at n = 3, 65, 257): 12.2 at n = 257
LAPACK_TRI_RESID = 0.5         # the same three for the tridiagonal solver, normalised by n eps max(|d|, |e|) as the older test of
LAPACK_TRI_ORTH = 0.5          #   chase_hip_stedc has it: scipy.linalg.eigh_tridiagonal(lapack_driver="stev"), values against
LAPACK_TRI_VALUE = 0.5         #   its "stebz" driver; all three 0.5 at n = 2
K_QR_ORTH, K_QR_SPAN, K_QR_TRIL = MARGIN * LAPACK_QR_ORTH, MARGIN * LAPACK_QR_SPAN, MARGIN * LAPACK_QR_TRIL
K_QR_G = MARGIN * 1.0                    # against LAPACK's Q: 8 kappa_2(V) n eps as it stands (two LAPACK front ends among themselves: LAPACK_QR_G)
K_EIG_RESID, K_EIG_ORTH, K_EIG_VALUE = MARGIN * LAPACK_EIG_RESID, MARGIN * LAPACK_EIG_ORTH, MARGIN * LAPACK_EIG_VALUE
# CHASE_HIP_TRIDIAG_MRRR=1 (host dstemr): MRRR promises |z_i^T z_j| = O(n eps) only and LAPACK's own dstemr loses that much on
# these inputs - ||Z^T Z - I||_F / sqrt(n) = 390 eps at n = 257, where divide & conquer stays at 17 eps.  The device path with
# the switch set reproduces LAPACK's figures (385 eps; max entry 11.9 n eps against 12.2): the cause is the algorithm, not a
# kernel.  That route is therefore held to 8 x LAPACK's MRRR, and the older 50 eps of test_heevd_matches_scipy, which was
# written for divide & conquer and never ran MRRR, is not applied to it.
K_MRRR_ORTH = MARGIN * LAPACK_MRRR_ORTH
K_TRI_RESID, K_TRI_ORTH, K_TRI_VALUE = (min(MARGIN * LAPACK_TRI_RESID, 10.0), min(MARGIN * LAPACK_TRI_ORTH, 10.0),
                                        min(MARGIN * LAPACK_TRI_VALUE, 10.0))       # never above the older test's 10 n eps


def gamma(k, cplx=False):
    g = k * EPS / (1.0 - k * EPS)
    return g * 2.0 * math.sqrt(2.0) if cplx else g


def dt_of(cplx):
    return np.complex128 if cplx else np.float64


def rnd(rng, shape, cplx):
    a = rng.standard_normal(shape)
    if cplx:
        a = a + 1j * rng.standard_normal(shape)
    return np.asfortranarray(a.astype(dt_of(cplx)))


def _unitary(rng, n, cplx):
    q, r = np.linalg.qr(rnd(rng, (n, n), cplx))
    return q


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def hpd(rng, n, cplx, kappa):
    """Hermitian positive definite, Q diag(geomspace(1, 1 / kappa)) Q^H, symmetrised (real diagonal)"""
    if n == 0:
        return np.zeros((0, 0), dtype=dt_of(cplx), order="F")
    q = _unitary(rng, n, cplx)
    a = (q * np.geomspace(1.0, 1.0 / kappa, n)[None, :]) @ q.conj().T
    return np.asfortranarray((a + a.conj().T) / 2)


def padded(a, ld, canary=CANARY):
    """a in the first rows of an ld x cols Fortran array whose extra rows hold the canary (a finite odd value, or NaN)"""
    a = np.asarray(a)
    out = np.full((ld, a.shape[1]), canary, dtype=a.dtype, order="F")
    out[:a.shape[0]] = a
    return out


def same_padding(out, rows, canary=CANARY):
    """the rows below `rows` still hold the canary, bit for bit (NaN included)"""
    pad = np.ascontiguousarray(out[rows:])
    want = np.full(pad.shape, canary, dtype=pad.dtype)
    return pad.tobytes() == want.tobytes()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def herm_cases(rng, n, cplx, only_random=False):
    """the eigensolver's inputs: name -> Hermitian n x n (only_random: the first one alone, the same matrix)"""
    x = rnd(rng, (n, n), cplx)
    out = {"random": np.asfortranarray(x + x.conj().T)}
    if only_random:
        return out
    lam = np.repeat(np.arange(1.0, n // 2 + 2), 2)[:n]              # every eigenvalue twice ...
    q = _unitary(rng, n, cplx)
    a = (q * lam[None, :]) @ q.conj().T
    if n > 1:
        a[:, 0] = 0; a[0, :] = 0
    a[0, 0] = 7.5                                                   # ... and a decoupled first row / column: tau = 0
    out["double_decoupled"] = (a + a.conj().T) / 2
    e = rnd(rng, (max(n - 1, 0),), cplx)
    out["tridiagonal"] = np.diag(rng.standard_normal(n)).astype(dt_of(cplx)) + np.diag(e, -1) + np.diag(e.conj(), 1)
    out["diagonal"] = np.diag(rng.standard_normal(n)).astype(dt_of(cplx))
    out["scaled_identity"] = (-2.5 * np.eye(n)).astype(dt_of(cplx))
    return {k: np.asfortranarray(v.astype(dt_of(cplx))) for k, v in out.items()}


def qr_cases(rng, m, n, cplx):
    """the QR inputs: name -> m x n.  Only "random" is well conditioned (kappa_2 <= 1e3 is asserted where it matters)."""
    v = rnd(rng, (m, n), cplx)
    out = {"random": v}
    z = v.copy(); z[:, n // 2] = 0
    out["zero_column"] = z
    if n > 1:
        d = v.copy(); d[:, n // 2] = d[:, 0]
        out["duplicate_column"] = d
    t = np.zeros((m, n), dtype=dt_of(cplx), order="F")
    t[:n] = np.triu(rng.standard_normal((n, n)))                    # zero tails, real pivots: tau = 0, H = I
    out["upper_triangular"] = t
    if cplx:
        t2 = np.zeros((m, n), dtype=np.complex128, order="F")
        t2[:n] = np.triu(rnd(rng, (n, n), True))                    # zero tail under a complex pivot: xn2 == 0 && ai != 0
        out["upper_triangular_complex_diagonal"] = t2
    return out


def tridiag_cases(n, rng):
    m = (n - 1) // 2
    dg = np.concatenate([np.abs(np.arange(21) - 10.0)] * (n // 21))
    eg = np.ones(len(dg) - 1); eg[20::21] = 1e-8
    ez = rng.standard_normal(n - 1); ez[::7] = 0.0
    k = np.arange(1, n)
    return {
        "random": (rng.standard_normal(n), rng.standard_normal(n - 1)),
        "toeplitz_1_2_1": (2.0 * np.ones(n), np.ones(n - 1)),
        "wilkinson": (np.abs(np.arange(n) - m).astype(float), np.ones(n - 1)),
        "glued_wilkinson": (dg, eg),
        "clustered": (np.ones(n), 1e-9 * rng.standard_normal(n - 1)),
        "graded": (10.0 ** (-np.arange(n) * 12.0 / n), 10.0 ** (-np.arange(1, n) * 12.0 / n)),
        "zero_couplings": (rng.standard_normal(n), ez),
        "clement": (np.zeros(n), np.sqrt(k * (n - k)) * 1e3),
        "zero_matrix": (np.zeros(n), np.zeros(n - 1)),
        "negative_couplings": (rng.standard_normal(n), -np.abs(rng.standard_normal(n - 1))),
    }


def small_tridiag_cases(n, rng):
    """tridiag_cases for every n >= 1: below 21 rows glued_wilkinson (21 rows per glued block) does not exist and is left out"""
    if n >= 21:
        return tridiag_cases(n, rng)
    m = (n - 1) // 2
    ez = rng.standard_normal(n - 1); ez[::7] = 0.0
    k = np.arange(1, n)
    return {
        "random": (rng.standard_normal(n), rng.standard_normal(n - 1)),
        "toeplitz_1_2_1": (2.0 * np.ones(n), np.ones(n - 1)),
        "wilkinson": (np.abs(np.arange(n) - m).astype(float), np.ones(n - 1)),
        "clustered": (np.ones(n), 1e-9 * rng.standard_normal(n - 1)),
        "graded": (10.0 ** (-np.arange(n) * 12.0 / n), 10.0 ** (-np.arange(1, n) * 12.0 / n)),
        "zero_couplings": (rng.standard_normal(n), ez),
        "clement": (np.zeros(n), np.sqrt(k * (n - k)) * 1e3),
        "zero_matrix": (np.zeros(n), np.zeros(n - 1)),
        "negative_couplings": (rng.standard_normal(n), -np.abs(rng.standard_normal(n - 1))),
    }


# ---- long double products ------------------------------------------------------------------------------------------------------
def _planes(a):
    a = np.asarray(a)
    return (a.real.astype(LD), a.imag.astype(LD)) if np.iscomplexobj(a) else (a.astype(LD), None)


def ld_matmul(a, b, conj_a=False):
    """op(a) b in long double, complex data as two real planes; returns (re, im) with im None for real data.
    conj_a: op(a) = a^H (a^T for real data)"""
    ar, ai = _planes(a)
    br, bi = _planes(b)
    if conj_a:
        ar = ar.T
        ai = None if ai is None else -ai.T
    if ai is None and bi is None:
        return ar @ br, None
    z = lambda p, like: np.zeros(like.shape, dtype=LD) if p is None else p
    ai, bi = z(ai, ar), z(bi, br)
    return ar @ br - ai @ bi, ar @ bi + ai @ br


def _absdiff(re, im, ref):
    rr, ri = _planes(ref)
    dr = re - rr
    if im is None and ri is None:
        return np.abs(dr)
    di = (0 if im is None else im) - (0 if ri is None else ri)
    return np.hypot(dr, di)


def _max_ratio(err, bound, mask=None):
    """max err / bound over the mask; a zero bound demands a zero error; anything non-finite is infinitely wrong"""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    if mask is not None:
        err, bound = err[mask], bound[mask]
    if err.size == 0:
        return 0.0
    if not np.all(np.isfinite(err)):
        return math.inf
    safe = np.where(bound > 0, bound, 1)
    r = np.where(err == 0, 0, np.where(bound > 0, err / safe, np.inf))
    return float(np.max(r))


# ---- derived bounds: factor 1 -------------------------------------------------------------------------------------------------
def chol_ratio(A, R):
    """max_ij |R^H R - A|_ij / (gamma(n+1) (|R|^H |R|)_ij) on the upper triangle, R taken as triu (Higham Thm 10.3)"""
    n = A.shape[0]
    if n == 0:
        return 0.0
    cplx = np.iscomplexobj(A)
    R = np.triu(np.asarray(R)[:n, :n])
    if not np.all(np.isfinite(R)):
        return math.inf
    re, im = ld_matmul(R, R, conj_a=True)
    err = _absdiff(re, im, A)
    aR = np.abs(R).astype(LD)
    return _max_ratio(err, gamma(n + 1, cplx) * (aR.T @ aR), np.triu(np.ones((n, n), dtype=bool)))


def solve_ratio(X, R, V):
    """max |X R - V|_ij / (gamma(n) (|X| |R|)_ij), R taken as triu (Higham Thm 8.5, by rows)"""
    n = R.shape[1]
    cplx = np.iscomplexobj(V) or np.iscomplexobj(R)
    R = np.triu(np.asarray(R)[:n, :n])
    if not np.all(np.isfinite(X)):
        return math.inf
    re, im = ld_matmul(X, R)
    err = _absdiff(re, im, V)
    return _max_ratio(err, gamma(n, cplx) * (np.abs(X).astype(LD) @ np.abs(R).astype(LD)))


def product_reference(A, B):
    """(A^H B in long double planes, the bound gamma(k) |A|^T |B|): formed once where several results share the operands"""
    cplx = np.iscomplexobj(A) or np.iscomplexobj(B)
    re, im = ld_matmul(A, B, conj_a=True)
    return re, im, gamma(A.shape[0], cplx) * (np.abs(A).astype(LD).T @ np.abs(B).astype(LD))


def product_ratio(C, A, B, mask=None, ref=None):
    """max |C - A^H B|_ij / (gamma(k) (|A|^T |B|)_ij) on the mask (Higham eq. 3.13); k = 0 demands C = 0 exactly"""
    if not np.all(np.isfinite(np.asarray(C)[mask] if mask is not None else C)):
        return math.inf
    re, im, bound = ref if ref is not None else product_reference(A, B)
    return _max_ratio(_absdiff(re, im, C), bound, mask)


def upper_mask(n):
    return np.triu(np.ones((n, n), dtype=bool))


# ---- the numpy model of the device's blocked algorithms (explicit inverses of the 64-wide diagonal blocks) ---------------------
NB = 64


def _inv_upper(r):
    import scipy.linalg as sla
    return sla.solve_triangular(r, np.eye(r.shape[0], dtype=r.dtype), lower=False)


def model_potrf(A, skip_last_update=False):
    """chase_hip_potrf_upper: per 64-block potf2 + inverse, row panel R_jr = T^H A_jr, full trailing update.  Returns the
    n x n array as the device leaves it (upper triangle R; the lower triangle is whatever the trailing updates made of it).
    skip_last_update: seeded defect - the trailing update in front of the last (ragged) block is left out."""
    A = np.array(A, order="F", copy=True)
    n = A.shape[0]
    for j0 in range(0, n, NB):
        nb = min(NB, n - j0)
        jj = slice(j0, j0 + nb)
        Rjj = np.linalg.cholesky(np.triu(A[jj, jj]) + np.triu(A[jj, jj], 1).conj().T).conj().T
        A[jj, jj] = np.triu(Rjj) + np.tril(A[jj, jj], -1)
        rest = n - j0 - nb
        if rest > 0:
            T = _inv_upper(Rjj)
            rr = slice(j0 + nb, n)
            A[jj, rr] = T.conj().T @ A[jj, rr]
            if skip_last_update and rest <= NB:
                continue
            A[rr, rr] -= A[jj, rr].conj().T @ A[jj, rr]
    return A


def model_trsm(R, Vp, m, wb=NB, zero_inv_col=None, skip_last_update=False, ld_bug=False):
    """chase_hip_trsm_right_upper on the padded buffer Vp (ldv x n, Fortran order; rows >= m are padding): left-looking over
    blocks of wb columns, 64-column steps with rank-64 updates inside a block, X_j = V_j T_j through a panel buffer that is
    copied back with the leading dimension ldv.  Returns the buffer.  Seeded defects: zero_inv_col = (block, column) zeroes
    one column of one inverse; skip_last_update leaves the last block's long update out; ld_bug copies the panel back with
    the extent m where the leading dimension belongs."""
    Vp = np.array(Vp, order="F", copy=True)
    ldv, n = Vp.shape
    R = np.triu(np.asarray(R)[:n, :n])
    flat = Vp.reshape(-1, order="F")                      # a view: Vp is Fortran-contiguous
    assert np.shares_memory(flat, Vp)
    for J0 in range(0, n, wb):
        w = min(wb, n - J0)
        Jend = J0 + w
        if J0 > 0 and not (skip_last_update and Jend == n):
            Vp[:m, J0:Jend] -= Vp[:m, :J0] @ R[:J0, J0:Jend]
        for j0 in range(J0, Jend, NB):
            nb = min(NB, Jend - j0)
            T = _inv_upper(R[j0:j0 + nb, j0:j0 + nb])
            if zero_inv_col is not None and zero_inv_col[0] == j0 // NB:
                T[:, zero_inv_col[1]] = 0
            P = Vp[:m, j0:j0 + nb] @ T
            ld = m if ld_bug else ldv
            for c in range(nb):                           # copy2d(P, m -> V_j, ld)
                flat[j0 * ldv + c * ld: j0 * ldv + c * ld + m] = P[:, c]
            rest = Jend - j0 - nb
            if rest > 0:
                Vp[:m, j0 + nb:Jend] -= P @ R[j0:j0 + nb, j0 + nb:Jend]
    return Vp


# ---- measured bounds: QR -----------------------------------------------------------------------------------------------------
def qr_raw(V, Q):
    """(max |Q^H Q - I|, ||V - Q Q^H V||_F / ||V||_F, ||tril(Q^H V, -1)||_F / ||V||_F), each divided by n eps"""
    n = V.shape[1]
    G = Q.conj().T @ Q - np.eye(n)
    R = Q.conj().T @ V
    nv = np.linalg.norm(V)
    nv = nv if nv > 0 else 1.0
    ne = n * EPS
    return np.max(np.abs(G)) / ne, np.linalg.norm(V - Q @ R) / nv / ne, np.linalg.norm(np.tril(R, -1)) / nv / ne


def qr_ratios(V, Q):
    """orthogonality, span and triangularity of Q against V, each divided by its bound: K n eps (8 x LAPACK, above) and the older
    normwise thresholds of test_houseqr_orthogonality_and_span (25 eps, 1e-12, 1e-11), whichever is tighter."""
    n = V.shape[1]
    if not np.all(np.isfinite(Q)):
        return {"finite": math.inf}
    ne = n * EPS
    orth, span, tril = qr_raw(V, Q)
    orth_old = np.linalg.norm(Q.conj().T @ Q - np.eye(n)) / math.sqrt(n)
    return {"orth": orth / K_QR_ORTH,
            "orth_old": orth_old / (25 * EPS),
            "span": span / min(K_QR_SPAN, 1e-12 / ne),
            "tril": tril / min(K_QR_TRIL, 1e-11 / ne)}


def qr_g_raw(V, Q, Qref):
    """G = Qref^H Q: (largest off-diagonal modulus, largest | |G_jj| - 1 |), each divided by kappa_2(V) n eps"""
    n = V.shape[1]
    kappa = np.linalg.cond(V)
    assert kappa <= 1e3, kappa
    G = Qref.conj().T @ Q
    dg = np.diag(G)
    s = kappa * n * EPS
    return np.max(np.abs(G - np.diag(dg))) / s, np.max(np.abs(np.abs(dg) - 1)) / s


def qr_vs_lapack_ratios(V, Q):
    """G = Q_lapack^H Q must be diagonal with unit-modulus entries: the NESTED column spaces agree (span-only checks do not see
    two columns mixed inside the span).  Well-conditioned V only (kappa_2 <= 1e3); bound 8 kappa_2(V) n eps."""
    import scipy.linalg as sla
    if not np.all(np.isfinite(Q)):
        return {"finite": math.inf}
    off, dg = qr_g_raw(V, Q, sla.qr(V, mode="economic")[0])
    return {"g_off": off / K_QR_G, "g_diag": dg / K_QR_G}


# ---- measured bounds: eigensolvers -------------------------------------------------------------------------------------------
def eig_raw(A, w, Z, wref):
    """(max_j ||A z_j - w_j z_j||_2 / ||A||_2, max |Z^H Z - I|, max |w - wref| / ||A||_2), each divided by n eps"""
    n = A.shape[0]
    na = max(np.max(np.abs(wref)), 1e-300)
    ne = n * EPS
    Rm = A @ Z - Z * w[None, :]
    G = Z.conj().T @ Z - np.eye(n)
    return np.max(np.linalg.norm(Rm, axis=0)) / na / ne, np.max(np.abs(G)) / ne, np.max(np.abs(w - wref)) / na / ne


def eig_ratios(A, w, Z, mrrr=False):
    """residual per pair, orthogonality and eigenvalues against LAPACK, each divided by K n eps (||A||_2) (8 x LAPACK, above), plus
    the older normwise assertions of test_heevd_matches_scipy (100 eps max|w|, 1e-12 ||A||_F, 50 eps).  mrrr: the result comes
    from the MRRR route - orthogonality against 8 x LAPACK's MRRR instead (see K_MRRR_ORTH)."""
    import scipy.linalg as sla
    n = A.shape[0]
    if not (np.all(np.isfinite(Z)) and np.all(np.isfinite(w))):
        return {"finite": math.inf}
    wref = sla.eigvalsh(A)
    resid, orth, value = eig_raw(A, w, Z, wref)
    Rm = A @ Z - Z * w[None, :]
    G = Z.conj().T @ Z - np.eye(n)
    out = {"ascending": 0.0 if np.all(np.diff(w) >= 0) else math.inf,
           "resid": resid / K_EIG_RESID, "orth": orth / (K_MRRR_ORTH if mrrr else K_EIG_ORTH), "value": value / K_EIG_VALUE,
           "resid_old": np.linalg.norm(Rm) / (1e-12 * max(np.linalg.norm(A), 1e-300)),
           "orth_old": np.linalg.norm(G) / math.sqrt(n) / (50 * EPS),
           "value_old": np.max(np.abs(w - wref)) / (100 * EPS * max(np.max(np.abs(w)), 1e-300))}
    if mrrr:
        del out["orth_old"]
    return out


def tridiag_raw(d, e, w, Z, wref):
    """the same three for a tridiagonal matrix, normalised by n eps max(|d|, |e|) like the older test of chase_hip_stedc"""
    n = len(d)
    T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
    nrm = max(np.max(np.abs(d)), np.max(np.abs(e)) if n > 1 else 0.0, 1e-300)
    s = n * EPS * nrm
    return (np.max(np.abs(T @ Z - Z * w[None, :])) / s, np.max(np.abs(Z.T @ Z - np.eye(n))) / (n * EPS),
            np.max(np.abs(w - wref)) / s)


def tridiag_reference(d, e):
    import scipy.linalg as sla
    if len(d) == 1:
        return np.array(d, dtype=float), np.ones((1, 1))
    return sla.eigh_tridiagonal(np.asarray(d, dtype=float), np.asarray(e, dtype=float), lapack_driver="stev")    # (stemr does not converge on every case here)


def tridiag_ratios(d, e, w, Z):
    if not (np.all(np.isfinite(Z)) and np.all(np.isfinite(w))):
        return {"finite": math.inf}
    resid, orth, value = tridiag_raw(d, e, w, Z, tridiag_reference(d, e)[0])
    return {"ascending": 0.0 if np.all(np.diff(w) >= 0) else math.inf,
            "resid": resid / K_TRI_RESID, "orth": orth / K_TRI_ORTH, "value": value / K_TRI_VALUE}


def worst(ratios):
    """(largest ratio, its name) of a checker's dict"""
    k = max(ratios, key=lambda x: ratios[x])
    return float(ratios[k]), k


# ---- the shapes the GPU tests run (shared with the CPU self-test, which measures LAPACK on exactly these) ---------------------
POTRF_SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 200]
QR_SHAPES = [(1, 1), (2, 1), (33, 32), (65, 33), (129, 64), (130, 130)]
HEEVD_GPU_SIZES = [3, 33, 34, 64, 65, 130, 257, 513]
HEEVD_HOST_SIZES = [1, 2, 150]
STEDC_SIZES = [1, 2, 128, 129, 257, 513]


def seed_of(*key):
    """one reproducible seed per case, the same in every process"""
    s = 12345
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return s
