"""The checkers of tests/dense_chain_refs.py are checked themselves, without a GPU.  Two kinds of test per checker:
* pass: LAPACK's result - and the numpy model of our blocked, inverse-based algorithms where there is one - stays inside every
  bound on the inputs the GPU tests use; the measured LAPACK constants are measured again here;
* seeded defects: a result that carries ONE defect fails.  Two of the defects pass the older normwise tolerances of
  tests/test_gpu_kernels.py (test_a_wrong_entry_... and test_swapped_eigenvectors_... say which and show it): the evidence that
  the new bounds are tighter."""
import numpy as np
import pytest
import scipy.linalg as sla
import dense_chain_refs as D

EPS = D.EPS


def _chol(A):
    return np.linalg.cholesky(A).conj().T


# ---- derived bounds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("kappa", [10.0, 1e10])
def test_cholesky_bound_holds_for_lapack_and_for_the_blocked_model(cplx, kappa):
    worst = 0.0
    for n in D.POTRF_SIZES + [333]:
        A = D.hpd(np.random.default_rng(D.seed_of(1, n, cplx)), n, cplx, kappa)
        for R in (_chol(A), D.model_potrf(A)):
            worst = max(worst, D.chol_ratio(A, R))
    assert worst <= 0.5, worst                   # the bound is used as it stands: the references sit well inside it


@pytest.mark.parametrize("cplx", [False, True])
def test_solve_bound_holds_for_lapack_and_for_the_blocked_model(cplx):
    worst = 0.0
    for n in D.POTRF_SIZES + [333]:
        for m in (1, 150):
            rng = np.random.default_rng(D.seed_of(2, m, n, cplx))
            R = _chol(D.hpd(rng, n, cplx, 1e5))
            V = D.rnd(rng, (m, n), cplx)
            Xl = sla.solve_triangular(R, V.conj().T, trans="C", lower=False).conj().T         # X R = V
            worst = max(worst, D.solve_ratio(Xl, R, V))
            for wb in (64, 128):
                Vp = D.model_trsm(R, D.padded(V, m + 3), m, wb=wb)
                assert D.same_padding(Vp, m)
                worst = max(worst, D.solve_ratio(Vp[:m], R, V))
    assert worst <= 0.5, worst


@pytest.mark.parametrize("cplx", [False, True])
def test_product_bound_holds_for_numpy_and_demands_exact_zero_for_k_0(cplx):
    rng = np.random.default_rng(7)
    for n, k in ((1, 1), (129, 1), (129, 0), (200, 333)):
        A, B = D.rnd(rng, (k, n), cplx), D.rnd(rng, (k, n), cplx)
        C = A.conj().T @ B
        assert D.product_ratio(C, A, B) <= 0.5
        assert D.product_ratio(C, A, B, D.upper_mask(n)) <= 0.5
        C[n // 2, n - 1] += 1e-10 * (1 + abs(C[n // 2, n - 1]))
        assert D.product_ratio(C, A, B, D.upper_mask(n)) > 1
        assert D.product_ratio(C, A, B, ~D.upper_mask(n)) <= 0.5          # ... and only where the mask looks


def test_a_wrong_entry_of_R_fails_the_cholesky_bound_and_passes_the_older_tolerance():
    """One entry of R off by 1e-10 relative.  On a well-conditioned matrix both the new bound and test_potrf_and_trsm's
    50 eps ||A||_F see it.  On a GRADED matrix (A = S B S, S = diag(1 .. 1e-5)) the same defect in the last column changes
    A[n-1, n-1] by ~1e-20: it PASSES the older normwise tolerance (50 eps ||A||_F ~ 1e-13) and fails the componentwise bound by
    orders of magnitude."""
    n = 65
    rng = np.random.default_rng(11)
    A = D.hpd(rng, n, False, 10.0)
    R = _chol(A)
    R[3, 40] *= 1 + 1e-10
    assert D.chol_ratio(A, R) > 1
    S = np.geomspace(1.0, 1e-5, n)
    G = np.asfortranarray(S[:, None] * A * S[None, :])
    Rg = _chol(G)
    assert D.chol_ratio(G, Rg) <= 0.5 and D.chol_ratio(G, D.model_potrf(G)) <= 0.5
    Rg[10, n - 1] *= 1 + 1e-10
    assert np.linalg.norm(Rg.conj().T @ Rg - G) <= 50 * EPS * np.linalg.norm(G)           # the older assertion: passes
    assert D.chol_ratio(G, Rg) > 10                                                        # the new one: fails


@pytest.mark.parametrize("cplx", [False, True])
def test_seeded_defects_of_the_blocked_factorisation_and_solve_fail(cplx):
    n, m = 129, 150
    rng = np.random.default_rng(D.seed_of(3, n, cplx))
    A = D.hpd(rng, n, cplx, 1e5)
    assert D.chol_ratio(A, D.model_potrf(A)) <= 0.5
    assert D.chol_ratio(A, D.model_potrf(A, skip_last_update=True)) > 1           # the last ragged block's update skipped
    R = _chol(A)
    V = D.rnd(rng, (m, n), cplx)
    Vp = D.padded(V, m + 3)
    for wb in (64, 128):
        good = D.model_trsm(R, Vp, m, wb=wb)
        assert D.solve_ratio(good[:m], R, V) <= 0.5 and D.same_padding(good, m)
        bad = D.model_trsm(R, Vp, m, wb=wb, zero_inv_col=(1, 5))                     # one column of one 64-block inverse zeroed
        assert D.solve_ratio(bad[:m], R, V) > 1
        bad = D.model_trsm(R, Vp, m, wb=wb, skip_last_update=True)
        assert D.solve_ratio(bad[:m], R, V) > 1
        bad = D.model_trsm(R, Vp, m, wb=wb, ld_bug=True)                              # the extent where the leading dimension belongs
        assert D.solve_ratio(bad[:m], R, V) > 1 and not D.same_padding(bad, m)
        same = D.model_trsm(R, V, m, wb=wb, ld_bug=True)                              # ld == extent: the defect is invisible,
        assert D.same_bits(same, good[:m])                                           # which is why the GPU tests pad


def test_padding_checker_sees_one_element_and_handles_nan():
    a = np.arange(12.0).reshape(4, 3)
    for canary in (D.CANARY, np.nan):
        p = D.padded(a, 7, canary)
        assert p.flags.f_contiguous and np.array_equal(p[:4], a) and D.same_padding(p, 4, canary)
        p[6, 1] = 7.25000000000001
        assert not D.same_padding(p, 4, canary)
    z = D.padded(a.astype(complex), 5)
    z[4, 2] = 7.25 + 1e-300j
    assert not D.same_padding(z, 4)
    assert D.same_bits(np.array([np.nan, 0.0]), np.array([np.nan, 0.0])) and not D.same_bits(np.array([0.0]), np.array([-0.0]))


# ---- measured bounds -------------------------------------------------------------------------------------------------------
def test_the_margin_constants_are_eight_times_what_lapack_was_measured_at():
    assert D.MARGIN == 8.0
    assert (D.K_QR_ORTH, D.K_QR_SPAN, D.K_QR_TRIL) == (8 * D.LAPACK_QR_ORTH, 8 * D.LAPACK_QR_SPAN, 8 * D.LAPACK_QR_TRIL)
    assert D.K_QR_G == 8.0 and D.LAPACK_QR_G <= 8.0
    assert (D.K_EIG_RESID, D.K_EIG_ORTH, D.K_EIG_VALUE) == (8 * D.LAPACK_EIG_RESID, 8 * D.LAPACK_EIG_ORTH, 8 * D.LAPACK_EIG_VALUE)
    assert (D.K_TRI_RESID, D.K_TRI_ORTH, D.K_TRI_VALUE) == (4.0, 4.0, 4.0) and 8 * D.LAPACK_TRI_RESID <= 10.0


def _qr_inputs():
    for m, n in D.QR_SHAPES:
        for cplx in (False, True):
            for name, V in D.qr_cases(np.random.default_rng(D.seed_of(3, m, n, cplx)), m, n, cplx).items():
                yield (m, n, cplx, name), V


def test_lapack_qr_stays_inside_the_measured_constants_and_passes_the_checkers():
    mx = np.zeros(4)
    for tag, V in _qr_inputs():
        Q = sla.qr(V, mode="economic")[0]
        g = (0.0, 0.0)
        if tag[3] == "random" and np.linalg.cond(V) <= 1e3:
            g = D.qr_g_raw(V, np.linalg.qr(V)[0], Q)
            assert D.worst(D.qr_vs_lapack_ratios(V, np.linalg.qr(V)[0]))[0] <= 1, tag
        mx = np.maximum(mx, list(D.qr_raw(V, Q)) + [max(g)])
        assert D.worst(D.qr_ratios(V, Q))[0] <= 1, (tag, D.qr_ratios(V, Q))
    assert np.all(mx <= [D.LAPACK_QR_ORTH, D.LAPACK_QR_SPAN, D.LAPACK_QR_TRIL, D.LAPACK_QR_G]), mx


def _q_from_reflectors(V, drop=None):
    """Q = H_0 ... H_{n-1} I(:, :n) from LAPACK's geqrf, optionally with one reflector left out"""
    (h, tau), _ = sla.qr(V, mode="raw")
    m, n = V.shape
    Q = np.eye(m, n, dtype=V.dtype)
    for j in reversed(range(n)):
        if j == drop:
            continue
        v = np.zeros(m, dtype=V.dtype); v[j] = 1; v[j + 1:] = h[j + 1:, j]
        Q -= tau[j] * np.outer(v, v.conj() @ Q)
    return Q


@pytest.mark.parametrize("cplx", [False, True])
def test_a_dropped_reflector_and_two_mixed_columns_fail_the_qr_checkers(cplx):
    m, n = 129, 64
    V = D.qr_cases(np.random.default_rng(D.seed_of(3, m, n, cplx)), m, n, cplx)["random"]
    Q = _q_from_reflectors(V)
    assert D.worst(D.qr_ratios(V, Q))[0] <= 1 and D.worst(D.qr_vs_lapack_ratios(V, Q))[0] <= 1
    for drop in (0, 31, 63):
        Qd = _q_from_reflectors(V, drop)
        r = D.qr_ratios(V, Qd)
        assert r["orth"] <= 1 and r["span"] > 1e3, (drop, r)             # still orthonormal: only the span / triangle see it
    c, s = np.cos(1e-9), np.sin(1e-9)                                     # two columns rotated INSIDE the span by 1e-9
    Qm = Q.copy()
    Qm[:, 5], Qm[:, 6] = c * Q[:, 5] - s * Q[:, 6], s * Q[:, 5] + c * Q[:, 6]
    r = D.qr_ratios(V, Qm)
    assert r["orth"] <= 1 and r["span"] <= 1                              # span-only checks are blind to it ...
    assert D.qr_vs_lapack_ratios(V, Qm)["g_off"] > 1                      # ... the comparison with LAPACK's Q is not
    Qn = Q.copy(); Qn[7, 7] = np.nan
    assert D.worst(D.qr_ratios(V, Qn))[0] == np.inf


def _eig_inputs(sizes, kinds=None):
    for n in sizes:
        for cplx in (False, True):
            for name, A in D.herm_cases(np.random.default_rng(D.seed_of(4, n, cplx)), n, cplx, kinds == ["random"]).items():
                yield (n, cplx, name), A


def test_lapack_heevd_stays_inside_the_measured_constants_and_passes_the_checker():
    mx = np.zeros(3)
    import itertools
    # every kind at the in-process sizes; the children's larger sizes (200, 600, 700) run the random kind only
    for tag, A in itertools.chain(_eig_inputs(D.HEEVD_GPU_SIZES + D.HEEVD_HOST_SIZES), _eig_inputs([200, 600, 700], ["random"])):
        assert np.array_equal(A, A.conj().T), tag
        w, Z = sla.eigh(A, driver="evd")
        mx = np.maximum(mx, D.eig_raw(A, w, Z, sla.eigvalsh(A)))
        assert D.worst(D.eig_ratios(A, w, Z))[0] <= 1, (tag, D.eig_ratios(A, w, Z))
    assert np.all(mx <= [D.LAPACK_EIG_RESID, D.LAPACK_EIG_ORTH, D.LAPACK_EIG_VALUE]), mx


def test_lapack_mrrr_loses_the_orthogonality_its_constant_says():
    """the cause written next to K_MRRR_ORTH, shown: LAPACK's dstemr on LAPACK's own tridiagonalisation of the MRRR child's inputs
    stays inside LAPACK_MRRR_ORTH and misses the 50 eps that divide & conquer keeps"""
    from scipy.linalg import lapack
    mx, frob = 0.0, 0.0
    for tag, A in _eig_inputs([3, 65, 257]):
        n = tag[0]
        _, d, e, _, info = (lapack.zhetrd if tag[1] else lapack.dsytrd)(A, lower=1)
        assert info == 0
        Z = sla.eigh_tridiagonal(d, e, lapack_driver="stemr")[1]
        G = Z.T @ Z - np.eye(n)
        mx = max(mx, np.max(np.abs(G)) / (n * EPS))
        frob = max(frob, np.linalg.norm(G) / np.sqrt(n) / EPS)
    assert D.K_MRRR_ORTH == 8 * D.LAPACK_MRRR_ORTH and D.LAPACK_EIG_ORTH < mx <= D.LAPACK_MRRR_ORTH, mx
    assert frob > 50, frob


def test_lapack_tridiagonal_solver_stays_inside_the_measured_constants():
    mx = np.zeros(3)
    for n in D.STEDC_SIZES:
        for name, (d, e) in D.small_tridiag_cases(n, np.random.default_rng(D.seed_of(5, n))).items():
            w, Z = D.tridiag_reference(d, e)
            wb = sla.eigh_tridiagonal(d, e, eigvals_only=True, lapack_driver="stebz") if len(d) > 1 else w
            mx = np.maximum(mx, D.tridiag_raw(d, e, w, Z, wb))
            assert D.worst(D.tridiag_ratios(d, e, w, Z))[0] <= 1, (n, name)
            Zs = Z.copy()
            if len(d) > 2 and name == "random":
                Zs[:, [0, 1]] = Zs[:, [1, 0]]
                assert D.tridiag_ratios(d, e, w, Zs)["resid"] > 1
    assert np.all(mx <= [D.LAPACK_TRI_RESID, D.LAPACK_TRI_ORTH, D.LAPACK_TRI_VALUE]), mx


def test_tridiag_cases_are_the_ones_the_older_test_used():
    c = D.tridiag_cases(100, np.random.default_rng(105))
    assert list(c) == ["random", "toeplitz_1_2_1", "wilkinson", "glued_wilkinson", "clustered", "graded", "zero_couplings",
                       "clement", "zero_matrix", "negative_couplings"]
    assert len(c["glued_wilkinson"][0]) == 84 and c["glued_wilkinson"][1][20] == 1e-8 and c["zero_couplings"][1][7] == 0.0
    assert "glued_wilkinson" not in D.small_tridiag_cases(2, np.random.default_rng(1))


def test_swapped_eigenvectors_fail_the_eigen_checker_and_a_close_pair_passes_the_older_tolerance():
    """Two eigenvectors swapped without their eigenvalues.  On a random matrix every check sees it.  For a pair whose eigenvalues
    differ by 5e-12 ||A||_2 at n = 700 the swap leaves a residual of 5e-12 ||A||_2 in two columns: it PASSES all three
    assertions of test_heevd_matches_scipy (1e-12 ||A||_F = 1.3e-11 ||A||_2 there) and fails the per-pair residual bound
    (9.6 n eps ||A||_2 = 1.5e-12 ||A||_2)."""
    n = 130
    A = D.herm_cases(np.random.default_rng(D.seed_of(4, n, True)), n, True)["random"]
    w, Z = sla.eigh(A, driver="evd")
    Zs = Z.copy(); Zs[:, [40, 41]] = Zs[:, [41, 40]]
    r = D.eig_ratios(A, w, Zs)
    assert r["resid"] > 1e3 and r["orth"] <= 1 and r["value"] <= 1
    ws = w.copy(); ws[[40, 41]] = ws[[41, 40]]
    assert D.eig_ratios(A, ws, Zs)["ascending"] == np.inf
    n = 700
    rng = np.random.default_rng(9)
    X = D.rnd(rng, (n, n), False)
    w0, Q = sla.eigh(X + X.T, driver="evd")
    w0[351] = w0[350] + 5e-12 * np.max(np.abs(w0))
    A = (Q * w0[None, :]) @ Q.T
    A = np.asfortranarray((A + A.T) / 2)
    w, Z = sla.eigh(A, driver="evd")
    assert D.worst(D.eig_ratios(A, w, Z))[0] <= 1
    Zs = Z.copy(); Zs[:, [350, 351]] = Zs[:, [351, 350]]
    assert np.max(np.abs(w - sla.eigvalsh(A))) <= 100 * EPS * np.abs(w).max()              # the three older assertions: pass
    assert np.linalg.norm(A @ Zs - Zs * w[None, :]) <= 1e-12 * np.linalg.norm(A)
    assert np.linalg.norm(Zs.T @ Zs - np.eye(n)) / np.sqrt(n) <= 50 * EPS
    r = D.eig_ratios(A, w, Zs)
    assert r["resid"] > 1 and r["resid_old"] <= 1, r                                       # the new one: fails
