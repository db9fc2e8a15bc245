"""The checkers of tests/gev_sp_refs.py checked themselves, and the ABI of the single-precision generalized problem, without a
GPU: LAPACK's fp32 routines stay inside every bound (and inside the constant written down for ssygst / chegst); the fp32 numpy
models of the device's blocked algorithms stay inside them on the sizes the GPU test runs; each planted fault is caught; the
library exports every new symbol - the s / c names of the C interface included, which the pattern of tests/test_capi_symbols.py
does not see - and every new entry point rejects a NULL context."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg as sla

import gev_sp_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPLX = pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
HIP_SYMBOLS = ["chase_hip_gemm_s_op", "chase_hip_gemm_c_op", "chase_hip_trsm_left_upper_sp", "chase_hip_trmm_left_upper_sp",
               "chase_hip_potrf_upper_blocked_sp", "chase_hip_hegst_upper_sp", "chase_hip_gev_reduce_sp",
               "chase_hip_gev_backtransform_sp", "chase_hip_gev_starttransform_sp"]
C_SYMBOLS = [p + "chase_gev_" + n for p in "sc" for n in ("reduce_", "reduce_itype_", "backtransform_", "backtransform_itype_",
                                                            "starttransform_")]
EINVAL = -1001


@pytest.fixture(scope="module")
def hegst_table():
    """(cplx, n, kappa) -> (A, U, LAPACK's raw ratio, the model's result): formed once"""
    out = {}
    for cplx in (False, True):
        for (n, kappa) in R.hegst_cases():
            A, U = R.hegst_inputs(n, cplx, kappa)
            out[(cplx, n, kappa)] = (A, U, R.hegst_raw(A, U, R.lapack_hegst(A, U)), R.model_hegst(A, U))
    return out


def test_lapack_hegst_stays_inside_the_measured_constant(hegst_table):
    worst = max((v[2], k) for k, v in hegst_table.items())
    print("LAPACK's largest fp32 ratio:", worst)
    assert worst[0] <= R.LAPACK_HEGST_SP
    assert worst[0] > R.LAPACK_HEGST_SP / 2                  # and the constant is what was measured, not a loose guess
    assert R.K_HEGST_SP == R.MARGIN * R.LAPACK_HEGST_SP and R.MARGIN == 8.0 and R.EPS32 == 2.0 ** -23


def test_hegst_model_stays_inside_the_bound_and_is_exactly_hermitian(hegst_table):
    peak = 0.0
    for key, (A, U, _, Cm) in hegst_table.items():
        assert Cm.dtype == A.dtype
        peak = max(peak, R.hegst_ratio(A, U, Cm))
        assert R.hegst_ratio(A, U, Cm) <= 1, key
        assert R.exactly_hermitian(Cm), key
    print("fp32 model of the two-solve reduction, largest ratio:", peak)


@CPLX
def test_product_checker_accepts_numpy_and_rejects_an_unconjugated_op(cplx):
    for (m, n, k) in R.GEMM_SHAPES:
        A, B, C0 = R.gemm_inputs(m, n, k, cplx)
        Ah = np.asfortranarray(A.conj().T)
        for (alpha, beta) in ((1.0, 0.0), (-1.0, 1.0)):
            ref = (np.float32(alpha) * (A @ B) + np.float32(beta) * C0).astype(A.dtype)
            assert R.gemm_ratio(ref, "N", alpha, A, B, beta, C0) <= 1, (m, n, k)
            assert R.gemm_ratio(ref, "C", alpha, Ah, B, beta, C0) <= 1, (m, n, k)
            if cplx and k > 1:
                bad = (np.float32(alpha) * (Ah.T @ B) + np.float32(beta) * C0).astype(A.dtype)      # op C without the conjugation
                assert R.gemm_ratio(bad, "C", alpha, Ah, B, beta, C0) > 1, (m, n, k)


@CPLX
def test_solve_and_product_models_stay_inside_the_bounds(cplx):
    peak_s = peak_m = 0.0
    for n in R.TRMM_N:
        for nrhs in R.TRSM_NRHS:
            Rm, B = R.trsm_inputs(n, nrhs, cplx)
            for op in "NC":
                if n in R.TRSM_N:
                    Xp = R.model_trsm_left(R.nan_lower(Rm), R.padded(B, n + 3), n, op)
                    assert Xp.dtype == B.dtype
                    peak_s = max(peak_s, R.left_solve_ratio(Xp[:n], Rm, B, op))
                    assert R.left_solve_ratio(Xp[:n], Rm, B, op) <= 1 and R.same_padding(Xp, n), (n, nrhs, op)
                Yp = R.model_trmm_left(R.nan_lower(Rm), R.padded(B, n + 3), n, op)
                peak_m = max(peak_m, R.trmm_ratio(Yp[:n], Rm, B, op))
                assert R.trmm_ratio(Yp[:n], Rm, B, op) <= 1 and R.same_padding(Yp, n), (n, nrhs, op)
    print("fp32 models, largest ratios: solve", peak_s, "product", peak_m)
    Rm, B = R.trsm_inputs(200, 33, cplx)                     # LAPACK's own fp32 solve and product pass as well
    for op, t in (("N", 0), ("C", 2)):
        X = sla.solve_triangular(Rm, B, trans=t)
        assert X.dtype == B.dtype and R.left_solve_ratio(X, Rm, B, op) <= 1
        trmm = sla.blas.ctrmm if cplx else sla.blas.strmm
        Y = trmm(1.0, Rm, B, side=0, lower=0, trans_a=t)
        assert Y.dtype == B.dtype and R.trmm_ratio(Y, Rm, B, op) <= 1


@CPLX
def test_cholesky_checker_accepts_lapack_and_the_model_on_every_case(cplx):
    for (n, ob) in R.POTRF_CASES:
        for kappa in R.POTRF_KAPPAS_SP + [1e6]:              # a device failure at 1e4 is a defect, not conditioning
            A = R.potrf_input(n, cplx, kappa)
            assert R.chol_ratio(A, R.lapack_potrf(A)) <= 1, (n, kappa)
            if kappa > 1e4:
                continue
            An = np.asfortranarray(np.triu(A) + np.tril(np.full(A.shape, R.CANARY, dtype=A.dtype), -1))
            Rm = R.model_potrf_blocked(An, ob)
            assert Rm.dtype == A.dtype and R.chol_ratio(A, Rm) <= 1, (n, ob, kappa)
            il = np.tril_indices(n, -1)
            assert R.same_bits(Rm[il], An[il])


def _check_pipeline(H, S, U, C, lam, X, rho):
    n = H.shape[0]
    r = R.gev_resid_ld(H, S, lam, X)
    wref = sla.eigh(R.wide(H), R.wide(S), eigvals_only=True)
    lmin, nC = sla.eigvalsh(R.wide(S))[0], np.linalg.norm(R.wide(C), 2)
    verr = R.value_errors(lam, wref)
    rb = np.array([R.gev_residual_bound(H, S, U, C, lam[j], X[:, j], rho[j]) for j in range(len(lam))])
    vb = np.array([R.gev_value_bound(r[j], lmin, n, nC) for j in range(len(lam))])
    return r, rb, verr, vb


@CPLX
def test_lapack_fp32_pipeline_stays_inside_the_assembled_bounds(cplx):
    H, S = R.solve_inputs(cplx)
    nev = R.SOLVE_NEV
    U, Cm, lam, Y, rho, X = R.lapack_pipeline(H, S, nev)
    assert 0.5 < np.linalg.norm(R.wide(Cm), 2) < 2                                   # the scaling of solve_inputs
    assert R.chol_ratio(S, U) <= 1 and R.hegst_ratio(H, U, Cm) <= 1 and R.left_solve_ratio(X, U, Y, "N") <= 1
    r, rb, verr, vb = _check_pipeline(H, S, U, Cm, lam, X, rho)
    print("LAPACK fp32 pipeline: largest residual", r.max(), "bound", rb.min(), "largest value error", verr.max())
    assert np.all(r <= rb) and np.all(verr <= vb)
    assert R.orth_ratio(X, S, U) <= 1
    # a worst-case bound in fp32 is wide (about 1e-2 here, against residuals of 1e-6); what it still rejects is an eigenvalue of
    # the wrong sign.  The sharp checks of a solve are the value errors and the reduction's own ratios above.
    bad = R.gev_resid_ld(H, S, -lam[:1], X[:, :1])[0]
    assert bad > rb[0]
    for step in (1, 2):                                                              # the pencils of the sequence are 1e-3 away
        H2, S2 = R.solve_inputs(cplx, step)
        dH = np.linalg.norm(R.wide(H2) - R.wide(H), 2) / np.linalg.norm(R.wide(H), 2)
        assert 5e-4 < dH < 2e-3 and (step == 2) == (not R.same_bits(S2, S))
        R.lapack_potrf(S2)


def test_planted_faults_are_caught():
    cplx = True
    # a skipped last trailing update in the Cholesky
    A = R.potrf_input(321, cplx, 10.0)
    assert R.chol_ratio(A, R.model_potrf_blocked(A, 128)) <= 1 < R.chol_ratio(A, R.model_potrf_blocked(A, 128, skip_last_update=True))
    # an unconjugated op C: in the solve, in the product and between the two solves of the reduction
    Rm, B = R.trsm_inputs(129, 33, cplx)
    assert R.left_solve_ratio(R.model_trsm_left(Rm, B, 129, "C", unconjugated=True), Rm, B, "C") > 1
    assert R.trmm_ratio(R.model_trmm_left(Rm, B, 129, "C", unconjugated=True), Rm, B, "C") > 1
    Ah, U = R.hegst_inputs(321, cplx, 10.0)
    assert R.hegst_ratio(Ah, U, R.model_hegst(Ah, U)) <= 1 < R.hegst_ratio(Ah, U, R.model_hegst(Ah, U, unconjugated=True))
    # a block inverse with one zeroed column, a back-solve that ignores ldx
    for op in "NC":
        assert R.left_solve_ratio(R.model_trsm_left(Rm, B, 129, op, zero_inv_col=(1, 5)), Rm, B, op) > 1
    assert R.left_solve_ratio(R.model_trsm_left(Rm, R.padded(B, 132), 129, "N", ld_bug=True)[:129], Rm, B, "N") > 1
    # one missing 1/2 A11 U12 (the recurrence is not what the device runs; the checker has to see the term all the same)
    assert R.hegst_ratio(Ah, U, R.model_hegst_missed_half(Ah, U)) > 1
    Ah2, U2 = R.hegst_inputs(129, False, 1e3)
    assert R.hegst_ratio(Ah2, U2, R.model_hegst_missed_half(Ah2, U2)) > 1
    # Hermitian only to rounding, or an imaginary diagonal of -0, is not exactly Hermitian
    Cm = R.model_hegst(Ah, U)
    Cm2 = Cm.copy(); Cm2[5, 3] = np.nextafter(Cm2[5, 3].real, np.float32(9)) + 1j * Cm2[5, 3].imag
    Cm3 = Cm.copy(); Cm3[4, 4] = complex(Cm3[4, 4].real, -0.0)
    assert R.exactly_hermitian(Cm) and not R.exactly_hermitian(Cm2) and not R.exactly_hermitian(Cm3)


def test_library_headers_and_binding_have_the_entry_points():
    lib = ctypes.CDLL(os.path.join(ROOT, "chase_amd", "lib", "libchase_hip.so"))
    assert not [n for n in HIP_SYMBOLS + C_SYMBOLS if not hasattr(lib, n)]
    hdr = open(os.path.join(ROOT, "include", "chase_hip.h")).read()
    assert all(re.search(r"\b%s\s*\(" % n, hdr) for n in HIP_SYMBOLS)
    chdr = open(os.path.join(ROOT, "include", "chase_c_interface.h")).read()
    assert len(C_SYMBOLS) == 10 and all(re.search(r"\b%s\s*\(" % n, chdr) for n in C_SYMBOLS)
    from chase_amd import capi
    assert all(getattr(capi.lib, n).argtypes for n in HIP_SYMBOLS)
    for m in ("gemm32op", "trsm_left_upper_sp", "trmm_left_upper_sp", "potrf_upper_blocked_sp", "hegst_upper_sp", "gev_reduce_sp",
              "gev_backtransform_sp", "gev_starttransform_sp"):
        assert callable(getattr(capi.Context, m))
    for m in ("set", "get", "solve", "stats", "resid", "reduced", "factor", "start_vectors", "update", "eigenpairs", "gev_residuals",
              "close"):
        assert callable(getattr(capi.SpGevSolver, m))
    assert isinstance(capi.SpGevSolver.ritzv, property)


def test_entry_points_reject_a_null_context_whatever_else_is_wrong():
    from chase_amd import capi
    L = capi.lib
    p = 4096                                                          # never dereferenced: the context is checked first
    one = (ctypes.c_float * 2)(1.0, 0.0)
    assert L.chase_hip_gemm_s_op(None, b"C", 4, 4, 4, 1.0, p, 4, p, 4, 0.0, p, 4) == EINVAL
    assert L.chase_hip_gemm_c_op(None, b"N", 4, 4, 4, one, p, 4, p, 4, one, p, 4) == EINVAL
    for op in (b"N", b"C", b"X"):
        assert L.chase_hip_trsm_left_upper_sp(None, 0, op, 4, 2, p, 4, p, 4) == EINVAL
        assert L.chase_hip_trmm_left_upper_sp(None, 1, op, 4, 2, p, 4, p, 3) == EINVAL
    assert L.chase_hip_potrf_upper_blocked_sp(None, 0, 4, p, 4, 0) == EINVAL
    assert L.chase_hip_hegst_upper_sp(None, 1, 4, p, 4, p, 4) == EINVAL
    assert L.chase_hip_gev_reduce_sp(None, 0, 1, 4, p, 4, p, 4) == EINVAL
    assert L.chase_hip_gev_backtransform_sp(None, 0, 4, 2, p, 4, p, 4) == EINVAL
    assert L.chase_hip_gev_starttransform_sp(None, 0, 4, 2, p, 4, p, 4) == EINVAL
    assert b"NULL ctx" in L.chase_hip_last_error()
    # the C interface checks its arguments before it looks for a device: a leading dimension below N, and itype 2 / 3
    info = ctypes.c_int(0)
    n, ld, one_i, two, three = (ctypes.c_int(v) for v in (4, 3, 1, 2, 3))
    buf = (ctypes.c_float * 64)()
    ref = ctypes.byref
    L.schase_gev_reduce_(ref(n), buf, ref(ld), buf, ref(n), ref(info))
    assert info.value == EINVAL
    for f, it in ((L.schase_gev_reduce_itype_, two), (L.cchase_gev_reduce_itype_, three)):
        info.value = 0
        f(ref(it), ref(one_i), ref(n), buf, ref(n), buf, ref(n), ref(info))
        assert info.value == EINVAL
    for f in (L.schase_gev_backtransform_itype_, L.cchase_gev_backtransform_itype_, L.schase_gev_starttransform_,
              L.cchase_gev_starttransform_):
        info.value = 0
        f(ref(two), ref(n), ref(two), buf, ref(n), buf, ref(n), ref(info))
        assert info.value == EINVAL
    info.value = 0
    L.cchase_gev_backtransform_(ref(n), ref(n), buf, ref(n), buf, ref(ld), ref(info))
    assert info.value == EINVAL
