"""The checkers of tests/gev_refs.py checked themselves, and the ABI of the generalized problem, without a GPU: LAPACK stays
inside the constant written down for it; the numpy models of the device's blocked algorithms stay inside every bound on every
size the GPU test runs, alone and as a whole pipeline; each planted fault is caught; the library exports the nine new symbols
and its five chase_hip_* entry points reject a NULL context (with it every other bad argument: the argument checks that need a
live context - op, block sizes, leading dimensions - run in tests/test_gpu_gev.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg as sla

import gev_refs as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPLX = pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
HIP_SYMBOLS = ["chase_hip_trsm_left_upper", "chase_hip_potrf_upper_blocked", "chase_hip_hegst_upper", "chase_hip_gev_reduce",
               "chase_hip_gev_backtransform"]
C_SYMBOLS = ["dchase_gev_reduce_", "zchase_gev_reduce_", "dchase_gev_backtransform_", "zchase_gev_backtransform_"]


@pytest.fixture(scope="module")
def hegst_table():
    """(cplx, n, nb, kappa) -> (A, U, LAPACK's raw ratio, the model's result): formed once"""
    out = {}
    for cplx in (False, True):
        for (n, nb, kappa) in G.hegst_cases():
            A, U = G.hegst_inputs(n, cplx, kappa)
            out[(cplx, n, nb, kappa)] = (A, U, G.hegst_raw(A, U, G.lapack_hegst(A, U)), G.model_hegst(A, U, nb))
    return out


def test_lapack_hegst_stays_inside_the_measured_constant(hegst_table):
    worst = max((v[2], k) for k, v in hegst_table.items())
    print("LAPACK's largest ratio:", worst)
    assert worst[0] <= G.LAPACK_HEGST
    assert worst[0] > G.LAPACK_HEGST / 2                      # and the constant is what was measured, not a loose guess
    assert G.K_HEGST == G.MARGIN * G.LAPACK_HEGST and G.MARGIN == 8.0


def test_hegst_model_stays_inside_the_bound_and_is_exactly_hermitian(hegst_table):
    for key, (A, U, _, Cm) in hegst_table.items():
        assert G.hegst_ratio(A, U, Cm) <= 1, key
        assert G.exactly_hermitian(Cm), key


@CPLX
def test_left_solve_model_stays_inside_the_bound(cplx):
    for n in G.TRSM_N:
        for nrhs in G.TRSM_NRHS:
            R, B = G.trsm_inputs(n, nrhs, cplx)
            for op in "NC":
                Xp = G.model_trsm_left(G.nan_lower(R), G.padded(B, n + 3), n, op)
                assert G.left_solve_ratio(Xp[:n], R, B, op) <= 1, (n, nrhs, op)
                assert G.same_padding(Xp, n)
    R, B = G.trsm_inputs(200, 33, cplx)                      # LAPACK's own solve passes as well
    for op, t in (("N", 0), ("C", 2)):
        assert G.left_solve_ratio(sla.solve_triangular(R, B, trans=t), R, B, op) <= 1


@CPLX
def test_blocked_cholesky_model_stays_inside_the_bound_and_leaves_the_lower_triangle(cplx):
    for (n, ob) in G.POTRF_CASES:
        for kappa in G.POTRF_KAPPAS:
            A = G.potrf_input(n, cplx, kappa)
            An = np.asfortranarray(np.triu(A) + np.tril(np.full(A.shape, G.CANARY), -1))
            Rm = G.model_potrf_blocked(An, ob)
            assert G.chol_ratio(A, Rm) <= 1, (n, ob, kappa)
            il = np.tril_indices(n, -1)
            assert G.same_bits(Rm[il], An[il])


@CPLX
def test_whole_pipeline_model_stays_inside_the_assembled_bounds(cplx):
    H, S = G.solve_inputs(cplx)
    n, nev = G.SOLVE_N, G.SOLVE_NEV
    U, Cm, lam, Y, rho, X = G.model_pipeline(H, S, nev)
    assert G.chol_ratio(S, U) <= 1 and G.hegst_ratio(H, U, Cm) <= 1 and G.left_solve_ratio(X, U, Y, "N") <= 1
    r = G.gev_resid_ld(H, S, lam, X)
    wref = sla.eigh(H, S, eigvals_only=True)
    lmin, nC = sla.eigvalsh(S)[0], np.linalg.norm(Cm, 2)
    verr = G.value_errors(lam, wref)
    for j in range(nev):
        assert r[j] <= G.gev_residual_bound(H, S, U, Cm, lam[j], X[:, j], rho[j]), j
        assert verr[j] <= G.gev_value_bound(r[j], lmin, n, nC), j
    assert G.orth_ratio(X, S, U) <= 1
    # the bound is a worst-case one (about 5e-8 here, against residuals of 1e-11) but not vacuous: an eigenvalue wrong in its
    # sixth digit misses it by orders of magnitude
    bad = G.gev_resid_ld(H, S, lam[:1] * (1 + 1e-5), X[:, :1])[0]
    print("residual", r[0], "bound", G.gev_residual_bound(H, S, U, Cm, lam[0], X[:, 0], rho[0]), "with lambda (1 + 1e-5)", bad)
    assert bad > 100 * G.gev_residual_bound(H, S, U, Cm, lam[0], X[:, 0], rho[0])


def test_planted_faults_are_caught():
    cplx = True
    # a skipped last trailing update: in the Cholesky and in the reduction
    A = G.potrf_input(321, cplx, 10.0)
    assert G.chol_ratio(A, G.model_potrf_blocked(A, 128)) <= 1 < G.chol_ratio(A, G.model_potrf_blocked(A, 128, skip_last_update=True))
    Ah, U = G.hegst_inputs(321, cplx, 10.0)
    assert G.hegst_ratio(Ah, U, G.model_hegst(Ah, U, 128, skip_last_update=True)) > 1
    # one missing 1/2 A11 U12
    assert G.hegst_ratio(Ah, U, G.model_hegst(Ah, U, 128, miss_half=True)) > 1
    Ah2, U2 = G.hegst_inputs(129, False, 1e5)
    assert G.hegst_ratio(Ah2, U2, G.model_hegst(Ah2, U2, 64, miss_half=True)) > 1
    # an unconjugated op C, a block inverse with one zeroed column
    R, B = G.trsm_inputs(129, 33, cplx)
    assert G.left_solve_ratio(G.model_trsm_left(R, B, 129, "C", unconjugated=True), R, B, "C") > 1
    for op in "NC":
        assert G.left_solve_ratio(G.model_trsm_left(R, B, 129, op, zero_inv_col=(1, 5)), R, B, op) > 1
    # a back-solve that ignores ldx: wrong rows or a damaged canary
    Xp = G.model_trsm_left(R, G.padded(B, 132), 129, "N", ld_bug=True)
    assert G.left_solve_ratio(Xp[:129], R, B, "N") > 1
    assert G.left_solve_ratio(G.model_trsm_left(R, G.padded(B, 132), 129, "N")[:129], R, B, "N") <= 1
    # a result that is Hermitian only to rounding is not exactly Hermitian
    Cm = G.model_hegst(Ah2, U2)
    Cm2 = Cm.copy(); Cm2[5, 3] = np.nextafter(Cm2[5, 3], 1)
    assert G.exactly_hermitian(Cm) and not G.exactly_hermitian(Cm2)
    Z = G.model_hegst(Ah, U, 128); Z[4, 4] = complex(Z[4, 4].real, -0.0)
    assert not G.exactly_hermitian(Z)                                # imaginary diagonal -0


def test_library_header_and_binding_have_the_entry_points():
    lib = ctypes.CDLL(os.path.join(ROOT, "chase_amd", "lib", "libchase_hip.so"))
    assert not [n for n in HIP_SYMBOLS + C_SYMBOLS if not hasattr(lib, n)]
    hdr = open(os.path.join(ROOT, "include", "chase_hip.h")).read()
    assert all(re.search(r"\b%s\s*\(" % n, hdr) for n in HIP_SYMBOLS)
    chdr = open(os.path.join(ROOT, "include", "chase_c_interface.h")).read()
    assert all(re.search(r"\b%s\s*\(" % n, chdr) for n in C_SYMBOLS)
    from chase_amd import capi
    assert all(getattr(capi.lib, n).argtypes for n in HIP_SYMBOLS)
    for m in ("trsm_left_upper", "potrf_upper_blocked", "hegst_upper", "gev_reduce", "gev_backtransform"):
        assert callable(getattr(capi.Context, m))
    for m in ("set", "get", "solve", "stats", "resid", "eigenpairs", "gev_residuals"):
        assert callable(getattr(capi.GevSolver, m))


def test_entry_points_reject_a_null_context_whatever_else_is_wrong():
    from chase_amd import capi
    L, EINVAL = capi.lib, -1001
    p = 4096                                                          # never dereferenced: the context is checked first
    for op in (b"N", b"C", b"T"):
        assert L.chase_hip_trsm_left_upper(None, 0, op, 4, 2, p, 4, p, 4) == EINVAL
    assert L.chase_hip_trsm_left_upper(None, 1, b"N", 4, 2, p, 3, p, 4) == EINVAL          # ld < n
    assert L.chase_hip_potrf_upper_blocked(None, 0, 4, p, 4, 0) == EINVAL
    assert L.chase_hip_potrf_upper_blocked(None, 0, 4, p, 3, 0) == EINVAL
    assert L.chase_hip_hegst_upper(None, 1, 4, p, 4, p, 4, 0) == EINVAL
    assert L.chase_hip_hegst_upper(None, 1, 4, p, 4, p, 3, 0) == EINVAL
    assert L.chase_hip_gev_reduce(None, 0, 4, p, 4, p, 4) == EINVAL
    assert L.chase_hip_gev_reduce(None, 0, 4, p, 3, p, 4) == EINVAL
    assert L.chase_hip_gev_backtransform(None, 0, 4, 2, p, 4, p, 4) == EINVAL
    assert L.chase_hip_gev_backtransform(None, 0, 4, 2, p, 4, p, 3) == EINVAL
    assert b"NULL ctx" in L.chase_hip_last_error()
    # the C interface checks its arguments before it looks for a device
    info = ctypes.c_int(0)
    n, ld = ctypes.c_int(4), ctypes.c_int(3)
    buf = (ctypes.c_double * 32)()
    L.dchase_gev_reduce_(ctypes.byref(n), buf, ctypes.byref(ld), buf, ctypes.byref(n), ctypes.byref(info))
    assert info.value == EINVAL
    info.value = 0
    L.zchase_gev_backtransform_(ctypes.byref(n), ctypes.byref(n), buf, ctypes.byref(n), buf, ctypes.byref(ld), ctypes.byref(info))
    assert info.value == EINVAL
