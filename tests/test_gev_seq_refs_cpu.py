"""The checkers of tests/gev_seq_refs.py checked themselves, and the ABI of the sequence / itype additions, without a GPU: the
numpy models of the triangular product and of the product reduction stay inside their derived bounds on every size the GPU
test runs; LAPACK's own xHEGST (itype 2, 3) passes the same checker; each planted fault is caught; whole pipelines of the
models stay inside the assembled bounds for itype 2 and 3; the library exports the new symbols and they reject a NULL context."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg as sla

import gev_refs as G
import gev_seq_refs as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPLX = pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
HIP_SYMBOLS = ["chase_hip_trmm_left_upper", "chase_hip_hegst_product_upper", "chase_hip_gev_reduce_itype",
               "chase_hip_gev_backtransform_itype", "chase_hip_gev_starttransform"]
C_SYMBOLS = [p + n for p in "dz" for n in ("chase_gev_reduce_itype_", "chase_gev_backtransform_itype_", "chase_gev_starttransform_")]


@CPLX
def test_triangular_product_model_stays_inside_the_bound(cplx):
    """U carries NaN below its diagonal and the buffer three canary rows, as on the GPU"""
    for n in Q.TRMM_N:
        for ncols in Q.TRMM_NCOLS:
            U, X = Q.trmm_inputs(n, ncols, cplx)
            for op in "NC":
                Yp = Q.model_trmm_left(G.nan_lower(U), G.padded(X, n + 3), n, op)
                assert Q.tri_product_ratio(Yp[:n], U, X, op) <= 1, (n, ncols, op)
                assert G.same_padding(Yp, n)
    U, X = Q.trmm_inputs(200, 33, cplx)                      # BLAS's own product passes as well
    assert Q.tri_product_ratio(np.triu(U) @ X, U, X, "N") <= 1 and Q.tri_product_ratio(np.triu(U).conj().T @ X, U, X, "C") <= 1


@CPLX
def test_round_trips_of_the_models_stay_inside_the_summed_bounds(cplx):
    for (n, ncols) in Q.ROUNDTRIP_CASES:
        U, X = Q.trmm_inputs(n, ncols, cplx)
        for op in "NC":
            Y = Q.model_trmm_left(U, X, n, op)
            assert Q.roundtrip_ratio(G.model_trsm_left(U, Y, n, op), X, U, Y, op) <= 1, (n, ncols, op)
            W = G.model_trsm_left(U, X, n, op)
            assert Q.solve_then_product_ratio(Q.model_trmm_left(U, W, n, op), X, U, W, op) <= 1, (n, ncols, op)


@CPLX
def test_product_reduction_model_and_lapack_stay_inside_the_bound(cplx):
    for n in Q.HEGSTP_N:
        for kappa in Q.HEGSTP_KAPPAS:
            A, U = G.hegst_inputs(n, cplx, kappa)
            Cm = Q.model_hegst_product(G.nan_lower(A), G.nan_lower(U))
            assert Q.product_reduction_ratio(A, U, Cm) <= 1, (n, kappa)
            assert G.exactly_hermitian(Cm), (n, kappa)
            for itype in (2, 3):
                assert Q.product_reduction_ratio(A, U, Q.lapack_hegst_product(itype, A, U)) <= 1, (n, kappa, itype)


def test_planted_faults_are_caught():
    cplx = True
    U, X = Q.trmm_inputs(321, 33, cplx)
    Un = G.nan_lower(U)
    # an unconjugated op C
    assert Q.tri_product_ratio(Q.model_trmm_left(Un, X, 321, "C", unconjugated=True), U, X, "C") > 1
    for op in "NC":
        # a diagonal block used as a full square: the NaN below the diagonal shows it, and so would any finite value
        assert Q.tri_product_ratio(Q.model_trmm_left(Un, X, 321, op, diag_full=True), U, X, op) > 1
        Uf = np.asfortranarray(np.triu(U) + np.tril(np.ones_like(U), -1))
        assert Q.tri_product_ratio(Q.model_trmm_left(Uf, X, 321, op, diag_full=True), U, X, op) > 1
        assert Q.tri_product_ratio(Q.model_trmm_left(Uf, X, 321, op), U, X, op) <= 1
        # the long product of the last block skipped
        assert Q.tri_product_ratio(Q.model_trmm_left(Un, X, 321, op, skip_last_long=True), U, X, op) > 1
        # a tile written back with n where ldx belongs: wrong rows or a damaged canary
        Yp = Q.model_trmm_left(Un, G.padded(X, 324), 321, op, ld_bug=True)
        assert Q.tri_product_ratio(Yp[:321], U, X, op) > 1 or not G.same_padding(Yp, 321)
        assert Q.tri_product_ratio(Q.model_trmm_left(Un, G.padded(X, 324), 321, op)[:321], U, X, op) <= 1
    # the real flavour of the same defects at the smallest size that has two blocks
    Ur, Xr = Q.trmm_inputs(257, 33, False)
    assert Q.tri_product_ratio(Q.model_trmm_left(Ur, Xr, 257, "N", skip_last_long=True), Ur, Xr, "N") > 1
    assert Q.tri_product_ratio(Q.model_trmm_left(Ur, Xr, 257, "C", skip_last_long=True), Ur, Xr, "C") > 1
    # the product reduction completed from the triangle it must not read
    A, Uh = G.hegst_inputs(129, cplx, 10.0)
    assert Q.product_reduction_ratio(A, Uh, Q.model_hegst_product(G.nan_lower(A), Uh, wrong_mirror=True)) > 1
    Al = np.asfortranarray(np.triu(A) + np.tril(np.ones_like(A), -1))
    assert Q.product_reduction_ratio(A, Uh, Q.model_hegst_product(Al, Uh, wrong_mirror=True)) > 1
    assert Q.product_reduction_ratio(A, Uh, Q.model_hegst_product(Al, Uh)) <= 1
    # a result one ulp off, and one that is not exactly Hermitian
    Cm = Q.model_hegst_product(A, Uh)
    bad = Cm.copy(); bad[7, 3] *= 1 + 1e-9; bad[3, 7] = np.conj(bad[7, 3])
    assert Q.product_reduction_ratio(A, Uh, bad) > 1
    Cm2 = Cm.copy(); Cm2[5, 3] = np.nextafter(Cm2[5, 3].real, 1) + 1j * Cm2[5, 3].imag
    assert G.exactly_hermitian(Cm) and not G.exactly_hermitian(Cm2)


@CPLX
@pytest.mark.parametrize("itype", [2, 3])
def test_whole_pipeline_models_stay_inside_the_assembled_bounds(cplx, itype):
    H, S = G.solve_inputs(cplx)
    n, nev = G.SOLVE_N, G.SOLVE_NEV
    U, Cm, lam, Y, rho, X = Q.model_pipeline_itype(itype, H, S, nev)
    assert G.chol_ratio(S, U) <= 1 and Q.product_reduction_ratio(G.herm_full(H), U, Cm) <= 1
    assert (G.left_solve_ratio(X, U, Y, "N") if itype == 2 else Q.tri_product_ratio(X, U, Y, "C")) <= 1
    r = Q.pencil_resid_ld(itype, H, S, lam, X)
    wref = sla.eigh(H, S, type=itype, eigvals_only=True)
    nC = np.linalg.norm(Cm, 2)
    verr = G.value_errors(lam, wref)
    for j in range(nev):
        assert r[j] <= Q.gev_residual_bound_itype(itype, H, S, U, Cm, lam[j], X[:, j], rho[j]), j
        assert verr[j] <= Q.gev_value_bound_itype(itype, r[j], X[:, j], S, n, nC), j
    assert Q.orth_ratio_itype(itype, X, S, U) <= 1
    # worst-case bounds, but not vacuous: an eigenvalue wrong in its sixth digit misses them by orders of magnitude
    b0 = Q.gev_residual_bound_itype(itype, H, S, U, Cm, lam[0], X[:, 0], rho[0])
    bad = Q.pencil_resid_ld(itype, H, S, lam[:1] * (1 + 1e-5), X[:, :1])[0]
    print("itype", itype, "residual", r[0], "bound", b0, "with lambda (1 + 1e-5)", bad)
    assert bad > 100 * b0


@CPLX
def test_perturbed_pencils_are_what_the_sequence_tests_say(cplx):
    H0, S0 = G.solve_inputs(cplx)
    H1, S1 = Q.perturbed_pencil(H0, S0, 25, cplx)
    assert np.linalg.norm(H1 - H0, 2) == pytest.approx(1e-3 * np.linalg.norm(H0, 2), rel=1e-10)
    assert np.linalg.norm(S1 - S0, 2) == pytest.approx(1e-3 * sla.eigvalsh(S0)[0], rel=1e-6)
    assert sla.eigvalsh(S1)[0] > 0.99 * sla.eigvalsh(S0)[0]
    assert np.array_equal(H1, H1.conj().T) and np.array_equal(S1, S1.conj().T)
    H2, S2 = Q.perturbed_pencil(H1, S1, 26, cplx, with_s=False)
    assert S2 is S1 and not G.same_bits(H2, H1)


def test_library_header_and_binding_have_the_entry_points():
    lib = ctypes.CDLL(os.path.join(ROOT, "chase_amd", "lib", "libchase_hip.so"))
    assert not [n for n in HIP_SYMBOLS + C_SYMBOLS if not hasattr(lib, n)]
    hdr = open(os.path.join(ROOT, "include", "chase_hip.h")).read()
    assert all(re.search(r"\b%s\s*\(" % n, hdr) for n in HIP_SYMBOLS)
    chdr = open(os.path.join(ROOT, "include", "chase_c_interface.h")).read()
    assert all(re.search(r"\b%s\s*\(" % n, chdr) for n in C_SYMBOLS)
    from chase_amd import capi
    assert all(getattr(capi.lib, n).argtypes for n in HIP_SYMBOLS)
    for m in ("trmm_left_upper", "hegst_product_upper", "gev_reduce_itype", "gev_backtransform_itype", "gev_starttransform"):
        assert callable(getattr(capi.Context, m))
    for m in ("update", "start_vectors", "eigenpairs", "gev_residuals"):
        assert callable(getattr(capi.GevSolver, m))


def test_entry_points_reject_a_null_context_and_the_c_interface_a_bad_itype():
    from chase_amd import capi
    L, EINVAL = capi.lib, -1001
    p = 4096                                                          # never dereferenced: the context is checked first
    assert L.chase_hip_trmm_left_upper(None, 0, b"N", 4, 2, p, 4, p, 4) == EINVAL
    assert L.chase_hip_hegst_product_upper(None, 1, 4, p, 4, p, 4) == EINVAL
    assert L.chase_hip_gev_reduce_itype(None, 0, 2, 1, 4, p, 4, p, 4) == EINVAL
    assert L.chase_hip_gev_backtransform_itype(None, 0, 3, 4, 2, p, 4, p, 4) == EINVAL
    assert L.chase_hip_gev_starttransform(None, 0, 3, 4, 2, p, 4, p, 4) == EINVAL
    assert b"NULL ctx" in L.chase_hip_last_error()
    # the C interface checks its arguments before it looks for a device
    info = ctypes.c_int(0)
    n, ld, one = ctypes.c_int(4), ctypes.c_int(3), ctypes.c_int(1)
    buf = (ctypes.c_double * 32)()
    R = ctypes.byref
    for bad in (0, 4, -1):
        it = ctypes.c_int(bad)
        info.value = 0
        L.dchase_gev_reduce_itype_(R(it), R(one), R(n), buf, R(n), buf, R(n), R(info))
        assert info.value == EINVAL
        info.value = 0
        L.zchase_gev_backtransform_itype_(R(it), R(n), R(n), buf, R(n), buf, R(n), R(info))
        assert info.value == EINVAL
        info.value = 0
        L.dchase_gev_starttransform_(R(it), R(n), R(n), buf, R(n), buf, R(n), R(info))
        assert info.value == EINVAL
    it, two = ctypes.c_int(2), ctypes.c_int(2)
    info.value = 0
    L.dchase_gev_reduce_itype_(R(it), R(two), R(n), buf, R(n), buf, R(n), R(info))              # factor outside 0 / 1
    assert info.value == EINVAL
    info.value = 0
    L.dchase_gev_starttransform_(R(it), R(n), R(n), buf, R(n), buf, R(ld), R(info))             # ldv < N
    assert info.value == EINVAL
