"""The single-precision generalized problem H x = lambda S x on the GPU - chase_hip_gemm_s_op / _c_op, chase_hip_trsm_left_upper_sp,
chase_hip_trmm_left_upper_sp, chase_hip_potrf_upper_blocked_sp, chase_hip_hegst_upper_sp (hegs2_diag at n <= 64),
chase_hip_gev_reduce_sp / _backtransform_sp / _starttransform_sp, SpGevSolver and the C interface - held against the checkers of
tests/gev_sp_refs.py: componentwise bounds with factor 1 and EPS32 for the products, the solve and the factorisation, two
bit-for-bit contracts for the product, 8 x LAPACK's measured fp32 error for the two-sided reduction, the assembled a-priori
bounds for whole solves.  Real and complex, leading dimensions once tight and once padded by 3 rows of a canary that must survive
bit for bit; the triangles the contracts call "never read" hold NaN.  The smallest sizes at which each kernel can still go wrong:
one block, the 64-wide steps and their ragged rests, a second 256-row block, several outer blocks (outer_nb = 128)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla

import gev_sp_refs as R

pytestmark = pytest.mark.gpu
CPLX = pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
PAD = pytest.mark.parametrize("pad", [0, 3], ids=["ld=extent", "ld=extent+3"])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1001


@pytest.fixture(scope="module")
def gctx(ctx):
    from chase_amd.capi import lib
    lib.chase_hip_ctx_set_phase(ctx.h, 0)
    return ctx


def _up(ctx, a):
    a = np.asarray(a)
    assert a.dtype in (np.float32, np.complex64)
    return ctx.empty(a.shape, a.dtype).upload(a)


def _run(ctx, fn, *bufs):
    """uploads the padded fp32 host buffers (the row count IS the leading dimension), calls fn(device arrays), downloads them all"""
    dev = [_up(ctx, b) for b in bufs]
    rc = fn(*dev)
    out = [d.download() for d in dev]
    for d in dev:
        d.free()
    return rc, out


# ---- gemm32op ---------------------------------------------------------------------------------------------------------------------
@CPLX
@PAD
@pytest.mark.parametrize("ab", [(1.0, 0.0), (-1.0, 1.0)], ids=["alpha=1,beta=0", "alpha=-1,beta=1"])
def test_gemm32op_bitwise_contracts_and_bound(gctx, cplx, pad, ab):
    """op N is gemm32 bit for bit; op C is op N on the explicitly formed A^H bit for bit; both within gamma32(k) of the long double
    product; rows beyond m keep the canary; beta = 0 does not read C (it holds NaN)"""
    alpha, beta = ab
    peak = 0.0
    for (m, n, k) in R.GEMM_SHAPES:
        A, B, C0 = R.gemm_inputs(m, n, k, cplx)
        Ah = np.asfortranarray(A.conj().T)                                 # k x m
        if beta == 0:
            C0 = np.full_like(C0, np.nan)
        Ap, Ahp, Bp, Cp = R.padded(A, m + pad), R.padded(Ah, k + pad), R.padded(B, k + pad), R.padded(C0, m + pad)
        outs = {}
        for name, op, a in (("gemm32", "N", Ap), ("opN", "N", Ap), ("opC", "C", Ahp)):
            f = gctx.gemm32 if name == "gemm32" else gctx.gemm32op
            _, (_, _, Cout) = _run(gctx, lambda dA, dB, dC: f(op, m, n, k, alpha, dA.ptr, dA.ld, dB.ptr, dB.ld, beta, dC.ptr, dC.ld,
                                                               cplx), a, Bp, Cp)
            assert R.same_padding(Cout, m), (name, m, n, k)
            outs[name] = Cout[:m]
        assert R.same_bits(outs["opN"], outs["gemm32"]), (m, n, k)
        assert R.same_bits(outs["opC"], outs["opN"]), (m, n, k)
        ref0 = np.zeros_like(C0) if beta == 0 else C0
        r = max(R.gemm_ratio(outs["opN"], "N", alpha, A, B, beta, ref0), R.gemm_ratio(outs["opC"], "C", alpha, Ah, B, beta, ref0))
        peak = max(peak, r)
        assert r <= 1, (m, n, k, r)
    print("gemm32op largest ratio:", peak)


def test_gemm32_still_refuses_op_c_and_gemm32op_takes_t_for_real_data(gctx):
    from chase_amd.capi import ChaseHipError, lib
    A, B, C0 = R.gemm_inputs(129, 130, 200, False)
    At = np.asfortranarray(A.T)
    dA, dB, dC = _up(gctx, At), _up(gctx, B), _up(gctx, C0)
    with pytest.raises(ChaseHipError) as e:
        gctx.gemm32("C", 129, 130, 200, 1.0, dA.ptr, 200, dB.ptr, 200, 0.0, dC.ptr, 129, False)
    assert e.value.code == EINVAL and "opA" in str(e.value)
    gctx.gemm32op("C", 129, 130, 200, 1.0, dA.ptr, 200, dB.ptr, 200, 0.0, dC.ptr, 129, False)
    c1 = dC.download()
    gctx.gemm32op("T", 129, 130, 200, 1.0, dA.ptr, 200, dB.ptr, 200, 0.0, dC.ptr, 129, False)
    assert R.same_bits(dC.download(), c1)
    one = (np.ctypeslib.ctypes.c_float * 2)(1.0, 0.0)
    assert lib.chase_hip_gemm_c_op(gctx.h, b"T", 4, 4, 4, one, dA.ptr, 200, dB.ptr, 200, one, dC.ptr, 129) == EINVAL
    assert b"opA" in lib.chase_hip_last_error()
    for d in (dA, dB, dC):
        d.free()


# ---- trsm_left_upper_sp / trmm_left_upper_sp ------------------------------------------------------------------------------------------
@CPLX
@PAD
@pytest.mark.parametrize("op", ["N", "C"])
def test_trsm_left_upper_sp_componentwise_bound(gctx, cplx, pad, op):
    """R: the fp32-rounded reference factor of hpd(n, 1e5) with NaN in its strictly lower triangle - it is never read"""
    peak = 0.0
    for n in R.TRSM_N:
        for nrhs in R.TRSM_NRHS:
            Rm, B = R.trsm_inputs(n, nrhs, cplx)
            Rp, Bp = R.padded(R.nan_lower(Rm), n + pad), R.padded(B, n + pad)
            _, (Rout, Xp) = _run(gctx, lambda dR, dB: gctx.trsm_left_upper_sp(op, n, nrhs, dR.ptr, dR.ld, dB.ptr, dB.ld, cplx), Rp, Bp)
            r = R.left_solve_ratio(Xp[:n], Rm, B, op)
            peak = max(peak, r)
            assert r <= 1, (n, nrhs, r)
            assert R.same_padding(Xp, n) and R.same_bits(Rout, Rp), (n, nrhs)
    print("trsm_left_upper_sp largest ratio:", peak)


@CPLX
@PAD
@pytest.mark.parametrize("op", ["N", "C"])
def test_trmm_left_upper_sp_componentwise_bound(gctx, cplx, pad, op):
    peak = 0.0
    for n in R.TRMM_N:
        for nrhs in R.TRSM_NRHS:
            U, X = R.trsm_inputs(n, nrhs, cplx)
            Up, Xp = R.padded(R.nan_lower(U), n + pad), R.padded(X, n + pad)
            _, (Uout, Yp) = _run(gctx, lambda dU, dX: gctx.trmm_left_upper_sp(op, n, nrhs, dU.ptr, dU.ld, dX.ptr, dX.ld, cplx), Up, Xp)
            r = R.trmm_ratio(Yp[:n], U, X, op)
            peak = max(peak, r)
            assert r <= 1, (n, nrhs, r)
            assert R.same_padding(Yp, n) and R.same_bits(Uout, Up), (n, nrhs)
    print("trmm_left_upper_sp largest ratio:", peak)


# ---- potrf_upper_blocked_sp -----------------------------------------------------------------------------------------------------------
@CPLX
@PAD
@pytest.mark.parametrize("kappa", R.POTRF_KAPPAS_SP)
def test_potrf_upper_blocked_sp_bound_and_untouched_lower_triangle(gctx, cplx, pad, kappa):
    peak = 0.0
    for (n, ob) in R.POTRF_CASES:
        A = R.potrf_input(n, cplx, kappa)
        Ap = R.padded(R.nan_lower(A), n + pad)
        info, (Rp,) = _run(gctx, lambda dA: gctx.potrf_upper_blocked_sp(n, dA.ptr, dA.ld, cplx, ob), Ap)
        assert info == 0, (n, ob, info)
        r = R.chol_ratio(A, Rp[:n])
        peak = max(peak, r)
        assert r <= 1, (n, ob, r)
        il = np.tril_indices(n, -1)
        assert R.same_bits(Rp[:n][il], Ap[:n][il]), (n, ob)                  # the NaN canary below the diagonal, bit for bit
        assert R.same_padding(Rp, n), (n, ob)
    print("potrf_upper_blocked_sp largest ratio:", peak)


@CPLX
def test_potrf_upper_blocked_sp_info_is_the_first_bad_pivot(gctx, cplx):
    for (n, ob, p) in ((200, 0, 70), (321, 128, 70), (321, 128, 200)):
        A = R.potrf_input(n, cplx, 10.0).copy()
        A[p - 1, p - 1] = -1.0                                             # indefinite at pivot p (1-based)
        info, _ = _run(gctx, lambda dA: gctx.potrf_upper_blocked_sp(n, dA.ptr, dA.ld, cplx, ob), R.padded(R.nan_lower(A), n + 3))
        assert info == p, (n, ob, p, info)


# ---- hegs2_diag / hegst_upper_sp ------------------------------------------------------------------------------------------------------
def _check_hegst(gctx, cplx, pad, sizes):
    peak = 0.0
    for n in sizes:
        for kappa in R.HEGST_KAPPAS_SP:
            A, U = R.hegst_inputs(n, cplx, kappa)
            Ap, Up = R.padded(R.nan_lower(A), n + pad), R.padded(R.nan_lower(U), n + pad)      # only the upper triangles are read
            _, (Cp, Uout) = _run(gctx, lambda dA, dU: gctx.hegst_upper_sp(n, dA.ptr, dA.ld, dU.ptr, dU.ld, cplx), Ap, Up)
            r = R.hegst_ratio(A, U, Cp[:n])
            peak = max(peak, r)
            assert r <= 1, (n, kappa, r)
            assert R.exactly_hermitian(Cp[:n]), (n, kappa)
            assert R.same_padding(Cp, n) and R.same_bits(Uout, Up), (n, kappa)
    print("hegst_upper_sp largest ratio (error over 8 x LAPACK's):", peak)


@CPLX
@PAD
def test_hegs2_diag_sp_one_block_exactly_hermitian(gctx, cplx, pad):
    _check_hegst(gctx, cplx, pad, R.HEGS2_SIZES)


@CPLX
@PAD
def test_hegst_upper_sp_two_solves_exactly_hermitian(gctx, cplx, pad):
    _check_hegst(gctx, cplx, pad, R.HEGST_N)


# ---- gev_reduce_sp / transforms / argument checks ---------------------------------------------------------------------------------
@CPLX
def test_gev_reduce_sp_reports_the_pivot_and_leaves_A_alone(gctx, cplx):
    n, p = 200, 70
    A, _ = R.hegst_inputs(n, cplx, 10.0)
    S = R.potrf_input(n, cplx, 10.0).copy()
    S[p - 1, p - 1] = -1.0
    Ap = R.padded(R.nan_lower(A), n + 3)
    info, (Aout, _) = _run(gctx, lambda dA, dS: gctx.gev_reduce_sp(1, n, dA.ptr, dA.ld, dS.ptr, dS.ld, cplx), Ap, R.padded(S, n + 3))
    assert info == p and R.same_bits(Aout, Ap)
    from chase_amd.capi import SpGevSolver, ChaseHipError
    with pytest.raises(ChaseHipError) as e:
        SpGevSolver(gctx, R.herm_full(A), np.asfortranarray(S), 8, 8)
    assert e.value.code == p and e.value.pivot == p


@CPLX
def test_gev_reduce_sp_factor_0_reuses_the_stored_factor_bit_for_bit(gctx, cplx):
    n = 321
    A, _ = R.hegst_inputs(n, cplx, 10.0)
    S = R.potrf_input(n, cplx, 1e3)
    Ap, Sp = R.padded(R.nan_lower(A), n + 3), R.padded(R.nan_lower(S), n + 3)
    info, (C1, U1) = _run(gctx, lambda dA, dS: gctx.gev_reduce_sp(1, n, dA.ptr, dA.ld, dS.ptr, dS.ld, cplx), Ap, Sp)
    assert info == 0 and R.chol_ratio(S, U1[:n]) <= 1 and R.hegst_ratio(A, np.triu(U1[:n]), C1[:n]) <= 1
    info, (C0, U0) = _run(gctx, lambda dA, dS: gctx.gev_reduce_sp(0, n, dA.ptr, dA.ld, dS.ptr, dS.ld, cplx), Ap, U1)
    assert info == 0 and R.same_bits(C0, C1) and R.same_bits(U0, U1)


@CPLX
def test_start_then_back_transform_returns_the_block(gctx, cplx):
    """X -> U X -> U^{-1} (U X): the product within its bound, the solve within its bound of what the product left, and so the
    round trip within the sum of both: |X'' - X| <= |U^{-1}| (gamma32(n) |U| |X| + gamma32(n) |U| |X''|) componentwise"""
    for n, ncols in ((65, 33), (321, 130)):
        U, X = R.trsm_inputs(n, ncols, cplx)
        Up, Xp = R.padded(R.nan_lower(U), n + 3), R.padded(X, n + 3)
        _, (_, Yp) = _run(gctx, lambda dU, dX: gctx.gev_starttransform_sp(n, ncols, dU.ptr, dU.ld, dX.ptr, dX.ld, cplx), Up, Xp)
        assert R.trmm_ratio(Yp[:n], U, X, "N") <= 1 and R.same_padding(Yp, n)
        _, (_, Zp) = _run(gctx, lambda dU, dX: gctx.gev_backtransform_sp(n, ncols, dU.ptr, dU.ld, dX.ptr, dX.ld, cplx), Up, Yp)
        Z = Zp[:n]
        assert R.left_solve_ratio(Z, U, Yp[:n], "N") <= 1 and R.same_padding(Zp, n)
        g = R.gamma32(n, cplx)
        aU = np.abs(R.wide(np.triu(U)))
        bound = np.abs(np.linalg.inv(R.wide(np.triu(U)))) @ (g * aU @ (np.abs(R.wide(X)) + np.abs(R.wide(Z))))
        assert np.all(np.abs(R.wide(Z) - R.wide(X)) <= bound), (n, ncols)


def test_bad_arguments_are_einval(gctx):
    from chase_amd.capi import lib
    import ctypes
    d = gctx.empty((8, 8), np.float32)
    h, p = gctx.h, d.ptr
    for f in (lib.chase_hip_trsm_left_upper_sp, lib.chase_hip_trmm_left_upper_sp):
        assert f(h, 0, b"X", 4, 2, p, 8, p, 8) == EINVAL
        assert b"op must be" in lib.chase_hip_last_error()
        for args in ((4, 2, p, 3, p, 8), (4, 2, p, 8, p, 3), (-1, 2, p, 8, p, 8), (4, 2, None, 8, p, 8), (4, 2, p, 8, None, 8)):
            assert f(h, 0, b"N", *args) == EINVAL
        assert f(h, 0, b"N", 0, 2, None, 0, None, 0) == 0                             # empty operands are legal
    assert lib.chase_hip_potrf_upper_blocked_sp(h, 0, 4, p, 3, 0) == EINVAL
    assert lib.chase_hip_potrf_upper_blocked_sp(h, 0, 4, p, 8, 100) == EINVAL        # no multiple of 64
    assert lib.chase_hip_potrf_upper_blocked_sp(h, 0, -1, p, 8, 0) == EINVAL
    assert lib.chase_hip_potrf_upper_blocked_sp(h, 0, 4, None, 8, 0) == EINVAL
    assert lib.chase_hip_hegst_upper_sp(h, 0, 4, p, 8, p, 3) == EINVAL
    assert lib.chase_hip_hegst_upper_sp(h, 0, 4, None, 8, p, 8) == EINVAL
    assert lib.chase_hip_gev_reduce_sp(h, 0, 1, 4, p, 3, p, 8) == EINVAL
    assert lib.chase_hip_gev_reduce_sp(h, 0, 2, 4, p, 8, p, 8) == EINVAL             # factor is 0 or 1
    assert lib.chase_hip_gev_reduce_sp(h, 0, 1, -1, p, 8, p, 8) == EINVAL
    assert lib.chase_hip_gev_reduce_sp(h, 0, 1, 4, p, 8, None, 8) == EINVAL
    for f in (lib.chase_hip_gev_backtransform_sp, lib.chase_hip_gev_starttransform_sp):
        assert f(h, 0, 4, 2, p, 3, p, 8) == EINVAL
        assert f(h, 0, 4, 2, p, 8, p, 3) == EINVAL
        assert f(h, 0, 4, 2, None, 8, p, 8) == EINVAL
    d.free()
    # the C interface: itype 2 has no single-precision form
    info, n, two, one = (ctypes.c_int(v) for v in (0, 4, 2, 1))
    buf = (ctypes.c_float * 64)()
    lib.cchase_gev_reduce_itype_(ctypes.byref(two), ctypes.byref(one), ctypes.byref(n), buf, ctypes.byref(n), buf, ctypes.byref(n),
                                 ctypes.byref(info))
    assert info.value == EINVAL


# ---- whole solves ------------------------------------------------------------------------------------------------------------------
def _check_pairs(H, S, U, C, lam, X, rho, label):
    n = H.shape[0]
    r = R.gev_resid_ld(H, S, lam, X)
    wref = sla.eigh(R.wide(H), R.wide(S), eigvals_only=True)
    lmin, nC = sla.eigvalsh(R.wide(S))[0], np.linalg.norm(R.wide(C), 2)
    verr = R.value_errors(lam, wref)
    rb = np.array([R.gev_residual_bound(H, S, U, C, lam[j], X[:, j], rho[j]) for j in range(len(lam))])
    vb = np.array([R.gev_value_bound(r[j], lmin, n, nC) for j in range(len(lam))])
    print(label, "largest residual / bound:", float(np.max(r / rb)), "largest value error / bound:", float(np.max(verr / vb)),
          "largest residual:", float(np.max(r)), "largest value error:", float(np.max(verr)))
    return r, rb, verr, vb


def _solve_and_check(g, H, S, nev, label):
    C, U = g.reduced(), np.triu(g.factor())                                # before the solve: its diagonal shifts work on C in place
    st = g.solve()
    assert st["locked"] >= nev, st
    lam, X = g.eigenpairs()
    assert X.dtype == H.dtype and lam.dtype == np.float64
    resid, rho = g.gev_residuals(), g.resid()[:nev]
    assert R.chol_ratio(S, U) <= 1 and R.hegst_ratio(H, U, C) <= 1 and R.exactly_hermitian(C)
    r, rb, verr, vb = _check_pairs(H, S, U, C, lam, X, rho, label)
    assert np.all(resid <= rb), (resid, rb)                                 # the device's own residuals ...
    assert np.all(r <= rb) and np.all(verr <= vb)                           # ... and the long double ones, and the Ritz values
    assert R.orth_ratio(X, S, U) <= 1
    return st


@CPLX
def test_sp_gev_solver_whole_solve_and_sequence(gctx, cplx):
    from chase_amd.capi import SpGevSolver
    n, nev, nex = R.SOLVE_N, R.SOLVE_NEV, R.SOLVE_NEX
    H, S = R.solve_inputs(cplx)
    g = SpGevSolver(gctx, H, S, nev, nex)
    g.set(tol=R.SOLVE_TOL_SP)                                               # the float default, said aloud
    fp64_matrix = n * n * 8 * (2 if cplx else 1)
    assert g.dC.nbytes == H.nbytes and g.dU.nbytes == S.nbytes and g.dC.dtype == H.dtype      # the two matrices, in place, fp32
    print("device_bytes before the solve:", g.get("device_bytes"), "one fp64 matrix:", fp64_matrix)
    assert g.get("device_bytes") < fp64_matrix                              # the solver's own allocations hold no N^2 fp64 block
    _solve_and_check(g, H, S, nev, "SpGevSolver")
    assert g.get("device_bytes") < fp64_matrix
    # the sequence: H moves (factor = 0), then H and S move; each warm solve filters fewer vectors than a cold one
    for step in (1, 2):
        H2, S2 = R.solve_inputs(cplx, step)
        if step == 1:
            U_before = g.factor()
            g.update(H2)
            assert R.same_bits(g.factor(), U_before)                        # no second Cholesky
        else:
            g.update(H2, S2)
        Sk = S if step == 1 else S2
        warm = _solve_and_check(g, H2, Sk, nev, "SpGevSolver warm step %d" % step)
        c = SpGevSolver(gctx, H2, Sk, nev, nex)
        cold = c.solve()
        c.close()
        assert cold["locked"] >= nev
        print("step", step, "filtered vectors warm", warm["filtered_vecs"], "cold", cold["filtered_vecs"])
        assert warm["filtered_vecs"] < cold["filtered_vecs"], (step, warm, cold)
    g.close()


# ---- C interface -------------------------------------------------------------------------------------------------------------------
def test_plain_c_caller_of_the_single_precision_sequence(tmp_path):
    """examples/c_gev_sp.c: reduce -> cchase_ -> backtransform, then a second pencil with unchanged S (factor = 0, mode 'A'), from
    a C program; it checks its residuals itself and prints OK"""
    assert shutil.which("gcc") is not None
    exe, libdir = str(tmp_path / "c_gev_sp"), os.path.join(ROOT, "chase_amd", "lib")
    subprocess.run(["gcc", "-O2", "-std=c11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_gev_sp.c"),
                    "-L" + libdir, "-lchase_hip", "-Wl,-rpath," + libdir, "-lm", "-o", exe], check=True)
    p = subprocess.run([exe, "257"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("OK") and "FAILED" not in p.stdout, (p.stdout[-2000:], p.stderr[-2000:])
    assert "pencil 1 (mode A)" in p.stdout
