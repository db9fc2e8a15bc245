"""The generalized problem H x = lambda S x on the GPU - chase_hip_trsm_left_upper, chase_hip_potrf_upper_blocked,
chase_hip_hegst_upper (hegs2_diag at n <= 64), chase_hip_gev_reduce / _backtransform, GevSolver and the C interface - held against
the checkers of tests/gev_refs.py: componentwise bounds with factor 1 for the solve and the factorisation, 8 x LAPACK's measured
error for the two-sided reduction, the assembled a-priori bounds for whole solves.  Real and complex, every leading dimension
once tight and once padded by 3 rows of a canary that must survive bit for bit; the triangles the contracts call "never read"
hold NaN.  Sizes: one block, the 64-wide steps and their ragged rests, several outer blocks (outer_nb / nb = 128)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla

import gev_refs as G

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


def _run(ctx, fn, *bufs):
    """uploads the padded host buffers (the row count IS the leading dimension), calls fn(device arrays), downloads them all"""
    dev = [ctx.array(b) for b in bufs]
    rc = fn(*dev)
    out = [d.download() for d in dev]
    for d in dev:
        d.free()
    return rc, out


# ---- trsm_left_upper ---------------------------------------------------------------------------------------------------------------
@CPLX
@PAD
@pytest.mark.parametrize("op", ["N", "C"])
def test_trsm_left_upper_componentwise_bound(gctx, cplx, pad, op):
    """R: the reference factor of hpd(n, 1e5) with NaN in its strictly lower triangle - it is never read"""
    peak = 0.0
    for n in G.TRSM_N:
        for nrhs in G.TRSM_NRHS:
            R, B = G.trsm_inputs(n, nrhs, cplx)
            Rp, Bp = G.padded(G.nan_lower(R), n + pad), G.padded(B, n + pad)
            _, (Rout, Xp) = _run(gctx, lambda dR, dB: gctx.trsm_left_upper(op, n, nrhs, dR.ptr, dR.ld, dB.ptr, dB.ld, cplx), Rp, Bp)
            r = G.left_solve_ratio(Xp[:n], R, B, op)
            peak = max(peak, r)
            assert r <= 1, (n, nrhs, r)
            assert G.same_padding(Xp, n) and G.same_bits(Rout, Rp), (n, nrhs)
    print("trsm_left_upper largest ratio:", peak)


# ---- potrf_upper_blocked -----------------------------------------------------------------------------------------------------------
@CPLX
@PAD
@pytest.mark.parametrize("kappa", G.POTRF_KAPPAS)
def test_potrf_upper_blocked_bound_and_untouched_lower_triangle(gctx, cplx, pad, kappa):
    peak = 0.0
    for (n, ob) in G.POTRF_CASES:
        A = G.potrf_input(n, cplx, kappa)
        Ap = G.padded(G.nan_lower(A), n + pad)
        info, (Rp,) = _run(gctx, lambda dA: gctx.potrf_upper_blocked(n, dA.ptr, dA.ld, cplx, ob), Ap)
        assert info == 0, (n, ob, info)
        r = G.chol_ratio(A, Rp[:n])
        peak = max(peak, r)
        assert r <= 1, (n, ob, r)
        il = np.tril_indices(n, -1)
        assert G.same_bits(Rp[:n][il], Ap[:n][il]), (n, ob)                  # the NaN canary below the diagonal, bit for bit
        assert G.same_padding(Rp, n), (n, ob)
    print("potrf_upper_blocked largest ratio:", peak)


@CPLX
def test_potrf_upper_blocked_info_is_the_first_bad_pivot(gctx, cplx):
    for (n, ob, p) in ((200, 0, 70), (321, 128, 70), (321, 128, 200)):
        A = G.potrf_input(n, cplx, 10.0).copy()
        A[p - 1, p - 1] = -1.0                                             # indefinite at pivot p (1-based)
        info, _ = _run(gctx, lambda dA: gctx.potrf_upper_blocked(n, dA.ptr, dA.ld, cplx, ob), G.padded(G.nan_lower(A), n + 3))
        assert info == p, (n, ob, p, info)


# ---- hegs2_diag / hegst_upper ------------------------------------------------------------------------------------------------------
def _check_hegst(gctx, cplx, pad, cases):
    peak = 0.0
    for (n, nb) in cases:
        for kappa in G.HEGST_KAPPAS:
            A, U = G.hegst_inputs(n, cplx, kappa)
            Ap, Up = G.padded(G.nan_lower(A), n + pad), G.padded(G.nan_lower(U), n + pad)
            _, (Cp, Uout) = _run(gctx, lambda dA, dU: gctx.hegst_upper(n, dA.ptr, dA.ld, dU.ptr, dU.ld, cplx, nb), Ap, Up)
            r = G.hegst_ratio(A, U, Cp[:n])
            peak = max(peak, r)
            assert r <= 1, (n, nb, kappa, r)
            assert G.exactly_hermitian(Cp[:n]), (n, nb, kappa)
            assert G.same_padding(Cp, n) and G.same_bits(Uout, Up), (n, nb, kappa)
    print("hegst_upper largest ratio (error over 8 x LAPACK's):", peak)


@CPLX
@PAD
def test_hegs2_diag_one_block_exactly_hermitian(gctx, cplx, pad):
    _check_hegst(gctx, cplx, pad, [(n, 0) for n in G.HEGS2_SIZES])


@CPLX
@PAD
def test_hegst_upper_blocked_recurrence_exactly_hermitian(gctx, cplx, pad):
    _check_hegst(gctx, cplx, pad, G.HEGST_CASES)


# ---- gev_reduce / argument checks --------------------------------------------------------------------------------------------------
@CPLX
def test_gev_reduce_reports_the_pivot_and_leaves_A_alone(gctx, cplx):
    n, p = 200, 70
    A, _ = G.hegst_inputs(n, cplx, 10.0)
    S = G.potrf_input(n, cplx, 10.0).copy()
    S[p - 1, p - 1] = -1.0
    Ap = G.padded(G.nan_lower(A), n + 3)
    info, (Aout, _) = _run(gctx, lambda dA, dS: gctx.gev_reduce(n, dA.ptr, dA.ld, dS.ptr, dS.ld, cplx), Ap, G.padded(S, n + 3))
    assert info == p and G.same_bits(Aout, Ap)
    from chase_amd.capi import GevSolver, ChaseHipError
    with pytest.raises(ChaseHipError) as e:
        GevSolver(gctx, G.herm_full(A), np.asfortranarray(S), 8, 8)
    assert e.value.code == p and e.value.pivot == p


def test_bad_arguments_are_einval(gctx):
    from chase_amd.capi import lib
    d = gctx.empty((8, 8), np.float64)
    h, p = gctx.h, d.ptr
    assert lib.chase_hip_trsm_left_upper(h, 0, b"T", 4, 2, p, 8, p, 8) == EINVAL
    assert b"op must be" in lib.chase_hip_last_error()
    for args in ((4, 2, p, 3, p, 8), (4, 2, p, 8, p, 3), (-1, 2, p, 8, p, 8), (4, 2, None, 8, p, 8)):
        assert lib.chase_hip_trsm_left_upper(h, 0, b"N", *args) == EINVAL
    assert lib.chase_hip_potrf_upper_blocked(h, 0, 4, p, 3, 0) == EINVAL
    assert lib.chase_hip_potrf_upper_blocked(h, 0, 4, p, 8, 100) == EINVAL           # no multiple of 64
    assert lib.chase_hip_hegst_upper(h, 0, 4, p, 8, p, 3, 0) == EINVAL
    assert lib.chase_hip_hegst_upper(h, 0, 4, p, 8, p, 8, -64) == EINVAL
    assert lib.chase_hip_gev_reduce(h, 0, 4, p, 3, p, 8) == EINVAL
    assert lib.chase_hip_gev_backtransform(h, 0, 4, 2, p, 3, p, 8) == EINVAL
    assert lib.chase_hip_gev_backtransform(h, 0, 4, 2, p, 8, p, 3) == EINVAL
    assert lib.chase_hip_trsm_left_upper(h, 0, b"N", 0, 2, None, 0, None, 0) == 0    # empty operands are legal
    d.free()


# ---- whole solves ------------------------------------------------------------------------------------------------------------------
def _check_pairs(H, S, U, C, lam, X, rho, label):
    n = H.shape[0]
    r = G.gev_resid_ld(H, S, lam, X)
    wref = sla.eigh(H, S, eigvals_only=True)
    lmin, nC = sla.eigvalsh(S)[0], np.linalg.norm(C, 2)
    verr = G.value_errors(lam, wref)
    rb = np.array([G.gev_residual_bound(H, S, U, C, lam[j], X[:, j], rho[j]) for j in range(len(lam))])
    vb = np.array([G.gev_value_bound(r[j], lmin, n, nC) for j in range(len(lam))])
    print(label, "largest residual / bound:", float(np.max(r / rb)), "largest value error / bound:", float(np.max(verr / vb)),
          "largest residual:", float(np.max(r)))
    return r, rb, verr, vb


@CPLX
def test_gev_solver_whole_solve(gctx, cplx):
    from chase_amd.capi import GevSolver, Solver
    H, S = G.solve_inputs(cplx)
    n, nev, nex = G.SOLVE_N, G.SOLVE_NEV, G.SOLVE_NEX
    g = GevSolver(gctx, H, S, nev, nex)
    C, U = g.reduced(), np.triu(g.factor())                                # before the solve: its diagonal shifts work on C in place
    g.set(tol=G.SOLVE_TOL)
    st = g.solve()
    assert st["locked"] >= nev
    lam, X = g.eigenpairs()
    resid, rho = g.gev_residuals(), g.resid()[:nev]
    g.close()
    assert G.chol_ratio(S, U) <= 1 and G.hegst_ratio(H, U, C) <= 1 and G.exactly_hermitian(C)
    r, rb, verr, vb = _check_pairs(H, S, U, C, lam, X, rho, "GevSolver")
    assert np.all(resid <= rb), (resid, rb)                                 # the device's own residuals ...
    assert np.all(r <= rb) and np.all(verr <= vb)                           # ... and the long double ones, and the Ritz values
    assert G.orth_ratio(X, S, U) <= 1
    # the front end adds nothing to the iteration: a plain Solver on the downloaded reduced matrix takes the same path
    s = Solver(gctx, np.asfortranarray(C), nev, nex)
    s.set(tol=G.SOLVE_TOL)
    st2 = s.solve()
    s.close()
    assert (st2["iterations"], st2["filtered_vecs"]) == (st["iterations"], st["filtered_vecs"])


# ---- C interface -------------------------------------------------------------------------------------------------------------------
def test_plain_c_caller_of_the_generalized_sequence(tmp_path):
    """examples/c_gev.c: reduce -> dchase_init_ / dchase_ / dchase_finalize_ -> backtransform from a C program, on the real
    whole-solve input; every printed residual passes the assembled bound (rho: the long double residual of the pair it wrote
    out), and an indefinite S gives info > 0 with H unchanged (the program checks that itself and prints it)."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    exe, libdir = str(tmp_path / "c_gev"), os.path.join(ROOT, "chase_amd", "lib")
    subprocess.run(["gcc", "-O2", "-std=c11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_gev.c"),
                    "-L" + libdir, "-lchase_hip", "-Wl,-rpath," + libdir, "-lm", "-o", exe], check=True)
    H, S = G.solve_inputs(False)
    n, nev = G.SOLVE_N, G.SOLVE_NEV
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(H.tobytes(order="F")); f.write(S.tobytes(order="F"))
    p = subprocess.run([exe, str(n), fin, fout], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "C_GEV_OK" in p.stdout, (p.stdout[-2000:], p.stderr[-2000:])
    assert int(re.search(r"indefinite S: info = (-?\d+)", p.stdout).group(1)) > 0
    raw = np.fromfile(fout, dtype=np.float64)
    assert raw.size == nev + 2 * n * nev + 2 * n * n
    lam, rest = raw[:nev], raw[nev:]
    Y, X = (rest[i * n * nev:(i + 1) * n * nev].reshape((n, nev), order="F") for i in range(2))
    C, SU = (rest[2 * n * nev + i * n * n:2 * n * nev + (i + 1) * n * n].reshape((n, n), order="F") for i in range(2))
    U = np.triu(SU)
    assert G.same_bits(np.tril(SU, -1), np.tril(S, -1))                      # S becomes U in its upper triangle only
    assert G.chol_ratio(S, U) <= 1 and G.hegst_ratio(H, U, C) <= 1 and G.exactly_hermitian(C)
    rho = G.gev_resid_ld(C, np.eye(n), lam, Y)
    r, rb, verr, vb = _check_pairs(H, S, U, C, lam, X, rho, "c_gev")
    printed = np.array([float(m) for m in re.findall(r"\|\| H x - lambda S x \|\| = (\S+)", p.stdout)])
    assert printed.size == nev and np.all(printed <= rb)
    assert float(re.search(r"largest generalized residual (\S+)", p.stdout).group(1)) == pytest.approx(printed.max(), rel=1e-2)
    assert np.all(r <= rb) and np.all(verr <= vb)
