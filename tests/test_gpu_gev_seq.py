"""Sequences of generalized problems and itype 2 / 3 on the GPU - chase_hip_trmm_left_upper (trmm_diag inside),
chase_hip_hegst_product_upper, chase_hip_gev_reduce_itype / _backtransform_itype / _starttransform, GevSolver(itype=...),
GevSolver.update and the C interface - held against the checkers of tests/gev_seq_refs.py and tests/gev_refs.py: derived
componentwise bounds with factor 1 for the products, the assembled a-priori bounds for whole solves.  Real and complex, every
leading dimension once tight and once padded by 3 rows of a canary that must survive bit for bit; the triangles the contracts
call "never read" hold NaN.  Sizes: one block, the 64-row steps and their ragged rests, the 256-row block boundary crossed once
and with a ragged rest."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla

import gev_refs as G
import gev_seq_refs as Q

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


# ---- trmm_left_upper ---------------------------------------------------------------------------------------------------------------
@CPLX
@PAD
@pytest.mark.parametrize("op", ["N", "C"])
def test_trmm_left_upper_componentwise_bound(gctx, cplx, pad, op):
    """U: the reference factor of hpd(n, 1e5) with NaN in its strictly lower triangle - it is never read"""
    peak = 0.0
    for n in Q.TRMM_N:
        for ncols in Q.TRMM_NCOLS:
            U, X = Q.trmm_inputs(n, ncols, cplx)
            Up, Xp = G.padded(G.nan_lower(U), n + pad), G.padded(X, n + pad)
            _, (Uout, Yp) = _run(gctx, lambda dU, dX: gctx.trmm_left_upper(op, n, ncols, dU.ptr, dU.ld, dX.ptr, dX.ld, cplx), Up, Xp)
            r = Q.tri_product_ratio(Yp[:n], U, X, op)
            peak = max(peak, r)
            assert r <= 1, (n, ncols, r)
            assert G.same_padding(Yp, n) and G.same_bits(Uout, Up), (n, ncols)
    print("trmm_left_upper largest ratio:", peak)


@CPLX
@PAD
@pytest.mark.parametrize("op", ["N", "C"])
def test_trsm_after_trmm_returns_the_block(gctx, cplx, pad, op):
    """op(U)^{-1} (op(U) X) = X within the sum of the two derived bounds: a second, independent line on the in-place order"""
    for (n, ncols) in Q.ROUNDTRIP_CASES:
        U, X = Q.trmm_inputs(n, ncols, cplx)
        Up, Xp = G.padded(G.nan_lower(U), n + pad), G.padded(X, n + pad)
        got = {}

        def both(dU, dX):
            gctx.trmm_left_upper(op, n, ncols, dU.ptr, dU.ld, dX.ptr, dX.ld, cplx)
            got["Y"] = dX.download()
            gctx.trsm_left_upper(op, n, ncols, dU.ptr, dU.ld, dX.ptr, dX.ld, cplx)
        _, (_, Zp) = _run(gctx, both, Up, Xp)
        r = Q.roundtrip_ratio(Zp[:n], X, U, got["Y"][:n], op)
        print("round trip", n, ncols, op, "ratio", r)
        assert r <= 1, (n, ncols, r)
        assert G.same_padding(Zp, n)


# ---- hegst_product_upper -----------------------------------------------------------------------------------------------------------
@CPLX
@PAD
def test_hegst_product_upper_bound_and_exactly_hermitian(gctx, cplx, pad):
    peak = 0.0
    for n in Q.HEGSTP_N:
        for kappa in Q.HEGSTP_KAPPAS:
            A, U = G.hegst_inputs(n, cplx, kappa)
            Ap, Up = G.padded(G.nan_lower(A), n + pad), G.padded(G.nan_lower(U), n + pad)
            _, (Cp, Uout) = _run(gctx, lambda dA, dU: gctx.hegst_product_upper(n, dA.ptr, dA.ld, dU.ptr, dU.ld, cplx), Ap, Up)
            r = Q.product_reduction_ratio(A, U, Cp[:n])
            peak = max(peak, r)
            assert r <= 1, (n, kappa, r)
            assert G.exactly_hermitian(Cp[:n]), (n, kappa)
            assert G.same_padding(Cp, n) and G.same_bits(Uout, Up), (n, kappa)
    print("hegst_product_upper largest ratio:", peak)


# ---- drivers -----------------------------------------------------------------------------------------------------------------------
@CPLX
def test_reduce_itype_1_is_gev_reduce_and_factor_0_is_the_two_sided_step(gctx, cplx):
    n = 200
    A, _ = G.hegst_inputs(n, cplx, 10.0)
    S = G.potrf_input(n, cplx, 10.0)
    Ap, Sp = G.padded(G.nan_lower(A), n + 3), G.padded(G.nan_lower(S), n + 3)
    i0, (C0, U0) = _run(gctx, lambda dA, dS: gctx.gev_reduce(n, dA.ptr, dA.ld, dS.ptr, dS.ld, cplx), Ap, Sp)
    for itype in (1, 2, 3):
        i1, (C1, U1) = _run(gctx, lambda dA, dS: gctx.gev_reduce_itype(itype, 1, n, dA.ptr, dA.ld, dS.ptr, dS.ld, cplx), Ap, Sp)
        assert i0 == 0 and i1 == 0 and G.same_bits(U1, U0)
        if itype == 1:
            assert G.same_bits(C1, C0)
        else:
            assert Q.product_reduction_ratio(G.herm_full(A), U1[:n], C1[:n]) <= 1 and G.exactly_hermitian(C1[:n])
        i2, (C2, U2) = _run(gctx, lambda dA, dS: gctx.gev_reduce_itype(itype, 0, n, dA.ptr, dA.ld, dS.ptr, dS.ld, cplx), Ap, U1)
        assert i2 == 0 and G.same_bits(C2, C1) and G.same_bits(U2, U1), itype
    # S not positive definite: the pivot, A untouched
    Sbad = S.copy(); Sbad[69, 69] = -1.0
    info, (Aout, _) = _run(gctx, lambda dA, dS: gctx.gev_reduce_itype(2, 1, n, dA.ptr, dA.ld, dS.ptr, dS.ld, cplx), Ap, G.padded(Sbad, n + 3))
    assert info == 70 and G.same_bits(Aout, Ap)


@CPLX
@PAD
@pytest.mark.parametrize("itype", [1, 2, 3])
def test_starttransform_then_backtransform_returns_the_block(gctx, cplx, pad, itype):
    for (n, ncols) in Q.ROUNDTRIP_CASES:
        U, X = Q.trmm_inputs(n, ncols, cplx)
        Up, Xp = G.padded(G.nan_lower(U), n + pad), G.padded(X, n + pad)
        got = {}

        def both(dU, dX):
            gctx.gev_starttransform(itype, n, ncols, dU.ptr, dU.ld, dX.ptr, dX.ld, cplx)
            got["Y"] = dX.download()
            gctx.gev_backtransform_itype(itype, n, ncols, dU.ptr, dU.ld, dX.ptr, dX.ld, cplx)
        _, (Uout, Zp) = _run(gctx, both, Up, Xp)
        Y = got["Y"][:n]
        if itype == 3:            # U^{-H} then U^H
            assert G.left_solve_ratio(Y, U, X, "C") <= 1, (n, ncols)
            r = Q.solve_then_product_ratio(Zp[:n], X, U, Y, "C")
        else:                     # U then U^{-1}
            assert Q.tri_product_ratio(Y, U, X, "N") <= 1, (n, ncols)
            r = Q.roundtrip_ratio(Zp[:n], X, U, Y, "N")
        assert r <= 1, (n, ncols, r)
        assert G.same_padding(Zp, n) and G.same_bits(Uout, Up)


def test_bad_arguments_are_einval(gctx):
    from chase_amd.capi import lib
    d = gctx.empty((8, 8), np.float64)
    h, p = gctx.h, d.ptr
    assert lib.chase_hip_trmm_left_upper(h, 0, b"T", 4, 2, p, 8, p, 8) == EINVAL
    assert b"op must be" in lib.chase_hip_last_error()
    for args in ((4, 2, p, 3, p, 8), (4, 2, p, 8, p, 3), (-1, 2, p, 8, p, 8), (4, -2, p, 8, p, 8), (4, 2, None, 8, p, 8), (4, 2, p, 8, None, 8)):
        assert lib.chase_hip_trmm_left_upper(h, 0, b"N", *args) == EINVAL
    assert lib.chase_hip_hegst_product_upper(h, 0, 4, p, 3, p, 8) == EINVAL
    assert lib.chase_hip_hegst_product_upper(h, 0, 4, p, 8, p, 3) == EINVAL
    assert lib.chase_hip_hegst_product_upper(h, 0, 4, None, 8, p, 8) == EINVAL
    for itype in (0, 4, -1):
        assert lib.chase_hip_gev_reduce_itype(h, 0, itype, 1, 4, p, 8, p, 8) == EINVAL
        assert lib.chase_hip_gev_backtransform_itype(h, 0, itype, 4, 2, p, 8, p, 8) == EINVAL
        assert lib.chase_hip_gev_starttransform(h, 0, itype, 4, 2, p, 8, p, 8) == EINVAL
    assert b"itype must be" in lib.chase_hip_last_error()
    assert lib.chase_hip_gev_reduce_itype(h, 0, 2, 2, 4, p, 8, p, 8) == EINVAL            # factor outside 0 / 1
    assert lib.chase_hip_gev_reduce_itype(h, 0, 2, 1, 4, p, 3, p, 8) == EINVAL
    assert lib.chase_hip_gev_reduce_itype(h, 0, 2, 1, 4, p, 8, None, 8) == EINVAL
    for f in (lib.chase_hip_gev_backtransform_itype, lib.chase_hip_gev_starttransform):
        assert f(h, 0, 3, 4, 2, p, 3, p, 8) == EINVAL
        assert f(h, 0, 3, 4, 2, p, 8, p, 3) == EINVAL
        assert f(h, 0, 3, 4, 2, None, 8, p, 8) == EINVAL
        assert f(h, 0, 3, 0, 2, None, 0, None, 0) == 0                                  # empty operands are legal
    assert lib.chase_hip_trmm_left_upper(h, 0, b"N", 0, 2, None, 0, None, 0) == 0
    assert lib.chase_hip_trmm_left_upper(h, 0, b"C", 4, 0, None, 4, None, 4) == 0
    assert lib.chase_hip_hegst_product_upper(h, 0, 0, None, 0, None, 0) == 0
    d.free()


# ---- whole solves ------------------------------------------------------------------------------------------------------------------
def _check_itype1(H, S, U, C, lam, X, rho, resid, label):
    """the assembled residual, value and S-orthonormality checks of test_gev_solver_whole_solve"""
    n = H.shape[0]
    assert G.chol_ratio(S, U) <= 1 and G.hegst_ratio(H, U, C) <= 1 and G.exactly_hermitian(C)
    r = G.gev_resid_ld(H, S, lam, X)
    wref = sla.eigh(H, S, eigvals_only=True)
    lmin, nC = sla.eigvalsh(S)[0], np.linalg.norm(C, 2)
    verr = G.value_errors(lam, wref)
    rb = np.array([G.gev_residual_bound(H, S, U, C, lam[j], X[:, j], rho[j]) for j in range(len(lam))])
    vb = np.array([G.gev_value_bound(r[j], lmin, n, nC) for j in range(len(lam))])
    print(label, "largest residual / bound:", float(np.max(r / rb)), "largest value error / bound:", float(np.max(verr / vb)),
          "largest residual:", float(np.max(r)))
    assert np.all(resid <= rb), (resid, rb)
    assert np.all(r <= rb) and np.all(verr <= vb)
    assert G.orth_ratio(X, S, U) <= 1


def _warm_step(gctx, g, H, S, cplx, label, with_s):
    """update -> solve on g; checks (a) the pairs, (b) that a plain Solver from the same start takes the same path, (c) that
    the warm solve filters fewer vectors than a cold one.  Returns the warm stats."""
    from chase_amd.capi import GevSolver, Solver
    nev, nex = G.SOLVE_NEV, G.SOLVE_NEX
    g.update(H, S if with_s else None)
    C, U = g.reduced(), np.triu(g.factor())
    V0, rv = g.start_vectors(), g.ritzv.copy()
    st = g.solve()
    assert st["locked"] >= nev
    lam, X = g.eigenpairs()
    _check_itype1(H, S, U, C, lam, X, g.resid()[:nev], g.gev_residuals(), label)                       # (a)
    s = Solver(gctx, np.asfortranarray(C), nev, nex, V=V0.copy(order="F"))
    s.ritzv[:] = rv
    s.set(tol=G.SOLVE_TOL, approx=1)
    st2 = s.solve()
    s.close()
    assert (st2["iterations"], st2["filtered_vecs"]) == (st["iterations"], st["filtered_vecs"])        # (b)
    c = GevSolver(gctx, H, S, nev, nex)
    c.set(tol=G.SOLVE_TOL)
    stc = c.solve()
    c.close()
    print(label, "warm:", st["iterations"], "iterations,", st["filtered_vecs"], "filtered vectors; cold:", stc["iterations"], ",",
          stc["filtered_vecs"])
    assert st["filtered_vecs"] < stc["filtered_vecs"]                                                  # (c)
    return st


@CPLX
def test_gev_solver_warm_sequence(gctx, cplx):
    from chase_amd.capi import GevSolver
    H0, S0 = G.solve_inputs(cplx)
    H1, S1 = Q.perturbed_pencil(H0, S0, 25, cplx)
    H2, _ = Q.perturbed_pencil(H1, S1, 26, cplx, with_s=False)
    g = GevSolver(gctx, H0, S0, G.SOLVE_NEV, G.SOLVE_NEX)
    g.set(tol=G.SOLVE_TOL)
    assert g.solve()["locked"] >= G.SOLVE_NEV
    _warm_step(gctx, g, H1, S1, cplx, "S changed", True)
    block, fac = g.solver.V.copy(order="F"), g.factor()
    g.update(H2)                                                   # the same update _warm_step repeats: it changes nothing twice
    assert G.same_bits(g.start_vectors(), block) and G.same_bits(g.factor(), fac)
    _warm_step(gctx, g, H2, S1, cplx, "S unchanged", False)
    assert G.same_bits(g.factor(), fac)
    g.close()


def _check_itype23(itype, H, S, U, C, lam, X, rho, resid, label):
    n = H.shape[0]
    assert G.chol_ratio(S, U) <= 1 and Q.product_reduction_ratio(G.herm_full(H), U, C) <= 1 and G.exactly_hermitian(C)
    r = Q.pencil_resid_ld(itype, H, S, lam, X)
    wref = sla.eigh(H, S, type=itype, eigvals_only=True)
    nC = np.linalg.norm(C, 2)
    verr = G.value_errors(lam, wref)
    rb = np.array([Q.gev_residual_bound_itype(itype, H, S, U, C, lam[j], X[:, j], rho[j]) for j in range(len(lam))])
    vb = np.array([Q.gev_value_bound_itype(itype, r[j], X[:, j], S, n, nC) for j in range(len(lam))])
    print(label, "largest residual / bound:", float(np.max(r / rb)), "largest value error / bound:", float(np.max(verr / vb)),
          "largest residual:", float(np.max(r)))
    assert np.all(resid <= rb), (resid, rb)
    assert np.all(r <= rb) and np.all(verr <= vb)
    assert Q.orth_ratio_itype(itype, X, S, U) <= 1


@CPLX
@pytest.mark.parametrize("itype", [2, 3])
def test_gev_solver_itype_2_and_3(gctx, cplx, itype):
    from chase_amd.capi import GevSolver
    H, S = G.solve_inputs(cplx)
    nev, nex = G.SOLVE_NEV, G.SOLVE_NEX
    g = GevSolver(gctx, H, S, nev, nex, itype=itype)
    C, U = g.reduced(), np.triu(g.factor())
    g.set(tol=G.SOLVE_TOL)
    st = g.solve()
    assert st["locked"] >= nev
    lam, X = g.eigenpairs()
    _check_itype23(itype, H, S, U, C, lam, X, g.resid()[:nev], g.gev_residuals(), "itype %d cold" % itype)
    if itype == 3:                                                 # one warm update: the U^{-H} start transform end to end
        H1, S1 = Q.perturbed_pencil(H, S, 25, cplx)
        g.update(H1, S1)
        C1, U1 = g.reduced(), np.triu(g.factor())
        st1 = g.solve()
        assert st1["locked"] >= nev
        lam1, X1 = g.eigenpairs()
        _check_itype23(itype, H1, S1, U1, C1, lam1, X1, g.resid()[:nev], g.gev_residuals(), "itype 3 warm")
        print("itype 3 cold:", st["filtered_vecs"], "warm:", st1["filtered_vecs"], "filtered vectors")
        assert st1["filtered_vecs"] < st["filtered_vecs"]
    g.close()


# ---- C interface -------------------------------------------------------------------------------------------------------------------
def test_plain_c_caller_of_a_warm_started_sequence(tmp_path):
    """examples/c_gev_sequence.c: three pencils, the first cold, the others from the previous vectors through
    dchase_gev_starttransform_ and mode 'A'; every printed residual passes the assembled bound (rho: the long double residual of
    the pair it wrote out) and every warm step prints fewer filtered vectors than the cold first one."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    exe, libdir = str(tmp_path / "c_gev_sequence"), os.path.join(ROOT, "chase_amd", "lib")
    subprocess.run(["gcc", "-O2", "-std=c11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_gev_sequence.c"),
                    "-L" + libdir, "-lchase_hip", "-Wl,-rpath," + libdir, "-lm", "-o", exe], check=True)
    H0, S0 = G.solve_inputs(False)
    H1, S1 = Q.perturbed_pencil(H0, S0, 25, False)
    H2, S2 = Q.perturbed_pencil(H1, S1, 26, False)
    pencils = [(H0, S0), (H1, S1), (H2, S2)]
    n, nev = G.SOLVE_N, G.SOLVE_NEV
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        for (H, S) in pencils:
            f.write(H.tobytes(order="F")); f.write(S.tobytes(order="F"))
    p = subprocess.run([exe, str(n), fin, fout], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "C_GEV_SEQUENCE_OK" in p.stdout, (p.stdout[-2000:], p.stderr[-2000:])
    raw = np.fromfile(fout, dtype=np.float64)
    per = nev + 2 * n * nev + 2 * n * n
    assert raw.size == 3 * per
    filt = [int(m) for m in re.findall(r"step \d \(mode .\): (\d+) filtered vectors", p.stdout)]
    assert len(filt) == 3 and all(0 < w < filt[0] for w in filt[1:]), filt
    for k, (H, S) in enumerate(pencils):
        blk = raw[k * per:(k + 1) * per]
        lam, rest = blk[:nev], blk[nev:]
        Y, X = (rest[i * n * nev:(i + 1) * n * nev].reshape((n, nev), order="F") for i in range(2))
        C, SU = (rest[2 * n * nev + i * n * n:2 * n * nev + (i + 1) * n * n].reshape((n, n), order="F") for i in range(2))
        U = np.triu(SU)
        rho = G.gev_resid_ld(C, np.eye(n), lam, Y)
        printed = np.array([float(m) for m in re.findall(r"step %d pair \d+: .* \|\| H x - lambda S x \|\| = (\S+)" % k, p.stdout)])
        assert printed.size == nev
        _check_itype1(H, S, U, C, lam, X, rho, printed, "c_gev_sequence step %d" % k)
