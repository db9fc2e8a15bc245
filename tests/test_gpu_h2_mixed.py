"""The pseudo-Hermitian solver's opt-in fp32 H^2 filter (h2_mixed_precision) on the GPU: chase_hip_axpy_sp against its
componentwise bound, the switch at operator level (what enters fp32, what never does, the counters, the bound propagated through
product - product - axpy), whole solves with the key off and on against the fixtures' spectra and the CPU emulation of
tests/h2_mixed_ref.py, and the refusals of every other solver.

Bounds, u = 2^-24.  A product: (N + 8) u real / (2 N + 16) u complex times |alpha| |A| |B| + |beta| |C0|, the bound
tests/test_gpu_mixed_precision.py derives and checks for the fp32 MFMA kernels.  The axpy: tests/h2_mixed_ref.py; for a complex
element the modulus of the error is at most sqrt(2) times the larger component bound, which is at most
3u / (1 - 3u) (|gamma| |x| + |y|)."""
import os
import sys

import numpy as np
import pytest
from conftest import REF_FIX, read_ref_matrix

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import h2_mixed_ref as R  # noqa: E402
from rank_threads import run_ranks  # noqa: E402

pytestmark = pytest.mark.gpu
U = R.U
SP_KEYS = ("hemm_sp_calls", "hemm_sp_vecs", "sp_filters", "sp_h_converts")
STAT_KEYS = ("iterations", "filtered_vecs", "lanczos_vecs", "locked", "lowerb", "upperb", "lambda_")


# ---- 1. axpy_sp -----------------------------------------------------------------------------------------------------------------

def _operands(m, n, ld, cplx, seed=3):
    rng = np.random.default_rng(seed)
    st = np.complex64 if cplx else np.float32
    scale = 10.0 ** rng.integers(-4, 4, (ld, n))
    X = rng.standard_normal((ld, n)) * scale
    Y = rng.standard_normal((ld, n)) * scale
    if cplx:
        X = X + 1j * rng.standard_normal((ld, n)) * scale
        Y = Y + 1j * rng.standard_normal((ld, n))
    X, Y = np.asfortranarray(X.astype(st)), np.asfortranarray(Y.astype(st))
    X[m:] = np.nan                                   # rows >= m of a column: never read ...
    Y[m:] = st(-7.5)                                 # ... and never written (the sentinel keeps its bytes)
    return X, Y


# m = 133, n = 5: guarded elements (ld 133) and the 16-byte path with a rest (ld 136: 133 = 4 * 33 + 1 floats, 266 = 4 * 66 + 2);
# 2050 x 3: more than one block along a column
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("m,n,ld", [(133, 5, 133), (133, 5, 136), (2050, 3, 2052)], ids=["ld133", "ld136-16B", "2050-16B"])
def test_axpy_sp_within_the_componentwise_bound(ctx, cplx, m, n, ld):
    st = np.complex64 if cplx else np.float32
    X, Y = _operands(m, n, ld, cplx)
    dX, dY = ctx.empty((ld, n), st).upload(X), ctx.empty((ld, n), st)
    try:
        for gamma in ([-0.2, 1.75] if not cplx else [-0.2, 0.3 - 0.7j]):
            dY.upload(Y)
            ctx.axpy_sp(m, n, gamma, dX.ptr, ld, dY.ptr, ld, cplx)
            got = dY.download()
            assert dX.download().tobytes() == X.tobytes()                       # X is bitwise unchanged
            assert got[m:].tobytes() == Y[m:].tobytes()                         # the pad keeps its bytes
            assert np.all(np.isfinite(got[:m]))
            worst = R.axpy_sp_within_bound(gamma, X[:m], Y[:m], got[:m])
            print(f"axpy_sp {'c' if cplx else 's'} {m}x{n} ld {ld} gamma={gamma}: max err / bound = {worst:.3f}")
            assert worst <= 1.0
            assert got[:m].tobytes() != Y[:m].tobytes()
    finally:
        dX.free(); dY.free()


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_axpy_sp_empty_extents_and_bad_shapes(ctx, cplx):
    from chase_amd.capi import ChaseHipError
    st = np.complex64 if cplx else np.float32
    m, n, ld = 133, 5, 136
    X, Y = _operands(m, n, ld, cplx)
    dX, dY = ctx.empty((ld, n), st).upload(X), ctx.empty((ld, n), st).upload(Y)
    try:
        ctx.axpy_sp(m, 0, 1.5, dX.ptr, ld, dY.ptr, ld, cplx)                    # n = 0
        ctx.axpy_sp(0, n, 1.5, dX.ptr, ld, dY.ptr, ld, cplx)                    # m = 0
        assert dY.download().tobytes() == Y.tobytes() and dX.download().tobytes() == X.tobytes()
        with pytest.raises(ChaseHipError) as e:
            ctx.axpy_sp(m, n, 1.5, dX.ptr, m - 1, dY.ptr, ld, cplx)
        assert e.value.code == -1001 and "axpy_sp" in str(e.value)
    finally:
        dX.free(); dY.free()


# ---- 2. operator level ----------------------------------------------------------------------------------------------------------

NEV, NEX, LOCKED = 12, 8, 3
NE = NEV + NEX
STEPS = [(1e-3, 0.0, -0.2, 0), (2e-3, -0.3, -0.4, 0), (2e-3, -0.25, -0.4, 3)]     # tests/test_gpu_pseudo.py


@pytest.fixture(scope="module")
def matrices(ctx):
    return {"complex-fixture": read_ref_matrix("cdouble_random_BSE.bin", 200, 200, True),
            "real-fixture": read_ref_matrix("double_random_BSE.bin", 200, 200, False),
            # N = 202 is no multiple of 4: the shadows' leading dimension is padded to 204, tile edges in both directions
            "bse202": np.asfortranarray(ctx.gen_bse(202, True, dmin=1.0, dmax=11.0, offdiag=1e-3, seed=7).download())}


def _set_resid(s, value):
    """the buffer the driver writes its residuals into (chase_hip_solver_resid)"""
    from chase_amd.capi import lib
    p = lib.chase_hip_solver_resid(s.h)
    np.ctypeslib.as_array(p, shape=(s.ncol,))[:] = value


def _bracketed_steps(s, steps):
    s.FilterPhaseStart()
    for (a, b, g, off) in steps:
        s.HEMM_H2(NE, a, b, g, off)
    if len(steps) % 2:
        s.HEMM_H2(0, 0, 0, 0, 0)                                                  # even number of swaps
    s.FilterPhaseEnd()


def _h2_leg(ctx, H, key, resid, again=False):
    """Start, initVecs, QR, Lock(3), residuals := resid, one bracketed filter call of STEPS (again: and a second, shorter one)"""
    from chase_amd.capi import PseudoSolver
    N, cplx = H.shape[0], bool(np.iscomplexobj(H))
    dH = ctx.array(H)
    s = PseudoSolver(ctx, None, NEV, NEX, h_on_device_ptr=dH.ptr, N=N, cplx=cplx)
    if key is not None:
        s.set(h2_mixed_precision=key)
    s.Start(); s.initVecs(True); s.QR(0, 1.0); s.Lock(LOCKED)
    _set_resid(s, resid)
    V0 = s.peek_v()
    h0 = ctx.hash64(dH.ptr, N, N, N, cplx)
    _bracketed_steps(s, STEPS)
    out = dict(V0=V0, V=s.peek_v(), h0=h0, h1=ctx.hash64(dH.ptr, N, N, N, cplx), dp=s.get("hemm_calls"),
               **{k: s.get(k) for k in SP_KEYS})
    if again:
        _bracketed_steps(s, STEPS[:2])
        out["again"] = dict(dp=s.get("hemm_calls"), **{k: s.get(k) for k in SP_KEYS})
        s.set(reset_counters=1)
        out["reset"] = dict(dp=s.get("hemm_calls"), **{k: s.get(k) for k in SP_KEYS})
    s.close()
    dH.free()
    return out


def _h2_reference(H, V0):
    """STEPS (and the zero-column call) in fp64 on the fp32-rounded operands, with the bound of the fp32 evaluation propagated
    through product, product and axpy of every step.  Returns (columns [LOCKED, NE) of V1 at the end, their bounds)."""
    cplx = bool(np.iscomplexobj(H))
    st, wide = (np.complex64, np.complex128) if cplx else (np.float32, np.float64)
    N = H.shape[0]
    Hs = H.astype(st).astype(wide)
    aH = np.abs(Hs)
    g = ((2 * N + 16) if cplx else (N + 8)) * U
    ga = np.sqrt(2.0) * 3 * U / (1 - 3 * U) if cplx else 2 * U / (1 - 2 * U)
    X1 = V0[:, :NE].astype(st).astype(wide)
    X2 = X1.copy()                       # V2 = V1 after QR(0, .) (and the first step, beta = 0, does not read it)
    E1, E2 = np.zeros((N, NE)), np.zeros((N, NE))
    for (a, b, gm, off) in STEPS:
        a, b, gm = (float(np.float32(v)) for v in (a, b, gm))                    # what the kernels are given
        sl = slice(LOCKED + off, NE)
        x, ex = X1[:, sl], E1[:, sl]
        T = Hs @ x
        eT = g * (aH @ (np.abs(x) + ex)) + aH @ ex
        Y = a * (Hs @ T)
        eY = g * abs(a) * (aH @ (np.abs(T) + eT)) + abs(a) * (aH @ eT)
        if b != 0:
            Y = Y + b * X2[:, sl]
            eY = eY + g * abs(b) * (np.abs(X2[:, sl]) + E2[:, sl]) + abs(b) * E2[:, sl]
        Z = Y + gm * x
        eZ = ga * (abs(gm) * (np.abs(x) + ex) + np.abs(Y) + eY) + eY + abs(gm) * ex
        X2[:, sl], E2[:, sl] = Z, eZ
        X1, X2, E1, E2 = X2, X1, E2, E1
    if len(STEPS) % 2:
        X1, X2, E1, E2 = X2, X1, E2, E1
    return X1[:, LOCKED:], E1[:, LOCKED:]


@pytest.mark.parametrize("name", ["complex-fixture", "real-fixture", "bse202"])
def test_switch_at_operator_level(ctx, matrices, name):
    H = matrices[name]
    cplx = bool(np.iscomplexobj(H))
    st, wide = (np.complex64, np.complex128) if cplx else (np.float32, np.float64)
    r = _h2_leg(ctx, H, 1, 1.0, again=True)
    V0, V = r["V0"], r["V"]
    assert V[:, :LOCKED].tobytes() == V0[:, :LOCKED].tobytes()                   # locked columns: never touched
    assert V[:, NE:].tobytes() == V0[:, NE:].tobytes()                           # nor any column of the second half
    F = V[:, LOCKED:NE]
    assert np.array_equal(F, F.astype(st).astype(wide))                          # the filtered ones came back from fp32
    assert r["h0"] == r["h1"]                                                    # H never moves
    ncols = [NE - LOCKED - off for (_, _, _, off) in STEPS]
    assert r["hemm_sp_calls"] == 6 and r["dp"] == 0 and r["sp_filters"] == 1 and r["sp_h_converts"] == 1
    assert r["hemm_sp_vecs"] == sum(2 * c for c in ncols) == 96
    # a second bracketed call on the same solver: H is not converted again
    assert r["again"]["sp_h_converts"] == 1 and r["again"]["sp_filters"] == 2 and r["again"]["hemm_sp_calls"] == 10
    assert r["again"]["dp"] == 0
    assert all(v == 0 for v in r["reset"].values())                              # reset_counters clears sp_h_converts too
    want, bound = _h2_reference(H, V0)
    err = np.abs(F - want)
    assert np.all(bound > 0)
    print(f"operator level {name}: max err / bound = {np.max(err / bound):.2e}, max |V| = {np.max(np.abs(F)):.3e}")
    assert np.all(err <= bound)
    # below the threshold nothing runs in fp32, and the bits are those of a solver that was never told about the key
    lo = _h2_leg(ctx, H, 1, 1e-4)
    off = _h2_leg(ctx, H, None, 1e-4)
    assert lo["hemm_sp_calls"] == 0 and lo["sp_filters"] == 0 and lo["sp_h_converts"] == 0 and lo["dp"] == 6
    assert lo["V"].tobytes() == off["V"].tobytes()
    assert off["dp"] == 6 and all(off[k] == 0 for k in SP_KEYS)
    # key = 0 is a solver without the key, whatever the residuals
    zero = _h2_leg(ctx, H, 0, 1.0)
    assert zero["V"].tobytes() == off["V"].tobytes() and zero["dp"] == 6 and all(zero[k] == 0 for k in SP_KEYS)
    assert not np.array_equal(lo["V"][:, LOCKED:NE], F)                          # (the two paths do differ)


# ---- 3. whole solves ------------------------------------------------------------------------------------------------------------

def _solve_case(ctx, name):
    if name == "complex-fixture":
        H = read_ref_matrix("cdouble_random_BSE.bin", 200, 200, True)
        eigs = np.fromfile(os.path.join(REF_FIX, "eigs_cdouble_random_BSE.bin"), dtype=np.complex128).real
        return H, np.sort(eigs[eigs > 0]), 20, 20, dict(tol=1e-10, deg=20, opt=1, maxiter=25, numlanczos=10, lanczositer=50), "complex"
    if name == "real-fixture":
        H = read_ref_matrix("double_random_BSE.bin", 200, 200, False)
        eigs = np.fromfile(os.path.join(REF_FIX, "eigs_double_random_BSE.bin"), dtype=np.float64)
        return H, np.sort(eigs[eigs > 0]), 20, 20, dict(tol=1e-10, numlanczos=10, lanczositer=50), "real"
    H = np.asfortranarray(ctx.gen_bse(400, True, dmin=1.0, dmax=11.0, offdiag=1e-3, seed=7).download())
    ev = np.linalg.eigvals(H).real
    return H, np.sort(ev[ev > 0]), 16, 10, dict(tol=1e-10, numlanczos=10, lanczositer=50), None


@pytest.mark.parametrize("name", ["complex-fixture", "real-fixture", "bse400"])
def test_whole_solve_off_and_on(ctx, name):
    from chase_amd.capi import PseudoSolver
    H, pos, nev, nex, settings, kind = _solve_case(ctx, name)
    plain = PseudoSolver(ctx, H, nev, nex)                    # never heard of the key
    plain.set(**settings)
    st_plain = plain.solve()
    lam_plain = plain.ritzv.copy()
    plain.close()

    s = PseudoSolver(ctx, H, nev, nex)
    s.set(h2_mixed_precision=0, **settings)
    assert s.get("h2_mixed_precision") == 0
    st_off = s.solve()
    assert all(s.get(k) == 0 for k in SP_KEYS) and s.get("hemm_calls") > 0
    assert {k: st_off[k] for k in STAT_KEYS} == {k: st_plain[k] for k in STAT_KEYS}
    assert s.ritzv.tobytes() == lam_plain.tobytes()

    s.set(h2_mixed_precision=1, reset_counters=1)
    assert s.get("h2_mixed_precision") == 1 and s.get("mixed_precision") == 0
    st_on = s.solve()
    lam = s.ritzv[:nev].copy()
    resid = s.resid()[:nev]
    V = s.V[:, :nev]
    r_host = np.linalg.norm(H @ V - V * lam[None, :], axis=0)
    print(f"{name} {nev}/{nex}: fp64 {st_off['iterations']} iterations / {st_off['filtered_vecs']} filtered vectors, mixed "
          f"{st_on['iterations']} / {st_on['filtered_vecs']}, {int(s.get('hemm_sp_calls'))} fp32 and {int(s.get('hemm_calls'))} fp64 "
          f"filter products, {int(s.get('sp_filters'))} filter calls in fp32, max residual {np.max(resid):.2e}, host "
          f"{np.max(r_host):.2e}, eigenvalue error {np.max(np.abs(np.sort(lam) - pos[:nev])):.2e}")
    assert st_on["locked"] >= nev
    assert np.all(np.isfinite(lam)) and np.max(resid) <= 1e-10
    assert np.max(r_host) <= 1e-10
    assert np.max(np.abs(np.sort(lam) - pos[:nev])) <= 1e-9
    assert s.get("sp_filters") >= 1 and s.get("hemm_sp_calls") > 0 and s.get("hemm_calls") > 0       # into fp32 and back out
    assert s.get("sp_h_converts") == 1
    assert st_on["iterations"] <= st_off["iterations"] + 1
    if kind is not None:
        emu = R.emulated(kind, nev, nex)["mixed"]
        print(f"  CPU emulation: {emu['iterations']} iterations / {emu['filtered_vecs']} filtered vectors")
        assert abs(st_on["iterations"] - emu["iterations"]) <= 1
    s.set(reset_counters=1)
    assert all(s.get(k) == 0 for k in SP_KEYS)
    s.close()


# ---- 4. refusals and inertness --------------------------------------------------------------------------------------------------

def _bse64(ctx):
    return np.asfortranarray(ctx.gen_bse(64, True, dmin=1.0, dmax=11.0, offdiag=1e-3, seed=7).download())


def test_key_values_and_hermitian_refusal(ctx):
    from chase_amd.capi import ChaseHipError, PseudoSolver, Solver
    from oracle import chase_oracle as O
    s = Solver(ctx, O.clement(64, False), 4, 4)
    assert s.get("h2_mixed_precision") == 0 and s.get("sp_h_converts") == 0
    with pytest.raises(ChaseHipError) as e:
        s.set(h2_mixed_precision=1)
    assert e.value.code == -1001 and "h2_mixed_precision" in str(e.value)
    s.set(h2_mixed_precision=0)
    assert s.get("h2_mixed_precision") == 0
    s.FilterPhaseStart(); s.FilterPhaseEnd()                   # the bracket is valid for every solver kind
    s.close()
    p = PseudoSolver(ctx, _bse64(ctx), 4, 4)
    assert p.get("h2_mixed_precision") == 0
    p.set(h2_mixed_precision=1)
    assert p.get("h2_mixed_precision") == 1 and p.get("mixed_precision") == 0          # a key of its own
    for bad in (2, -1, 0.5):
        with pytest.raises(ChaseHipError) as e:
            p.set(h2_mixed_precision=bad)
        assert e.value.code == -1001 and "h2_mixed_precision" in str(e.value)
    assert p.get("h2_mixed_precision") == 1
    p.set(h2_mixed_precision=0)
    assert p.get("h2_mixed_precision") == 0
    p.close()


def _scenario_grid_refuses(ctx, grid, comm, N, pseudo):
    from chase_amd import dist as cd
    from chase_amd.capi import ChaseHipError
    rl, cl = cd.Layout(N, 0, grid.nprow), cd.Layout(N, 0, grid.npcol)
    if pseudo:
        dH = cd.gen_bse_local(ctx, N, True, rl, cl, grid.myrow, grid.mycol, dmin=1.0, dmax=11.0, offdiag=1e-3, seed=7)
        s = cd.DistPseudoSolver(ctx, grid, dH, N, 4, 4, True, 0, 0)
    else:
        dH = cd.gen_clement_local(ctx, N, False, rl, cl, grid.myrow, grid.mycol)
        s = cd.DistSolver(ctx, grid, dH, N, 4, 4, False, 0, 0)
    assert s.get("h2_mixed_precision") == 0
    try:
        s.set(h2_mixed_precision=1)
        raise AssertionError("a grid solver accepted h2_mixed_precision = 1")
    except ChaseHipError as e:
        assert e.code == -1001 and "h2_mixed_precision" in str(e)
    s.set(h2_mixed_precision=0)
    assert s.get("h2_mixed_precision") == 0 and s.get("sp_h_converts") == 0
    s.close()


@pytest.mark.parametrize("pseudo", [False, True], ids=["hermitian", "pseudo"])
def test_grid_solvers_refuse_the_key(pseudo):
    run_ranks(2, 1, _scenario_grid_refuses, 64, pseudo, transport="host")


def _small_solve(ctx):
    from chase_amd.capi import PseudoSolver
    s = PseudoSolver(ctx, _bse64(ctx), 4, 4)
    s.set(tol=1e-10, numlanczos=10, lanczositer=50)
    s.solve()
    return s


def test_environment_variable_alone_switches_it_on(ctx, monkeypatch):
    monkeypatch.setenv("CHASE_HIP_H2_MIXED_PRECISION", "1")
    s = _small_solve(ctx)
    assert s.get("h2_mixed_precision") == 1 and s.get("mixed_precision") == 0
    assert s.get("hemm_sp_calls") > 0 and s.get("sp_filters") >= 1 and s.get("sp_h_converts") == 1
    assert np.max(s.resid()[:4]) <= 1e-10
    s.close()


def test_hermitian_variables_leave_the_pseudo_solve_alone(ctx, monkeypatch):
    monkeypatch.setenv("CHASE_HIP_MIXED_PRECISION", "1")
    monkeypatch.setenv("CHASE_HIP_SP_PRODUCT", "bf16x3")
    monkeypatch.setenv("CHASE_HIP_SP_PREPACK", "1")
    s = _small_solve(ctx)
    for key in ("h2_mixed_precision", "mixed_precision", "sp_product", "sp_prepack") + SP_KEYS:
        assert s.get(key) == 0, key
    assert s.get("hemm_calls") > 0
    s.close()
