"""Scenarios of the mixed-precision filter on a process grid (pChaseHip with mixed_precision = 1): the filter's local products
run on fp32 operands on the matrix cores, every rank's partial product is written and summed in fp64.  A scenario is
fn(ctx, grid, comm, ...) like those of tests/dist_scenarios.py; the ranks are threads (tests/rank_threads.py).

Error bound of the operator scenario.  u = 2^-24, v = 2^-53, p = ranks of the grid.  One distributed product
alpha op(Hs) X + beta C of fp32 operands Hs, X: rank r accumulates its local inner products (length k_r, sum over the ranks of a
group = N) by fp32 fma in some order - error at most gamma_{k_r} |Hs_r||X_r| (Higham (3.5)), complex arithmetic from four real
products doubles the chain -, forms alpha acc + beta C in fp64 (a handful of roundings of size v) and the group sums the p_g
partial results in fp64 (p_g - 1 more).  Since gamma_{k_r} <= gamma_N and the |Hs_r||X_r| add up to |Hs||X|:

    |dev - exact| <= g |alpha| |Hs||X| + w (|alpha| |Hs||X| + |beta| |C|),   g = (N + 8 | 2N + 16) u,  w = (8 + p) v

(the (k + 8 | 2k + 16) u of tests/test_gpu_mixed_precision.py with k = N; the beta term carries no fp32 error).  Two steps:

    R1 = a1 Hs^H X0,                X0 = fl32(V0)            device: R1d = R1 + d1,  |d1| <= e1 = g a1 |Hs||X0| + w a1 |Hs||X0|
    R2 = a2 Hs fl32(R1) + b2 V0     (beta term on the fp64 V0)

The device rounds ITS intermediate: |fl32(R1d) - fl32(R1)| <= |fl32(R1d) - R1d| + |R1d - R1| + |R1 - fl32(R1)|
<= u (|R1| + e1) + e1 + u |R1| =: dx, so with X1 = fl32(R1)

    |V - R2| <= |a2| |Hs| dx + g |a2| |Hs| (|X1| + dx) + w (|a2| |Hs| (|X1| + dx) + |b2| |V0|)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from chase_amd import dist as cd  # noqa: E402
from chase_amd.capi import lib  # noqa: E402
from oracle import chase_oracle as O  # noqa: E402

U32, U64 = 2.0 ** -24, 2.0 ** -53
STAT_KEYS = ("iterations", "filtered_vecs", "lanczos_vecs", "locked", "lowerb", "upperb", "lambda_")     # tests/test_gpu_mixed_precision.py
NEV, NEX, LOCK, SHIFT = 60, 36, 5, 40.0
STEPS = [(0.01, 0.0), (0.02, -0.3)]                      # the filter's pattern: beta = 0 first


def _set_resid(s, value):
    """the buffer the driver writes its residuals into (chase_hip_solver_resid): what Shift decides from"""
    np.ctypeslib.as_array(lib.chase_hip_solver_resid(s.h), shape=(s.ncol,))[:] = value


def _gather(comm, grid, rl, N, block):
    """the global column-type block from the ranks' pieces; the replicas over the grid columns must agree bit for bit"""
    objs = comm.all_gather_object((grid.myrow, grid.mycol, block))
    V = np.zeros((N, block.shape[1]), dtype=block.dtype)
    for (i, j, blk) in objs:
        if j == 0:
            V[rl.globals_of(i), :] = blk
    for (i, j, blk) in objs:
        assert V[rl.globals_of(i), :].tobytes() == blk.tobytes(), "column-type replicas differ"      # (both in logical order)
    return V


def _filter_leg(ctx, grid, comm, H, Vstart, cplx, mb, mixed, resid):
    """Start, fixed start block, QR, Lock, residuals := resid, Shift(-c), two filter products over the unlocked columns, unshift"""
    N, n = H.shape[0], NEV + NEX
    rl, cl = cd.Layout(N, mb, grid.nprow), cd.Layout(N, mb, grid.npcol)
    rows = rl.globals_of(grid.myrow)
    dH = ctx.array(cd.local_block_of(H, rl, cl, grid.myrow, grid.mycol))
    s = cd.DistSolver(ctx, grid, dH, N, NEV, NEX, cplx, mb, mb)
    if grid.nprow * grid.npcol > 1:
        s.set(panel_cols=64)                                   # 91 unlocked columns: two panels, the second one ragged
    if mixed is not None:
        s.set(mixed_precision=mixed)
    s.Start(); s.upload_local_V(Vstart[rows, :]); s.initVecs(False); s.QR(0, 1.0); s.Lock(LOCK)
    _set_resid(s, resid)
    V0 = s.local_V()
    m_loc, n_loc = dH.shape
    h0 = ctx.hash64(dH.ptr, m_loc, n_loc, m_loc, cplx)
    s.Shift(-SHIFT)
    for (a, b) in STEPS:
        s.HEMM(n - LOCK, a, b, 0)
    s.Shift(SHIFT, True)
    V = s.local_V()
    out = dict(V0=V0, V=V, h0=h0, h1=ctx.hash64(dH.ptr, m_loc, n_loc, m_loc, cplx), sp=s.get("hemm_sp_calls"),
               dp=s.get("hemm_calls"), sp_vecs=s.get("hemm_sp_vecs"), sp_filters=s.get("sp_filters"), rl=rl)
    s.close()
    dH.free()
    return out


def scenario_operator(ctx, grid, comm, N, cplx, mb):
    """the switch at operator level on the grid: what is rounded to fp32, what never is, and the propagated bound (module
    docstring) against the numpy emulation in fp64 on fp32-rounded operands"""
    n = NEV + NEX
    H = O.clement(N, cplx)
    Vstart = comm.once(("start", N, cplx), lambda: O.random_start_vectors(N, n, cplx))
    st, wide = (np.complex64, np.complex128) if cplx else (np.float32, np.float64)
    r = _filter_leg(ctx, grid, comm, H, Vstart, cplx, mb, 1, 1.0)
    rl = r["rl"]
    assert r["V"][:, :LOCK].tobytes() == r["V0"][:, :LOCK].tobytes()         # locked columns: never touched
    assert r["h0"] == r["h1"]                                                # fp64 H_loc restored bit for bit
    assert r["sp"] == 2 and r["dp"] == 0 and r["sp_vecs"] == 2 * (n - LOCK) and r["sp_filters"] == 1
    V0 = _gather(comm, grid, rl, N, r["V0"])
    V = _gather(comm, grid, rl, N, r["V"])

    def emulate():
        Hs = (H - SHIFT * np.eye(N)).astype(st).astype(wide)
        X0 = V0[:, LOCK:].astype(st).astype(wide)
        (a1, _), (a2, b2) = STEPS
        p = grid.nprow * grid.npcol
        g, w = ((2 * N + 16) if cplx else (N + 8)) * U32, (8 + p) * U64
        aH = np.abs(Hs)
        R1 = a1 * (Hs.conj().T @ X0)
        e1 = (g + w) * abs(a1) * (aH.T @ np.abs(X0))
        X1 = R1.astype(st).astype(wide)
        dx = U32 * (np.abs(R1) + e1) + e1 + U32 * np.abs(R1)
        R2 = a2 * (Hs @ X1) + b2 * V0[:, LOCK:]
        hx = abs(a2) * (aH @ (np.abs(X1) + dx))
        e2 = abs(a2) * (aH @ dx) + g * hx + w * (hx + abs(b2) * np.abs(V0[:, LOCK:]))
        return R2, e2
    R2, e2 = comm.once(("emulate", N, cplx, mb, grid.nprow, grid.npcol), emulate)
    err = np.abs(V[:, LOCK:] - R2)
    if comm.rank == 0:
        print(f"grid operator level {grid.nprow}x{grid.npcol} mb={mb} N={N} {'complex' if cplx else 'real'}: "
              f"max err / bound = {np.max(err / e2):.3f}")
    assert np.all(err <= e2), float(np.max(err / e2))
    # below the threshold nothing runs in fp32, and the bits are those of a solver that was never told about the switch
    lo = _filter_leg(ctx, grid, comm, H, Vstart, cplx, mb, 1, 1e-4)
    off = _filter_leg(ctx, grid, comm, H, Vstart, cplx, mb, None, 1e-4)
    assert lo["sp"] == 0 and lo["dp"] == 2 and lo["sp_filters"] == 0
    assert lo["V"].tobytes() == off["V"].tobytes()
    diff = comm.all_gather_object(not np.array_equal(lo["V"][:, LOCK:], r["V"][:, LOCK:]))
    assert any(diff)                                                         # (the two paths do differ)


def scenario_pseudo_refuses(ctx, grid, comm):
    from chase_amd.capi import ChaseHipError
    N = 64
    rl, cl = cd.Layout(N, 0, grid.nprow), cd.Layout(N, 0, grid.npcol)
    dH = cd.gen_bse_local(ctx, N, True, rl, cl, grid.myrow, grid.mycol)
    s = cd.DistPseudoSolver(ctx, grid, dH, N, 4, 4, True, 0, 0)
    try:
        s.set(mixed_precision=1)
        raise AssertionError("the pseudo-Hermitian grid solver accepted mixed_precision = 1")
    except ChaseHipError as e:
        assert e.code == -1001 and "mixed_precision" in str(e)
    s.set(mixed_precision=0)                                 # turning it off is what the solver does anyway
    assert s.get("mixed_precision") == 0
    s.close()


def scenario_solve_off_and_on(ctx, grid, comm, N, nev, nex, cplx, mb):
    """whole solves on the grid: a solver set to 0 gives the bits of one never told; with the switch on the solve converges
    to the same accuracy in at most one more iteration, having gone into fp32 and back out"""
    H = O.clement(N, cplx)
    exact = comm.once(("eigvalsh", N, cplx), lambda: np.linalg.eigvalsh(H))[:nev]
    rl, cl = cd.Layout(N, mb, grid.nprow), cd.Layout(N, mb, grid.npcol)
    dH = ctx.array(cd.local_block_of(H, rl, cl, grid.myrow, grid.mycol))
    plain = cd.DistSolver(ctx, grid, dH, N, nev, nex, cplx, mb, mb)          # never heard of the key
    plain.set(deg=20, device_rng=1)
    st_plain = plain.solve()
    lam_plain = plain.ritzv.copy()
    plain.close()

    s = cd.DistSolver(ctx, grid, dH, N, nev, nex, cplx, mb, mb)
    s.set(deg=20, device_rng=1, mixed_precision=0)
    assert s.get("mixed_precision") == 0
    st_off = s.solve()
    assert s.get("hemm_sp_calls") == 0 and s.get("sp_filters") == 0
    assert {k: st_off[k] for k in STAT_KEYS} == {k: st_plain[k] for k in STAT_KEYS}
    assert s.ritzv.tobytes() == lam_plain.tobytes()

    s.set(mixed_precision=1, reset_counters=1)
    assert s.get("mixed_precision") == 1
    st_on = s.solve()
    lam = s.ritzv[:nev].copy()
    if comm.rank == 0:
        print(f"grid {grid.nprow}x{grid.npcol} clement({N}, {cplx}) {nev}/{nex} mb={mb}: fp64 {st_off['iterations']} iterations / "
              f"{st_off['filtered_vecs']} filtered vectors, mixed {st_on['iterations']} / {st_on['filtered_vecs']}, "
              f"{int(s.get('hemm_sp_vecs'))} columns in fp32 over {int(s.get('sp_filters'))} filter calls")
    assert st_on["locked"] >= nev
    assert np.max(s.resid()[:nev]) <= 1e-10
    V = _gather(comm, grid, rl, N, s.local_V()[:, :nev])                     # (asserts bit-identical replicas)
    r_host = O.residuals(H, lam, V)
    assert np.max(r_host) < 1e-8
    r_dev = s.recompute_residuals(nev)
    assert np.max(np.abs(r_dev - r_host)) <= 1e-12 * np.abs(H).max()         # the bar of tests/dist_scenarios.py scenario_solve
    assert np.max(np.abs(np.sort(lam) - exact)) < 1e-9
    assert s.get("sp_filters") >= 1 and s.get("hemm_sp_calls") > 0 and s.get("hemm_calls") > 0      # into fp32 and back out
    assert st_on["iterations"] <= st_off["iterations"] + 1, (st_on["iterations"], st_off["iterations"])
    allv = comm.all_gather_object(s.ritzv.copy())
    assert all(np.array_equal(allv[0], a) for a in allv)                     # identical Ritz values on every rank
    s.set(reset_counters=1)
    assert s.get("hemm_sp_calls") == 0 and s.get("hemm_sp_vecs") == 0 and s.get("sp_filters") == 0
    s.close()
    dH.free()
