"""Scenarios of the bf16x3 split product on a process grid (pChaseHip with mixed_precision = 1 and sp_product = 1): the filter's
local products run on the bf16 matrix cores with split fp32 operands, every rank's partial product is written and summed in
fp64.  A scenario is fn(ctx, grid, comm, ...) like those of tests/mixed_grid_scenarios.py, whose helpers and whose propagated
two-step bound are used here with the chain constant of the split product, g = (6N + 16 | 12N + 32) u (tests/bf16x3_ref.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bf16x3_ref as R  # noqa: E402
from chase_amd import dist as cd  # noqa: E402
from mixed_grid_scenarios import LOCK, NEV, NEX, SHIFT, STEPS, U32, U64, _gather, _set_resid  # noqa: E402
from oracle import chase_oracle as O  # noqa: E402

COUNTERS = ("hemm_sp_calls", "hemm_sp_split_calls", "hemm_calls", "hemm_sp_vecs", "sp_filters")


def _filter_leg(ctx, grid, comm, H, Vstart, cplx, mb, keys, resid):
    """Start, fixed start block, QR, Lock, residuals := resid, Shift(-c), two filter products over the unlocked columns, unshift"""
    N, n = H.shape[0], NEV + NEX
    rl, cl = cd.Layout(N, mb, grid.nprow), cd.Layout(N, mb, grid.npcol)
    rows = rl.globals_of(grid.myrow)
    dH = ctx.array(cd.local_block_of(H, rl, cl, grid.myrow, grid.mycol))
    s = cd.DistSolver(ctx, grid, dH, N, NEV, NEX, cplx, mb, mb)
    s.set(panel_cols=64, **keys)                               # 91 unlocked columns: two panels, the second one ragged
    s.Start(); s.upload_local_V(Vstart[rows, :]); s.initVecs(False); s.QR(0, 1.0); s.Lock(LOCK)
    _set_resid(s, resid)
    V0 = s.local_V()
    m_loc, n_loc = dH.shape
    h0 = ctx.hash64(dH.ptr, m_loc, n_loc, m_loc, cplx)
    s.Shift(-SHIFT)
    for (a, b) in STEPS:
        s.HEMM(n - LOCK, a, b, 0)
    s.Shift(SHIFT, True)
    out = dict(V0=V0, V=s.local_V(), h0=h0, h1=ctx.hash64(dH.ptr, m_loc, n_loc, m_loc, cplx), rl=rl,
               counters=tuple(s.get(k) for k in COUNTERS))
    s.close()
    dH.free()
    same = comm.all_gather_object(out["counters"])
    assert all(c == same[0] for c in same), same               # every rank sees the same counters
    return out


def scenario_operator(ctx, grid, comm, N, cplx, mb):
    n = NEV + NEX
    H = O.clement(N, cplx)
    Vstart = comm.once(("start", N, cplx), lambda: O.random_start_vectors(N, n, cplx))
    st, wide = (np.complex64, np.complex128) if cplx else (np.float32, np.float64)
    r = _filter_leg(ctx, grid, comm, H, Vstart, cplx, mb, dict(mixed_precision=1, sp_product=1), 1.0)
    rl = r["rl"]
    assert r["V"][:, :LOCK].tobytes() == r["V0"][:, :LOCK].tobytes()         # locked columns: never touched
    assert r["h0"] == r["h1"]                                                # fp64 H_loc restored bit for bit
    assert r["counters"] == (2, 2, 0, 2 * (n - LOCK), 1)
    V0 = _gather(comm, grid, rl, N, r["V0"])
    V = _gather(comm, grid, rl, N, r["V"])

    def emulate():                                             # tests/mixed_grid_scenarios.py, module docstring
        Hs = (H - SHIFT * np.eye(N)).astype(st).astype(wide)
        X0 = V0[:, LOCK:].astype(st).astype(wide)
        (a1, _), (a2, b2) = STEPS
        p = grid.nprow * grid.npcol
        g, w = R.gamma(N, cplx), (8 + p) * U64
        aH = np.abs(Hs)
        R1 = a1 * (Hs.conj().T @ X0)
        e1 = (g + w) * abs(a1) * (aH.T @ np.abs(X0))
        X1 = R1.astype(st).astype(wide)
        dx = U32 * (np.abs(R1) + e1) + e1 + U32 * np.abs(R1)
        R2 = a2 * (Hs @ X1) + b2 * V0[:, LOCK:]
        hx = abs(a2) * (aH @ (np.abs(X1) + dx))
        e2 = abs(a2) * (aH @ dx) + g * hx + w * (hx + abs(b2) * np.abs(V0[:, LOCK:]))
        return R2, e2
    R2, e2 = comm.once(("emulate3", N, cplx, mb, grid.nprow, grid.npcol), emulate)
    err = np.abs(V[:, LOCK:] - R2)
    if comm.rank == 0:
        print(f"grid operator level bf16x3 {grid.nprow}x{grid.npcol} mb={mb} N={N} {'complex' if cplx else 'real'}: "
              f"max err / bound = {np.max(err / e2):.2e}")
    assert np.all(err <= e2), float(np.max(err / e2))
    # below the threshold no fp32 product runs: the bits of a solver never told about either key; so with mixed_precision off
    off = _filter_leg(ctx, grid, comm, H, Vstart, cplx, mb, {}, 1e-4)
    lo = _filter_leg(ctx, grid, comm, H, Vstart, cplx, mb, dict(mixed_precision=1, sp_product=1), 1e-4)
    alone = _filter_leg(ctx, grid, comm, H, Vstart, cplx, mb, dict(sp_product=1), 1.0)
    for x in (lo, alone):
        assert x["counters"] == (0, 0, 2, 0, 0)
        assert x["V"].tobytes() == off["V"].tobytes()
    # sp_product = 0: the fp32 MFMA path, bit for bit that of a solver that only had mixed_precision = 1
    f32 = _filter_leg(ctx, grid, comm, H, Vstart, cplx, mb, dict(mixed_precision=1), 1.0)
    f32_0 = _filter_leg(ctx, grid, comm, H, Vstart, cplx, mb, dict(mixed_precision=1, sp_product=0), 1.0)
    assert f32_0["counters"] == (2, 0, 0, 2 * (n - LOCK), 1) and f32["counters"] == f32_0["counters"]
    assert f32_0["V"].tobytes() == f32["V"].tobytes()


def scenario_solve(ctx, grid, comm, N, nev, nex, cplx, mb):
    """a whole grid solve with both switches on: the bars of the fp32 path (tests/mixed_grid_scenarios.py)"""
    H = O.clement(N, cplx)
    exact = comm.once(("eigvalsh", N, cplx), lambda: np.linalg.eigvalsh(H))[:nev]
    rl, cl = cd.Layout(N, mb, grid.nprow), cd.Layout(N, mb, grid.npcol)
    dH = ctx.array(cd.local_block_of(H, rl, cl, grid.myrow, grid.mycol))
    s = cd.DistSolver(ctx, grid, dH, N, nev, nex, cplx, mb, mb)
    s.set(deg=20, device_rng=1)
    st_off = s.solve()                                                       # fp64
    assert s.get("hemm_sp_calls") == 0 and s.get("hemm_sp_split_calls") == 0
    s.set(mixed_precision=1, sp_product=1, reset_counters=1)
    assert s.get("sp_product") == 1
    st_on = s.solve()
    lam = s.ritzv[:nev].copy()
    if comm.rank == 0:
        print(f"grid {grid.nprow}x{grid.npcol} clement({N}, {cplx}) {nev}/{nex} mb={mb}: fp64 {st_off['iterations']} iterations / "
              f"{st_off['filtered_vecs']} filtered vectors, bf16x3 {st_on['iterations']} / {st_on['filtered_vecs']}, "
              f"{int(s.get('hemm_sp_vecs'))} columns in fp32 over {int(s.get('sp_filters'))} filter calls")
    assert st_on["locked"] >= nev
    assert np.max(s.resid()[:nev]) <= 1e-10
    V = _gather(comm, grid, rl, N, s.local_V()[:, :nev])                     # (asserts bit-identical replicas)
    assert np.max(O.residuals(H, lam, V)) < 1e-8
    assert np.max(np.abs(np.sort(lam) - exact)) < 1e-9
    assert st_on["iterations"] <= st_off["iterations"] + 1, (st_on["iterations"], st_off["iterations"])
    assert s.get("sp_filters") >= 1 and s.get("hemm_sp_split_calls") > 0 and s.get("hemm_calls") > 0
    assert s.get("hemm_sp_split_calls") == s.get("hemm_sp_calls")
    same = comm.all_gather_object((tuple(s.get(k) for k in COUNTERS), s.ritzv.tobytes()))
    assert all(x == same[0] for x in same)                                   # counters and Ritz values identical on every rank
    s.close()
    dH.free()


def scenario_pseudo_refuses(ctx, grid, comm):
    from chase_amd.capi import ChaseHipError
    N = 64
    rl, cl = cd.Layout(N, 0, grid.nprow), cd.Layout(N, 0, grid.npcol)
    dH = cd.gen_bse_local(ctx, N, True, rl, cl, grid.myrow, grid.mycol)
    s = cd.DistPseudoSolver(ctx, grid, dH, N, 4, 4, True, 0, 0)
    try:
        s.set(sp_product=1)
        raise AssertionError("the pseudo-Hermitian grid solver accepted sp_product = 1")
    except ChaseHipError as e:
        assert e.code == -1001 and "sp_product" in str(e)
    s.set(sp_product=0)
    assert s.get("sp_product") == 0
    s.close()
