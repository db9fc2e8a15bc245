"""Scenario of sp_prepack on a process grid: the grid solvers do not pack H (op C and the fp64 epilogue from a packed block are
not built), so they refuse sp_prepack = 1 and accept 0.  fn(ctx, grid, comm, ...) like those of tests/sp_bf16x3_grid_scenarios.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from chase_amd import dist as cd  # noqa: E402
from oracle import chase_oracle as O  # noqa: E402


def scenario_grid_refuses(ctx, grid, comm, N, cplx):
    from chase_amd.capi import ChaseHipError
    H = O.clement(N, cplx)
    rl, cl = cd.Layout(N, 0, grid.nprow), cd.Layout(N, 0, grid.npcol)
    dH = ctx.array(cd.local_block_of(H, rl, cl, grid.myrow, grid.mycol))
    s = cd.DistSolver(ctx, grid, dH, N, 4, 4, cplx, 0, 0)
    assert s.get("sp_prepack") == 0
    try:
        s.set(sp_prepack=1)
        raise AssertionError("the grid solver accepted sp_prepack = 1")
    except ChaseHipError as e:
        assert e.code == -1001 and "sp_prepack" in str(e)
    s.set(sp_prepack=0)
    assert s.get("sp_prepack") == 0
    for k in ("hemm_sp_packed_calls", "sp_pack_full", "sp_pack_diag"):
        assert s.get(k) == 0
    s.close()
    dH.free()
