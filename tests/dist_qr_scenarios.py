"""Scenarios of tests/test_gpu_dist_qr.py: fn(ctx, grid, comm, ...) on the rank threads of one process (tests/rank_threads.py).
scenario_houseqr_dist calls chase_hip_houseqr_dist directly, with row counts, offsets and a leading dimension that
pChaseHip::householder() never passes; scenario_householder_caller goes through DistSolver.QR, which derives the offset from the
layout.  A scenario hands what rank 0 gathered to the test through the dict `out`; the assertions on it are the test's."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from chase_amd import dist as cd  # noqa: E402
from chase_amd.capi import lib, check  # noqa: E402
import dense_chain_refs as D  # noqa: E402
import dist_qr_refs as Q  # noqa: E402


def houseqr_dist(ctx, grid, cplx, buf, mloc, n, offset):
    """one collective call on this rank's padded block (ldv = its row count) -> the buffer as the device left it"""
    dV = ctx.array(buf)
    try:
        check(lib.chase_hip_houseqr_dist(ctx.h, grid.h, cd.COL, int(cplx), mloc, n, dV.ptr, buf.shape[0], offset), "houseqr_dist")
        return dV.download()
    finally:
        dV.free()


def scenario_houseqr_dist(ctx, grid, comm, name, cplx, out):
    """every input of one case of dist_qr_refs.CASES, twice: out[kind] = {"V": stacked input, "bufs": per grid column the ranks'
    buffers in rank order, "again": the same of the second call} on rank 0"""
    _, nprow, npcol, counts, n = Q.CASE[name]
    assert (grid.nprow, grid.npcol) == (nprow, npcol)
    offsets, slices = Q.stacked_split(sum(counts), counts)
    mloc, off = counts[grid.myrow], offsets[grid.myrow]
    cases = comm.once(("qr inputs", name, cplx), lambda: Q.inputs(name, cplx))
    for kind, V in cases.items():
        buf = D.padded(V[slices[grid.myrow]], mloc + Q.PAD)
        got = [houseqr_dist(ctx, grid, cplx, buf, mloc, n, off) for _ in range(2)]
        objs = comm.all_gather_object((grid.myrow, grid.mycol, got))
        if comm.rank == 0:
            by = {(i, j): g for i, j, g in objs}
            out[kind] = {"V": V,
                         "bufs": [[by[(i, j)][0] for i in range(nprow)] for j in range(npcol)],
                         "again": [[by[(i, j)][1] for i in range(nprow)] for j in range(npcol)]}


def caller_inputs(N, n, cplx):
    """the blocks scenario_householder_caller uploads, rows in GLOBAL order: "random" and "duplicate_column" of qr_cases, and
    "cholqr_breaks": a block whose columns 0 and n / 2 are the same vector of 256 entries +-1 and zeros elsewhere.  Its Gram
    matrix has G_00 = G_0k = G_kk = 256 EXACTLY in any summation order, so the Cholesky factorisation computes r_00 = 16,
    r_0k = 16 and the pivot 256 - 16^2 = 0 minus squares: it fails at column n / 2 + 1 by construction (with the rounded entries of
    "duplicate_column" that pivot is +-1e-14 and the sign is luck)."""
    rng = np.random.default_rng(D.seed_of(3, N, n, cplx))
    c = D.qr_cases(rng, N, n, cplx)
    b = c["random"].copy()
    u = np.zeros(N)
    u[rng.permutation(N)[:256]] = rng.choice([-1.0, 1.0], 256)
    b[:, 0] = u
    b[:, n // 2] = u
    return {"random": c["random"], "duplicate_column": c["duplicate_column"], "cholqr_breaks": b}


def scenario_householder_caller(ctx, grid, comm, cplx, mb, out, N=600, n=70):
    """pChaseHip::householder() at 300 / 200 rows per rank: requested (cholqr = 0) on "random" and "duplicate_column", and as what
    CholQR falls through to when potrf fails ("cholqr_breaks", CholQR enabled).  out[(kind, cholqr)] = {"V", "Q" (both in the
    stacked order of the column group), "variant", "replicas_equal"} on rank 0"""
    rl, cl = cd.Layout(N, mb, grid.nprow), cd.Layout(N, mb, grid.npcol)
    rows = rl.globals_of(grid.myrow)
    stacked = np.concatenate([rl.globals_of(i) for i in range(grid.nprow)])
    dH = ctx.array(cd.local_block_of(np.eye(N, dtype=D.dt_of(cplx)), rl, cl, grid.myrow, grid.mycol))       # never used by QR
    blocks = comm.once(("caller inputs", N, n, cplx), lambda: caller_inputs(N, n, cplx))
    for kind, cholqr, cond in (("random", 0, 1e3), ("duplicate_column", 0, 1e3), ("cholqr_breaks", 1, 10.0)):
        V = blocks[kind]
        s = cd.DistSolver(ctx, grid, dH, N, n // 2, n - n // 2, cplx, mb, mb)
        s.set(cholqr=cholqr)
        s.Start()
        s.upload_local_V(V[rows, :]); s.initVecs(False)
        s.QR(0, cond)
        variant = int(s.get("qr_variant"))
        objs = comm.all_gather_object((grid.myrow, grid.mycol, s.local_V(), variant))
        s.close()
        if comm.rank == 0:
            by = {(i, j): blk for i, j, blk, _ in objs}
            Qs = [np.concatenate([by[(i, j)] for i in range(grid.nprow)], axis=0) for j in range(grid.npcol)]
            out[(kind, cholqr)] = {"V": V[stacked, :], "Q": Qs[0], "variant": sorted({v for _, _, _, v in objs}),
                                   "replicas_equal": all(D.same_bits(Qs[0], q) for q in Qs[1:])}
    dH.free()
