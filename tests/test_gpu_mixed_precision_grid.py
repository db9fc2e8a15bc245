"""Mixed-precision Chebyshev filter on the process grid: the fp32-input MFMA product with an fp64 result (op(A) = N and C) against
an fp64 reference within the worst-case bound of an fma chain, the list form of the diagonal copy bit for bit, the switch at
operator level on several grids and transports (tests/mixed_grid_scenarios.py) and whole grid solves with the switch off and on.

Bound of the product (Higham, Accuracy and Stability, (3.5) / gamma_n, as in tests/test_gpu_mixed_precision.py): the inner
product of length k is accumulated by fp32 fma in any order, error at most gamma_k |A||B| with (k + 8) u, u = 2^-24 (complex
arithmetic from four real products doubles the chain: (2k + 16) u); alpha acc + beta C is then formed in fp64 from fp64 scalars
and an fp64 C - at most four products and three sums per component: 8 v, v = 2^-53, on |alpha||A||B| + |beta||C0|.  The beta
term carries no fp32 error:

    ((k + 8) | (2k + 16)) u |alpha| |A||B|  +  8 v (|alpha| |A||B| + |beta| |C0|)"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mixed_grid_scenarios as M  # noqa: E402
from rank_threads import run_ranks  # noqa: E402

pytestmark = pytest.mark.gpu
U, V64 = 2.0 ** -24, 2.0 ** -53

# (m, n, k, padding of lda, ldb, ldc over the operand's rows, first column of B and C inside a wider array)
SHAPES = [(1, 1, 1, 0, 0, 0, 0),
          (128, 128, 64, 0, 0, 0, 0),                 # whole tiles
          (130, 70, 37, 0, 0, 0, 0),                  # ragged every way, nothing aligned
          (257, 129, 515, 0, 0, 0, 0),                # several tiles plus rests
          (1001, 160, 1001, 0, 0, 0, 1),              # the filter's shape at odd N: B, C start at column 1 - unaligned base
          (130, 70, 40, 2, 0, 2, 0),                  # 16-byte paths (aligned leading dimensions) with ragged rows and columns
          (70, 33, 300, 0, 0, 0, 0),                  # one ragged tile, long K: m << k as on a rank
          (130, 7, 0, 0, 1, 0, 0),                    # k = 0: beta C
          # 128-column tiles, ragged in m and n with a K rest: on a device with num_cu = 256 compute units 65 row panels give 260
          # tiles of 128 x 64 against 130 of 128 x 128, two rounds either way (every shape above picks 64-column tiles there)
          (8200, 250, 37, 0, 0, 0, 0)]
SCALARS = {False: [(1.0, 0.0), (0.37, -1.25), (-2.5, 1.0)],                         # tests/test_gpu_mixed_precision.py
           True: [(1.0, 0.0), (0.37, -1.25), (0.3 - 0.7j, 1.1 + 0.4j)]}


def _rand(rng, shape, cplx, dtype):
    a = rng.standard_normal(shape)
    if cplx:
        a = a + 1j * rng.standard_normal(shape)
    return np.asfortranarray(a.astype(dtype))


def _lds(shape, op):
    """leading dimensions: A is m x k for N (lda >= m), k x m for C (lda >= k); the padded case is 16-byte aligned on either
    (132 for m = 130, 44 for k = 40)"""
    m, n, k, pa, pb, pc, c0 = shape
    return max(1, m + pa if op == "N" else k + 2 * pa), max(1, k + pb), m + pc


@pytest.fixture(scope="module")
def operands():
    """operands and their fp64 products, made once per (shape, type, op)"""
    rng = np.random.default_rng(20250212)
    out = {}
    for cplx in (False, True):
        st, wide = (np.complex64, np.complex128) if cplx else (np.float32, np.float64)
        for sh in SHAPES:
            m, n, k, pa, pb, pc, c0 = sh
            for op in ("N", "C"):
                lda, ldb, ldc = _lds(sh, op)
                A = _rand(rng, (lda, max(k, 1) if op == "N" else m), cplx, st)       # (k = 0: a column nobody reads)
                Bw = _rand(rng, (ldb, n + c0), cplx, st)
                Cw = _rand(rng, (ldc, n + c0), cplx, wide)
                opA = A[:m, :k].astype(wide) if op == "N" else A[:k, :m].astype(wide).conj().T
                B = Bw[:k, c0:].astype(wide)
                out[(cplx, sh, op)] = (A, Bw, Cw, opA @ B, np.abs(opA) @ np.abs(B))
    return out


@pytest.mark.parametrize("op", ["N", "C"])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:3])) + ("u" if s[6] else "") + ("v" if s[3] else ""))
def test_widened_product_within_the_fma_chain_bound(ctx, operands, shape, cplx, op):
    m, n, k, pa, pb, pc, c0 = shape
    lda, ldb, ldc = _lds(shape, op)
    A, Bw, Cw, P, absP = operands[(cplx, shape, op)]
    st, wide = (np.complex64, np.complex128) if cplx else (np.float32, np.float64)
    dA, dB = ctx.empty(A.shape, st).upload(A), ctx.empty(Bw.shape, st).upload(Bw)
    dC = ctx.empty(Cw.shape, wide)
    try:
        for (alpha, beta) in SCALARS[cplx]:                                 # fp64 scalars, rounded by nobody
            C0 = Cw.copy(order="F")
            if beta == 0:
                C0[:] = np.nan                                              # beta == 0: C is not read
            runs = []
            for _ in range(2):
                dC.upload(C0)
                ctx.gemm32w(op, m, n, k, alpha, dA.ptr, lda, dB.offset(c0), ldb, beta, dC.offset(c0), ldc, cplx)
                runs.append(dC.download())
            got = runs[0]
            assert runs[0].tobytes() == runs[1].tobytes()                   # bitwise reproducible
            ref = wide(alpha) * P
            bound = (((2 * k + 16) if cplx else (k + 8)) * U + 8 * V64) * abs(alpha) * absP
            if beta != 0:
                ref = ref + wide(beta) * C0[:m, c0:]
                bound = bound + 8 * V64 * abs(beta) * np.abs(C0[:m, c0:])
            assert np.all(np.isfinite(got[:m, c0:]))
            err = np.abs(got[:m, c0:] - ref)
            ratio = np.max(err / bound) if np.all(bound > 0) else (0.0 if np.all(err[bound == 0] == 0) else np.inf)
            print(f"gemm32w {'cz' if cplx else 'sd'}{op} {m}x{n}x{k} alpha={alpha} beta={beta}: max err / bound = {ratio:.3f}")
            assert np.all(err <= bound), (alpha, beta, float(ratio))
            # nothing outside the m x n window was written: rows below m, the columns in front of it
            keep = C0.copy()
            keep[:m, c0:] = got[:m, c0:]
            assert got.tobytes() == keep.tobytes()
    finally:
        for d in (dA, dB, dC):
            d.free()


@pytest.mark.parametrize("cplx", [False, True])
def test_widened_product_refuses_a_bad_op(ctx, cplx):
    from chase_amd.capi import ChaseHipError
    st, wide = (np.complex64, np.complex128) if cplx else (np.float32, np.float64)
    d = ctx.empty((8, 8), st).upload(np.zeros((8, 8), st))
    c = ctx.empty((8, 8), wide).upload(np.zeros((8, 8), wide))
    for bad in ("X", "T") if cplx else ("X",):                           # real: T is C; complex: T is no operation of this product
        with pytest.raises(ChaseHipError) as e:
            ctx.gemm32w(bad, 8, 8, 8, 1.0, d.ptr, 8, d.ptr, 8, 0.0, c.ptr, 8, cplx)
        assert e.value.code == -1001 and "opA" in str(e.value)            # CHASE_HIP_EINVAL, with a message
    if not cplx:
        ctx.gemm32w("T", 8, 8, 8, 1.0, d.ptr, 8, d.ptr, 8, 0.0, c.ptr, 8, cplx)
    ctx.gemm32w("N", 0, 8, 8, 1.0, d.ptr, 8, d.ptr, 8, 0.0, c.ptr, 8, cplx)    # m == 0 / n == 0: nothing to do
    ctx.gemm32w("C", 8, 0, 8, 1.0, d.ptr, 8, d.ptr, 8, 0.0, c.ptr, 8, cplx)
    assert not np.any(c.download())
    d.free(); c.free()


@pytest.mark.parametrize("cplx", [False, True])
def test_diag_list_d2s_changes_the_listed_entries_only(ctx, cplx):
    """the lists pChaseHip builds for rank (1, 0) of a 2 x 2 block-cyclic layout (nb = 16, N = 100): local positions of the
    global diagonal inside the rank's block"""
    from chase_amd import dist as cd
    N, nb = 100, 16
    rl, cl = cd.Layout(N, nb, 2), cd.Layout(N, nb, 2)
    rows, cols = [], []
    for l, g in enumerate(rl.globals_of(1)):
        if cl.owner(int(g)) == 0:
            rows.append(l); cols.append(cl.local(int(g)))
    assert len(rows) == 0                                                  # off-diagonal rank of a square grid with mb = nb: none
    for l, g in enumerate(rl.globals_of(1)):                               # rank (1, 1) owns the blocks 1, 3, 5 of the diagonal
        if cl.owner(int(g)) == 1:
            rows.append(l); cols.append(cl.local(int(g)))
    cnt = len(rows)
    assert cnt == 48
    m, n, ldh, ldhs = rl.count(1), cl.count(1), rl.count(1) + 3, rl.count(1) + 4
    rng = np.random.default_rng(11)
    dt, st = (np.complex128, np.complex64) if cplx else (np.float64, np.float32)
    H = rng.standard_normal((ldh, n)) + (1j * rng.standard_normal((ldh, n)) if cplx else 0)
    H = np.asfortranarray(H.astype(dt))
    Hs0 = np.asfortranarray((rng.standard_normal((ldhs, n)) + (1j if cplx else 0)).astype(st))
    dH, dHs = ctx.empty((ldh, n), dt).upload(H), ctx.empty((ldhs, n), st).upload(Hs0)
    dr = ctx.empty((cnt, 1), np.int32).upload(np.array(rows, np.int32).reshape(-1, 1))
    dc = ctx.empty((cnt, 1), np.int32).upload(np.array(cols, np.int32).reshape(-1, 1))
    ctx.diag_list_d2s(dH.ptr, ldh, dHs.ptr, ldhs, dr.ptr, dc.ptr, cnt, cplx)
    want = Hs0.copy()
    want[rows, cols] = H[rows, cols].astype(st)
    assert dHs.download().tobytes() == want.tobytes()
    ctx.diag_list_d2s(dH.ptr, ldh, dHs.ptr, ldhs, dr.ptr, dc.ptr, 0, cplx)             # an empty list is legal
    assert dHs.download().tobytes() == want.tobytes()
    for d in (dH, dHs, dr, dc):
        d.free()


# grid (rows x columns), N, complex, block length (0: block layout), transport
OPERATOR_CASES = [(2, 1, 300, False, 0, "host"), (2, 2, 300, True, 0, "host"), (2, 2, 300, False, 16, "shared"),
                  (2, 2, 300, True, 16, "host"), (4, 2, 301, True, 0, "shared"), (4, 2, 301, False, 0, "host"),
                  (1, 1, 300, False, 0, "host"), (1, 1, 300, True, 0, "shared")]


@pytest.mark.parametrize("nprow,npcol,N,cplx,mb,transport", OPERATOR_CASES,
                         ids=[f"{a}x{b}-N{N}-{'z' if c else 'd'}-mb{mb}-{t}" for (a, b, N, c, mb, t) in OPERATOR_CASES])
def test_switch_at_operator_level_on_the_grid(nprow, npcol, N, cplx, mb, transport):
    run_ranks(nprow, npcol, M.scenario_operator, N, cplx, mb, transport=transport)


def test_pseudo_hermitian_grid_solver_refuses_the_switch():
    run_ranks(2, 1, M.scenario_pseudo_refuses)


SOLVES = [(2, 2, 256, 24, 16, True, 0, "host"), (2, 2, 1001, 100, 60, False, 64, "host"), (4, 2, 640, 40, 24, False, 32, "shared")]


@pytest.mark.parametrize("nprow,npcol,N,nev,nex,cplx,mb,transport", SOLVES,
                         ids=["2x2-clement256-complex", "2x2-clement1001-real-nb64", "4x2-clement640-real-mb32-shared"])
def test_whole_grid_solve_off_and_on(nprow, npcol, N, nev, nex, cplx, mb, transport):
    run_ranks(nprow, npcol, M.scenario_solve_off_and_on, N, nev, nex, cplx, mb, transport=transport)
