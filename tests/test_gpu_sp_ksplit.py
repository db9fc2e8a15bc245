"""K split of the wide single-precision products under gemm_min_rounds (chase_hip_gemm_sd / _cz and their bf16x3 twins, op N
and op C): while the context's gemm_min_rounds is > 0 a product with too few tiles is cut into K pieces, each an ordinary product
into an fp64 slab, and the slabs are summed in piece order.  Shapes come from the plan query (chase_hip_gemm_sp_plan), never from
literals: k = s min_piece_k + r is cut into min(8, s) pieces.

Exact operands.  Integers in [-3, 3] are exact in bf16 and fp32, a term is at most 9 (complex: 18) and k at most 8 * 1024 + 37, so
every partial sum is an integer below 2^24: every order of summation gives the same bits and the result must EQUAL the integer
product - any indexing error at a piece boundary shows.

Random operands.  The bound of tests/test_gpu_mixed_precision_grid.py (test_widened_product_within_the_fma_chain_bound), unchanged:
((k + 8) | (2k + 16)) u |alpha| |A||B| + 8 v (|alpha| |A||B| + |beta| |C0|).  A piece's fma chain is shorter than the whole-K
chain it replaces and the fp64 sum of sk slabs adds at most sk v.  (The worst-case chain constant of the bf16x3 product is six
times that of an fma chain, tests/bf16x3_ref.py; on random operands it stays far inside the fma bound, which is asserted for all
four entry points.)"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bf16x3_ref as R  # noqa: E402
import sp_bf16x3_grid_scenarios as S3  # noqa: E402
from mixed_grid_scenarios import LOCK, NEV, NEX, SHIFT, STEPS, U32, U64, _gather  # noqa: E402
from rank_threads import run_ranks  # noqa: E402

pytestmark = pytest.mark.gpu
U, V64 = 2.0 ** -24, 2.0 ** -53
KINDS = [(split, cplx, op) for split in (False, True) for cplx in (False, True) for op in ("N", "C")]
KIND_IDS = [("bf16x3" if s else "fp32") + ("-z" if c else "-d") + o for (s, c, o) in KINDS]
# m x n, first column of B and C inside a wider array: ragged in 64-column tiles with nothing 16-byte aligned at an odd k and an
# unaligned base; whole tiles with every operand 16-byte aligned at r = 0 (every piece starts on a 16-byte boundary: the fast loads)
MN = [(130, 70, 1), (256, 128, 0)]
SCALARS = {False: [(1.0, 0.0), (0.37, -1.25), (-2.5, 1.0)],                          # tests/test_gpu_mixed_precision_grid.py
           True: [(1.0, 0.0), (0.37, -1.25), (0.3 - 0.7j, 1.1 + 0.4j)]}


def _plan(ctx, split, cplx, op, m, n, k, min_rounds):
    from chase_amd import capi
    return capi.gemm_sp_plan(cplx, op, m, n, k, split=split, num_cu=ctx.info()["num_cu"], min_rounds=min_rounds)


def _types(cplx):
    return (np.complex64, np.complex128) if cplx else (np.float32, np.float64)


def _ints(rng, shape, cplx, dtype):
    a = rng.integers(-3, 4, shape).astype(np.float64)
    if cplx:
        a = a + 1j * rng.integers(-3, 4, shape)
    return np.asfortranarray(a.astype(dtype))


def _rand(rng, shape, cplx, dtype):
    a = rng.standard_normal(shape)
    if cplx:
        a = a + 1j * rng.standard_normal(shape)
    return np.asfortranarray(a.astype(dtype))


def _op(A, op, m, k, wide):
    return A[:m, :k].astype(wide) if op == "N" else A[:k, :m].astype(wide).conj().T


def _run(ctx, min_rounds, split, cplx, op, m, n, k, alpha, dA, lda, dB, ldb, c0, beta, dC, ldc, C0):
    """one product with the context's gemm_min_rounds at min_rounds (0 again afterwards, whatever happens)"""
    dC.upload(C0)
    ctx.set_gemm_min_rounds(min_rounds)
    try:
        ctx.gemm32w(op, m, n, k, alpha, dA.ptr, lda, dB.offset(c0), ldb, beta, dC.offset(c0), ldc, cplx, split=split)
    finally:
        ctx.set_gemm_min_rounds(0)
    return dC.download()


@pytest.mark.parametrize("mn", MN, ids=["130x70u", "256x128"])
@pytest.mark.parametrize("split,cplx,op", KINDS, ids=KIND_IDS)
def test_pieces_of_exact_operands_sum_to_the_integer_product(ctx, split, cplx, op, mn):
    m, n, c0 = mn
    st, wide = _types(cplx)
    mp = _plan(ctx, split, cplx, op, m, n, 1, 4)["min_piece_k"]
    kmax = 8 * mp + 37
    assert 18 * kmax < 2 ** 24
    rng = np.random.default_rng(20250301 + 2 * split + cplx)
    # one set of operands for every k: its leading k rows / columns
    ldk = kmax + (0 if c0 else 3)                                            # odd, or a multiple of 4: 16-byte aligned columns
    A = _ints(rng, (m, kmax) if op == "N" else (ldk, m), cplx, st)
    Bw = _ints(rng, (ldk, n + c0), cplx, st)
    C0 = _ints(rng, (m, n + c0), cplx, wide)
    lda, ldb, ldc = A.shape[0], ldk, m
    dA, dB = ctx.empty(A.shape, st).upload(A), ctx.empty(Bw.shape, st).upload(Bw)
    dC = ctx.empty(C0.shape, wide)
    alpha = 2j if cplx else 0.5                                              # powers of two; beta = 0
    seen = set()
    try:
        for s in (2, 3, 8):
            for r in (0, 37):
                k = s * mp + r
                want = wide(alpha) * (_op(A, op, m, k, wide) @ Bw[:k, c0:].astype(wide))
                outs = {}
                for rounds in (0, 4, 16):
                    p = _plan(ctx, split, cplx, op, m, n, k, rounds)
                    assert p["sk"] == (1 if rounds == 0 else s), (k, rounds, p)
                    assert rounds == 0 or ((p["sk"] - 1) * p["kchunk"] < k <= p["sk"] * p["kchunk"] and p["kchunk"] % 16 == 0)
                    seen.add(p["sk"])
                    got = _run(ctx, rounds, split, cplx, op, m, n, k, alpha, dA, lda, dB, ldb, c0, 0.0, dC, ldc, C0)
                    # the integer product, bit for bit (+ 0.0: one sign for a zero)
                    assert (got[:, c0:] + 0.0).tobytes() == (want + 0.0).tobytes(), (k, rounds, p)
                    assert got[:, :c0].tobytes() == C0[:, :c0].tobytes()
                    outs[rounds] = got
                assert outs[4].tobytes() == outs[0].tobytes() and outs[16].tobytes() == outs[0].tobytes(), k
        assert seen == {1, 2, 3, 8}
    finally:
        for d in (dA, dB, dC):
            d.free()


@pytest.mark.parametrize("mn", MN, ids=["130x70u", "256x128"])
@pytest.mark.parametrize("split,cplx,op", KINDS, ids=KIND_IDS)
def test_pieces_of_random_operands_within_the_fma_chain_bound(ctx, split, cplx, op, mn):
    m, n, c0 = mn
    st, wide = _types(cplx)
    mp = _plan(ctx, split, cplx, op, m, n, 1, 4)["min_piece_k"]
    kmax = 8 * mp + 37
    rng = np.random.default_rng(20250302 + 2 * split + cplx)
    pad = 3 if c0 else 2                                                     # ldc > m: odd rows unaligned, even rows 16-byte aligned
    ldk = kmax + (0 if c0 else 3)                                            # odd, or a multiple of 4: 16-byte aligned columns
    A = _rand(rng, (m, kmax) if op == "N" else (ldk, m), cplx, st)
    Bw = _rand(rng, (ldk, n + c0), cplx, st)
    Cw = _rand(rng, (m + pad, n + c0 + 2), cplx, wide)                       # sentinel rows below m, sentinel columns beyond n
    lda, ldb, ldc = A.shape[0], ldk, m + pad
    dA, dB = ctx.empty(A.shape, st).upload(A), ctx.empty(Bw.shape, st).upload(Bw)
    dC = ctx.empty(Cw.shape, wide)
    try:
        for (s, r) in ((2, 37), (3, 0), (8, 37)):
            k = s * mp + r
            assert _plan(ctx, split, cplx, op, m, n, k, 4)["sk"] == s
            opA, B = _op(A, op, m, k, wide), Bw[:k, c0:].astype(wide)
            P, absP = opA @ B, np.abs(opA) @ np.abs(B)
            for (alpha, beta) in SCALARS[cplx]:
                C0 = Cw.copy(order="F")
                if beta == 0:
                    C0[:] = np.nan                                           # beta == 0: C is not read
                runs = [_run(ctx, 4, split, cplx, op, m, n, k, alpha, dA, lda, dB, ldb, c0, beta, dC, ldc, C0) for _ in range(2)]
                got = runs[0]
                assert runs[0].tobytes() == runs[1].tobytes()                # bitwise reproducible
                ref = wide(alpha) * P
                bound = (((2 * k + 16) if cplx else (k + 8)) * U + 8 * V64) * abs(alpha) * absP
                if beta != 0:
                    ref = ref + wide(beta) * C0[:m, c0:c0 + n]
                    bound = bound + 8 * V64 * abs(beta) * np.abs(C0[:m, c0:c0 + n])
                assert np.all(np.isfinite(got[:m, c0:c0 + n]))
                err = np.abs(got[:m, c0:c0 + n] - ref)
                print(f"gemm32w {'3' if split else ''}{'cz' if cplx else 'sd'}{op} {m}x{n}x{k} in {s} pieces alpha={alpha} beta={beta}: "
                      f"max err / bound = {np.max(err / bound):.3f}")
                assert np.all(err <= bound), (k, alpha, beta, float(np.max(err / bound)))
                # nothing outside the m x n window was written: rows below m, the columns in front of and beyond it
                keep = C0.copy()
                keep[:m, c0:c0 + n] = got[:m, c0:c0 + n]
                assert got.tobytes() == keep.tobytes()
    finally:
        for d in (dA, dB, dC):
            d.free()


@pytest.mark.parametrize("split,cplx,op", KINDS, ids=KIND_IDS)
def test_below_the_minimum_piece_length_nothing_changes(ctx, split, cplx, op):
    m, n = 130, 70
    st, wide = _types(cplx)
    mp = _plan(ctx, split, cplx, op, m, n, 1, 4)["min_piece_k"]
    k = 2 * mp - 1
    assert _plan(ctx, split, cplx, op, m, n, k, 4)["sk"] == 1
    rng = np.random.default_rng(20250303)
    A = _rand(rng, (m, k) if op == "N" else (k, m), cplx, st)
    B = _rand(rng, (k, n), cplx, st)
    C0 = _rand(rng, (m, n), cplx, wide)
    dA, dB, dC = ctx.empty(A.shape, st).upload(A), ctx.empty(B.shape, st).upload(B), ctx.empty(C0.shape, wide)
    alpha, beta = SCALARS[cplx][2]
    try:
        ctx.gemm_sp_counters(reset=True)
        whole = _run(ctx, 0, split, cplx, op, m, n, k, alpha, dA, A.shape[0], dB, k, 0, beta, dC, m, C0)
        same = _run(ctx, 4, split, cplx, op, m, n, k, alpha, dA, A.shape[0], dB, k, 0, beta, dC, m, C0)
        assert same.tobytes() == whole.tobytes()
        assert ctx.gemm_sp_counters() == (2, 0, 0)
        # k = 0: beta C (leading dimensions of operands nobody reads may be anything legal)
        got = _run(ctx, 4, split, cplx, op, m, n, 0, alpha, dA, A.shape[0], dB, k, 0, beta, dC, m, C0)
        assert np.all(np.abs(got - wide(beta) * C0) <= 8 * V64 * abs(beta) * np.abs(C0))
        # m = 0 or n = 0: nothing to do, status 0, C untouched
        dC.upload(C0)
        ctx.set_gemm_min_rounds(4)
        ctx.gemm32w(op, 0, n, k, alpha, dA.ptr, A.shape[0], dB.ptr, k, beta, dC.ptr, m, cplx, split=split)
        ctx.gemm32w(op, m, 0, k, alpha, dA.ptr, A.shape[0], dB.ptr, k, beta, dC.ptr, m, cplx, split=split)
        assert dC.download().tobytes() == C0.tobytes()
    finally:
        ctx.set_gemm_min_rounds(0)
        for d in (dA, dB, dC):
            d.free()


@pytest.mark.parametrize("split,cplx", [(False, False), (False, True), (True, False), (True, True)],
                         ids=["fp32-d", "fp32-z", "bf16x3-d", "bf16x3-z"])
def test_counters_follow_the_plan(ctx, split, cplx):
    m, n = 130, 70
    st, wide = _types(cplx)
    mp = _plan(ctx, split, cplx, "N", m, n, 1, 4)["min_piece_k"]
    ks = [mp, 2 * mp, 3 * mp + 37, 9 * mp]
    kmax = max(ks)
    A = np.asfortranarray(np.ones((kmax, m), st))                            # k x m: op C
    B = np.asfortranarray(np.ones((kmax, n), st))
    dA, dB = ctx.empty(A.shape, st).upload(A), ctx.empty(B.shape, st).upload(B)
    dC = ctx.empty((m, n), wide).upload(np.zeros((m, n), wide))
    try:
        ctx.gemm_sp_counters(reset=True)
        assert ctx.gemm_sp_counters() == (0, 0, 0)
        calls = splits = pieces = 0
        for rounds in (0, 4):
            ctx.set_gemm_min_rounds(rounds)
            for k in ks:
                sk = _plan(ctx, split, cplx, "C", m, n, k, rounds)["sk"]
                ctx.gemm32w("C", m, n, k, 1.0, dA.ptr, kmax, dB.ptr, kmax, 0.0, dC.ptr, m, cplx, split=split)
                calls += 1
                splits += sk > 1
                pieces += sk if sk > 1 else 0
                assert ctx.gemm_sp_counters() == (calls, splits, pieces), (rounds, k)
                assert np.array_equal(dC.download(), np.full((m, n), k, wide))
        assert splits == 3 and pieces == 2 + 3 + 8
        ctx.set_gemm_min_rounds(0)
        dS = ctx.empty((m, n), st)
        ctx.gemm32("N", m, n, 64, 1.0, dA.ptr, kmax, dB.ptr, kmax, 0.0, dS.ptr, m, cplx, split=split)      # narrow: not counted
        dS.free()
        assert ctx.gemm_sp_counters(reset=True) == (calls, splits, pieces)
        assert ctx.gemm_sp_counters() == (0, 0, 0)
    finally:
        ctx.set_gemm_min_rounds(0)
        for d in (dA, dB, dC):
            d.free()


# ---- the grid: 2 x 2 rank threads on the shared-device transport ---------------------------------------------------------------
def _local(N):
    from chase_amd import dist as cd
    return cd.Layout(N, 0, 2).count(0)


def _smallest_splitting_N(num_cu, cplx, split, panel_cols=64, rounds=4):
    """the smallest N (a multiple of 256) at which a rank of a 2 x 2 block layout cuts a panel product of the filter"""
    from chase_amd import capi
    for N in range(256, 16385, 256):
        loc = _local(N)
        if any(capi.gemm_sp_plan(cplx, op, loc, panel_cols, loc, split=split, num_cu=num_cu, min_rounds=rounds)["sk"] > 1 for op in "NC"):
            return N
    raise AssertionError("no N up to 16384 splits")


def scenario_split_on_the_grid(ctx, grid, comm, N, cplx, split, with_off_legs):
    """one operator-level filter step (tests/mixed_grid_scenarios.py: two products over the unlocked columns) with the filter in
    single precision and the default pipeline: the panel products are cut (panel_rounds = 4 is the default), the result is within
    the propagated bound of that module's docstring against the fp64 emulation, the replicas agree bit for bit; with
    panel_rounds = 0 nothing is cut and the bits are those of a context that never cut anything."""
    from oracle import chase_oracle as O
    n = NEV + NEX
    H = comm.once(("clement", N, cplx), lambda: O.clement(N, cplx))
    Vstart = comm.once(("start", N, cplx), lambda: O.random_start_vectors(N, n, cplx))
    st, wide = _types(cplx)
    keys = dict(mixed_precision=1, sp_product=int(split))
    sp_counters = (2, 2 if split else 0, 0, 2 * (n - LOCK), 1)               # S3.COUNTERS: both products in single precision
    off = None
    if with_off_legs:
        assert ctx.gemm_sp_counters(reset=True)[1] == 0                      # a fresh context: it has never cut a product
        off = S3._filter_leg(ctx, grid, comm, H, Vstart, cplx, 0, dict(keys, panel_rounds=0), 1.0)
        assert off["counters"] == sp_counters
        w, s, p = ctx.gemm_sp_counters(reset=True)
        assert w == 4 and s == 0 and p == 0                                  # two panels per product, none cut
    r = S3._filter_leg(ctx, grid, comm, H, Vstart, cplx, 0, keys, 1.0)
    assert r["counters"] == sp_counters
    w, s, p = ctx.gemm_sp_counters(reset=True)
    loc = _local(N)
    from chase_amd import capi
    want = [capi.gemm_sp_plan(cplx, op, loc, wcols, loc, split=split, num_cu=ctx.info()["num_cu"], min_rounds=4)["sk"]
            for op in "CN" for wcols in (64, n - LOCK - 64)]                 # 91 unlocked columns: a panel of 64 and one of 27
    assert w == 4 and s == sum(x > 1 for x in want) and p == sum(x for x in want if x > 1), (w, s, p, want)
    cut = comm.all_gather_object(s)
    assert any(c > 0 for c in cut), cut                                      # (every rank has the same local shape here: all do)
    rl = r["rl"]
    assert r["V"][:, :LOCK].tobytes() == r["V0"][:, :LOCK].tobytes() and r["h0"] == r["h1"]
    V0 = _gather(comm, grid, rl, N, r["V0"])                                 # (asserts bit-identical replicas)
    V = _gather(comm, grid, rl, N, r["V"])

    def emulate():                                                           # tests/mixed_grid_scenarios.py, module docstring
        Hs = (H - SHIFT * np.eye(N)).astype(st).astype(wide)
        X0 = V0[:, LOCK:].astype(st).astype(wide)
        (a1, _), (a2, b2) = STEPS
        g = R.gamma(N, cplx) if split else ((2 * N + 16) if cplx else (N + 8)) * U32
        wv = (8 + grid.nprow * grid.npcol) * U64
        aH = np.abs(Hs)
        R1 = a1 * (Hs.conj().T @ X0)
        e1 = (g + wv) * abs(a1) * (aH.T @ np.abs(X0))
        X1 = R1.astype(st).astype(wide)
        dx = U32 * (np.abs(R1) + e1) + e1 + U32 * np.abs(R1)
        R2 = a2 * (Hs @ X1) + b2 * V0[:, LOCK:]
        hx = abs(a2) * (aH @ (np.abs(X1) + dx))
        e2 = abs(a2) * (aH @ dx) + g * hx + wv * (hx + abs(b2) * np.abs(V0[:, LOCK:]))
        return R2, e2
    R2, e2 = comm.once(("emulate", N, cplx, split), emulate)
    err = np.abs(V[:, LOCK:] - R2)
    if comm.rank == 0:
        print(f"grid operator level, K pieces {want}, {'bf16x3' if split else 'fp32'} 2x2 N={N}: max err / bound = {np.max(err / e2):.2e}")
    assert np.all(err <= e2), float(np.max(err / e2))
    if with_off_legs:
        again = S3._filter_leg(ctx, grid, comm, H, Vstart, cplx, 0, dict(keys, panel_rounds=0), 1.0)
        assert ctx.gemm_sp_counters(reset=True) == (4, 0, 0)
        assert again["V"].tobytes() == off["V"].tobytes()                    # after the context has cut products and grown its workspace


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "bf16x3"])
def test_grid_filter_step_cuts_its_panel_products(ctx, split):
    cplx = True
    N = _smallest_splitting_N(ctx.info()["num_cu"], cplx, split)
    assert N == (4096 if split else 2048)                                    # local K = two minimum pieces (512 / 1024 complex)
    run_ranks(2, 2, scenario_split_on_the_grid, N, cplx, split, not split, transport="shared")
