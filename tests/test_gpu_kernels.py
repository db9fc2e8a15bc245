"""Parity of every hot-path kernel (through the C ABI) against the CPU oracle / numpy on seeded inputs. GPU only."""
import ctypes as C
import os
import math
import numpy as np
import pytest
from conftest import read_ref_matrix
from oracle import chase_oracle as O
from dense_chain_refs import tridiag_cases as _tridiag_cases

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
# fp64 tolerance: every product must agree with the fp64 numpy result to a few ulp of sum|a||b| (no reduced precision)
GEMM_TOL = 4e-15


def rnd(rng, shape, cplx):
    a = rng.standard_normal(shape)
    if cplx:
        a = a + 1j * rng.standard_normal(shape)
    return np.asfortranarray(a)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("op", ["N", "C"])
@pytest.mark.parametrize("shape", [(128, 128, 64), (130, 67, 45), (1, 1, 1), (17, 300, 1000), (300, 17, 33),
                                   (512, 192, 777), (64, 64, 4096), (200, 140, 5000), (257, 129, 8), (0, 5, 3)])
def test_gemm_matches_numpy(ctx, cplx, op, shape):
    m, n, k = shape
    rng = np.random.default_rng(1234 + m + 3 * n + 7 * k)
    A = rnd(rng, (m, k) if op == "N" else (k, m), cplx)
    B = rnd(rng, (k, n), cplx)
    Cm = rnd(rng, (m, n), cplx)
    alpha = (0.7 - 0.3j) if cplx else 0.7
    for beta in (0.0, (-0.4 + 0.2j) if cplx else -0.4):
        dA, dB, dC = ctx.array(A), ctx.array(B), ctx.array(Cm)
        ctx.gemm(op, m, n, k, alpha, dA.ptr, max(dA.ld, 1), dB.ptr, max(dB.ld, 1), beta, dC.ptr, max(dC.ld, 1), cplx)
        got = dC.download()
        opA = A if op == "N" else A.conj().T
        ref = alpha * (opA @ B) + beta * Cm
        scale = abs(alpha) * (np.abs(opA) @ np.abs(B)) + abs(beta) * np.abs(Cm) + 1e-300
        if m and n:
            assert np.max(np.abs(got - ref) / scale) < GEMM_TOL
        for d in (dA, dB, dC):
            d.free()


@pytest.mark.parametrize("op", ["N", "C"])
@pytest.mark.parametrize("shape", [(256, 64, 512), (256, 70, 512), (384, 133, 1024), (128, 200, 4096), (2048, 320, 2048),
                                   (130, 64, 512), (256, 64, 516)])
def test_filter_phase_gemm_3m_matches_numpy(ctx, op, shape):
    """Products issued between FilterPhaseStart/End (phase 1) use the three-multiplication complex scheme when the shape
    allows it (whole 128-row tiles, K a multiple of 8) and the four-multiplication kernel otherwise (last two shapes);
    both must meet the same componentwise bound, whole and ragged widths, K-split tails, beta != 0."""
    from chase_amd.capi import lib
    m, n, k = shape
    rng = np.random.default_rng(77 + m + 3 * n + 7 * k)
    A = rnd(rng, (m, k) if op == "N" else (k, m), True)
    B = rnd(rng, (k, n), True)
    Cm = rnd(rng, (m, n), True)
    alpha = 0.7 - 0.3j
    opA = A if op == "N" else A.conj().T
    lib.chase_hip_ctx_set_phase(ctx.h, 1)
    try:
        for beta in (0.0, -0.4 + 0.2j):
            dA, dB, dC = ctx.array(A), ctx.array(B), ctx.array(Cm)
            ctx.gemm(op, m, n, k, alpha, dA.ptr, dA.ld, dB.ptr, dB.ld, beta, dC.ptr, dC.ld, True)
            got = dC.download()
            ref = alpha * (opA @ B) + beta * Cm
            scale = abs(alpha) * (np.abs(opA) @ np.abs(B)) + abs(beta) * np.abs(Cm)
            assert np.max(np.abs(got - ref) / scale) < 4 * GEMM_TOL
            for d in (dA, dB, dC):
                d.free()
    finally:
        lib.chase_hip_ctx_set_phase(ctx.h, 0)


@pytest.mark.parametrize("op", ["N", "C"])
@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("shape", [(256, 40, 512), (384, 64, 1024), (130, 33, 77), (256, 5, 8192), (1024, 48, 4096),
                                   (128, 17, 16), (2048, 133, 2048), (4096, 300, 4096), (4096, 200, 4100), (513, 60, 1000)])
def test_real_narrow_tile_matches_numpy(ctx, op, phase, shape):
    """Real products on the 128 x 64 tile (three LDS stages, software-pipelined K loop): blocks of at most 64 columns and the
    ragged rest of a width (133 = 128 + 5, 300 = 256 + 44, 200 = 128 + 72 in two narrow tiles of 48); LDS-DMA path (whole row
    tiles, even leading dimensions) and the guarded register path (ragged M, partial K tile), K-split tails, beta != 0."""
    from chase_amd.capi import lib
    m, n, k = shape
    rng = np.random.default_rng(991 + m + 3 * n + 7 * k)
    A = rnd(rng, (m, k) if op == "N" else (k, m), False)
    B = rnd(rng, (k, n), False)
    Cm = rnd(rng, (m, n), False)
    opA = A if op == "N" else A.T
    lib.chase_hip_ctx_set_phase(ctx.h, phase)
    try:
        for beta in (0.0, -0.4):
            dA, dB, dC = ctx.array(A), ctx.array(B), ctx.array(Cm)
            ctx.gemm(op, m, n, k, 0.7, dA.ptr, dA.ld, dB.ptr, dB.ld, beta, dC.ptr, dC.ld, False)
            got = dC.download()
            ref = 0.7 * (opA @ B) + beta * Cm
            scale = 0.7 * (np.abs(opA) @ np.abs(B)) + abs(beta) * np.abs(Cm) + 1e-300
            assert np.max(np.abs(got - ref) / scale) < GEMM_TOL
            for d in (dA, dB, dC):
                d.free()
    finally:
        lib.chase_hip_ctx_set_phase(ctx.h, 0)


def test_gemm_beta_zero_ignores_nan_in_c(ctx):
    rng = np.random.default_rng(0)
    A, B = rnd(rng, (64, 32), False), rnd(rng, (32, 16), False)
    dA, dB = ctx.array(A), ctx.array(B)
    dC = ctx.array(np.full((64, 16), np.nan))
    ctx.gemm("N", 64, 16, 32, 1.0, dA.ptr, 64, dB.ptr, 32, 0.0, dC.ptr, 64, False)
    assert np.all(np.isfinite(dC.download()))


def test_gemm_strided_views_and_column_offsets(ctx):
    # the filter works on column windows [locked+offset, +ncols) of wider buffers (chase_cpu.hpp:497-504)
    rng = np.random.default_rng(5)
    N, n = 300, 40
    H, V, W = rnd(rng, (N, N), True), rnd(rng, (N, n), True), rnd(rng, (N, n), True)
    dH, dV, dW = ctx.array(H), ctx.array(V), ctx.array(W)
    c0, nc = 7, 21
    ctx.gemm("N", N, nc, N, 0.3 + 0.1j, dH.ptr, N, dV.offset(c0), N, -0.5, dW.offset(c0), N, True)
    got = dW.download()
    ref = W.copy()
    ref[:, c0:c0 + nc] = (0.3 + 0.1j) * (H @ V[:, c0:c0 + nc]) - 0.5 * W[:, c0:c0 + nc]
    assert np.max(np.abs(got - ref)) < 1e-11
    assert np.array_equal(got[:, :c0], W[:, :c0]) and np.array_equal(got[:, c0 + nc:], W[:, c0 + nc:])


def test_gemm_rejects_bad_arguments(ctx):
    from chase_amd.capi import ChaseHipError
    d = ctx.array(np.zeros((4, 4)))
    with pytest.raises(ChaseHipError):
        ctx.gemm("X", 4, 4, 4, 1.0, d.ptr, 4, d.ptr, 4, 0.0, d.ptr, 4, False)
    with pytest.raises(ChaseHipError):
        ctx.gemm("N", 4, 4, 4, 1.0, d.ptr, 2, d.ptr, 4, 0.0, d.ptr, 4, False)


def test_hemm_known_answer_49_986(ctx):
    # the reference's HEMM KAT (tests/linalg/internal/mpi/hemm.cpp:36-119) through the Impl's HEMM virtual
    from chase_amd.capi import Solver
    H = np.ones((10, 10), order="F")
    V = np.full((10, 4), 2.0, order="F")
    s = Solver(ctx, H, 2, 2, V=V)
    s.Start()
    s.initVecs(False)                       # V1 = V2 = 2; H -> device
    # make V2 == 3: V2 = 0*H*V1... use HEMM itself: beta path needs V2 = 3, so upload via a second solver-free route
    lib = __import__("chase_amd.capi", fromlist=["lib"]).lib
    s.HEMM(4, 0.0, 1.5, 0)                  # V2 = 1.5 * V2 = 3 on all 4 columns, swap -> V1 == 3, V2 == 2
    s.HEMM(0, 0.0, 0.0, 0)                  # ncols == 0: pure pointer swap -> V1 == 2, V2 == 3
    s.HEMM(2, 2.0, 3.0, 0)
    v = s.peek_v()
    assert np.all(v[:, :2] == 49.0) and np.all(v[:, 2:] == 3.0)
    s.HEMM(2, 2.0, 3.0, 0)
    v = s.peek_v()
    assert np.all(v[:, :2] == 986.0) and np.all(v[:, 2:] == 2.0)
    s.close()


@pytest.mark.parametrize("cplx", [False, True])
def test_cholqr_reference_fixtures(ctx, cplx):
    # same fixtures and thresholds as tests/linalg/internal/cpu/cholqr1.cpp:31-126
    from chase_amd.capi import lib, check
    pre = "matrix_cdouble_" if cplx else "matrix_double_"
    m, n = 100, 50

    def run(name, variant):
        V = read_ref_matrix(pre + name, m, n, cplx)
        dV = ctx.array(V)
        dA = ctx.empty((n, n), V.dtype)
        info = lib.chase_hip_cholqr(ctx.h, int(cplx), m, n, dV.ptr, m, dA.ptr, n, variant, m)
        assert info >= 0, lib.chase_hip_last_error()
        Q = dV.download()
        dV.free(); dA.free()
        return info, Q, V

    info, Q, _ = run("cond_10.bin", 1)
    assert info == 0 and abs(O.orthogonality(Q) - EPS) <= 15 * EPS
    info, Q, _ = run("cond_1e4.bin", 1)
    assert info == 0 and EPS < O.orthogonality(Q) < 1.0
    info, Q, V = run("cond_ill.bin", 1)
    assert 0 < info <= n and np.array_equal(Q, V)          # failed first potrf leaves V untouched
    info, Q, _ = run("cond_1e4.bin", 2)
    assert info == 0 and abs(O.orthogonality(Q) - EPS) <= 15 * EPS
    info, _, _ = run("cond_ill.bin", 2)
    assert 0 < info <= n
    info, Q, V = run("cond_ill.bin", 3)
    assert info == 0 and abs(O.orthogonality(Q) - EPS) <= 10 * EPS
    # Q spans the same space: V = Q (Q^H V)
    assert np.linalg.norm(V - Q @ (Q.conj().T @ V)) <= 1e-10 * np.linalg.norm(V)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("shape", [(100, 50), (777, 130), (2048, 256), (300, 300), (65, 1)])
def test_houseqr_orthogonality_and_span(ctx, cplx, shape):
    from chase_amd.capi import lib
    m, n = shape
    rng = np.random.default_rng(m * 31 + n)
    V = rnd(rng, (m, n), cplx)
    V[:, n // 2] = V[:, 0] * (1 + 1e-13)                   # nearly dependent columns: CholQR territory is left
    dV = ctx.array(V)
    rc = lib.chase_hip_houseqr(ctx.h, int(cplx), m, n, dV.ptr, m)
    assert rc == 0, lib.chase_hip_last_error()
    Q = dV.download()
    assert O.orthogonality(Q) <= 25 * EPS                  # tests/linalg/internal/mpi/householder_qr.cpp:46-93
    R = Q.conj().T @ V
    assert np.linalg.norm(V - Q @ R) <= 1e-12 * np.linalg.norm(V)
    assert np.linalg.norm(np.tril(R, -1)) <= 1e-11 * np.linalg.norm(R)   # R is upper triangular


@pytest.mark.parametrize("nb", ["8", "17", "48", "200"])
def test_houseqr_panel_width_knob_of_the_reference(ctx, nb, monkeypatch):
    """CHASE_HOUSEHOLDER_NB (Impl/pchase_cpu/pchase_cpu.hpp:590-596, pchase_gpu.hpp:1065: the outer block width of the
    reference's Householder QR; tests/linalg/internal/nccl/householder_qr.cpp:218-260 runs its test with the env knobs set):
    read at every call, any width up to the panel kernels' capacity (larger values are clamped), same assertions"""
    from chase_amd.capi import lib
    monkeypatch.setenv("CHASE_HOUSEHOLDER_NB", nb)
    for cplx, (m, n) in ((False, (500, 130)), (True, (301, 97))):
        rng = np.random.default_rng(7)
        V = rnd(rng, (m, n), cplx)
        dV = ctx.array(V)
        assert lib.chase_hip_houseqr(ctx.h, int(cplx), m, n, dV.ptr, m) == 0, lib.chase_hip_last_error()
        Q = dV.download()
        assert O.orthogonality(Q) <= 25 * EPS
        R = Q.conj().T @ V
        assert np.linalg.norm(V - Q @ R) <= 1e-12 * np.linalg.norm(V)
        assert np.linalg.norm(np.tril(R, -1)) <= 1e-11 * np.linalg.norm(R)


@pytest.mark.parametrize("cplx", [False, True])
def test_houseqr_on_ill_conditioned_fixture(ctx, cplx):
    from chase_amd.capi import lib
    pre = "matrix_cdouble_" if cplx else "matrix_double_"
    V = read_ref_matrix(pre + "cond_ill.bin", 100, 50, cplx)
    dV = ctx.array(V)
    assert lib.chase_hip_houseqr(ctx.h, int(cplx), 100, 50, dV.ptr, 100) == 0
    assert O.orthogonality(dV.download()) <= 25 * EPS


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200, 333])
def test_potrf_and_trsm(ctx, cplx, n):
    from chase_amd.capi import lib
    rng = np.random.default_rng(n)
    X = rnd(rng, (2 * n + 3, n), cplx)
    A = np.asfortranarray(X.conj().T @ X + n * np.eye(n))
    dA = ctx.array(A)
    info = lib.chase_hip_potrf_upper(ctx.h, int(cplx), n, dA.ptr, n)
    assert info == 0
    R = np.triu(dA.download())
    assert np.linalg.norm(R.conj().T @ R - A) <= 50 * EPS * np.linalg.norm(A)
    m = 150
    V = rnd(rng, (m, n), cplx)
    dV = ctx.array(V)
    assert lib.chase_hip_trsm_right_upper(ctx.h, int(cplx), m, n, dA.ptr, n, dV.ptr, m) == 0
    Xs = dV.download()
    assert np.linalg.norm(Xs @ R - V) <= 1e-12 * np.linalg.norm(V) * np.linalg.cond(R)
    # not positive definite -> LAPACK info
    A2 = A.copy(); k = n // 2; A2[k, k] = -1.0
    dA2 = ctx.array(A2)
    info = lib.chase_hip_potrf_upper(ctx.h, int(cplx), n, dA2.ptr, n)
    assert info == k + 1


def test_plane_fed_3m_loop_on_random_shapes(ctx):
    """Round 6's 3M loop has its own prologue / epilogue cases (1, 2, 3, 4+ K steps; the plane ring's two stages; ragged and
    uniform-ragged column tiles; K-split tails; leading dimensions larger than the block; column offsets into B and C): 40 seeded
    random shapes with m a multiple of 128 and k of 8 (the shapes that take the three-multiplication kernels as they stand), both ops,
    alpha / beta complex, against numpy to a few ulp of sum |a||b| - and the surroundings of C untouched."""
    from chase_amd.capi import lib, gemm_counters
    rng = np.random.default_rng(606)
    lib.chase_hip_ctx_set_phase(ctx.h, 1)
    try:
        for t in range(40):
            m = 128 * int(rng.integers(1, 9))
            k = 8 * int(rng.choice([1, 2, 3, 4, 5, 7, 16, 33, 64, 130]))
            n = int(rng.choice([1, 15, 16, 17, 40, 63, 64, 65, 100, 128, 133, 200]))
            op = "N" if t % 2 == 0 else "C"
            rounds = 4 if t % 5 == 0 else 0
            lib.chase_hip_ctx_set_gemm_min_rounds(ctx.h, rounds)
            pa, pb, pc = int(rng.integers(0, 3)) * 2, int(rng.integers(0, 3)), int(rng.integers(0, 5))
            A = rnd(rng, ((m if op == "N" else k) + pa, k if op == "N" else m), True)
            B, Cm = rnd(rng, (k + pb, n + 2), True), rnd(rng, (m + pc, n + 2), True)
            opA = A[:m, :] if op == "N" else A[:k, :].conj().T
            alpha, beta = 0.7 - 0.2j, (0.0 if t % 3 == 0 else -0.4 + 0.1j)
            dA, dB, dC = ctx.array(A), ctx.array(B), ctx.array(Cm)
            gemm_counters(ctx, 1, reset=True)
            ctx.gemm(op, m, n, k, alpha, dA.ptr, A.shape[0], dB.offset(1), B.shape[0], beta, dC.offset(1), Cm.shape[0], True)
            model, execd, _ = gemm_counters(ctx, 1)
            got = dC.download()
            ref = Cm.copy()
            ref[:m, 1:n + 1] = alpha * (opA @ B[:k, 1:n + 1]) + beta * Cm[:m, 1:n + 1]
            bound = (np.abs(opA) @ np.abs(B[:k, 1:n + 1])).max() + np.abs(Cm).max()
            assert np.max(np.abs(got - ref)) <= 16 * EPS * bound, (t, op, m, n, k, rounds)
            assert np.array_equal(got[m:, :], Cm[m:, :]) and np.array_equal(got[:, 0], Cm[:, 0]) and np.array_equal(got[:, n + 1], Cm[:, n + 1])
            assert execd == pytest.approx(0.75 * model), (t, op, m, n, k)          # it really ran on three multiplications
            for a in (dA, dB, dC):
                a.free()
    finally:
        lib.chase_hip_ctx_set_gemm_min_rounds(ctx.h, 0)
        lib.chase_hip_ctx_set_phase(ctx.h, 0)


def test_three_multiplication_products_keep_their_bits_across_rounds(ctx):
    """Round 6 rebuilt the 3M filter loop (V-side operand sums from a precomputed plane, another MFMA order, another LDS layout)
    under the condition that NOTHING changes numerically: the plane holds the same IEEE sums, the accumulators are independent.
    tests/golden/gemm3m_hashes.json holds the 64-bit content hashes of 26 products (whole tiles, ragged and uniform-ragged
    widths, K-split tails, rims cut off as 4M products, both ops, phases 1 and 2) that round 2-5's loop and round 6's produced
    identically on one device; the inputs are device-generated from fixed seeds, so the hashes pin the kernels' bits from now on."""
    import json
    from chase_amd.capi import lib
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm3m_hashes.json")))["rows"]
    assert len(gold) == 26
    try:
        for g in gold:
            if g["m"] * g["n"] * g["k"] > 3e11:                  # the two N = 16384 x 2560 products: 0.2 s each, once is enough
                if g["phase"] == 2:
                    continue
            op, m, n, k = g["op"], g["m"], g["n"], g["k"]
            ra = (m, k) if op == "N" else (k, m)
            dA = ctx.empty(ra, np.complex128); dB = ctx.empty((k, n), np.complex128); dC = ctx.empty((m, n), np.complex128)
            for (d, r, c, seed) in ((dA, ra[0], ra[1], 1), (dB, k, n, 2), (dC, m, n, 3)):
                assert lib.chase_hip_fill_normal(ctx.h, 1, r, c, d.ptr, r, 0, 0, r, seed) == 0
            lib.chase_hip_ctx_set_phase(ctx.h, g["phase"])
            ctx.gemm(op, m, n, k, 0.5 - 0.25j, dA.ptr, ra[0], dB.ptr, k, 0.25 + 0.5j, dC.ptr, m, True)
            h = ctx.hash64(dC.ptr, m, n, m, True)
            for a in (dA, dB, dC):
                a.free()
            assert "%016x" % h == g["hash"], (g, "%016x" % h)
    finally:
        lib.chase_hip_ctx_set_phase(ctx.h, 0)


@pytest.mark.parametrize("cplx", [False, True])
def test_reference_small_kernel_known_answers(ctx, cplx):
    """The reference's own known-answer tests of the small helpers on the path, same inputs and expected values:
    absTrace (tests/linalg/internal/cuda/absTrace.cpp:27-53: 3x3 in ld 4, entries i+1, buffer[5] = -4 -> 16),
    shiftDiagonal (cuda/shiftDiagonal.cpp:28-62: 4x3, shift -2 -> {-1,2,3,4,5,4,7,8,9,10,9,12}),
    lacpy full copy (cuda/lacpy.cpp:28-58: 3x3 out of ld 4 into ld 3)."""
    from chase_amd.capi import lib, check
    dt = np.complex128 if cplx else np.float64
    buf = np.arange(1, 13, dtype=dt)
    b = buf.copy(); b[5] = -4
    dA = ctx.array(np.asfortranarray(b.reshape((4, 3), order="F")))
    out = C.c_double(0)
    check(lib.chase_hip_abs_trace(ctx.h, int(cplx), 3, dA.ptr, 4, C.byref(out)), "abs_trace")
    assert out.value == 16.0
    dB = ctx.array(np.asfortranarray(buf.reshape((4, 3), order="F")))
    check(lib.chase_hip_shift_diag(ctx.h, int(cplx), 3, dB.ptr, 4, -2.0), "shift")
    assert np.array_equal(dB.download().ravel(order="F"), np.array([-1, 2, 3, 4, 5, 4, 7, 8, 9, 10, 9, 12], dtype=dt))
    dS = ctx.array(np.asfortranarray(buf.reshape((4, 3), order="F")))
    dT = ctx.empty((3, 3), dt)
    check(lib.chase_hip_lacpy(ctx.h, int(cplx), 3, 3, dS.ptr, 4, dT.ptr, 3), "lacpy")
    assert np.array_equal(dT.download(), buf.reshape((4, 3), order="F")[:3, :])


@pytest.mark.parametrize("cplx", [False, True])
def test_shift_swap_lacpy_resid(ctx, cplx):
    from chase_amd.capi import lib, check
    rng = np.random.default_rng(11)
    N, n = 257, 19
    H = rnd(rng, (N, N), cplx)
    dH = ctx.array(H)
    check(lib.chase_hip_shift_diag(ctx.h, int(cplx), N, dH.ptr, N, -2.5), "shift")
    ref = H.copy(); ref[np.arange(N), np.arange(N)] += -2.5          # exact: tests/linalg/internal/mpi/shiftDiagonal.cpp
    assert np.array_equal(dH.download(), ref)
    V = rnd(rng, (N, n), cplx)
    dV = ctx.array(V)
    check(lib.chase_hip_swap_cols(ctx.h, int(cplx), N, dV.ptr, N, 2, 17), "swap")
    ref = V.copy(); ref[:, [2, 17]] = ref[:, [17, 2]]
    assert np.array_equal(dV.download(), ref)
    dW = ctx.empty((N, n), V.dtype)
    check(lib.chase_hip_lacpy(ctx.h, int(cplx), N - 5, n - 3, dV.ptr + 2 * V.itemsize, N, dW.ptr, N), "lacpy")
    assert np.array_equal(dW.download()[:N - 5, :n - 3], ref[2:N - 3, :n - 3])
    # residual norms vs the oracle
    W = rnd(rng, (N, n), cplx)
    lam = rng.standard_normal(n)
    dW.upload(W)
    out = np.zeros(n)
    check(lib.chase_hip_resid_norms(ctx.h, int(cplx), N, n, dW.ptr, N, dV.ptr, N, lam.ctypes.data, out.ctypes.data, 0), "resid")
    want = np.linalg.norm(W - ref * lam[None, :], axis=0)
    assert np.max(np.abs(out - want) / want) < 1e-14
    # deferred permutation == the same sequence of swaps
    src = np.array([3, 0, 5], dtype=np.int32); dst = np.array([0, 5, 3], dtype=np.int32)
    check(lib.chase_hip_permute_cols(ctx.h, int(cplx), N, dV.ptr, N, dW.ptr, N, src.ctypes.data_as(C.POINTER(C.c_int)),
                                     dst.ctypes.data_as(C.POINTER(C.c_int)), 3), "permute")
    ref2 = ref.copy(); ref2[:, dst] = ref[:, src]
    assert np.array_equal(dV.download(), ref2)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n", [150, 385, 700])          # < 384: host LAPACK; >= 384: GPU tridiagonalisation path
def test_heevd_matches_scipy(ctx, cplx, n):
    from chase_amd.capi import lib, check
    import scipy.linalg as sla
    rng = np.random.default_rng(3)
    X = rnd(rng, (n, n), cplx)
    A = np.asfortranarray(X + X.conj().T)
    dA = ctx.array(A)
    w = np.zeros(n)
    check(lib.chase_hip_heevd(ctx.h, int(cplx), n, dA.ptr, n, w.ctypes.data), "heevd")
    Z = dA.download()
    assert np.max(np.abs(w - sla.eigvalsh(A))) <= 100 * EPS * np.abs(w).max()
    assert np.linalg.norm(A @ Z - Z * w[None, :]) <= 1e-12 * np.linalg.norm(A)
    assert O.orthogonality(Z) <= 50 * EPS


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n", [3, 4, 65, 257])
def test_heevd_gpu_small_and_degenerate(ctx, cplx, n):
    """GPU tridiagonalisation on tiny sizes and on a matrix with repeated eigenvalues / zero sub-columns."""
    from chase_amd.capi import lib
    import scipy.linalg as sla
    rng = np.random.default_rng(n)
    X = rnd(rng, (n, n), cplx)
    Q, _ = np.linalg.qr(X)
    lam = np.repeat(np.arange(1.0, n // 2 + 2), 2)[:n]            # every eigenvalue twice
    A = np.asfortranarray((Q * lam[None, :]) @ Q.conj().T)
    A[:, 0] = 0; A[0, :] = 0; A[0, 0] = 7.5                        # decoupled first row/column: tau = 0 branch
    A = np.asfortranarray((A + A.conj().T) / 2)
    dA = ctx.array(A)
    w = np.zeros(n)
    assert lib.chase_hip_heevd_gpu(ctx.h, int(cplx), n, dA.ptr, n, w.ctypes.data) == 0, lib.chase_hip_last_error()
    Z = dA.download()
    assert np.max(np.abs(w - sla.eigvalsh(A))) <= 200 * EPS * np.abs(w).max()
    assert np.linalg.norm(A @ Z - Z * w[None, :]) <= 1e-12 * max(1.0, np.linalg.norm(A))
    assert O.orthogonality(Z) <= 100 * EPS


# ---- matrix files (the reference's raw column-major input format) -------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
def test_matrix_file_roundtrip_and_shards(ctx, tmp_path, cplx):
    """save -> load round trip; block and block-cyclic shards read from the file equal the slices of the matrix;
    the reference's own fixture file loads bit-exactly; a short file is an error (matrix.hpp:313-360)."""
    from chase_amd import dist as cd
    from chase_amd.capi import lib
    rng = np.random.default_rng(5)
    N = 75
    A = rng.standard_normal((N, N)) + (1j * rng.standard_normal((N, N)) if cplx else 0)
    A = np.asfortranarray(A.astype(np.complex128 if cplx else np.float64))
    path = tmp_path / "A.bin"
    ctx.save_matrix(path, ctx.array(A))
    assert np.array_equal(np.fromfile(path, dtype=A.dtype).reshape(N, N, order="F"), A)
    assert np.array_equal(ctx.load_matrix(path, N, cplx).download(), A)
    for (mb, pr, pc) in [(0, 2, 2), (0, 3, 2), (8, 2, 3), (16, 4, 2)]:
        rl, cl = cd.Layout(N, mb, pr), cd.Layout(N, mb, pc)
        for i in range(pr):
            for j in range(pc):
                blk = cd.load_matrix_local(ctx, path, N, cplx, rl, cl, i, j).download()
                assert np.array_equal(blk, A[np.ix_(rl.globals_of(i), cl.globals_of(j))])
    # a larger file is accepted (leading N x N of the byte stream), a smaller one is refused
    assert np.array_equal(ctx.load_matrix(path, N - 5, cplx).download(),
                          np.fromfile(path, dtype=A.dtype)[: (N - 5) ** 2].reshape(N - 5, N - 5, order="F"))
    with pytest.raises(Exception):
        ctx.load_matrix(path, N + 1, cplx)
    with pytest.raises(Exception):
        ctx.load_matrix(tmp_path / "missing.bin", N, cplx)
    if cplx:   # the reference's own BSE fixture file (tests/linalg/internal/BSE_matrices), as its tests read it
        import os
        from conftest import REF_FIX
        ref = read_ref_matrix("cdouble_random_BSE.bin", 200, 200, True)
        assert np.array_equal(ctx.load_matrix(os.path.join(REF_FIX, "cdouble_random_BSE.bin"), 200, True).download(), ref)


# ---- sign flips / conjugation of the pseudo-Hermitian path ---------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
def test_flip_lower_half_sign_known_answer(ctx, cplx):
    """tests/linalg/internal/cpu/flipSign.cpp:27-54 (cuda/flipSign.cpp): 10 x 10 of ones, the lower half of every column
    changes sign, the upper half is untouched — with the sequential kernel and with the block / block-cyclic variant that
    decides by GLOBAL row index (mpi/flipSign.hpp:20-100)."""
    from chase_amd.capi import lib, check
    N = 10
    one = np.ones((N, N), dtype=np.complex128 if cplx else np.float64, order="F")
    d = ctx.array(one)
    check(lib.chase_hip_scale_rows(ctx.h, int(cplx), N, N, d.ptr, N, N // 2, -1.0), "scale_rows")
    got = d.download()
    assert np.all(got[: N // 2] == 1) and np.all(got[N // 2:] == -1)
    # distributed: every rank of a p-rank block / block-cyclic row distribution flips exactly its rows with g >= N/2
    N = 37
    for (nb, p) in [(0, 1), (0, 2), (0, 3), (4, 2), (5, 3), (64, 2)]:
        bl = nb if nb else (N // p if N % p == 0 else N // p + 1)
        for q in range(p):
            gl = [g for g in range(N) if (g // bl) % p == q]
            m = len(gl)
            if m == 0:
                continue
            x = (np.arange(m * 3, dtype=np.float64).reshape(m, 3, order="F") + 1.0).astype(one.dtype)
            d = ctx.array(np.asfortranarray(x))
            check(lib.chase_hip_scale_rows_bc(ctx.h, int(cplx), m, 3, d.ptr, m, N // 2, bl, p, q, -1.0), "scale_rows_bc")
            want = x.copy()
            want[[i for i, g in enumerate(gl) if g >= N // 2], :] *= -1
            assert np.array_equal(d.download(), want), (nb, p, q)


def test_conj_inplace(ctx):
    from chase_amd.capi import lib, check
    rng = np.random.default_rng(9)
    X = np.asfortranarray(rng.standard_normal((33, 5)) + 1j * rng.standard_normal((33, 5)))
    d = ctx.array(X)
    check(lib.chase_hip_conj(ctx.h, 33, 5, d.ptr, 33), "conj")
    assert np.array_equal(d.download(), X.conj())



def _ld_matmul(A, B):
    Ar, Ai = A.real.astype(np.longdouble), A.imag.astype(np.longdouble)
    Br, Bi = B.real.astype(np.longdouble), B.imag.astype(np.longdouble)
    return (Ar @ Br - Ai @ Bi), (Ar @ Bi + Ai @ Br)


@pytest.mark.parametrize("imag_scale", [1.0, 1e-8])
def test_three_vs_four_multiplication_accuracy(ctx, imag_scale):
    """The filter's three-multiplication complex scheme (HISTORY.md §3.1c) against a long-double product, next to the
    four-multiplication kernel (the reference's zgemm arithmetic), on generic AND on nearly real operands (the bench matrix
    is nearly real): 3M must meet the NORMWISE bound |C - AB| <= c k eps |A||B| (entrywise in terms of the moduli), 4M the
    componentwise-in-real-arithmetic bound on the real and on the imaginary part separately.  Also checks the switch: the
    3M launch executes 3/4 of the model flops, the 4M launch all of them; phase 1 (filter) and - since round 4 - phase 2
    (H-times-block of Rayleigh-Ritz / residuals) take 3M, phase 3 (verification products) and phase 0 never do."""
    from chase_amd.capi import lib, gemm_counters
    rng = np.random.default_rng(3)
    m, k, n = 256, 4096, 64
    H = rng.standard_normal((m, k)) + 1j * imag_scale * rng.standard_normal((m, k))
    V = rng.standard_normal((k, n)) + 1j * imag_scale * rng.standard_normal((k, n))
    A, B = np.asfortranarray(H), np.asfortranarray(V)
    Rr, Ri = _ld_matmul(A, B)
    mod = np.abs(A) @ np.abs(B)                                           # |A||B| with complex moduli
    re_scale = np.abs(A.real) @ np.abs(B.real) + np.abs(A.imag) @ np.abs(B.imag)
    im_scale = np.abs(A.real) @ np.abs(B.imag) + np.abs(A.imag) @ np.abs(B.real)
    dA, dB = ctx.array(A), ctx.array(B)
    res = {}
    for name, phase, on in (("4M", 1, 0), ("3M", 1, 1), ("phase2", 2, 1), ("phase3", 3, 1), ("phase0", 0, 1)):
        lib.chase_hip_set_gemm3m(on)
        lib.chase_hip_ctx_set_phase(ctx.h, phase)
        try:
            m0, e0, _ = gemm_counters(ctx, phase)
            dC = ctx.array(np.zeros((m, n), dtype=complex, order="F"))
            ctx.gemm("N", m, n, k, 1.0, dA.ptr, m, dB.ptr, k, 0.0, dC.ptr, m, True)
            C = dC.download()
            m1, e1, _ = gemm_counters(ctx, phase)
        finally:
            lib.chase_hip_ctx_set_phase(ctx.h, 0)
            lib.chase_hip_set_gemm3m(1)
        er = np.abs(C.real.astype(np.longdouble) - Rr).astype(np.float64)
        ei = np.abs(C.imag.astype(np.longdouble) - Ri).astype(np.float64)
        res[name] = (er, ei, (e1 - e0) / (m1 - m0))
        assert m1 - m0 == 2.0 * 4 * m * n * k
    # executed share of the model flops: exactly 3/4 for the 3M launches, 1 for 4M, verification and ordinary products
    assert res["3M"][2] == 0.75 and res["4M"][2] == 1.0 and res["phase2"][2] == 0.75
    assert res["phase3"][2] == 1.0 and res["phase0"][2] == 1.0
    for name in ("4M", "phase3", "phase0"):
        er4, ei4, _ = res[name]
        assert np.max(er4 / re_scale) < 4 * GEMM_TOL and np.max(ei4 / im_scale) < 4 * GEMM_TOL  # componentwise (4M)
    er4, ei4, _ = res["4M"]
    for name in ("3M", "phase2"):
        er3, ei3, _ = res[name]
        assert np.max(np.hypot(er3, ei3) / mod) < 8 * GEMM_TOL                                  # normwise (3M)
    er3, ei3, _ = res["3M"]
    if imag_scale < 1e-4:
        # documents WHY 3M stays inside the filter: the tiny imaginary part inherits the real part's absolute error
        assert np.max(ei3 / im_scale) > 100 * np.max(ei4 / im_scale)
    for d in (dA, dB):
        d.free()


@pytest.mark.parametrize("cplx,n", [(True, 700), (False, 1100)])
def test_heevd_gpu_is_bitwise_reproducible(ctx, cplx, n):
    """The blocked tridiagonalisation runs many small dependent launches that share panel buffers between workgroups; every
    reduction has a fixed order, so repeated runs must agree bit for bit (a cross-workgroup race shows up here first: in
    round 2 one made a config-4 solve take 22 instead of 9 iterations under the profiler's timing)."""
    from chase_amd.capi import lib
    rng = np.random.default_rng(n)
    X = rnd(rng, (n, n), cplx)
    A = np.asfortranarray(X + X.conj().T)
    outs = []
    for rep in range(6):
        dA = ctx.array(A)
        w = np.zeros(n)
        assert lib.chase_hip_heevd_gpu(ctx.h, int(cplx), n, dA.ptr, n, w.ctypes.data) == 0, lib.chase_hip_last_error()
        outs.append((w.copy(), dA.download()))
        dA.free()
    for w, Z in outs[1:]:
        assert np.array_equal(w, outs[0][0]) and np.array_equal(Z, outs[0][1])
    w, Z = outs[0]
    assert np.linalg.norm(A @ Z - Z * w[None, :]) <= 1e-12 * np.linalg.norm(A)


def test_filter_gemm_is_bitwise_reproducible(ctx):
    """3M pipelined filter kernel (LDS stages refilled while fragments are re-read), split-K tail and uniform ragged tiling:
    identical operands must give identical bits on every launch."""
    from chase_amd.capi import lib
    rng = np.random.default_rng(9)
    N = 2048
    H, V, W = rnd(rng, (N, N), True), rnd(rng, (N, 200), True), rnd(rng, (N, 200), True)
    dH, dV = ctx.array(H), ctx.array(V)
    lib.chase_hip_ctx_set_phase(ctx.h, 1)
    try:
        for ncols in (200, 133, 64):
            outs = []
            for rep in range(5):
                dW = ctx.array(W)
                ctx.gemm("N", N, ncols, N, 0.3, dH.ptr, N, dV.ptr, N, -0.5, dW.ptr, N, True)
                outs.append(dW.download())
                dW.free()
            for o in outs[1:]:
                assert np.array_equal(o, outs[0])
            ref = 0.3 * (H @ V[:, :ncols]) - 0.5 * W[:, :ncols]
            assert np.max(np.abs(outs[0][:, :ncols] - ref)) < 1e-10
            assert np.array_equal(outs[0][:, ncols:], W[:, ncols:])
    finally:
        lib.chase_hip_ctx_set_phase(ctx.h, 0)


@pytest.mark.parametrize("cplx,op", [(True, "N"), (True, "C"), (False, "N")])
def test_gemm_in_k_pieces_for_shared_chip_launches(ctx, cplx, op):
    """chase_hip_ctx_set_gemm_min_rounds (the panel products of the pipelined distributed HEMM): a product with fewer tiles than
    `rounds` per workgroup slot runs as K pieces + the fixed-order slab reduction: same values as numpy, identical bits from
    launch to launch, and the same tolerance-level result as the undivided product."""
    from chase_amd.capi import lib
    rng = np.random.default_rng(21)
    m, k, n = 16384, 2048, (256 if cplx else 512)      # 128 x 4 tiles = exactly one round of the 512 slots: undivided by default
    A = rnd(rng, (m, k) if op == "N" else (k, m), cplx)
    B, Cin = rnd(rng, (k, n), cplx), rnd(rng, (m, n), cplx)
    dA, dB = ctx.array(A), ctx.array(B)
    ref = 0.3 * ((A if op == "N" else A.conj().T) @ B) - 0.5 * Cin
    scale = np.abs(A).sum(axis=1).max() if op == "N" else np.abs(A).sum(axis=0).max()
    outs = {}
    for phase in (1, 0):
        lib.chase_hip_ctx_set_phase(ctx.h, phase)
        for rounds in (0, 4):
            lib.chase_hip_ctx_set_gemm_min_rounds(ctx.h, rounds)
            res = []
            for rep in range(3):
                dC = ctx.array(Cin)
                ctx.gemm(op, m, n, k, 0.3, dA.ptr, A.shape[0], dB.ptr, k, -0.5, dC.ptr, m, cplx)
                res.append(dC.download()); dC.free()
            assert np.array_equal(res[0], res[1]) and np.array_equal(res[0], res[2])
            assert np.max(np.abs(res[0] - ref)) <= 64 * EPS * scale * np.abs(B).max()
            outs[(phase, rounds)] = res[0]
        assert not np.array_equal(outs[(phase, 0)], outs[(phase, 4)])       # the pieces really are summed in another order
    lib.chase_hip_ctx_set_gemm_min_rounds(ctx.h, 0)
    lib.chase_hip_ctx_set_phase(ctx.h, 0)


@pytest.mark.parametrize("op", ["N", "C"])
@pytest.mark.parametrize("m,k,n", [(1153, 1001, 96), (1280, 1003, 133), (1100, 1024, 64)])
def test_filter_gemm_of_arbitrary_size_uses_3m_for_the_bulk(ctx, op, m, k, n):
    """A filter product whose sizes are not multiples of the 128-row / 8-deep tiles: the launcher cuts it into a
    three-multiplication bulk and thin four-multiplication rims (instead of running everything on four multiplications).
    Result against numpy, untouched surroundings, and the books: executed flops strictly between 3/4 and all of the model."""
    from chase_amd.capi import lib, gemm_counters
    rng = np.random.default_rng(m + k + n)
    A = rnd(rng, (m, k) if op == "N" else (k, m), True)
    B, Cm = rnd(rng, (k, n + 3), True), rnd(rng, (m + 5, n + 3), True)
    opA = A if op == "N" else A.conj().T
    alpha, beta = 0.7 - 0.2j, -0.4 + 0.1j
    dA, dB, dC = ctx.array(A), ctx.array(B), ctx.array(Cm)
    lib.chase_hip_ctx_set_phase(ctx.h, 1)
    try:
        m0, e0, _ = gemm_counters(ctx, 1)
        ctx.gemm(op, m, n, k, alpha, dA.ptr, dA.ld, dB.ptr, dB.ld, beta, dC.ptr, dC.ld, True)
        got = dC.download()
        m1, e1, _ = gemm_counters(ctx, 1)
    finally:
        lib.chase_hip_ctx_set_phase(ctx.h, 0)
    ref = Cm.copy()
    ref[:m, :n] = alpha * (opA @ B[:, :n]) + beta * Cm[:m, :n]
    scale = abs(alpha) * (np.abs(opA) @ np.abs(B[:, :n])) + abs(beta) * np.abs(Cm[:m, :n])
    assert np.max(np.abs(got[:m, :n] - ref[:m, :n]) / scale) < 8 * GEMM_TOL
    assert np.array_equal(got[m:, :], Cm[m:, :]) and np.array_equal(got[:, n:], Cm[:, n:])
    ratio = (e1 - e0) / (m1 - m0)
    assert m1 - m0 == 2.0 * 4 * m * n * k and 0.75 < ratio < 0.80, ratio
    for d in (dA, dB, dC):
        d.free()


@pytest.mark.parametrize("n", [100, 129, 300, 1000, 2049])
def test_tridiagonal_divide_and_conquer_on_the_device(ctx, n):
    """chase_hip_stedc (secular equation, Gu-Eisenstat vectors and merge products on the GPU) on the matrices that break naive
    divide & conquer: residual, orthogonality and eigenvalues within a small multiple of n eps ||T|| (the reference's RR test
    allows 100 eps on well-separated spectra, tests/linalg/internal/cpu/rayleighRitz.cpp)."""
    from chase_amd.capi import lib, check
    rng = np.random.default_rng(5 + n)
    for name, (d, e) in _tridiag_cases(n, rng).items():
        nn = len(d)
        w = np.zeros(nn)
        dZ = ctx.empty((nn, nn), np.float64)
        dd, ee = np.ascontiguousarray(d, dtype=np.float64), np.ascontiguousarray(e, dtype=np.float64)
        check(lib.chase_hip_stedc(ctx.h, nn, dd.ctypes.data, ee.ctypes.data, w.ctypes.data, dZ.ptr, nn), "stedc")
        Z = dZ.download()
        dZ.free()
        T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
        nrm = max(np.max(np.abs(d)), np.max(np.abs(e)), 1e-300)
        assert np.all(np.diff(w) >= 0), name
        assert np.max(np.abs(T @ Z - Z * w[None, :])) <= 10 * nn * EPS * nrm, (name, np.max(np.abs(T @ Z - Z * w[None, :])) / (nn * EPS * nrm))
        assert np.max(np.abs(Z.T @ Z - np.eye(nn))) <= 10 * nn * EPS, (name, np.max(np.abs(Z.T @ Z - np.eye(nn))) / (nn * EPS))
        assert np.max(np.abs(w - np.linalg.eigvalsh(T))) <= 10 * nn * EPS * nrm, name


@pytest.mark.parametrize("cplx,n,k", [(True, 1280, 4096), (False, 1536, 2048), (True, 300, 1000), (False, 1100, 777)])
def test_herkx_upper_block_trapezoid_matches_numpy(ctx, cplx, n, k):
    """chase_hip_herkx: C = A^H B for a Hermitian product from the block columns' parts on and above the diagonal only
    (cublasTsyherk in the reference, cuda/cholqr.hpp:110-112): upper triangle equal to the full product, lower triangle the
    mirror (or untouched), and fewer model flops on the books than the full product for n >= 4 blocks."""
    from chase_amd.capi import lib, check, gemm_counters
    rng = np.random.default_rng(5)
    dt = np.complex128 if cplx else np.float64
    Q = rng.standard_normal((k, n)) + (1j * rng.standard_normal((k, n)) if cplx else 0)
    Q = np.asfortranarray(Q.astype(dt))
    S = rng.standard_normal((k, k)) + (1j * rng.standard_normal((k, k)) if cplx else 0)
    W = np.asfortranarray(((S + S.conj().T) @ Q).astype(dt))                  # W^H Q = Q^H (S + S^H) Q is Hermitian
    ref = W.conj().T @ Q
    scale = np.abs(W).T @ np.abs(Q)
    dW, dQ = ctx.array(W), ctx.array(Q)
    for mirror in (1, 0):
        C0 = np.full((n, n), 7.0, dtype=dt, order="F")
        dC = ctx.array(C0)
        m0, _, _ = gemm_counters(ctx, 0)
        check(lib.chase_hip_herkx(ctx.h, int(cplx), n, k, dW.ptr, k, dQ.ptr, k, dC.ptr, n, mirror), "herkx")
        m1, _, _ = gemm_counters(ctx, 0)
        C = dC.download()
        iu = np.triu_indices(n)
        assert np.max(np.abs(C[iu] - ref[iu]) / scale[iu]) < 8 * GEMM_TOL
        il = np.tril_indices(n, -1)
        if mirror:
            assert np.array_equal(C[il], np.conj(C.T)[il])
        elif n >= 1024:
            # untouched below the block trapezoid (inside a diagonal block the whole block is written)
            blk = il[0] // 256 > il[1] // 256
            assert np.all(C[il][blk] == 7.0)
        full = 2.0 * (4 if cplx else 1) * n * n * k
        if n >= 1024:
            assert (m1 - m0) < 0.7 * full, ((m1 - m0) / full)
        else:
            assert (m1 - m0) == full
        dC.free()
    # the Gram form: herk == herkx(V, V)
    dA = ctx.array(np.zeros((n, n), dtype=dt, order="F"))
    check(lib.chase_hip_herk(ctx.h, int(cplx), n, k, dQ.ptr, k, dA.ptr, n), "herk")
    G = dA.download()
    gref = Q.conj().T @ Q
    assert np.max(np.abs(G - gref) / (np.abs(Q).T @ np.abs(Q))) < 8 * GEMM_TOL
    for d in (dW, dQ, dA):
        d.free()


def test_hash64_tells_blocks_apart_and_is_reproducible(ctx):
    """chase_hip_hash64 (what the multi-rank tests compare instead of downloading replicas): equal content -> equal hash whatever
    the leading dimension and however often it is computed; one flipped bit, two swapped entries or a sign of zero -> another"""
    rng = np.random.default_rng(11)
    for cplx in (False, True):
        m, n = 1531, 37
        A = rng.standard_normal((m, n)) + (1j * rng.standard_normal((m, n)) if cplx else 0)
        dA = ctx.array(np.asfortranarray(A))
        h0 = ctx.hash64(dA.ptr, m, n, m, cplx)
        assert h0 != 0 and all(ctx.hash64(dA.ptr, m, n, m, cplx) == h0 for _ in range(5))
        big = np.zeros((m + 9, n), dtype=A.dtype, order="F")
        big[:m] = A
        dB = ctx.array(big)
        assert ctx.hash64(dB.ptr, m, n, m + 9, cplx) == h0                 # same content behind another leading dimension
        for change in ("bit", "swap", "negzero"):
            B = np.array(A, order="F")
            if change == "bit":
                v = B.reshape(-1, order="F").view(np.uint64)       # (a view: B is column-major)
                v[3 * m * (2 if cplx else 1) + 700] ^= np.uint64(1)
            elif change == "swap":
                B[[10, 11], 5] = B[[11, 10], 5]
            else:
                B[0, 0] = 0.0
                dZ = ctx.array(B)
                hz = ctx.hash64(dZ.ptr, m, n, m, cplx)
                B[0, 0] = -0.0 if not cplx else complex(-0.0, 0.0)
                dC = ctx.array(B)
                assert ctx.hash64(dC.ptr, m, n, m, cplx) != hz
                continue
            dC = ctx.array(B)
            assert ctx.hash64(dC.ptr, m, n, m, cplx) != h0, change
        assert ctx.hash64(dA.ptr, m, n - 1, m, cplx) != h0
