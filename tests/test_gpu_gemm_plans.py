"""Every launch plan of the GEMM (tests/gemm_plan_cases.py) on the device, against references that do not depend on the order
in which the kernel sums: an EXACT one (integer operands whose every partial sum is exact in fp64, so the product is the same
bits whatever the decomposition) and a long-double one on sampled entries of every tile class (the kernel's rounding error
alone, against the existing bounds).  Each case first asserts through chase_hip_gemm_plan, at the device's CU count, that it
reaches the class it is listed for.  GPU only."""
import numpy as np
import pytest

import gemm_plan_cases as G
from chase_amd.capi import check, gemm_plan, lib

pytestmark = pytest.mark.gpu
GEMM_TOL = 4e-15                       # test_gpu_kernels.py: 4M products; the 3M ones meet 4 * GEMM_TOL
# Exact products: |entries| <= 2^16 and k <= 2^14.  A 4M partial product is <= 2^32 and a sum of 2k of them <= 2^47; 3M's
# (ar +- ai)(br + bi) is <= 2^34 and its sums <= 2^48; each slab and the slab reduction are such sums.  alpha = 0.5 - 0.25i and
# beta = -2 + i scale them into multiples of 1/4 below 2^50: every value any scheme forms is exact in fp64 (and far above
# the 2^24 that fp32 would hold exactly).
IBOUND, KMAX = 2 ** 16, 2 ** 14
ALPHA, BETA = 0.5 - 0.25j, -2.0 + 1.0j


@pytest.fixture(scope="module")
def num_cu(ctx):
    return ctx.info()["num_cu"]


@pytest.fixture(scope="module")
def pool():
    """Random integers in [-2^16, 2^16] the cases' operands are views of (largest: C of the 2 x 2 rank's filter, 1.3 GB)."""
    rng = np.random.default_rng(4242)
    return rng.integers(-IBOUND, IBOUND + 1, size=170_000_000, dtype=np.int32).astype(np.float64)


def _take(pool, off, rows, cols, cplx):
    size = rows * cols * (2 if cplx else 1)
    off = off % (pool.size - size + 1)
    a = pool[off:off + size]
    if cplx:
        a = a.view(np.complex128)
    return a.reshape((cols, rows)).T                                   # column-major view


def _scalars(cplx):
    return (ALPHA, BETA) if cplx else (ALPHA.real, BETA.real)


def _run(ctx, c, A, lda, Bp, ldb, beta, Cp, ldc, alpha):
    lib.chase_hip_ctx_set_phase(ctx.h, c["phase"])
    lib.chase_hip_ctx_set_gemm_min_rounds(ctx.h, c["min_rounds"])
    try:
        ctx.gemm(c["op"], c["m"], c["n"], c["k"], alpha, A, lda, Bp, ldb, beta, Cp, ldc, c["cplx"])
    finally:
        lib.chase_hip_ctx_set_gemm_min_rounds(ctx.h, 0)
        lib.chase_hip_ctx_set_phase(ctx.h, 0)


def _tile_coords(t, gm, gn, gr):
    """gemm_mfma_f64.hip tile_coords: logical tile -> (row panel, column tile)"""
    g = t // (gr * gn)
    first = g * gr
    rows = min(gr, gm - first)
    r = t - g * gr * gn
    return first + r % rows, r // rows


def _sample_cols(plan):
    """first, middle and last column of every column tile of every launch"""
    s = set()
    for r in plan:
        for t in range(r["gn"]):
            c0 = r["col0"] + t * r["bn_cols"]
            w = min(r["bn_cols"], r["col0"] + r["n"] - c0)
            s |= {c0, c0 + w // 2, c0 + w - 1}
    return np.array(sorted(s))


def _sample_rows(m):
    return np.array(sorted({i for p in range(0, m, 128) for i in (p, p + 77, p + 127) if i < m} | {m - 1}))


def _setup(ctx, c, pool, num_cu, fill):
    cplx, op, m, n, k = c["cplx"], c["op"], c["m"], c["n"], c["k"]
    pa, pb, pc = c["pad"]
    cc = c["coff"]
    ra, ca = (m, k) if op == "N" else (k, m)
    A = fill(0, max(ra + pa, 1), max(ca, 1))
    B = fill(7_000_001, max(k + pb, 1), n + cc + 1)
    Cin = fill(31_000_003, m + pc, n + cc + 1)
    dA, dB, dC = ctx.array(A), ctx.array(B), ctx.array(Cin)
    lda, ldb, ldc = A.shape[0], B.shape[0], Cin.shape[0]
    Bp, Cp = dB.offset(cc), dC.offset(cc)
    plan = gemm_plan(cplx, op, m, n, k, lda=lda, ldb=ldb, aligned=(dA.ptr | Bp) % 16 == 0, phase=c["phase"], num_cu=num_cu,
                     min_rounds=c["min_rounds"])
    classes = G.plan_classes(plan, cplx, op)
    assert c["cls"] in classes, (c["name"], num_cu, sorted(classes))
    return A, B, Cin, dA, dB, dC, (lda, ldb, ldc, Bp, Cp), plan


def _op_rows(A, op, rows, m, k):
    return A[rows, :k] if op == "N" else A[:k, rows].conj().T


def _exact_refs(A, B, Cin, c, plan, alpha, beta):
    """alpha op(A) B + beta C on sampled rows (all columns) and sampled columns (all rows): every row panel and every column
    tile of every launch, so every output tile of the plan, whole or tail"""
    op, m, n, k, cc = c["op"], c["m"], c["n"], c["k"], c["coff"]
    R, S = _sample_rows(m), _sample_cols(plan)
    Bv = B[:k, cc:cc + n]
    prod_r = _op_rows(A, op, R, m, k) @ Bv
    if op == "N":
        prod_c = A[:m, :k] @ Bv[:, S]
    else:                                                              # A^H Bs = conj(Bs^H A)^T: no conjugated copy of A
        prod_c = (Bv[:, S].conj().T @ A[:k, :m]).conj().T
    return R, S, prod_r, prod_c


@pytest.mark.parametrize("name", [c["name"] for c in G.cases(256)])
def test_plan_case_exact_and_accurate(ctx, num_cu, pool, name):
    c = next(x for x in G.cases(num_cu) if x["name"] == name)
    cplx, op, m, n, k, cc = c["cplx"], c["op"], c["m"], c["n"], c["k"], c["coff"]
    assert k <= KMAX
    alpha, beta = _scalars(cplx)

    # ---- exact: integer operands, padded leading dimensions, column offsets into B and C, sentinels around C --------------
    A, B, Cin, dA, dB, dC, (lda, ldb, ldc, Bp, Cp), plan = _setup(
        ctx, c, pool, num_cu, lambda off, r, cl: _take(pool, off, r, cl, cplx))
    _run(ctx, c, dA.ptr, lda, Bp, ldb, beta, Cp, ldc, alpha)
    got = dC.download()
    R, S, prod_r, prod_c = _exact_refs(A, B, Cin, c, plan, alpha, beta)
    assert np.abs(prod_r).max() > 2 ** 24                              # beyond what fp32 sums hold exactly
    assert np.array_equal(got[R, cc:cc + n], alpha * prod_r + beta * Cin[R, cc:cc + n]), name
    assert np.array_equal(got[:m, cc + S], alpha * prod_c + beta * Cin[:m, cc + S]), name
    assert np.array_equal(got[m:, :], Cin[m:, :]) and np.array_equal(got[:, :cc], Cin[:, :cc])
    assert np.array_equal(got[:, cc + n:], Cin[:, cc + n:])
    del got
    # beta = 0 never reads C: prefilled with NaN (all bytes 0xff), it must come out as alpha op(A) B, exactly
    check(lib.chase_hip_memset(ctx.h, dC.ptr, 0xFF, dC.nbytes), "memset")
    _run(ctx, c, dA.ptr, lda, Bp, ldb, 0.0, Cp, ldc, alpha)
    got = dC.download()
    assert np.isfinite(got[:m, cc:cc + n]).all(), name
    assert np.array_equal(got[R, cc:cc + n], alpha * prod_r) and np.array_equal(got[:m, cc + S], alpha * prod_c), name
    assert np.isnan(got[m:, :]).all() and np.isnan(got[:, :cc]).all() and np.isnan(got[:, cc + n:]).all()
    del got, prod_r, prod_c

    # ---- accuracy: Gaussian operands (generated on the device), long-double reference on every tile class ------------------
    for (d, seed) in ((dA, 11), (dB, 12), (dC, 13)):
        check(lib.chase_hip_fill_normal(ctx.h, int(cplx), d.shape[0], d.shape[1], d.ptr, d.shape[0], 0, 0, d.shape[0], seed),
              "fill_normal")
    A, B, Cg = dA.download(), dB.download(), dC.download()
    _run(ctx, c, dA.ptr, lda, Bp, ldb, beta, Cp, ldc, alpha)
    got = dC.download()
    worst = _accuracy(A, B, Cg, got, c, plan, alpha, beta)
    print(f"\n{name} ({num_cu} CUs): worst |error| / bound per tile class: " +
          ", ".join(f"{cl} {v:.3f}" for cl, v in sorted(worst.items())))
    assert max(worst.values()) <= 1.0, (name, worst)
    for d in (dA, dB, dC):
        d.free()


def _accuracy(A, B, Cg, got, c, plan, alpha, beta):
    """worst |got - ref| / bound per tile class, ref in long double; bound = tol (|alpha| |op(A)||B| + |beta||C|), tol = GEMM_TOL
    for 4M launches and 4 GEMM_TOL for 3M ones"""
    assert np.finfo(np.longdouble).nmant >= 63
    cplx, op, m, n, k, cc = c["cplx"], c["op"], c["m"], c["n"], c["k"], c["coff"]
    rng = np.random.default_rng(5)
    samples = {}                                                       # (i, j) -> labels

    def add(i, j, label):
        samples.setdefault((int(i), int(j)), set()).add(label)

    def entries(r, bm, bn, label, both=True):
        i0, j0 = r["row0"] + 128 * bm, r["col0"] + bn * r["bn_cols"]
        i1, j1 = min(i0 + 128, r["row0"] + r["m"]), min(j0 + r["bn_cols"], r["col0"] + r["n"])
        add(i1 - 1, j1 - 1, label)
        if both:
            add(rng.integers(i0, i1), rng.integers(j0, j1), label)

    for r in plan:
        gm, gn, gr, full, tail = r["gm"], r["gn"], r["group_rows"], r["full_tiles"], r["tail_tiles"]
        for t in np.unique(np.linspace(0, full - 1, min(full, 48)).astype(int)) if full else []:
            entries(r, *_tile_coords(int(t), gm, gn, gr), "whole")
        for t in range(full, full + tail):
            entries(r, *_tile_coords(t, gm, gn, gr), "tail", both=tail <= 256)
        if gm % gr:
            for bn in np.unique(np.linspace(0, gn - 1, min(gn, 16)).astype(int)):
                entries(r, gm - 1, int(bn), "partial-group")
        for bm in np.unique(np.linspace(0, gm - 1, min(gm, 16)).astype(int)):
            entries(r, int(bm), gn - 1, "last-col-tile")
        if r["m"] % 128:
            for bn in range(gn):
                entries(r, gm - 1, bn, "row-rim")
        if r["beta_one"]:
            for bm in np.unique(np.linspace(0, gm - 1, min(gm, 16)).astype(int)):
                entries(r, int(bm), int(rng.integers(0, gn)), "k-rim")
    m3_of = lambda i, j: any(r["m3"] and r["row0"] <= i < r["row0"] + r["m"] and r["col0"] <= j < r["col0"] + r["n"]
                             for r in plan)
    keys = sorted(samples)
    I, J = np.array([p[0] for p in keys]), np.array([p[1] for p in keys])
    ld = np.clongdouble if cplx else np.longdouble
    worst = {}
    for s0 in range(0, len(keys), 256):
        i, j = I[s0:s0 + 256], J[s0:s0 + 256]
        a = (A[i, :k] if op == "N" else A[:k, i].conj().T)             # rows of op(A)
        b = B[:k, cc + j].T                                            # columns of B, as rows
        ref = (a.astype(ld) * b.astype(ld)).sum(axis=1) * ld(alpha) + ld(beta) * Cg[i, cc + j].astype(ld)
        err = np.abs(got[i, cc + j].astype(ld) - ref).astype(np.float64)
        scale = abs(alpha) * (np.abs(a) * np.abs(b)).sum(axis=1) + abs(beta) * np.abs(Cg[i, cc + j])
        for q in range(len(i)):
            tol = (4 if m3_of(i[q], j[q]) else 1) * GEMM_TOL
            ratio = err[q] / (tol * scale[q]) if scale[q] > 0 else err[q]
            for label in samples[(int(i[q]), int(j[q]))]:
                worst[label] = max(worst.get(label, 0.0), ratio)
    return worst


@pytest.mark.parametrize("name", [c["name"] for c in G.k0_cases()])
def test_k0_product_is_beta_c_exactly(ctx, num_cu, pool, name):
    """k = 0 (a rank that owns no rows of the block): C = beta C bit for bit in every phase, for both types, and C = 0 for beta = 0
    whatever C held"""
    c = next(x for x in G.k0_cases() if x["name"] == name)
    cplx, m, n, cc = c["cplx"], c["m"], c["n"], c["coff"]
    alpha, beta = _scalars(cplx)
    A, B, Cin, dA, dB, dC, (lda, ldb, ldc, Bp, Cp), plan = _setup(
        ctx, c, pool, num_cu, lambda off, r, cl: _take(pool, off, r, cl, cplx))
    assert not any(r["m3"] for r in plan)
    _run(ctx, c, dA.ptr, lda, Bp, ldb, beta, Cp, ldc, alpha)
    got = dC.download()
    ref = Cin.copy()
    ref[:m, cc:cc + n] = beta * Cin[:m, cc:cc + n]
    assert np.array_equal(got, ref), name
    check(lib.chase_hip_memset(ctx.h, dC.ptr, 0xFF, dC.nbytes), "memset")
    _run(ctx, c, dA.ptr, lda, Bp, ldb, 0.0, Cp, ldc, alpha)
    got = dC.download()
    assert np.array_equal(got[:m, cc:cc + n], np.zeros((m, n), got.dtype)) and np.isnan(got[m:, :]).all(), name
    for d in (dA, dB, dC):
        d.free()
