"""Mixed-precision Chebyshev filter on the GPU: the fp32 MFMA product against an fp64 reference within the worst-case bound of
an fma chain, the precision conversions bit for bit, the switch at operator level (what is rounded to fp32 and what never is) and
whole solves with the switch off and on.

Bound of the product (Higham, Accuracy and Stability, (3.5) / gamma_n): a length-k inner product accumulated by fma in ANY order
errs by at most gamma_k |a|.|b|; alpha, beta and the final sum add a handful of roundings: (k + 8) u (|alpha| |A||B| + |beta| |C0|),
u = 2^-24; complex arithmetic from four real products doubles the chain: (2k + 16) u with moduli.  Derived, not tuned: an
independent fp32 product (OpenBLAS) stays below 0.07 of it on these cases, a row of A rotated by one element exceeds it 1000-fold."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
from oracle import chase_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sp_gemm_hash_cases as HC  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
RESID_TOL = 1e-8          # tests/test_gpu_solve.py

# (m, n, k, lda, ldb, ldc, first column of B and C inside a wider array)
SHAPES = [(1, 1, 1, 1, 1, 1, 0),
          (128, 128, 64, 128, 64, 128, 0),                # whole tiles
          (130, 70, 37, 130, 37, 130, 0),                 # ragged every way
          (257, 129, 515, 257, 515, 257, 0),              # several tiles plus rests
          (1001, 160, 1001, 1001, 1001, 1001, 1),         # the filter's shape at odd N: B, C start at column 1 - unaligned base
          (130, 70, 40, 132, 40, 132, 0),                 # 16-byte path (aligned leading dimensions) with ragged rows and columns
          # 128-column tiles, ragged in m and n with a K rest: on a device with num_cu = 256 compute units 65 row panels give 260
          # tiles of 128 x 64 against 130 of 128 x 128, two rounds either way (every shape above picks 64-column tiles there)
          (8200, 250, 37, 8200, 37, 8200, 0)]
SCALARS = {False: [(1.0, 0.0), (0.37, -1.25), (-2.5, 1.0)],
           True: [(1.0, 0.0), (0.37, -1.25), (0.3 - 0.7j, 1.1 + 0.4j)]}


def _rand(rng, shape, cplx):
    a = rng.standard_normal(shape)
    if cplx:
        a = a + 1j * rng.standard_normal(shape)
    return np.asfortranarray(a.astype(np.complex64 if cplx else np.float32))


def _bound(k, cplx, alpha, A, B, beta, C0):
    g = ((2 * k + 16) if cplx else (k + 8)) * U
    b = abs(alpha) * (np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64))
    if beta != 0:
        b = b + abs(beta) * np.abs(C0).astype(np.float64)
    return g * b


@pytest.fixture(scope="module")
def operands():
    """operands and their fp64 products, made once per (shape, type)"""
    rng = np.random.default_rng(20240611)
    out = {}
    for cplx in (False, True):
        for sh in SHAPES:
            m, n, k, lda, ldb, ldc, c0 = sh
            A = _rand(rng, (lda, k), cplx)
            Bw = _rand(rng, (ldb, n + c0), cplx)
            Cw = _rand(rng, (ldc, n + c0), cplx)
            wide = np.complex128 if cplx else np.float64
            P = A[:m].astype(wide) @ Bw[:k, c0:].astype(wide)
            out[(cplx, sh)] = (A, Bw, Cw, P)
    return out


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:3])) + ("u" if s[6] else "") + ("v" if s[3] != s[0] else ""))
def test_f32_product_within_the_fma_chain_bound(ctx, operands, shape, cplx):
    m, n, k, lda, ldb, ldc, c0 = shape
    A, Bw, Cw, P = operands[(cplx, shape)]
    st = np.complex64 if cplx else np.float32
    wide = np.complex128 if cplx else np.float64
    dA, dB = ctx.empty(A.shape, st).upload(A), ctx.empty(Bw.shape, st).upload(Bw)
    dC = ctx.empty(Cw.shape, st)
    try:
        for (alpha, beta) in SCALARS[cplx]:
            a32, b32 = st(alpha), st(beta)                              # what the kernel is given
            C0 = Cw.copy(order="F")
            if beta == 0:
                C0[:] = np.nan                                          # beta == 0: C is not read
            runs = []
            for _ in range(2):
                dC.upload(C0)
                ctx.gemm32("N", m, n, k, alpha, dA.ptr, lda, dB.offset(c0), ldb, beta, dC.offset(c0), ldc, cplx)
                runs.append(dC.download())
            got = runs[0]
            assert runs[0].tobytes() == runs[1].tobytes()               # bitwise reproducible
            ref = wide(a32) * P
            if beta != 0:
                ref = ref + wide(b32) * C0[:m, c0:].astype(wide)
            bound = _bound(k, cplx, a32, A[:m], Bw[:k, c0:], b32, C0[:m, c0:])
            err = np.abs(got[:m, c0:].astype(wide) - ref)
            assert np.all(np.isfinite(got[:m, c0:]))
            print(f"gemm32 {'c' if cplx else 's'} {m}x{n}x{k} alpha={alpha} beta={beta}: max err / bound = {np.max(err / bound):.3f}")
            assert np.all(err <= bound), (alpha, beta, float(np.max(err / bound)))
            # nothing outside the m x n window was written: rows below m, the columns in front of it
            keep = C0.copy()
            keep[:m, c0:] = got[:m, c0:]
            assert got.tobytes() == keep.tobytes()
    finally:
        for d in (dA, dB, dC):
            d.free()


def test_single_precision_products_keep_their_bits(ctx):
    """tests/golden/sp_gemm_hashes.json holds the 64-bit content hashes of 72 products - fp32 MFMA and bf16x3, real and complex,
    narrow and wide, op N and C, both tile widths, 16-byte and guarded paths, both kernel tags, beta = 0 - as the two kernels
    produced them before their frame moved into gemm_sp_frame.h (tests/sp_gemm_hash_cases.py wrote it on a build of that commit).
    The inputs are device-generated from fixed seeds and the kernels have one summation order per element, so the hashes pin the
    kernels' bits: a change of the frame must not move one."""
    gold = json.load(open(HC.GOLDEN))
    # on another CU count the tile-width rule picks other widths: the hashes would still match (an element's sum does not depend
    # on the width) while the 128-column kernels went unrun
    assert ctx.info()["num_cu"] == gold["num_cu"] == 256
    gold = gold["rows"]
    assert len(gold) == HC.COUNT == 72
    rows = HC.run_cases(ctx)
    bad = [(g, r["hash"]) for g, r in zip(gold, rows) if g != r]
    assert not bad, bad[:4]


@pytest.mark.parametrize("cplx", [False, True])
def test_f32_product_refuses_op_c(ctx, cplx):
    from chase_amd.capi import ChaseHipError
    st = np.complex64 if cplx else np.float32
    d = ctx.empty((8, 8), st).upload(np.zeros((8, 8), st))
    with pytest.raises(ChaseHipError) as e:
        ctx.gemm32("C", 8, 8, 8, 1.0, d.ptr, 8, d.ptr, 8, 0.0, d.ptr, 8, cplx)
    assert e.value.code == -1001 and "opA" in str(e.value)            # CHASE_HIP_EINVAL, with a message
    d.free()


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("ld", [133, 136], ids=["ld133", "ld136-16B"])
def test_conversions_bitwise(ctx, cplx, ld):
    m, n = 130, 7
    rng = np.random.default_rng(7)
    dt, st = (np.complex128, np.complex64) if cplx else (np.float64, np.float32)
    X = rng.standard_normal((ld, n)) * 10.0 ** rng.integers(-30, 30, (ld, n))      # exponents over the fp32 range and beyond
    if cplx:
        X = X + 1j * rng.standard_normal((ld, n))
    X = np.asfortranarray(X.astype(dt))
    X[3, 2] = 0.1 + 2.0 ** -26                       # a tie-adjacent value and one exactly between two floats
    X[4, 2] = 1.0 + 2.0 ** -24
    dX = ctx.empty((ld, n), dt).upload(X)
    mark = np.full((ld, n), 7.0, dtype=st, order="F")
    dS = ctx.empty((ld, n), st).upload(mark)
    ctx.convert_d2s(m, n, dX.ptr, ld, dS.ptr, ld, cplx)
    S = dS.download()
    with np.errstate(over="ignore"):
        want = mark.copy()
        want[:m] = X[:m].astype(st)
    assert S.tobytes() == want.tobytes()             # round to nearest even like numpy, rows m.. untouched
    # and back: exact
    markd = np.full((ld, n), 5.0, dtype=dt, order="F")
    dD = ctx.empty((ld, n), dt).upload(markd)
    ctx.convert_s2d(m, n, dS.ptr, ld, dD.ptr, ld, cplx)
    wantd = markd.copy()
    wantd[:m] = S[:m].astype(dt)
    assert dD.download().tobytes() == wantd.tobytes()
    # the helpers on whole arrays
    assert ctx.to_double(ctx.to_single(dX)).download()[:m].tobytes() == X[:m].astype(st).astype(dt).tobytes()
    for d in (dX, dS, dD):
        d.free()


@pytest.mark.parametrize("cplx", [False, True])
def test_diag_d2s_changes_the_diagonal_only(ctx, cplx):
    n, ldh, ldhs = 37, 41, 40
    rng = np.random.default_rng(11)
    dt, st = (np.complex128, np.complex64) if cplx else (np.float64, np.float32)
    H = rng.standard_normal((ldh, n)) + (1j * rng.standard_normal((ldh, n)) if cplx else 0)
    H = np.asfortranarray(H.astype(dt))
    Hs0 = np.asfortranarray((rng.standard_normal((ldhs, n)) + (1j if cplx else 0)).astype(st))
    dH, dHs = ctx.empty((ldh, n), dt).upload(H), ctx.empty((ldhs, n), st).upload(Hs0)
    ctx.diag_d2s(n, dH.ptr, ldh, dHs.ptr, ldhs, cplx)
    want = Hs0.copy()
    for i in range(n):
        want[i, i] = st(H[i, i])
    assert dHs.download().tobytes() == want.tobytes()
    dH.free(); dHs.free()


def _set_resid(s, value):
    """the buffer the driver writes its residuals into (chase_hip_solver_resid)"""
    from chase_amd.capi import lib
    p = lib.chase_hip_solver_resid(s.h)
    np.ctypeslib.as_array(p, shape=(s.nev + s.nex,))[:] = value


def _filter_leg(ctx, H, cplx, mixed, resid):
    """Start, initVecs, QR, Lock(5), residuals := resid, Shift(-c), two filter products over the unlocked columns, unshift"""
    from chase_amd.capi import Solver
    N, nev, nex = H.shape[0], 20, 12
    dH = ctx.array(H)
    s = Solver(ctx, None, nev, nex, h_on_device_ptr=dH.ptr, N=N, cplx=cplx)
    if mixed is not None:
        s.set(mixed_precision=mixed)
    s.Start(); s.initVecs(True); s.QR(0, 1.0); s.Lock(5)
    _set_resid(s, resid)
    V0 = s.peek_v()
    h0 = ctx.hash64(dH.ptr, N, N, N, cplx)
    c = 40.0
    steps = [(0.01, 0.0), (0.02, -0.3)]                      # the filter's pattern: beta = 0 first
    s.Shift(-c)
    for (a, b) in steps:
        s.HEMM(nev + nex - 5, a, b, 0)
    s.Shift(c, True)
    V = s.peek_v()
    out = dict(V0=V0, V=V, h0=h0, h1=ctx.hash64(dH.ptr, N, N, N, cplx), sp=s.get("hemm_sp_calls"), dp=s.get("hemm_calls"),
               sp_vecs=s.get("hemm_sp_vecs"), sp_filters=s.get("sp_filters"), c=c, steps=steps)
    s.close()
    dH.free()
    return out


@pytest.mark.parametrize("cplx", [False, True])
def test_switch_at_operator_level(ctx, cplx):
    N = 300
    H = O.clement(N, cplx)
    r = _filter_leg(ctx, H, cplx, 1, 1.0)
    V0, V = r["V0"], r["V"]
    st, wide = (np.complex64, np.complex128) if cplx else (np.float32, np.float64)
    assert V[:, :5].tobytes() == V0[:, :5].tobytes()                         # locked columns: never touched
    assert np.array_equal(V[:, 5:], V[:, 5:].astype(st).astype(wide))        # the filtered ones came back from fp32
    assert r["h0"] == r["h1"]                                                # fp64 H restored bit for bit
    assert r["sp"] == 2 and r["dp"] == 0 and r["sp_vecs"] == 2 * 27 and r["sp_filters"] == 1
    # numpy emulation of the two steps in fp64 on the fp32 operands, error bound propagated through both
    Hs = (H - r["c"] * np.eye(N)).astype(st).astype(wide)
    X0 = V0[:, 5:].astype(st).astype(wide)
    (a1, _), (a2, b2) = [(float(np.float32(a)), float(np.float32(b))) for a, b in r["steps"]]
    g = ((2 * N + 16) if cplx else (N + 8)) * U
    aH = np.abs(Hs)
    R1 = a1 * (Hs @ X0)
    e1 = g * abs(a1) * (aH @ np.abs(X0))
    R2 = a2 * (Hs @ R1) + b2 * X0
    e2 = g * (abs(a2) * (aH @ (np.abs(R1) + e1)) + abs(b2) * np.abs(X0)) + abs(a2) * (aH @ e1)
    err = np.abs(V[:, 5:] - R2)
    print(f"operator level {'complex' if cplx else 'real'}: max err / bound = {np.max(err / e2):.3f}")
    assert np.all(err <= e2)
    # below the threshold nothing runs in fp32, and the bits are those of a solver that was never told about the switch
    lo = _filter_leg(ctx, H, cplx, 1, 1e-4)
    off = _filter_leg(ctx, H, cplx, None, 1e-4)
    assert lo["sp"] == 0 and lo["dp"] == 2 and lo["sp_filters"] == 0
    assert lo["V"].tobytes() == off["V"].tobytes()
    assert not np.array_equal(lo["V"][:, 5:], V[:, 5:])                      # (the two paths do differ)


SOLVES = [(256, False, 24, 16), (256, True, 24, 16), (1001, False, 100, 40)]      # odd N: every column unaligned
STAT_KEYS = ("iterations", "filtered_vecs", "lanczos_vecs", "locked", "lowerb", "upperb", "lambda_")


@pytest.mark.parametrize("N,cplx,nev,nex", SOLVES, ids=["clement256-real", "clement256-complex", "clement1001-real"])
def test_whole_solve_off_and_on(ctx, N, cplx, nev, nex):
    from chase_amd.capi import Solver
    H = O.clement(N, cplx)
    exact = np.linalg.eigvalsh(H)[:nev]
    plain = Solver(ctx, H, nev, nex)                    # never heard of the key
    st_plain = plain.solve()
    lam_plain = plain.ritzv.copy()
    plain.close()

    s = Solver(ctx, H, nev, nex)
    s.set(mixed_precision=0)
    assert s.get("mixed_precision") == 0
    st_off = s.solve()
    assert s.get("hemm_sp_calls") == 0 and s.get("sp_filters") == 0
    assert {k: st_off[k] for k in STAT_KEYS} == {k: st_plain[k] for k in STAT_KEYS}
    assert s.ritzv.tobytes() == lam_plain.tobytes()

    s.set(mixed_precision=1, reset_counters=1)
    assert s.get("mixed_precision") == 1
    st_on = s.solve()
    lam = s.ritzv[:nev].copy()
    print(f"clement({N}, {cplx}) {nev}/{nex}: fp64 {st_off['iterations']} iterations / {st_off['filtered_vecs']} filtered vectors, "
          f"mixed {st_on['iterations']} / {st_on['filtered_vecs']}, {int(s.get('hemm_sp_vecs'))} columns in fp32 over "
          f"{int(s.get('sp_filters'))} filter calls")
    assert st_on["locked"] >= nev
    assert np.max(s.resid()[:nev]) <= 1e-10
    assert np.max(O.residuals(H, lam, s.V[:, :nev])) < RESID_TOL
    assert np.max(np.abs(np.sort(lam) - exact)) < 1e-9
    assert s.get("sp_filters") >= 1 and s.get("hemm_sp_calls") > 0 and s.get("hemm_calls") > 0      # into fp32 and back out
    assert st_on["iterations"] <= st_off["iterations"] + 1
    s.set(reset_counters=1)
    assert s.get("hemm_sp_calls") == 0 and s.get("hemm_sp_vecs") == 0 and s.get("sp_filters") == 0
    s.close()


def test_pseudo_hermitian_solver_refuses_the_switch(ctx):
    from chase_amd.capi import ChaseHipError, PseudoSolver
    H = np.asfortranarray(ctx.gen_bse(64, True, dmin=1.0, dmax=11.0, offdiag=1e-3, seed=7).download())
    s = PseudoSolver(ctx, H, 4, 4)
    with pytest.raises(ChaseHipError) as e:
        s.set(mixed_precision=1)
    assert e.value.code == -1001 and "mixed_precision" in str(e.value)
    s.set(mixed_precision=0)                                 # turning it off is what the solver does anyway
    assert s.get("mixed_precision") == 0
    s.close()
