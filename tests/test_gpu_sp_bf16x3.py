"""bf16x3 split product of the mixed-precision filter on the GPU (chase_amd/csrc/gemm_mfma_bf16x3.hip, sp_product = 1): the
product against an fp64 reference within the bound of its accumulation chain, each of the six partial products exactly, the
refusals, the switch at operator level and whole solves, on one GPU and on process grids (tests/sp_bf16x3_grid_scenarios.py).

Bound (tests/bf16x3_ref.py): six exact partial products per k enter one fp32 accumulation of at most 6k additions of at most u
each, u = 2^-24, plus the dropped terms and the scalars: g = (6k + 16) u real, (12k + 32) u complex with moduli, on
|alpha||A||B| + |beta||C0|; the wide form adds 8 * 2^-53 for its fp64 epilogue.  The `u per addition` is an assumption about the
bf16 MFMA's internal sum (the fp32-input MFMA is documented as an exact fma chain, this one is not documented): every case prints
max err / bound.

The exact-term tests use operands whose inner products have ONE non-zero term with at most 24 significant bits (or small
integers whose partial sums stay below 2^24), so that whatever the order of the accumulation the result must be the fp64 product
bit for bit - a lost low-order partial product, which the bound above cannot see, changes it."""
import os
import sys

import numpy as np
import pytest
from oracle import chase_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bf16x3_ref as R  # noqa: E402
import sp_bf16x3_grid_scenarios as G  # noqa: E402
from rank_threads import run_ranks  # noqa: E402

pytestmark = pytest.mark.gpu
RESID_TOL = 1e-8          # tests/test_gpu_solve.py

# narrow form (tests/test_gpu_mixed_precision.py): (m, n, k, lda, ldb, ldc, first column of B and C inside a wider array)
NARROW = [(1, 1, 1, 1, 1, 1, 0),
          (128, 128, 64, 128, 64, 128, 0),                # whole tiles
          (130, 70, 37, 130, 37, 130, 0),                 # ragged every way
          (257, 129, 515, 257, 515, 257, 0),              # several tiles plus rests
          (1001, 160, 1001, 1001, 1001, 1001, 1),         # the filter's shape at odd N: B, C start at column 1 - unaligned base
          (130, 70, 40, 132, 40, 132, 0),                 # 16-byte path (aligned leading dimensions) with ragged rows and columns
          (5, 3, 11, 5, 11, 5, 0),                        # k below one MFMA step and no multiple of 8
          # 128-column tiles (real), ragged in m and n with a K rest: on a device with num_cu = 256 compute units 65 row panels give
          # 260 tiles of 128 x 64 against 130 of 128 x 128, two rounds either way (every shape above picks 64-column tiles there)
          (8200, 250, 37, 8200, 37, 8200, 0)]
# wide form (tests/test_gpu_mixed_precision_grid.py): (m, n, k, padding of lda, ldb, ldc, first column of B and C)
WIDE = [(1, 1, 1, 0, 0, 0, 0),
        (128, 128, 64, 0, 0, 0, 0),
        (130, 70, 37, 0, 0, 0, 0),
        (257, 129, 515, 0, 0, 0, 0),
        (1001, 160, 1001, 0, 0, 0, 1),
        (130, 70, 40, 2, 0, 2, 0),                        # 16-byte paths with ragged rows and columns
        (70, 33, 300, 0, 0, 0, 0),                        # one ragged tile, long K: m << k as on a rank
        (130, 7, 0, 0, 1, 0, 0),                          # k = 0: beta C
        (5, 3, 11, 0, 0, 0, 0),
        (8200, 250, 37, 0, 0, 0, 0)]                      # 128-column tiles (real) on num_cu = 256, as in NARROW
SCALARS = {False: [(1.0, 0.0), (0.37, -1.25), (-2.5, 1.0)],
           True: [(1.0, 0.0), (0.37, -1.25), (0.3 - 0.7j, 1.1 + 0.4j)]}


def _types(cplx):
    return (np.complex64, np.complex128) if cplx else (np.float32, np.float64)


def _rand(rng, shape, cplx, dtype):
    a = rng.standard_normal(shape)
    if cplx:
        a = a + 1j * rng.standard_normal(shape)
    return np.asfortranarray(a.astype(dtype))


def _wide_lds(shape, op):
    m, n, k, pa, pb, pc, c0 = shape
    return max(1, m + pa if op == "N" else k + 2 * pa), max(1, k + pb), m + pc


@pytest.fixture(scope="module")
def operands():
    """operands, their fp64 products and |A||B|, made once per (form, shape, type, op)"""
    rng = np.random.default_rng(20260117)
    out = {}
    for cplx in (False, True):
        st, wide = _types(cplx)
        for sh in NARROW:
            m, n, k, lda, ldb, ldc, c0 = sh
            A, Bw, Cw = _rand(rng, (lda, k), cplx, st), _rand(rng, (ldb, n + c0), cplx, st), _rand(rng, (ldc, n + c0), cplx, st)
            a, b = A[:m].astype(wide), Bw[:k, c0:].astype(wide)
            out[("narrow", cplx, sh, "N")] = (A, Bw, Cw, a @ b, np.abs(a) @ np.abs(b))
        for sh in WIDE:
            m, n, k, pa, pb, pc, c0 = sh
            for op in ("N", "C"):
                lda, ldb, ldc = _wide_lds(sh, op)
                A = _rand(rng, (lda, max(k, 1) if op == "N" else m), cplx, st)       # (k = 0: a column nobody reads)
                Bw, Cw = _rand(rng, (ldb, n + c0), cplx, st), _rand(rng, (ldc, n + c0), cplx, wide)
                a = A[:m, :k].astype(wide) if op == "N" else A[:k, :m].astype(wide).conj().T
                b = Bw[:k, c0:].astype(wide)
                out[("wide", cplx, sh, op)] = (A, Bw, Cw, a @ b, np.abs(a) @ np.abs(b))
    return out


def _check_product(ctx, operands, form, shape, cplx, op):
    st, wide = _types(cplx)
    m, n, k, c0 = shape[0], shape[1], shape[2], shape[6]
    lda, ldb, ldc = shape[3:6] if form == "narrow" else _wide_lds(shape, op)
    A, Bw, Cw, P, absP = operands[(form, cplx, shape, op)]
    ct = st if form == "narrow" else wide
    dA, dB = ctx.empty(A.shape, st).upload(A), ctx.empty(Bw.shape, st).upload(Bw)
    dC = ctx.empty(Cw.shape, ct)
    try:
        for (alpha, beta) in SCALARS[cplx]:
            al, be = (st(alpha), st(beta)) if form == "narrow" else (alpha, beta)      # what the kernel is given
            C0 = Cw.copy(order="F")
            if beta == 0:
                C0[:] = np.nan                                          # beta == 0: C is not read
            runs = []
            for _ in range(2):
                dC.upload(C0)
                if form == "narrow":
                    ctx.gemm32("N", m, n, k, alpha, dA.ptr, lda, dB.offset(c0), ldb, beta, dC.offset(c0), ldc, cplx, split=True)
                else:
                    ctx.gemm32w(op, m, n, k, alpha, dA.ptr, lda, dB.offset(c0), ldb, beta, dC.offset(c0), ldc, cplx, split=True)
                runs.append(dC.download())
            got = runs[0]
            assert runs[0].tobytes() == runs[1].tobytes()               # bitwise reproducible
            ref = wide(al) * P
            if beta != 0:
                ref = ref + wide(be) * C0[:m, c0:].astype(wide)
            bound = R.product_bound(k, cplx, al, absP, be, np.abs(C0[:m, c0:]).astype(np.float64), wide=(form == "wide"))
            assert np.all(np.isfinite(got[:m, c0:]))
            err = np.abs(got[:m, c0:].astype(wide) - ref)
            ratio = np.max(err / bound) if np.all(bound > 0) else (0.0 if np.all(err[bound == 0] == 0) else np.inf)
            print(f"bf16x3 {form} {'c' if cplx else 's'}{op} {m}x{n}x{k} alpha={alpha} beta={beta}: max err / bound = {ratio:.2e}")
            assert np.all(err <= bound), (alpha, beta, float(ratio))
            # nothing outside the m x n window was written: rows below m, the columns in front of it
            keep = C0.copy()
            keep[:m, c0:] = got[:m, c0:]
            assert got.tobytes() == keep.tobytes()
    finally:
        for d in (dA, dB, dC):
            d.free()


def _id(s):
    return "x".join(map(str, s[:3])) + ("u" if s[6] else "") + ("v" if s[3] not in (0, s[0]) else "")


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("shape", NARROW, ids=_id)
def test_split_product_within_the_chain_bound(ctx, operands, shape, cplx):
    _check_product(ctx, operands, "narrow", shape, cplx, "N")


@pytest.mark.parametrize("op", ["N", "C"])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("shape", WIDE, ids=_id)
def test_widened_split_product_within_the_chain_bound(ctx, operands, shape, cplx, op):
    _check_product(ctx, operands, "wide", shape, cplx, op)


# ---- each of the six partial products, exactly -----------------------------------------------------------------------------------

def _run_exact(ctx, form, op, A, B, cplx):
    """A: op(A) as an m x k array, B: k x n; returns the device product (alpha = 1, beta = 0 on a NaN C) and the fp64 one"""
    st, wide = _types(cplx)
    m, k = A.shape
    n = B.shape[1]
    Am = np.asfortranarray(A.astype(st)) if op == "N" else np.asfortranarray(A.astype(st).conj().T)
    Bm = np.asfortranarray(B.astype(st))
    assert np.array_equal(Am.astype(wide), A if op == "N" else A.conj().T) and np.array_equal(Bm.astype(wide), B)   # fp32 holds them
    ct = st if form == "narrow" else wide
    dA, dB = ctx.empty(Am.shape, st).upload(Am), ctx.empty(Bm.shape, st).upload(Bm)
    dC = ctx.empty((m, n), ct).upload(np.full((m, n), np.nan, dtype=ct, order="F"))
    try:
        if form == "narrow":
            ctx.gemm32("N", m, n, k, 1.0, dA.ptr, Am.shape[0], dB.ptr, k, 0.0, dC.ptr, m, cplx, split=True)
        else:
            ctx.gemm32w(op, m, n, k, 1.0, dA.ptr, Am.shape[0], dB.ptr, k, 0.0, dC.ptr, m, cplx, split=True)
        got = dC.download()
    finally:
        for d in (dA, dB, dC):
            d.free()
    want = A.astype(wide) @ B.astype(wide)
    return got, want.astype(ct)


def _odd24(rng, shape):
    """24-bit odd integers with a random sign whose three bf16 parts are all non-zero"""
    x = (rng.integers(2 ** 23, 2 ** 24, shape) | 1).astype(np.float64)
    a1, a2, a3 = R.split3(x.astype(np.float32))
    bad = (a2 == 0) | (a3 == 0)
    x[bad] = 11184811.0                                     # 0xAAAAAB: all three parts non-zero (tests/test_sp_bf16x3_cpu.py)
    return x * rng.choice([-1.0, 1.0], shape)


def _pow2(rng, shape, cplx):
    b = rng.choice([-1.0, 1.0], shape) * 2.0 ** rng.integers(-20, 21, shape)
    if cplx:
        b = b * rng.choice([1.0, 1j], shape)                # real or imaginary: every component of a product has one term
    return b


def _one_per_row(rng, m, k, values):
    """m x k, row r holds values[r] in column (r + shift) % k and zeros elsewhere"""
    A = np.zeros((m, k), dtype=values.dtype)
    A[np.arange(m), (np.arange(m) + int(rng.integers(0, k))) % k] = values
    return A


EXACT_FORMS = [("narrow", "N"), ("wide", "N"), ("wide", "C")]


@pytest.mark.parametrize("form,op", EXACT_FORMS, ids=["narrow-N", "wide-N", "wide-C"])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("k", [11, 16, 40])
def test_each_partial_product_is_exact(ctx, form, op, cplx, k):
    rng = np.random.default_rng(1000 * k + 10 * cplx + len(form))
    m, n = 70, 37
    wide = _types(cplx)[1]

    def big(shape):
        x = _odd24(rng, shape).astype(wide)
        return x + 1j * _odd24(rng, shape) if cplx else x
    cases = {
        # a = 24-bit odd integer (three non-zero parts), b = +-2^p: a1 b1, a2 b1, a3 b1
        "a-parts": (_one_per_row(rng, m, k, big(m)), _pow2(rng, (k, n), cplx).astype(wide)),
        # the roles swapped: a1 b1, a1 b2, a1 b3
        "b-parts": (_pow2(rng, (m, k), cplx).astype(wide), _one_per_row(rng, n, k, big(n)).T.copy()),
        # (1 + 2^-9)^2 = 1 + 2^-8 + 2^-18: a1 b1, a1 b2 + a2 b1 and a2 b2
        "a2b2": (_one_per_row(rng, m, k, np.full(m, 1.0 + 2.0 ** -9, dtype=wide)), np.full((k, n), 1.0 + 2.0 ** -9, dtype=wide)),
    }
    for name, (A, B) in cases.items():
        got, want = _run_exact(ctx, form, op, A, B, cplx)
        assert np.all(want != 0)
        assert got.tobytes() == want.tobytes(), (name, int(np.count_nonzero(got != want)))


@pytest.mark.parametrize("form,op", EXACT_FORMS, ids=["narrow-N", "wide-N", "wide-C"])
@pytest.mark.parametrize("cplx", [False, True])
def test_small_integer_product_is_exact(ctx, form, op, cplx):
    """dense operands |x| < 128 (one bf16 part each), ragged m, n, k over several tiles: every partial sum is an integer below
    2 * 515 * 127^2 < 2^24, so the whole product is exact whatever the order"""
    rng = np.random.default_rng(77 + cplx)
    m, n, k = 257, 131, 515
    wide = _types(cplx)[1]

    def ints(shape):
        x = rng.integers(-127, 128, shape).astype(wide)
        return x + 1j * rng.integers(-127, 128, shape) if cplx else x
    got, want = _run_exact(ctx, form, op, ints((m, k)), ints((k, n)), cplx)
    assert got.tobytes() == want.tobytes(), int(np.count_nonzero(got != want))


# ---- refusals -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cplx", [False, True])
def test_split_products_refuse_a_bad_op(ctx, cplx):
    from chase_amd.capi import ChaseHipError
    st, wide = _types(cplx)
    d = ctx.empty((8, 8), st).upload(np.zeros((8, 8), st))
    c = ctx.empty((8, 8), wide).upload(np.zeros((8, 8), wide))
    with pytest.raises(ChaseHipError) as e:
        ctx.gemm32("C", 8, 8, 8, 1.0, d.ptr, 8, d.ptr, 8, 0.0, d.ptr, 8, cplx, split=True)
    assert e.value.code == -1001 and "opA" in str(e.value)                # CHASE_HIP_EINVAL, with a message
    with pytest.raises(ChaseHipError) as e:
        ctx.gemm32w("X", 8, 8, 8, 1.0, d.ptr, 8, d.ptr, 8, 0.0, c.ptr, 8, cplx, split=True)
    assert e.value.code == -1001 and "opA" in str(e.value)
    ctx.gemm32w("N", 0, 8, 8, 1.0, d.ptr, 8, d.ptr, 8, 0.0, c.ptr, 8, cplx, split=True)    # m == 0 / n == 0: nothing to do
    ctx.gemm32w("C", 8, 0, 8, 1.0, d.ptr, 8, d.ptr, 8, 0.0, c.ptr, 8, cplx, split=True)
    assert not np.any(c.download())
    d.free(); c.free()


def test_sp_product_key_values_and_pseudo_hermitian_refusal(ctx):
    from chase_amd.capi import ChaseHipError, PseudoSolver, Solver
    s = Solver(ctx, O.clement(64, False), 4, 4)
    assert s.get("sp_product") == 0 and s.get("hemm_sp_split_calls") == 0          # default: the fp32 MFMA product
    s.set(sp_product=1)
    assert s.get("sp_product") == 1
    for bad in (2, -1, 0.5):
        with pytest.raises(ChaseHipError) as e:
            s.set(sp_product=bad)
        assert e.value.code == -1001 and "sp_product" in str(e.value)
    assert s.get("sp_product") == 1
    s.set(sp_product=0)
    assert s.get("sp_product") == 0
    s.close()
    H = np.asfortranarray(ctx.gen_bse(64, True, dmin=1.0, dmax=11.0, offdiag=1e-3, seed=7).download())
    p = PseudoSolver(ctx, H, 4, 4)
    with pytest.raises(ChaseHipError) as e:
        p.set(sp_product=1)
    assert e.value.code == -1001 and "sp_product" in str(e.value)
    p.set(sp_product=0)
    assert p.get("sp_product") == 0
    p.close()


# ---- the switch at operator level (the _filter_leg pattern of tests/test_gpu_mixed_precision.py) -------------------------------------

def _set_resid(s, value):
    from chase_amd.capi import lib
    np.ctypeslib.as_array(lib.chase_hip_solver_resid(s.h), shape=(s.nev + s.nex,))[:] = value


def _filter_leg(ctx, H, cplx, keys, resid):
    """Start, initVecs, QR, Lock(5), residuals := resid, Shift(-c), two filter products over the unlocked columns, unshift"""
    from chase_amd.capi import Solver
    N, nev, nex = H.shape[0], 20, 12
    dH = ctx.array(H)
    s = Solver(ctx, None, nev, nex, h_on_device_ptr=dH.ptr, N=N, cplx=cplx)
    s.set(**keys)
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
    out = dict(V0=V0, V=s.peek_v(), h0=h0, h1=ctx.hash64(dH.ptr, N, N, N, cplx), sp=s.get("hemm_sp_calls"), dp=s.get("hemm_calls"),
               split=s.get("hemm_sp_split_calls"), sp_vecs=s.get("hemm_sp_vecs"), sp_filters=s.get("sp_filters"), c=c, steps=steps)
    s.close()
    dH.free()
    return out


@pytest.mark.parametrize("cplx", [False, True])
def test_switch_at_operator_level(ctx, cplx):
    N = 300
    H = O.clement(N, cplx)
    st, wide = _types(cplx)
    r = _filter_leg(ctx, H, cplx, dict(mixed_precision=1, sp_product=1), 1.0)
    V0, V = r["V0"], r["V"]
    assert V[:, :5].tobytes() == V0[:, :5].tobytes()                         # locked columns: never touched
    assert np.array_equal(V[:, 5:], V[:, 5:].astype(st).astype(wide))        # the filtered ones came back from fp32
    assert r["h0"] == r["h1"]                                                # fp64 H restored bit for bit
    assert r["sp"] == 2 and r["split"] == 2 and r["dp"] == 0 and r["sp_vecs"] == 2 * 27 and r["sp_filters"] == 1
    # numpy emulation of the two steps in fp64 on the fp32 operands, error bound propagated through both
    Hs = (H - r["c"] * np.eye(N)).astype(st).astype(wide)
    X0 = V0[:, 5:].astype(st).astype(wide)
    (a1, _), (a2, b2) = [(float(np.float32(a)), float(np.float32(b))) for a, b in r["steps"]]
    g = R.gamma(N, cplx)
    aH = np.abs(Hs)
    R1 = a1 * (Hs @ X0)
    e1 = g * abs(a1) * (aH @ np.abs(X0))
    R2 = a2 * (Hs @ R1) + b2 * X0
    e2 = g * (abs(a2) * (aH @ (np.abs(R1) + e1)) + abs(b2) * np.abs(X0)) + abs(a2) * (aH @ e1)
    err = np.abs(V[:, 5:] - R2)
    print(f"operator level bf16x3 {'complex' if cplx else 'real'}: max err / bound = {np.max(err / e2):.2e}")
    assert np.all(err <= e2)
    # below the threshold no fp32 product runs, whatever sp_product says: the bits of a solver never told about either key
    off = _filter_leg(ctx, H, cplx, {}, 1e-4)
    lo = _filter_leg(ctx, H, cplx, dict(mixed_precision=1, sp_product=1), 1e-4)
    assert lo["sp"] == 0 and lo["split"] == 0 and lo["dp"] == 2 and lo["sp_filters"] == 0
    assert lo["V"].tobytes() == off["V"].tobytes()
    # sp_product without mixed_precision: no effect at all, also above the threshold
    alone = _filter_leg(ctx, H, cplx, dict(mixed_precision=0, sp_product=1), 1.0)
    assert alone["sp"] == 0 and alone["split"] == 0 and alone["dp"] == 2
    assert alone["V"].tobytes() == off["V"].tobytes()
    # sp_product = 0: the fp32 MFMA path, bit for bit that of a solver that only had mixed_precision = 1
    f32 = _filter_leg(ctx, H, cplx, dict(mixed_precision=1), 1.0)
    f32_0 = _filter_leg(ctx, H, cplx, dict(mixed_precision=1, sp_product=0), 1.0)
    assert f32_0["sp"] == 2 and f32_0["split"] == 0 and f32["split"] == 0
    assert f32_0["V"].tobytes() == f32["V"].tobytes()


# ---- whole solves -----------------------------------------------------------------------------------------------------------------

SOLVES = [(256, False, 24, 16), (256, True, 24, 16), (1001, False, 100, 40)]      # tests/test_gpu_mixed_precision.py


@pytest.mark.parametrize("N,cplx,nev,nex", SOLVES, ids=["clement256-real", "clement256-complex", "clement1001-real"])
def test_whole_solve_with_the_split_product(ctx, N, cplx, nev, nex):
    from chase_amd.capi import Solver
    H = O.clement(N, cplx)
    exact = np.linalg.eigvalsh(H)[:nev]
    s = Solver(ctx, H, nev, nex)
    st_off = s.solve()                                                        # fp64
    assert s.get("hemm_sp_calls") == 0 and s.get("hemm_sp_split_calls") == 0
    s.set(mixed_precision=1, sp_product=1, reset_counters=1)
    st_on = s.solve()
    lam = s.ritzv[:nev].copy()
    print(f"clement({N}, {cplx}) {nev}/{nex}: fp64 {st_off['iterations']} iterations / {st_off['filtered_vecs']} filtered vectors, "
          f"bf16x3 {st_on['iterations']} / {st_on['filtered_vecs']}, {int(s.get('hemm_sp_vecs'))} columns in fp32 over "
          f"{int(s.get('sp_filters'))} filter calls, {int(s.get('hemm_sp_split_calls'))} split products")
    assert st_on["locked"] >= nev
    assert np.max(s.resid()[:nev]) <= 1e-10
    assert np.max(O.residuals(H, lam, s.V[:, :nev])) < RESID_TOL
    assert np.max(np.abs(np.sort(lam) - exact)) < 1e-9
    assert st_on["iterations"] <= st_off["iterations"] + 1
    assert s.get("sp_filters") >= 1 and s.get("hemm_sp_split_calls") > 0 and s.get("hemm_calls") > 0     # into bf16x3 and back out
    assert s.get("hemm_sp_split_calls") == s.get("hemm_sp_calls")
    s.set(reset_counters=1)
    assert s.get("hemm_sp_split_calls") == 0
    s.close()


# ---- process grids (ranks as threads) ---------------------------------------------------------------------------------------------

# grid (rows x columns), N, complex, block length (0: block layout), transport
OPERATOR_CASES = [(2, 2, 300, True, 0, "host"), (2, 2, 300, False, 16, "shared"), (4, 2, 301, True, 0, "shared")]


@pytest.mark.parametrize("nprow,npcol,N,cplx,mb,transport", OPERATOR_CASES,
                         ids=[f"{a}x{b}-N{N}-{'z' if c else 'd'}-mb{mb}-{t}" for (a, b, N, c, mb, t) in OPERATOR_CASES])
def test_switch_at_operator_level_on_the_grid(nprow, npcol, N, cplx, mb, transport):
    run_ranks(nprow, npcol, G.scenario_operator, N, cplx, mb, transport=transport)


def test_whole_grid_solve_with_the_split_product():
    run_ranks(2, 2, G.scenario_solve, 256, 24, 16, True, 0, transport="host")


def test_pseudo_hermitian_grid_solver_refuses_the_split_product():
    run_ranks(2, 1, G.scenario_pseudo_refuses)
