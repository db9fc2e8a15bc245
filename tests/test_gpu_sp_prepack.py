"""bf16x3 product on a packed H on the GPU (chase_amd/csrc/gemm_mfma_bf16x3p.hip, sp_prepack = 1): the pack and its diagonal
refresh byte for byte against the numpy restatement of the layout (tests/bf16x3_pack_ref.py), the product bit for bit against the
unpacked bf16x3 product of the library and within the chain bound of tests/bf16x3_ref.py against fp64, the switch at operator
level and in whole solves (bits, iterations and counters of sp_product = 1 without it), a new matrix on the same solver, and
the refusals.

The packed product restates the kernel of gemm_mfma_bf16x3.hip with another way of bringing A into LDS: same tiles, same LDS
image, same six MFMAs per 16 k in the same order.  Hence `==` on bytes everywhere; the fp64 comparison is the independent one."""
import os
import sys

import numpy as np
import pytest
from oracle import chase_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bf16x3_pack_ref as PR  # noqa: E402
import bf16x3_ref as R  # noqa: E402
import sp_prepack_grid_scenarios as G  # noqa: E402
from rank_threads import run_ranks  # noqa: E402

pytestmark = pytest.mark.gpu

# the NARROW list of tests/test_gpu_sp_bf16x3.py: (m, n, k, lda, ldb, ldc, first column of B and C inside a wider array)
NARROW = [(1, 1, 1, 1, 1, 1, 0),
          (128, 128, 64, 128, 64, 128, 0),                # whole tiles
          (130, 70, 37, 130, 37, 130, 0),                 # ragged every way
          (257, 129, 515, 257, 515, 257, 0),              # several tiles plus rests
          (1001, 160, 1001, 1001, 1001, 1001, 1),         # the filter's shape at odd N: B, C start at column 1 - unaligned base
          (130, 70, 40, 132, 40, 132, 0),                 # 16-byte path (aligned leading dimensions) with ragged rows and columns
          (5, 3, 11, 5, 11, 5, 0),                        # k below one MFMA step and no multiple of 8
          (8200, 250, 37, 8200, 37, 8200, 0),             # 128-column tiles (real) on a device with 256 compute units
          (130, 7, 0, 130, 1, 130, 0)]                    # k = 0: beta C
SCALARS = {False: [(1.0, 0.0), (0.37, -1.25), (-2.5, 1.0)],
           True: [(1.0, 0.0), (0.37, -1.25), (0.3 - 0.7j, 1.1 + 0.4j)]}
PACK_SHAPES = [(1, 1), (128, 16), (129, 17), (5, 11), (300, 300), (257, 1000)]
TAIL = 256                                                # sentinel bytes behind a packed buffer


def _types(cplx):
    return (np.complex64, np.complex128) if cplx else (np.float32, np.float64)


def _rand(rng, shape, cplx, dtype):
    a = rng.standard_normal(shape)
    if cplx:
        a = a + 1j * rng.standard_normal(shape)
    return np.asfortranarray(a.astype(dtype))


def _id(s):
    return "x".join(map(str, s[:3])) + ("u" if s[6] else "") + ("v" if s[3] not in (0, s[0]) else "")


def _packed_buffer(ctx, nbytes):
    """a device buffer of nbytes + TAIL bytes, all 0xFF: unwritten padding and writes behind the end show"""
    return ctx.empty((nbytes + TAIL,), np.uint8).upload(np.full(nbytes + TAIL, 0xFF, np.uint8))


# ---- pack ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("src_f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("pad", [0, 3], ids=["lda=m", "lda=m+3"])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("m,k", PACK_SHAPES)
def test_pack_is_the_documented_layout_byte_for_byte(ctx, m, k, cplx, pad, src_f64):
    st, wide = _types(cplx)
    rng = np.random.default_rng(100000 * m + 10 * k + cplx)
    scale = 10.0 ** rng.uniform(-6, 6, (m + pad, k))                       # exponents all over: every part of the split is alive
    A = np.asfortranarray((_rand(rng, (m + pad, k), cplx, wide) * scale).astype(wide if src_f64 else st))
    want = PR.pack(A[:m].astype(st))                                       # fp64 source: rounded to fp32 first
    nbytes = ctx.bf16x3_pack_bytes(m, k, cplx)
    assert nbytes == want.size == PR.pack_bytes(m, k, cplx)
    dA, dP = ctx.empty(A.shape, A.dtype).upload(A), _packed_buffer(ctx, nbytes)
    try:
        ctx.bf16x3_pack(m, k, dA.ptr, m + pad, dP.ptr, cplx, src_f64=src_f64)
        got = dP.download()
    finally:
        dA.free(); dP.free()
    assert np.all(got[nbytes:] == 0xFF)                                    # nothing behind the end
    assert got[:nbytes].tobytes() == want.tobytes(), int(np.count_nonzero(got[:nbytes] != want))


def test_pack_of_nothing_is_a_no_op(ctx):
    assert ctx.bf16x3_pack_bytes(0, 7, False) == 0 and ctx.bf16x3_pack_bytes(7, 0, True) == 0
    dP = _packed_buffer(ctx, 0)
    ctx.bf16x3_pack(0, 7, None, 1, dP.ptr, False)
    ctx.bf16x3_pack(7, 0, None, 7, dP.ptr, True)
    ctx.bf16x3_pack_diag(0, None, 1, dP.ptr, False)
    assert np.all(dP.download() == 0xFF)
    dP.free()


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n", [1, 129, 300])
def test_pack_diag_leaves_the_bytes_of_a_full_pack(ctx, n, cplx):
    st, wide = _types(cplx)
    rng = np.random.default_rng(31 * n + cplx)
    H = _rand(rng, (n + 2, n), cplx, wide)                                 # ldh = n + 2
    nbytes = ctx.bf16x3_pack_bytes(n, n, cplx)
    dH, dP = ctx.empty(H.shape, wide).upload(H), _packed_buffer(ctx, nbytes)
    try:
        ctx.bf16x3_pack(n, n, dH.ptr, n + 2, dP.ptr, cplx, src_f64=True)
        before = dP.download()
        H2 = H.copy(order="F")
        idx = np.arange(n)
        H2[idx, idx] += wide(-37.25) if not cplx else wide(-37.25 + 0.5j)  # (the imaginary part too: every diagonal byte moves)
        dH.upload(H2)
        ctx.bf16x3_pack_diag(n, dH.ptr, n + 2, dP.ptr, cplx)
        got = dP.download()
    finally:
        dH.free(); dP.free()
    want = PR.pack(H2[:n].astype(st))
    assert before[:nbytes].tobytes() == PR.pack(H[:n].astype(st)).tobytes()
    assert before[:nbytes].tobytes() != want.tobytes()
    assert np.all(got[nbytes:] == 0xFF)
    assert got[:nbytes].tobytes() == want.tobytes(), int(np.count_nonzero(got[:nbytes] != want))


# ---- product ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def operands():
    """operands, their fp64 products and |A||B|, made once per (shape, type)"""
    rng = np.random.default_rng(20261020)
    out = {}
    for cplx in (False, True):
        st, wide = _types(cplx)
        for sh in NARROW:
            m, n, k, lda, ldb, ldc, c0 = sh
            A = _rand(rng, (lda, max(k, 1)), cplx, st)                     # (k = 0: a column nobody reads)
            Bw, Cw = _rand(rng, (ldb, n + c0), cplx, st), _rand(rng, (ldc, n + c0), cplx, st)
            a, b = A[:m, :k].astype(wide), Bw[:k, c0:].astype(wide)
            out[(cplx, sh)] = (A, Bw, Cw, a @ b, np.abs(a) @ np.abs(b))
    return out


def _products(ctx, operands, shape, cplx, unpacked):
    """for every (alpha, beta): C0 and the C of two packed runs (and of the unpacked bf16x3 product of the library)"""
    st, _ = _types(cplx)
    m, n, k, lda, ldb, ldc, c0 = shape
    A, Bw, Cw, _, _ = operands[(cplx, shape)]
    nbytes = ctx.bf16x3_pack_bytes(m, k, cplx)
    dA, dB, dC = ctx.empty(A.shape, st).upload(A), ctx.empty(Bw.shape, st).upload(Bw), ctx.empty(Cw.shape, st)
    dP = _packed_buffer(ctx, nbytes)
    out = []
    try:
        ctx.bf16x3_pack(m, k, dA.ptr, lda, dP.ptr, cplx)
        for (alpha, beta) in SCALARS[cplx]:
            C0 = Cw.copy(order="F")
            if beta == 0:
                C0[:] = np.nan                                             # beta == 0: C is not read
            runs = []
            for _ in range(2):
                dC.upload(C0)
                ctx.gemm32p(m, n, k, alpha, dP.ptr, dB.offset(c0), ldb, beta, dC.offset(c0), ldc, cplx)
                runs.append(dC.download())
            ref = None
            if unpacked:
                dC.upload(C0)
                ctx.gemm32("N", m, n, k, alpha, dA.ptr, lda, dB.offset(c0), ldb, beta, dC.offset(c0), ldc, cplx, split=True)
                ref = dC.download()
            out.append((alpha, beta, C0, runs, ref))
        assert np.all(dP.download()[nbytes:] == 0xFF)
    finally:
        for d in (dA, dB, dC, dP):
            d.free()
    return out


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("shape", NARROW, ids=_id)
def test_packed_product_is_the_split_product_bit_for_bit(ctx, operands, shape, cplx):
    for (alpha, beta, C0, runs, ref) in _products(ctx, operands, shape, cplx, unpacked=True):
        assert runs[0].tobytes() == runs[1].tobytes(), (alpha, beta)        # bitwise reproducible
        assert runs[0].tobytes() == ref.tobytes(), (alpha, beta, int(np.count_nonzero(runs[0] != ref)))


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("shape", NARROW, ids=_id)
def test_packed_product_within_the_chain_bound(ctx, operands, shape, cplx):
    st, wide = _types(cplx)
    m, n, k, c0 = shape[0], shape[1], shape[2], shape[6]
    P, absP = operands[(cplx, shape)][3:]
    for (alpha, beta, C0, runs, _) in _products(ctx, operands, shape, cplx, unpacked=False):
        got = runs[0]
        al, be = st(alpha), st(beta)                                        # what the kernel is given
        ref = wide(al) * P
        if beta != 0:
            ref = ref + wide(be) * C0[:m, c0:].astype(wide)
        bound = R.product_bound(k, cplx, al, absP, be, np.abs(C0[:m, c0:]).astype(np.float64))
        assert np.all(np.isfinite(got[:m, c0:]))
        err = np.abs(got[:m, c0:].astype(wide) - ref)
        ratio = np.max(err / bound) if np.all(bound > 0) else (0.0 if np.all(err[bound == 0] == 0) else np.inf)
        print(f"bf16x3p {'c' if cplx else 's'}N {m}x{n}x{k} alpha={alpha} beta={beta}: max err / bound = {ratio:.2e}")
        assert np.all(err <= bound), (alpha, beta, float(ratio))
        # nothing outside the m x n window was written: rows below m, the columns in front of it
        keep = C0.copy()
        keep[:m, c0:] = got[:m, c0:]
        assert got.tobytes() == keep.tobytes()


# ---- the switch at operator level (the _filter_leg pattern of tests/test_gpu_sp_bf16x3.py) -------------------------------------------

COUNTERS = ("hemm_sp_calls", "hemm_sp_split_calls", "hemm_sp_packed_calls", "sp_pack_full", "sp_pack_diag", "hemm_calls", "sp_filters")


def _set_resid(s, value):
    from chase_amd.capi import lib
    np.ctypeslib.as_array(lib.chase_hip_solver_resid(s.h), shape=(s.nev + s.nex,))[:] = value


def _filter_legs(ctx, H, cplx, rounds, resid):
    """Start, initVecs, QR, Lock(5), residuals := resid; then per round (keys, shift c): set the keys, Shift(-c), two filter
    products over the unlocked columns, unshift.  Returns V, the counters and the hash of the fp64 H after every round."""
    from chase_amd.capi import Solver
    N, nev, nex = H.shape[0], 20, 12
    dH = ctx.array(H)
    s = Solver(ctx, None, nev, nex, h_on_device_ptr=dH.ptr, N=N, cplx=cplx)
    s.Start(); s.initVecs(True); s.QR(0, 1.0); s.Lock(5)
    _set_resid(s, resid)
    h0 = ctx.hash64(dH.ptr, N, N, N, cplx)
    out = []
    for (keys, c) in rounds:
        s.set(**keys)
        s.Shift(-c)
        for (a, b) in [(0.01, 0.0), (0.02, -0.3)]:                         # the filter's pattern: beta = 0 first
            s.HEMM(nev + nex - 5, a, b, 0)
        s.Shift(c, True)
        out.append(dict(V=s.peek_v(), restored=ctx.hash64(dH.ptr, N, N, N, cplx) == h0, **{k: s.get(k) for k in COUNTERS}))
    s.close()
    dH.free()
    return out


def _counters(r):
    return tuple(int(r[k]) for k in COUNTERS)


@pytest.mark.parametrize("cplx", [False, True])
def test_switch_at_operator_level(ctx, cplx):
    H = O.clement(300, cplx)
    split, packed = dict(mixed_precision=1, sp_product=1, sp_prepack=0), dict(mixed_precision=1, sp_product=1, sp_prepack=1)
    # two filter calls with different shifts: a whole pack, then a diagonal refresh - the bits of the unpacked bf16x3 path
    u = _filter_legs(ctx, H, cplx, [(split, 40.0), (split, 33.5)], 1.0)
    p = _filter_legs(ctx, H, cplx, [(packed, 40.0), (packed, 33.5)], 1.0)
    #                       sp  split  packed  full  diag  dp  filters
    assert _counters(u[0]) == (2, 2, 0, 0, 0, 0, 1) and _counters(u[1]) == (4, 4, 0, 0, 0, 0, 2)
    assert _counters(p[0]) == (2, 2, 2, 1, 0, 0, 1)
    assert _counters(p[1]) == (4, 4, 4, 1, 1, 0, 2)
    for a, b in zip(u, p):
        assert a["restored"] and b["restored"]                             # the fp64 H hash is restored
        assert a["V"].tobytes() == b["V"].tobytes()
    assert u[0]["V"].tobytes() != u[1]["V"].tobytes()
    # residuals at 1e-4: no pack, no packed call, the bits of a solver without any key
    off = _filter_legs(ctx, H, cplx, [({}, 40.0)], 1e-4)
    lo = _filter_legs(ctx, H, cplx, [(packed, 40.0)], 1e-4)
    assert _counters(lo[0]) == (0, 0, 0, 0, 0, 2, 0) and lo[0]["V"].tobytes() == off[0]["V"].tobytes()
    # sp_prepack = 1 with sp_product = 0: the fp32 MFMA path's bits and no packed call; without mixed_precision: nothing at all
    f32 = _filter_legs(ctx, H, cplx, [(dict(mixed_precision=1), 40.0)], 1.0)
    f32p = _filter_legs(ctx, H, cplx, [(dict(mixed_precision=1, sp_product=0, sp_prepack=1), 40.0)], 1.0)
    assert _counters(f32p[0]) == (2, 0, 0, 0, 0, 0, 1) and f32p[0]["V"].tobytes() == f32[0]["V"].tobytes()
    assert f32[0]["V"].tobytes() != u[0]["V"].tobytes()
    alone = _filter_legs(ctx, H, cplx, [(dict(mixed_precision=0, sp_product=1, sp_prepack=1), 40.0)], 1.0)
    off1 = _filter_legs(ctx, H, cplx, [({}, 40.0)], 1.0)
    assert _counters(alone[0]) == (0, 0, 0, 0, 0, 2, 0) and alone[0]["V"].tobytes() == off1[0]["V"].tobytes()


@pytest.mark.parametrize("cplx", [False, True])
def test_toggling_the_keys_between_filter_calls_keeps_both_images_right(ctx, cplx):
    """packed, unpacked bf16x3, fp32 MFMA, packed again, each with another shift: the pack skipped two shifts and the fp32 shadow
    one - every round has the bits of a solver that ran the same products without sp_prepack"""
    H = O.clement(300, cplx)
    mp = dict(mixed_precision=1)
    shifts = (40.0, 33.5, 51.0, 28.25, 45.0)
    kinds = (dict(sp_product=1, sp_prepack=1), dict(sp_product=1, sp_prepack=0), dict(sp_product=0, sp_prepack=1),
             dict(sp_product=1, sp_prepack=1), dict(sp_product=1, sp_prepack=0))
    got = _filter_legs(ctx, H, cplx, [(dict(mp, **k), c) for k, c in zip(kinds, shifts)], 1.0)
    want = _filter_legs(ctx, H, cplx, [(dict(mp, sp_product=k["sp_product"]), c) for k, c in zip(kinds, shifts)], 1.0)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a["restored"] and a["V"].tobytes() == b["V"].tobytes(), i
    #                         sp  split  packed  full  diag  dp  filters
    assert _counters(got[-1]) == (10, 8, 4, 1, 1, 0, 5) and _counters(want[-1]) == (10, 8, 0, 0, 0, 0, 5)


# ---- whole solves -------------------------------------------------------------------------------------------------------------------

SOLVES = [(256, False, 24, 16), (256, True, 24, 16), (1001, False, 100, 40)]      # tests/test_gpu_sp_bf16x3.py


def _solve(s):
    st = s.solve()
    return dict(iterations=st["iterations"], filtered_vecs=st["filtered_vecs"], ritzv=s.ritzv.tobytes(), resid=s.resid().tobytes(),
                V=s.V.tobytes())


@pytest.mark.parametrize("N,cplx,nev,nex", SOLVES, ids=["clement256-real", "clement256-complex", "clement1001-real"])
def test_whole_solve_with_the_packed_product(ctx, N, cplx, nev, nex):
    from chase_amd.capi import Solver
    H = O.clement(N, cplx)
    s = Solver(ctx, H, nev, nex)
    s.set(mixed_precision=1, sp_product=1)
    want = _solve(s)
    assert s.get("hemm_sp_split_calls") > 0 and s.get("hemm_sp_packed_calls") == 0 and s.get("sp_pack_full") == 0
    s.close()
    s = Solver(ctx, H, nev, nex)
    s.set(mixed_precision=1, sp_product=1, sp_prepack=1)
    for again in range(2):                                                 # the second solve re-uploads H: one whole pack per solve
        s.set(reset_counters=1)
        got = _solve(s)
        print(f"clement({N}, {cplx}) {nev}/{nex} packed: {got['iterations']} iterations, {int(s.get('hemm_sp_packed_calls'))} packed "
              f"products over {int(s.get('sp_filters'))} filter calls, {int(s.get('sp_pack_diag'))} diagonal refreshes")
        assert got == want, [k for k in got if got[k] != want[k]]
        assert s.get("sp_filters") >= 1 and s.get("hemm_calls") > 0
        assert s.get("hemm_sp_packed_calls") == s.get("hemm_sp_split_calls") == s.get("hemm_sp_calls") > 0
        assert s.get("sp_pack_full") == 1 and s.get("sp_pack_diag") == s.get("sp_filters") - 1
    s.set(reset_counters=1)
    assert s.get("hemm_sp_packed_calls") == 0 and s.get("sp_pack_full") == 0 and s.get("sp_pack_diag") == 0
    s.close()


@pytest.mark.parametrize("cplx", [False, True])
def test_a_new_matrix_on_the_same_solver_invalidates_the_pack(ctx, cplx):
    from chase_amd.capi import Solver
    N, nev, nex = 256, 24, 16
    H1 = O.clement(N, cplx)
    H2 = np.asfortranarray(H1 + np.diag(np.linspace(-3.0, 3.0, N)) + 0.25 * (np.eye(N, k=2) + np.eye(N, k=-2)))
    keys = dict(mixed_precision=1, sp_product=1, sp_prepack=1)
    fresh = Solver(ctx, H2.copy(order="F"), nev, nex)
    fresh.set(**keys)
    want = _solve(fresh)
    assert fresh.get("sp_pack_full") == 1
    fresh.close()
    H = H1.copy(order="F")
    s = Solver(ctx, H, nev, nex)                                           # the solver keeps the caller's host H
    s.set(**keys)
    first = _solve(s)
    assert s.get("sp_pack_full") == 1 and first["ritzv"] != want["ritzv"]
    H[:] = H2                                                              # replaced in place: the next solve uploads it
    got = _solve(s)
    assert s.get("sp_pack_full") == 2
    assert got == want, [k for k in got if got[k] != want[k]]
    s.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

def test_sp_prepack_key_values_and_pseudo_hermitian_refusal(ctx):
    from chase_amd.capi import ChaseHipError, PseudoSolver, Solver
    s = Solver(ctx, O.clement(64, False), 4, 4)
    assert s.get("sp_prepack") == 0
    for k in ("hemm_sp_packed_calls", "sp_pack_full", "sp_pack_diag"):
        assert s.get(k) == 0
    s.set(sp_prepack=1)
    assert s.get("sp_prepack") == 1 and s.get("sp_product") == 0            # a key of its own
    for bad in (2, -1, 0.5):
        with pytest.raises(ChaseHipError) as e:
            s.set(sp_prepack=bad)
        assert e.value.code == -1001 and "sp_prepack" in str(e.value)
    assert s.get("sp_prepack") == 1
    s.set(sp_prepack=0)
    assert s.get("sp_prepack") == 0
    s.close()
    H = np.asfortranarray(ctx.gen_bse(64, True, dmin=1.0, dmax=11.0, offdiag=1e-3, seed=7).download())
    p = PseudoSolver(ctx, H, 4, 4)
    with pytest.raises(ChaseHipError) as e:
        p.set(sp_prepack=1)
    assert e.value.code == -1001 and "sp_prepack" in str(e.value)
    p.set(sp_prepack=0)
    assert p.get("sp_prepack") == 0
    p.close()


def test_packed_entry_points_refuse_bad_arguments(ctx):
    from chase_amd.capi import ChaseHipError
    d = ctx.empty((8, 8), np.float32).upload(np.zeros((8, 8), np.float32))
    dP = _packed_buffer(ctx, ctx.bf16x3_pack_bytes(8, 8, False))
    for call in (lambda: ctx.bf16x3_pack(8, 8, d.ptr, 7, dP.ptr, False),                   # lda < m
                 lambda: ctx.bf16x3_pack(-1, 8, d.ptr, 8, dP.ptr, False),
                 lambda: ctx.bf16x3_pack(8, 8, d.ptr, 8, dP.ptr + 4, False),               # packed not 16-byte aligned
                 lambda: ctx.bf16x3_pack_diag(8, d.ptr, 7, dP.ptr, False),
                 lambda: ctx.gemm32p(8, 8, 8, 1.0, dP.ptr, d.ptr, 7, 0.0, d.ptr, 8, False),  # ldb < k
                 lambda: ctx.gemm32p(8, 8, 8, 1.0, None, d.ptr, 8, 0.0, d.ptr, 8, False)):
        with pytest.raises(ChaseHipError) as e:
            call()
        assert e.value.code == -1001
    ctx.gemm32p(0, 8, 8, 1.0, dP.ptr, d.ptr, 8, 0.0, d.ptr, 8, False)                      # m == 0 / n == 0: nothing to do
    ctx.gemm32p(8, 0, 8, 1.0, dP.ptr, d.ptr, 8, 0.0, d.ptr, 8, False)
    assert not np.any(d.download()) and np.all(dP.download() == 0xFF)
    d.free(); dP.free()


def test_grid_solver_refuses_the_packed_product():
    run_ranks(2, 1, G.scenario_grid_refuses, 64, False, transport="host")
