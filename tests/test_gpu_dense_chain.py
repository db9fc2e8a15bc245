"""The dense chain between the filter and the Ritz pairs - herk / herkx, potrf_upper, trsm_right_upper, cholqr, houseqr, heevd /
heevd_gpu, stedc - called directly through the C ABI with the default switches and held against the checkers of
tests/dense_chain_refs.py: componentwise backward-error bounds with factor 1 (Cholesky, solve, product), 8 x LAPACK's own
measured error (QR, eigensolvers).  Real and complex, leading dimension equal to the extent and padded by 3 rows of a canary
that must survive bit for bit, at the smallest shapes that cross each edge: the 64-wide blocks of the factorisation and the
solve, the 32-wide panels of the tridiagonalisation, 128-row leaves and 512 rows of the divide & conquer, the 1792-row chunk
switch.  The documented input contracts (triangle never read, diagonal imaginary parts ignored, info of the first bad pivot,
tau = 0) are exercised as well.  The routes behind the CHASE_HIP_* switches run in child processes: tests/test_gpu_processes.py."""
import numpy as np
import pytest
import dense_chain_refs as D
import dense_chain_worker as W

pytestmark = pytest.mark.gpu
CPLX = pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
PAD = pytest.mark.parametrize("pad", [0, 3], ids=["ld=extent", "ld=extent+3"])


@pytest.fixture(scope="module")
def dctx(ctx):
    from chase_amd.capi import lib
    lib.chase_hip_ctx_set_phase(ctx.h, 0)          # four-multiplication complex products, as the Impls have it around these calls
    return ctx


def _ok(rep):
    print("largest ratios:", {k: float("%.3g" % v) for k, v in rep.peak.items()})
    assert not rep.bad, rep.bad[:8]
    assert rep.count > 0


def _nan_lower(A):
    return np.asfortranarray(np.triu(A) + np.tril(np.full(A.shape, np.nan), -1))


def _nan_upper(A):
    return np.asfortranarray(np.tril(A) + np.triu(np.full(A.shape, np.nan), 1))


# ---- potrf_upper ---------------------------------------------------------------------------------------------------------------
@CPLX
@PAD
@pytest.mark.parametrize("kappa", [10.0, 1e10])
def test_potrf_upper_componentwise_bound_and_lower_triangle_never_read(dctx, cplx, pad, kappa):
    rep = W.Report()
    for n in D.POTRF_SIZES:
        A = D.hpd(np.random.default_rng(D.seed_of(1, n, cplx)), n, cplx, kappa)
        info, Rp = W.potrf(dctx, D.padded(A, n + pad), n)
        label = ("potrf", n, cplx, pad, kappa)
        rep.require(label + ("info", info), info == 0)
        rep.add(label, D.chol_ratio(A, Rp[:n]))
        rep.require(label + ("padding",), D.same_padding(Rp, n))
        info2, Rn = W.potrf(dctx, D.padded(_nan_lower(A), n + pad), n)
        rep.require(label + ("lower never read",), info2 == 0 and D.same_bits(np.triu(Rn[:n]), np.triu(Rp[:n])))
    _ok(rep)


@CPLX
def test_potrf_upper_info_is_the_first_bad_pivot(dctx, cplx):
    n = 129
    A = D.hpd(np.random.default_rng(D.seed_of(1, n, cplx)), n, cplx, 10.0)
    for p in (0, 63, 64, n - 1):
        for bad in (-1.0, 0.0, np.nan):
            B = A.copy(); B[p, p] = bad
            if bad == 0.0:
                B[p, :] = 0; B[:, p] = 0                         # an exactly zero pivot: the row's updates are all zero as well
            assert W.potrf(dctx, D.padded(B, n + 3), n)[0] == p + 1, (p, bad)
    B = A.copy(); B[10, 10] = -1.0; B[100, 100] = -1.0
    assert W.potrf(dctx, B, n)[0] == 11                           # first failure wins
    assert W.potrf(dctx, np.zeros((0, 0), dtype=A.dtype, order="F"), 0)[0] == 0      # n = 0 is legal


# ---- trsm_right_upper ------------------------------------------------------------------------------------------------------------
@CPLX
@pytest.mark.parametrize("m", [1, 150, 257])
def test_trsm_right_upper_componentwise_bound(dctx, cplx, m):
    """R: the reference factor of hpd(n, 1e5) with NaN in its strict lower triangle; ldr and ldv padded independently"""
    rep = W.Report()
    pads = [(0, 0), (3, 0), (0, 5), (3, 5)]
    for i, n in enumerate(D.POTRF_SIZES):
        for pad_r, pad_v in (pads[i % 4], pads[(i + 1) % 4]):
            W.check_trsm(dctx, rep, m, n, cplx, pad_r, pad_v)
    _ok(rep)


# ---- herkx / herk -----------------------------------------------------------------------------------------------------------------
@CPLX
@PAD
def test_herkx_and_herk_on_the_one_gemm_route(dctx, cplx, pad):
    """n < 4 blocks of 256: one GEMM.  Upper triangle within the product bound; mirror = 1: the lower triangle is the exact
    conjugate; mirror = 0 on this route: the WHOLE block is the product.  k = 0 gives C = 0 on what is written."""
    rep = W.Report()
    for n, k in ((1, 1), (129, 1), (129, 0), (200, 333)):
        W.check_herkx(dctx, rep, n, k, cplx, pad=pad, full_flops=True)
        V = D.rnd(np.random.default_rng(D.seed_of(8, n, k, cplx)), (k, n), cplx)
        Gp = W.herkx(dctx, D.padded(V, k + pad), None, np.full((n + pad, n), D.CANARY, dtype=V.dtype, order="F"), n, k, 1)
        label = ("herk", n, k, cplx, pad)
        rep.add(label, D.product_ratio(Gp[:n], V, V, D.upper_mask(n)))
        il = np.tril_indices(n, -1)
        rep.require(label + ("mirror",), D.same_bits(Gp[:n][il], np.conj(Gp[:n].T)[il]))
        rep.require(label + ("padding",), D.same_padding(Gp, n))
    _ok(rep)


# ---- cholqr -----------------------------------------------------------------------------------------------------------------------
@CPLX
@pytest.mark.parametrize("variant", [1, 2, 3])
def test_cholqr_variants_with_padded_leading_dimensions(dctx, cplx, variant):
    rep = W.Report()
    for m, n in ((100, 50), (257, 65)):
        W.check_cholqr(dctx, rep, m, n, cplx, variant)
    _ok(rep)


# ---- houseqr ------------------------------------------------------------------------------------------------------------------------
@CPLX
@PAD
def test_houseqr_against_lapack_and_on_tau_zero_inputs(dctx, cplx, pad):
    """random input: orthogonality, span, triangularity and - where kappa_2(V) <= 1e3 - the nested column spaces against LAPACK's Q.
    Zero column, duplicate column, upper triangular (tau = 0: zero tail under a real pivot) and upper triangular with a complex
    diagonal (zero tail under a complex pivot): Q finite, orthonormal, spanning V, R triangular."""
    rep = W.Report()
    for m, n in D.QR_SHAPES:
        for kind, V in D.qr_cases(np.random.default_rng(D.seed_of(3, m, n, cplx)), m, n, cplx).items():
            Qp = W.houseqr(dctx, D.padded(V, m + pad), m, n)
            label = ("houseqr", m, n, cplx, pad, kind)
            rep.add(label, D.qr_ratios(V, Qp[:m]))
            rep.require(label + ("padding",), D.same_padding(Qp, m))
            if kind == "random" and np.linalg.cond(V) <= 1e3:
                rep.add(label + ("vs LAPACK",), D.qr_vs_lapack_ratios(V, Qp[:m]))
    _ok(rep)


# ---- heevd_gpu / heevd ------------------------------------------------------------------------------------------------------------
@CPLX
@pytest.mark.parametrize("n", D.HEEVD_GPU_SIZES)
def test_heevd_gpu_every_matrix_kind_and_its_input_contract(dctx, cplx, n):
    """32-wide panels full and ragged, host stedc below 512 rows, device divide & conquer at 513.  Lower triangle authoritative:
    NaN in the strict upper triangle - and, complex, garbage in the diagonal's imaginary parts - give bit-identical w and Z."""
    rep = W.Report()
    W.check_heevd(dctx, rep, n, cplx, W.HERM_KINDS, True, pad=3)
    W.check_heevd(dctx, rep, n, cplx, ["random"], True, pad=0)
    A = W.herm_input(n, cplx, "random")
    w, Z = W.heevd(dctx, A, n, True)
    B = _nan_upper(A)
    if cplx:
        B[np.arange(n), np.arange(n)] += 1j * np.linspace(-3.0, 1e300, n)
    w2, Z2 = W.heevd(dctx, B, n, True)
    rep.require(("heevd_gpu", n, cplx, "upper never read, diagonal imaginary parts ignored"), D.same_bits(w, w2) and D.same_bits(Z, Z2))
    _ok(rep)


def test_heevd_gpu_at_1800_rows_takes_the_128_column_chunk(dctx):
    """trailing sizes >= 1792 run the blocked tridiagonalisation's GEMV with chunks of 128 columns, below that with 64"""
    rep = W.Report()
    W.check_heevd(dctx, rep, 1800, False, ["random"], True, pad=0)
    _ok(rep)


@CPLX
@pytest.mark.parametrize("n", D.HEEVD_HOST_SIZES)
def test_heevd_host_path_with_padded_lda(dctx, cplx, n):
    rep = W.Report()
    W.check_heevd(dctx, rep, n, cplx, W.HERM_KINDS, False, pad=3)
    A = W.herm_input(n, cplx, "random")
    w, Zp = W.heevd(dctx, D.padded(A, n + 3), n, False)
    w2, Zp2 = W.heevd(dctx, D.padded(_nan_upper(A), n + 3), n, False)
    rep.require(("heevd", n, cplx, "upper never read"), D.same_bits(w, w2) and D.same_bits(Zp, Zp2))
    _ok(rep)


# ---- stedc ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", D.STEDC_SIZES)
def test_stedc_every_case_with_padded_ldz(dctx, n):
    """one leaf (<= 128 rows), one, two and three merge levels; every matrix of tridiag_cases (glued_wilkinson has its own size,
    a multiple of 21); the canary rows of Z untouched"""
    rep = W.Report()
    for name, (d, e) in D.small_tridiag_cases(n, np.random.default_rng(D.seed_of(5, n))).items():
        nn = len(d)
        for pad in (0, 3):
            w, Zp = W.stedc(dctx, d, e, nn + pad)
            rep.add(("stedc", n, name, pad), D.tridiag_ratios(d, e, w, Zp[:nn]))
            rep.require(("stedc", n, name, pad, "padding"), D.same_padding(Zp, nn))
    _ok(rep)
