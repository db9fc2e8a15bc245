"""Child process of tests/test_gpu_processes.py for the dense chain's CHASE_HIP_* switches, which are read once per process:
    python tests/dense_chain_worker.py CASE...
opens one Context, runs the named cases - each calls one entry point on fixed seeded inputs and applies the checkers of
tests/dense_chain_refs.py - and prints DENSE_CHAIN_OK (exit 0) or the failing ratios (exit 1).  The parent sets the switches in
the environment; a case is written for the route its switch set selects and says which.  The thin device wrappers at the top
(host arrays in, host arrays out, leading dimensions taken from the padded arrays) are what tests/test_gpu_dense_chain.py calls
in-process as well."""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dense_chain_refs as D                                       # noqa: E402


# ---- device wrappers: every matrix is a Fortran array whose row count IS its leading dimension --------------------------------
def _dev(ctx, a):
    a = np.asarray(a)
    return ctx.array(a if a.size else np.zeros((1, 1), dtype=a.dtype))          # (no zero-byte allocations)


def _back(d, like):
    out = d.download()
    d.free()
    return out if like.size else np.asfortranarray(like)


def potrf(ctx, Ap, n):
    """-> (info, buffer)"""
    from chase_amd.capi import lib
    dA = _dev(ctx, Ap)
    info = lib.chase_hip_potrf_upper(ctx.h, int(np.iscomplexobj(Ap)), n, dA.ptr, Ap.shape[0])
    return info, _back(dA, Ap)


def trsm(ctx, Rp, Vp, m, n):
    """-> (V buffer, R buffer)"""
    from chase_amd.capi import lib, check
    dR, dV = _dev(ctx, Rp), _dev(ctx, Vp)
    check(lib.chase_hip_trsm_right_upper(ctx.h, int(np.iscomplexobj(Vp)), m, n, dR.ptr, Rp.shape[0], dV.ptr, Vp.shape[0]), "trsm")
    return _back(dV, Vp), _back(dR, Rp)


def herkx(ctx, Ap, Bp, Cp, n, k, mirror):
    """C = A^H B; B None: chase_hip_herk(A).  -> C buffer"""
    from chase_amd.capi import lib, check
    cplx = int(np.iscomplexobj(Cp))
    dA, dC = _dev(ctx, Ap), _dev(ctx, Cp)
    if Bp is None:
        check(lib.chase_hip_herk(ctx.h, cplx, n, k, dA.ptr, Ap.shape[0], dC.ptr, Cp.shape[0]), "herk")
    else:
        dB = _dev(ctx, Bp)
        check(lib.chase_hip_herkx(ctx.h, cplx, n, k, dA.ptr, Ap.shape[0], dB.ptr, Bp.shape[0], dC.ptr, Cp.shape[0], mirror), "herkx")
        dB.free()
    dA.free()
    return _back(dC, Cp)


def cholqr(ctx, Vp, Ap, m, n, variant, m_global):
    """-> (info, V buffer, A buffer)"""
    from chase_amd.capi import lib
    dV, dA = _dev(ctx, Vp), _dev(ctx, Ap)
    info = lib.chase_hip_cholqr(ctx.h, int(np.iscomplexobj(Vp)), m, n, dV.ptr, Vp.shape[0], dA.ptr, Ap.shape[0], variant, m_global)
    return info, _back(dV, Vp), _back(dA, Ap)


def houseqr(ctx, Vp, m, n):
    from chase_amd.capi import lib, check
    dV = _dev(ctx, Vp)
    check(lib.chase_hip_houseqr(ctx.h, int(np.iscomplexobj(Vp)), m, n, dV.ptr, Vp.shape[0]), "houseqr")
    return _back(dV, Vp)


def heevd(ctx, Ap, n, direct):
    """direct: chase_hip_heevd_gpu, else chase_hip_heevd.  -> (w, Z buffer)"""
    from chase_amd.capi import lib, check
    dA = _dev(ctx, Ap)
    w = np.zeros(n)
    f = lib.chase_hip_heevd_gpu if direct else lib.chase_hip_heevd
    check(f(ctx.h, int(np.iscomplexobj(Ap)), n, dA.ptr, Ap.shape[0], w.ctypes.data), "heevd_gpu" if direct else "heevd")
    return w, _back(dA, Ap)


def stedc(ctx, d, e, ldz, canary=D.CANARY):
    """-> (w, Z buffer of ldz rows)"""
    from chase_amd.capi import lib, check
    n = len(d)
    dd = np.ascontiguousarray(d, dtype=np.float64)
    ee = np.ascontiguousarray(np.concatenate([e, [0.0]]), dtype=np.float64)     # (never an empty array behind the pointer)
    Zp = np.full((ldz, n), canary, order="F")
    dZ = _dev(ctx, Zp)
    w = np.zeros(n)
    check(lib.chase_hip_stedc(ctx.h, n, dd.ctypes.data, ee.ctypes.data, w.ctypes.data, dZ.ptr, ldz), "stedc")
    return w, _back(dZ, Zp)


def pseudo_rr(ctx, A, M):
    """-> (rc, ritz values, vectors)"""
    from chase_amd.capi import lib
    n = A.shape[0]
    dA, dM = _dev(ctx, A), _dev(ctx, M)
    ritz = np.zeros(n)
    rc = lib.chase_hip_pseudo_rr_small(ctx.h, int(np.iscomplexobj(A)), n, dA.ptr, dM.ptr, ritz.ctypes.data)
    dA.free()
    return rc, ritz, _back(dM, M)


# ---- checks shared by the cases here and by the in-process tests ----------------------------------------------------------------
class Report:
    """collects (label, ratios) and remembers what exceeded 1"""

    def __init__(self):
        self.bad, self.count, self.peak = [], 0, {}

    def add(self, label, ratios):
        if not isinstance(ratios, dict):
            ratios = {"ratio": ratios}
        for k, v in ratios.items():
            self.count += 1
            self.peak[k] = max(self.peak.get(k, 0.0), float(v))
            if not v <= 1:
                self.bad.append((label, k, float(v)))

    def require(self, label, ok):
        self.count += 1
        if not ok:
            self.bad.append((label, "required", float("inf")))


def herm_input(n, cplx, kind):
    return D.herm_cases(np.random.default_rng(D.seed_of(4, n, cplx)), n, cplx, kind == "random")[kind]


HERM_KINDS = ["random", "double_decoupled", "tridiagonal", "diagonal", "scaled_identity"]


def check_heevd(ctx, rep, n, cplx, kinds, direct, pad=3, mrrr=False):
    for kind in kinds:
        A = herm_input(n, cplx, kind)
        w, Zp = heevd(ctx, D.padded(A, n + pad), n, direct)
        label = ("heevd_gpu" if direct else "heevd", n, cplx, kind)
        rep.add(label, D.eig_ratios(A, w, Zp[:n], mrrr))
        rep.require(label + ("padding",), D.same_padding(Zp, n))


def check_trsm(ctx, rep, m, n, cplx, pad_r=3, pad_v=3):
    rng = np.random.default_rng(D.seed_of(2, m, n, cplx))
    R = np.linalg.cholesky(D.hpd(rng, n, cplx, 1e5)).conj().T
    Rn = np.asfortranarray(np.triu(R) + np.tril(np.full((n, n), np.nan), -1))         # the strict lower triangle is never read
    V = D.rnd(rng, (m, n), cplx)
    Rp = D.padded(Rn, n + pad_r)
    Xp, Rback = trsm(ctx, Rp, D.padded(V, m + pad_v), m, n)
    label = ("trsm", m, n, cplx, pad_r, pad_v)
    rep.add(label, D.solve_ratio(Xp[:m], R, V))
    rep.require(label + ("padding",), D.same_padding(Xp, m))
    rep.require(label + ("R unchanged",), D.same_bits(Rback, Rp))


def hermitian_product_input(n, k, cplx):
    """W, Q (k x n) with W^H Q Hermitian (the projection of Rayleigh-Ritz): W = (S + S^H) Q"""
    rng = np.random.default_rng(D.seed_of(6, n, k, cplx))
    Q = D.rnd(rng, (k, n), cplx)
    S = D.rnd(rng, (k, k), cplx)
    return np.asfortranarray((S + S.conj().T) @ Q), Q


def check_herkx(ctx, rep, n, k, cplx, pad=3, block=None, full_flops=None):
    """mirror 1 and 0.  block: the trapezoid's block width when that route is expected (below it the canary survives with
    mirror = 0), else the one-GEMM route, which writes the whole n x n block.  full_flops: None, or True / False - the model
    flops on the books equal / undercut the full product."""
    from chase_amd.capi import gemm_counters
    W, Q = hermitian_product_input(n, k, cplx)
    ref = D.product_reference(W, Q)
    il = np.tril_indices(n, -1)
    for mirror in (1, 0):
        C0 = np.full((n + pad, n), D.CANARY, dtype=Q.dtype, order="F")
        m0 = gemm_counters(ctx, 0)[0]
        Cp = herkx(ctx, D.padded(W, k + pad), D.padded(Q, k + pad), C0, n, k, mirror)
        m1 = gemm_counters(ctx, 0)[0]
        label = ("herkx", n, k, cplx, mirror, pad)
        C = Cp[:n]
        rep.require(label + ("padding",), D.same_padding(Cp, n))
        rep.add(label + ("upper",), D.product_ratio(C, W, Q, D.upper_mask(n), ref))
        if mirror:
            rep.require(label + ("mirror",), D.same_bits(C[il], np.conj(C.T)[il]))
        elif block:
            below = il[0] // block > il[1] // block
            rep.require(label + ("canary below the trapezoid",), bool(np.all(C[il][below] == D.CANARY)))
            inside = np.zeros((n, n), dtype=bool); inside[il[0][~below], il[1][~below]] = True
            rep.add(label + ("diagonal blocks",), D.product_ratio(C, W, Q, inside, ref))
        else:
            rep.add(label + ("whole block",), D.product_ratio(C, W, Q, None, ref))     # one GEMM: the whole block is the product
        if full_flops is not None:
            full = 2.0 * (4 if cplx else 1) * n * n * k
            rep.require(label + ("flops", m1 - m0, full), (m1 - m0) == full if full_flops else (m1 - m0) < 0.7 * full)


def check_cholqr(ctx, rep, m, n, cplx, variant):
    rng = np.random.default_rng(D.seed_of(7, m, n, cplx))
    V = D.rnd(rng, (m, n), cplx)
    A0 = np.full((n + 3, n), D.CANARY, dtype=V.dtype, order="F")
    info, Qp, Ap = cholqr(ctx, D.padded(V, m + 3), A0, m, n, variant, 4 * m if variant == 3 else m)
    label = ("cholqr", m, n, cplx, variant)
    Q = Qp[:m]
    rep.require(label + ("info", info), info == 0)
    rep.require(label + ("padding",), D.same_padding(Qp, m) and D.same_padding(Ap, n))
    # tests/linalg/internal/cpu/cholqr1.cpp:31-126 as test_cholqr_reference_fixtures has it (well-conditioned input: every variant)
    orth = np.linalg.norm(Q.conj().T @ Q - np.eye(n)) / np.sqrt(n)
    rep.add(label + ("orthogonality",), abs(orth - D.EPS) / (15 * D.EPS))
    rep.add(label + ("span",), np.linalg.norm(V - Q @ (Q.conj().T @ V)) / (1e-10 * np.linalg.norm(V)))
    if variant == 1:
        rep.add(label + ("V = Q triu(A)",), D.solve_ratio(Q, Ap[:n], V))               # "A receives the last R"


def pseudo_input(n, cplx):
    """the inputs of test_pseudo_rayleigh_ritz_dense_core"""
    rng = np.random.default_rng(17)

    def herm(scale):
        X = rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if cplx else 0)
        return scale * (X + X.conj().T) / 2
    A = herm(0.05) + np.diag(np.linspace(1.0, 9.0, n))                     # Q^H S H Q: Hermitian positive definite
    M = herm(0.05) + np.diag(np.where(np.arange(n) % 2 == 0, 1.0, -1.0))  # Q^H S Q: Hermitian indefinite
    A = np.asfortranarray(A.astype(D.dt_of(cplx)))
    return A, np.asfortranarray(M.astype(A.dtype))


def check_pseudo_rr(ctx, rep, n, cplx):
    """the assertions of test_pseudo_rayleigh_ritz_dense_core"""
    import scipy.linalg as sla
    A, M = pseudo_input(n, cplx)
    rc, ritz, X = pseudo_rr(ctx, A, M)
    label = ("pseudo_rr_small", n, cplx)
    rep.require(label + ("rc", rc), rc == 0)
    if rc != 0:
        return
    mu = sla.eigh(M, A, eigvals_only=True)
    want = 1.0 / mu[::-1]
    h = n // 2
    rep.add(label + ("ritz values",), np.max(np.abs(ritz - want) / np.abs(want)) / 1e-10)
    rep.add(label + ("normalised",), np.max(np.abs(np.linalg.norm(X[:, :h], axis=0) - 1)) / 1e-12)
    Rm = A @ X[:, :h] - (M @ X[:, :h]) * ritz[:h]
    rep.add(label + ("residual",), np.max(np.linalg.norm(Rm, axis=0)) / (1e-10 * np.linalg.norm(A, 2) * np.max(np.abs(ritz[:h]))))
    A[5, 5] = -1.0
    rc = pseudo_rr(ctx, A, M)[0]
    rep.require(label + ("not positive definite", rc), 0 < rc <= n)


# ---- the cases, by switch set -------------------------------------------------------------------------------------------------
def _expect_env(**want):
    for k, v in want.items():
        assert os.environ.get(k) == v, "this case is written for %s=%s (found %r)" % (k, v, os.environ.get(k))


def blocks_trsm(ctx, rep):
    """CHASE_HIP_TRSM_BLOCK=128: wide blocks of 128 and of 72 / 8 columns - the rank-64 update INSIDE a block (rest = 64, rest = 8)"""
    _expect_env(CHASE_HIP_TRSM_BLOCK="128")
    for n in (129, 200, 333):
        for cplx in (False, True):
            check_trsm(ctx, rep, 150, n, cplx)


def blocks_herkx(ctx, rep):
    """CHASE_HIP_HERK_BLOCK=128: 515 columns = a trapezoid of five block columns, the last 3 wide"""
    _expect_env(CHASE_HIP_HERK_BLOCK="128")
    for cplx in (False, True):
        check_herkx(ctx, rep, 515, 300, cplx, block=128, full_flops=False)


def blocks_cholqr(ctx, rep):
    _expect_env(CHASE_HIP_TRSM_BLOCK="128", CHASE_HIP_HERK_BLOCK="128")
    for cplx in (False, True):
        check_cholqr(ctx, rep, 257, 65, cplx, 2)


def blocks_heevd_gpu(ctx, rep):
    """CHASE_HIP_APPLYQ_BLOCK=64: 199 reflectors = four back-transformation panels, the last 7 wide, two sub-blocks each"""
    _expect_env(CHASE_HIP_APPLYQ_BLOCK="64")
    for cplx in (False, True):
        check_heevd(ctx, rep, 200, cplx, ["random"], True)


def firstgen_heevd_gpu(ctx, rep):
    """CHASE_HIP_TRD_UNBLOCKED=1 + CHASE_HIP_TRIDIAG_MRRR=1: the trd_* kernels and the host stemr"""
    _expect_env(CHASE_HIP_TRD_UNBLOCKED="1", CHASE_HIP_TRIDIAG_MRRR="1")
    for n in (3, 65, 257):
        for cplx in (False, True):
            check_heevd(ctx, rep, n, cplx, HERM_KINDS, True, mrrr=True)


def firstgen_herkx(ctx, rep):
    """CHASE_HIP_HERK_BLOCK=0: one GEMM at a size that takes the trapezoid by default; the books hold the full product"""
    _expect_env(CHASE_HIP_HERK_BLOCK="0")
    check_herkx(ctx, rep, 1100, 300, False, full_flops=True)


def firstgen_pseudo_rr(ctx, rep):
    """CHASE_HIP_PSEUDO_RR_DEVICE=0 at n = 400 >= 384: host pre / post around the device eigensolver (the middle branch)"""
    _expect_env(CHASE_HIP_PSEUDO_RR_DEVICE="0")
    check_pseudo_rr(ctx, rep, 400, False)


def device3_heevd(ctx, rep):
    """CHASE_HIP_HEEVD_GPU_MIN=1: chase_hip_heevd goes to the device from 3 rows on; 1 and 2 rows stay on the host and succeed"""
    _expect_env(CHASE_HIP_HEEVD_GPU_MIN="1", CHASE_HIP_STEDC_GPU_MIN="1")
    for n in (1, 2, 3, 65, 129, 150):
        for cplx in (False, True):
            check_heevd(ctx, rep, n, cplx, HERM_KINDS if n <= 3 else ["random", "double_decoupled"], False)


def device3_heevd_gpu(ctx, rep):
    """CHASE_HIP_STEDC_GPU_MIN=1: the device divide & conquer below 512 rows - one merge level (129) and two (257)"""
    _expect_env(CHASE_HIP_STEDC_GPU_MIN="1")
    for n in (129, 257):
        for cplx in (False, True):
            check_heevd(ctx, rep, n, cplx, HERM_KINDS, True)


def device3_pseudo_rr(ctx, rep):
    """the device core at n = 96: a two-block Cholesky, heevd_gpu and the device divide & conquer under it"""
    _expect_env(CHASE_HIP_HEEVD_GPU_MIN="1")
    check_pseudo_rr(ctx, rep, 96, True)


def allhost_heevd(ctx, rep):
    """CHASE_HIP_HEEVD_GPU_MIN=0: host LAPACK at a size that goes to the device by default"""
    _expect_env(CHASE_HIP_HEEVD_GPU_MIN="0", CHASE_HIP_STEDC_GPU_MIN="0")
    for cplx in (False, True):
        check_heevd(ctx, rep, 700, cplx, ["random"], False)


def allhost_heevd_gpu(ctx, rep):
    """CHASE_HIP_STEDC_GPU_MIN=0: host dstedc under the device tridiagonalisation at 600 >= 512 rows"""
    _expect_env(CHASE_HIP_STEDC_GPU_MIN="0")
    for cplx in (False, True):
        check_heevd(ctx, rep, 600, cplx, ["random"], True)


def allhost_pseudo_rr(ctx, rep):
    _expect_env(CHASE_HIP_HEEVD_GPU_MIN="0")
    check_pseudo_rr(ctx, rep, 400, False)
    check_pseudo_rr(ctx, rep, 400, True)


CASES = {f.__name__: f for f in (blocks_trsm, blocks_herkx, blocks_cholqr, blocks_heevd_gpu, firstgen_heevd_gpu, firstgen_herkx,
                                 firstgen_pseudo_rr, device3_heevd, device3_heevd_gpu, device3_pseudo_rr, allhost_heevd,
                                 allhost_heevd_gpu, allhost_pseudo_rr)}


def main(argv):
    import time
    from chase_amd.capi import Context, lib
    unknown = [a for a in argv if a not in CASES]
    if unknown or not argv:
        print("unknown or missing cases:", unknown, "- known:", sorted(CASES))
        return 2
    rep = Report()
    with Context(0) as ctx:
        lib.chase_hip_ctx_set_phase(ctx.h, 0)
        for name in argv:
            t0 = time.monotonic()
            before = len(rep.bad)
            CASES[name](ctx, rep)
            print("%-22s %s  %.1f s  peaks %s" % (name, "ok" if len(rep.bad) == before else "FAILED", time.monotonic() - t0,
                                                  {k: round(v, 3) for k, v in rep.peak.items()}), flush=True)
            rep.peak = {}
    for b in rep.bad:
        print("EXCEEDED", b)
    if rep.bad:
        return 1
    print("DENSE_CHAIN_OK", rep.count, "checks")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
