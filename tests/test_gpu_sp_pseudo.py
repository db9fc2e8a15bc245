"""The single-precision pseudo-Hermitian solver (capi.SpPseudoSolver, chase_hip_solver_create_pseudo_sp, cchase_pseudo_) on the GPU.

1. the two new fp32 kernels bit for bit against numpy: padded ld, sentinel rim and neighbouring columns that must come back
   untouched, a 16-byte-aligned and a 4-byte-offset base pointer, real and complex;
2. the operators one by one on the tiny fixture (N = 10, h = 5 odd) and on N = 200, real and complex;
3. whole solves of the four cases of the emulation (tests/sp_pseudo_ref.py);
4. the cchase_*pseudo* sequence through ctypes;
5. the refused switches, the ignored environment variables and memory (no fp64 matrix on the device).
The test matrix is a float fixture of the reference divided by 64 (exact in fp32).  u = 2^-24 throughout."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import h2_mixed_ref as H2  # noqa: E402
import sp_pseudo_ref as R  # noqa: E402
import sp_solver_ref as SP  # noqa: E402
from oracle import chase_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
U = R.U
EINVAL = -1001
SENT = 777.0


def _st(cplx): return np.complex64 if cplx else np.float32


def _rand(rng, shape, cplx):
    a = rng.standard_normal(shape)
    if cplx:
        a = a + 1j * rng.standard_normal(shape)
    return np.asfortranarray(a.astype(_st(cplx)))


class _Window:
    """An m x n fp32 / complex fp32 matrix inside a flat float buffer on the device: leading dimension ld, one sentinel column
    on either side, sentinel pad rows, and `off` floats (4 bytes each) in front, so that the base pointer is 16-byte aligned
    (off = 0, ld * floats per element a multiple of 4) or not."""

    def __init__(self, ctx, A, ld, off):
        self.m, self.n = A.shape
        self.e = 2 if np.iscomplexobj(A) else 1
        self.ld, self.off, self.dtype = ld, off, A.dtype
        self.size = off + ld * self.e * (self.n + 2) + 5
        self.host = np.full(self.size, SENT, dtype=np.float32)
        self.view(self.host)[:self.m, 1:self.n + 1] = A
        self.dev = ctx.empty((self.size,), np.float32).upload(self.host)
        self.ptr = self.dev.ptr + 4 * (off + ld * self.e)                 # first element of the matrix

    def view(self, flat):
        """the ld x (n + 2) matrix inside a flat buffer (a view: writable)"""
        body = flat[self.off:self.off + self.ld * self.e * (self.n + 2)]
        return body.view(self.dtype).reshape((self.ld, self.n + 2), order="F")

    def expect(self, A_new):
        want = self.host.copy()
        self.view(want)[:self.m, 1:self.n + 1] = A_new
        return want


# ---- 1. kernels, bitwise --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_scale_rows_sp_bit_for_bit(ctx, cplx, off):
    rng = np.random.default_rng(11 + cplx + 2 * off)
    # the issue's shapes, and one whose columns take more than one block (2050 rows)
    for m, n in [(m, n) for m in (1, 7, 64, 257) for n in (1, 3)] + [(2050, 2)]:
        for ld in (m + 3, (m + 7) & ~3):                                  # an odd-ish padded ld and a multiple of 4
            for row0 in sorted({0, 3 if m > 3 else 1, m}):
                for s in (-1.0, np.float32(0.001)):
                    A = _rand(rng, (m, n), cplx)
                    w = _Window(ctx, A, ld, off)
                    ctx.scale_rows_sp(m, n, w.ptr, ld, row0, s, cplx)
                    got = w.dev.download()
                    want = R.scale_rows_sp_ref(A, row0, s)
                    if s == -1.0:
                        neg = A.copy(); neg[row0:, :] = -A[row0:, :]
                        assert want.tobytes() == neg.tobytes()            # s = -1 is negation
                    else:
                        ref = A.copy()                                    # x * float32(0.001), component by component
                        if cplx:
                            ref.real[row0:] = A.real[row0:] * np.float32(0.001); ref.imag[row0:] = A.imag[row0:] * np.float32(0.001)
                        else:
                            ref[row0:] = A[row0:] * np.float32(0.001)
                        assert want.tobytes() == ref.tobytes()
                    assert got.tobytes() == w.expect(want).tobytes(), (m, n, ld, row0, float(s))
                    w.dev.free()


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_kconj_sp_bit_for_bit(ctx, cplx, off):
    rng = np.random.default_rng(23 + cplx + 2 * off)
    # the issue's sizes (h = 1, 5, 129: odd; 258 complex floats per half: even), h even (N = 256) and more than one block (N = 4100)
    for N, n in [(N, n) for N in (2, 10, 258) for n in (1, 3)] + [(256, 2), (4100, 2)]:
        for ldf, lds in ((N + 3, N + 5), ((N + 3) & ~3, (N + 3) & ~3)):
            A = _rand(rng, (N, n), cplx)
            first = _Window(ctx, A, ldf, off)
            second = _Window(ctx, _rand(rng, (N, n), cplx), lds, off)
            ctx.kconj_sp(N, n, first.ptr, ldf, second.ptr, lds, cplx)
            assert first.dev.download().tobytes() == first.host.tobytes()              # the source is read only
            assert second.dev.download().tobytes() == second.expect(R.kconj_sp_ref(A)).tobytes(), (N, n, ldf, lds)
            first.dev.free(); second.dev.free()


def test_kernel_argument_checks_and_empty_extents(ctx):
    from chase_amd.capi import lib
    d = ctx.empty((64,), np.float32).upload(np.zeros(64, dtype=np.float32))
    sr, kc = lib.chase_hip_scale_rows_sp, lib.chase_hip_kconj_sp
    bad = [sr(ctx.h, 0, 8, 2, d.ptr, 7, 0, 1.0), sr(ctx.h, 0, 8, 2, d.ptr, 8, 9, 1.0), sr(ctx.h, 0, 8, 2, d.ptr, 8, -1, 1.0),
           sr(ctx.h, 0, -1, 2, d.ptr, 8, 0, 1.0), sr(ctx.h, 0, 8, 2, None, 8, 0, 1.0),
           kc(ctx.h, 0, 7, 1, d.ptr, 8, d.ptr + 128, 8), kc(ctx.h, 0, 8, 1, d.ptr, 7, d.ptr + 128, 8),
           kc(ctx.h, 0, 8, 1, d.ptr, 8, d.ptr + 128, 7), kc(ctx.h, 0, 8, 1, None, 8, d.ptr + 128, 8)]
    assert all(rc == EINVAL for rc in bad), bad
    empty = [sr(ctx.h, 1, 0, 2, None, 8, 0, 2.0), sr(ctx.h, 1, 8, 0, None, 8, 0, 2.0), sr(ctx.h, 1, 8, 2, d.ptr, 8, 8, 2.0),
             kc(ctx.h, 1, 0, 2, None, 8, None, 8), kc(ctx.h, 1, 8, 0, None, 8, None, 8)]
    assert all(rc == 0 for rc in empty), empty
    assert not d.download().any()
    d.free()


# ---- 2. operators ---------------------------------------------------------------------------------------------------------------

def _h2_step_reference(H, x, y, a, b, g):
    """One H^2 step in fp64 on the fp32 operands x (V1 columns) and y (V2 columns), and the bound of its fp32 evaluation propagated
    through product, product and axpy.  gp = product_gamma: an fp32 product alpha A B + beta C is off by at most
    gp (|alpha| |A| |B| + |beta| |C|) in modulus.
        T = H x                      |T^ - T| <= eT = gp |H| |x|
        Y = a H T + b y              |Y^ - Y| <= eY = gp (|a| |H| (|T| + eT) + |b| |y|) + |a| |H| eT
        Z = Y + g x                  the axpy errs by at most axpy_sp_bound(g, x, Y^) per component, |Y^| <= |Y| + eY per component
    """
    cplx = np.iscomplexobj(H)
    a, b, g = (float(np.float32(v)) for v in (a, b, g))                        # what the kernels are given
    Hw, aH = R.widen(H), np.abs(R.widen(H))
    xw, yw = R.widen(x), R.widen(y)
    gp = SP.product_gamma(H.shape[0], cplx)
    T = Hw @ xw
    eT = gp * (aH @ np.abs(xw))
    Y = a * (Hw @ T) + b * yw
    eY = gp * (abs(a) * (aH @ (np.abs(T) + eT)) + abs(b) * np.abs(yw)) + abs(a) * (aH @ eT)
    Z = Y + g * xw
    if cplx:
        sur = (np.abs(Y.real) + eY) + 1j * (np.abs(Y.imag) + eY)
        br, bi = H2.axpy_sp_bound(g, x, sur)
        ea = np.sqrt(br * br + bi * bi)
    else:
        ea = H2.axpy_sp_bound(g, x, np.abs(Y) + eY)
    return Z, eY + ea


def _qr_bound(N):
    """|| Q^H Q - I ||_F / sqrt(n) of the fp32 rounding of an fp64-orthonormal N x n block: Q32 = Q + E with |E_ij| <= u |Q_ij|, so
    ||E||_F <= u ||Q||_F = u sqrt(n) and ||E||_2 <= ||E||_F;  Q32^H Q32 - I = Q^H E + E^H Q + E^H E + (Q^H Q - I), whose Frobenius
    norm is at most 2 ||Q||_2 ||E||_F + ||E||_2 ||E||_F + d = sqrt(n) (2 u + u^2 sqrt(n)) + d, d the fp64 factorisation's own
    loss of orthogonality (CholQR2 / Householder: a modest multiple of N 2^-53, far below sqrt(N) u sqrt(n)).  Divided by
    sqrt(n): 2 u + u^2 sqrt(n) + d / sqrt(n) <= (sqrt(N) + 2) u."""
    return (np.sqrt(N) + 2) * U


OPERATOR_CASES = [("tiny", False), ("tiny", True), ("200", False), ("200", True)]


@pytest.mark.parametrize("size,cplx", OPERATOR_CASES, ids=["%s-%s" % (s, "complex" if c else "real") for s, c in OPERATOR_CASES])
def test_operators_on_fp32_data(ctx, size, cplx, capsys):
    from chase_amd.capi import SpPseudoSolver
    kind = "complex" if cplx else "real"
    H = R.fixture(kind, tiny=(size == "tiny"))
    N = H.shape[0]
    nev, nex, L = (2, 2, 1) if size == "tiny" else (12, 8, 3)
    ne, nc, h = nev + nex, 2 * (nev + nex), N // 2
    ldh = N + 6                                                # the caller's device matrix in place at a padded ld
    hH = np.full((ldh, N), SENT, dtype=H.dtype, order="F"); hH[:N] = H
    dH = ctx.empty((ldh, N), H.dtype).upload(hH)
    s = SpPseudoSolver(ctx, None, nev, nex, h_on_device_ptr=dH.ptr, N=N, cplx=cplx, ldh=ldh)
    assert (s.get("tol"), s.get("deg"), s.get("maxdeg"), s.get("lanczositer")) == (1e-5, 10, 18, 12)
    assert s.V.shape == (N, nc) and s.V.dtype == H.dtype and s.ritzv.shape == (nc,) and s.resid().shape == (nc,)
    rng = np.random.default_rng(N + cplx)
    V0 = _rand(rng, (N, nc), cplx)
    s.V[:, :] = V0
    s.Start(); s.initVecs(False)
    assert np.array_equal(s.peek_v(), R.widen(V0))
    # QR of the whole block: the rounding of an fp64-orthonormal block
    s.QR(0, 1.0)
    A0 = s.peek_v()
    dev = np.linalg.norm(A0.conj().T @ A0 - np.eye(nc)) / np.sqrt(nc)
    print(f"QR(0) {size} {kind}: ||Q^H Q - I||_F / sqrt(n) = {dev:.3e}, bound {_qr_bound(N):.3e}")
    assert dev <= _qr_bound(N)
    assert np.array_equal(A0, R.widen(R.narrow(A0)))
    # lock L pairs the way the driver does: the K-conjugates of the first L columns go to the last L
    s.ApplyKconjugate(L); s.Lock(L)
    A1 = s.peek_v()
    assert np.array_equal(R.narrow(A1[:, nc - L:]), R.kconj_sp_ref(R.narrow(A0[:, :L])))
    assert np.array_equal(A1[:, :nc - L], A0[:, :nc - L])
    X = R.narrow(A1)

    # HEMM_H2: one bracketed call of two steps, the second on fewer columns; then a call that only swaps
    (a1, g1), (a2, b2, g2) = (1.7, -0.31), (-2.3, 0.6, 0.17)
    s.set(reset_counters=1)
    s.FilterPhaseStart()
    s.HEMM_H2(2 * (ne - L), a1, 0.0, g1, 0)                    # the reference's run past the first half: clipped to it
    Z1 = s.peek_v()
    s.HEMM_H2(ne - L, a2, b2, g2, 2)
    Z2 = s.peek_v()
    s.HEMM_H2(ne - L, a2, b2, g2, ne - L)                      # c0 = nev + nex: only swaps the buffers
    Z3 = s.peek_v()
    s.HEMM_H2(ne - L, a2, b2, g2, ne - L)                      # ... and back: an even number of swaps, as in a filter call
    Z4 = s.peek_v()
    s.FilterPhaseEnd()
    want, bound = _h2_step_reference(H, X[:, L:ne], X[:, L:ne], a1, 0.0, g1)
    err = np.abs(Z1[:, L:ne] - want)
    print(f"HEMM_H2 step 1 {size} {kind}: max err / bound = {np.max(err / bound):.3f}")
    assert np.all(bound > 0) and np.all(err <= bound)
    # the two buffers before the call: V1 = A1, V2 = A0 (QR(0) left the same block in both; ApplyKconjugate wrote V1's tail only)
    keep = np.r_[0:L, ne:nc]
    assert np.array_equal(Z1[:, keep], A0[:, keep])            # locked columns and the whole second half: bit-identical
    x2 = R.narrow(Z1[:, L + 2:ne])
    want, bound = _h2_step_reference(H, x2, X[:, L + 2:ne], a2, b2, g2)
    err = np.abs(Z2[:, L + 2:ne] - want)
    print(f"HEMM_H2 step 2 {size} {kind}: max err / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    keep2 = np.r_[0:L + 2, ne:nc]
    assert np.array_equal(Z2[:, keep2], A1[:, keep2])          # every column outside [c0, c0 + ncols) of this buffer
    assert np.array_equal(Z3, Z1) and np.array_equal(Z4, Z2)   # ... and of the other one: the swap-only calls show both unchanged
    assert s.get("hemm_calls") == 0 and s.get("hemm_sp_calls") == 4 and s.get("sp_filters") == 1
    assert s.get("hemm_sp_vecs") == 2 * (ne - L) + 2 * (ne - L - 2)
    with pytest.raises(Exception):
        s.HEMM(ne - L, 1.0, 0.0, 0)                            # the pseudo-Hermitian filter has no HEMM

    # ApplyKconjugate of the unlocked first half
    blk = ne - L
    s.ApplyKconjugate(blk)
    K = s.peek_v()
    assert np.array_equal(R.narrow(K[:, ne:nc - L]), R.kconj_sp_ref(R.narrow(Z4[:, L:ne])))
    keep = np.r_[0:ne, nc - L:nc]
    assert np.array_equal(K[:, keep], Z4[:, keep])

    # QR with locked columns: the active block is the rounding of an fp64-orthonormal one, S-orthogonal to the locked vectors
    s.QR(L, 50.0)
    assert s.get("qr_variant") == 2                            # 1e1 < 50 < 1e4: the single-precision thresholds
    Q = s.peek_v()
    assert np.array_equal(Q[:, :L], A1[:, :L]) and np.array_equal(Q[:, nc - L:], A1[:, nc - L:])      # locked columns keep their bits
    Qa = Q[:, L:nc - L]
    na = nc - 2 * L
    dev = np.linalg.norm(Qa.conj().T @ Qa - np.eye(na)) / np.sqrt(na)
    SL = O.flip_lower_half(Q[:, np.r_[0:L, nc - L:nc]])
    devs = np.linalg.norm(Qa.conj().T @ SL) / np.sqrt(na)
    print(f"QR(L) {size} {kind}: ||Q^H Q - I||_F / sqrt(n) = {dev:.3e}, ||Q^H S V_locked||_F / sqrt(n) = {devs:.3e}, "
          f"bound {_qr_bound(N):.3e}")
    assert dev <= _qr_bound(N)
    # each locked column has norm <= 1 + 2u; rounding Qa moves Qa^H (S v) by at most u sqrt(na) ||v|| in the Frobenius norm per column
    assert devs <= _qr_bound(N) * np.sqrt(2 * L)

    # Rayleigh-Ritz: against the oracle's rayleighRitz_v2 on the widened H and Q; the allowance is 8 x what the emulation's RR
    # deviates from that reference on the same Q (a different summation order in two fp32-accumulated products, nothing more)
    s.RR(blk, L)
    n = 2 * blk
    ref_w, _ = O.rayleighRitz_v2(R.widen(H), Q[:, L:L + n])
    emu = R.OracleSpPseudo(H, nev, nex)
    emu.locked = L
    emu.V1 = np.asfortranarray(R.narrow(Q)); emu.V2 = emu.V1.copy(order="F")
    emu_w = np.zeros(n)
    emu.RR(emu_w, blk)
    dev_emu = float(np.max(np.abs(emu_w - ref_w)))
    dev_gpu = float(np.max(np.abs(s.ritzv[L:L + n] - ref_w)))
    print(f"RR {size} {kind}: max |ritz - rayleighRitz_v2| GPU {dev_gpu:.3e}, emulation {dev_emu:.3e}, ratio "
          f"{dev_gpu / dev_emu if dev_emu else float('inf'):.3f}")
    assert dev_gpu <= 8 * dev_emu
    V = s.peek_v()
    assert np.array_equal(V[:, :L], A1[:, :L]) and np.array_equal(V[:, nc - L:], A1[:, nc - L:])

    # residuals against fp64 on the same fp32 data
    r = s.Resd(L)
    ref = SP.host_residuals(H, s.ritzv[L:ne], V[:, L:ne])
    rb = SP.resid_product_bound(H, V[:, L:ne]) + 1e-13
    print(f"Resd {size} {kind}: max |resd - fp64| / bound = {float(np.max(np.abs(r - ref) / rb)):.3f}")
    assert np.all(np.abs(r - ref) <= rb)
    assert np.array_equal(s.resid()[L:ne], r)
    lam = s.ritzv.copy()
    rr = s.recompute_residuals(ne, lam)
    assert np.all(np.abs(rr[L:] - ref) <= rb)                  # a fresh product of all first-half columns
    refl = SP.host_residuals(H, lam[:L], s.peek_v()[:, :L])
    assert np.all(np.abs(rr[:L] - refl) <= SP.resid_product_bound(H, s.peek_v()[:, :L]) + 1e-13)

    # deferred swaps reach the fp32 block; End downloads it
    P0 = s.peek_v()
    s.Swap(L, ne - 1)
    P = s.peek_v()
    order = list(range(nc)); order[L], order[ne - 1] = order[ne - 1], order[L]
    assert np.array_equal(P, P0[:, order])
    with pytest.raises(Exception):
        s.set(device_rng=1)
    s.End()
    assert np.array_equal(R.widen(s.V), P)
    assert np.array_equal(dH.download(), hH)                   # H bit for bit, pads included
    s.close(); dH.free()


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_random_start_block_and_lanczos(ctx, cplx):
    """initVecs(random): the emulation's block bit for bit (host normals rounded to fp32, lower half times fl32(0.001) in fp32).
    lanczos_for_H2: in exact arithmetic the Ritz values of the S-inner-product recurrence lie inside the spectrum, so the upper
    bound of H^2 cannot exceed lambda_max^2; the fp32-input products err by product_gamma = 2.5e-5 relative at most, which 1e-3
    covers with room.  The emulation's figures are printed next to the solver's."""
    from chase_amd.capi import SpPseudoSolver
    kind = "complex" if cplx else "real"
    H = R.fixture(kind)
    nev, nex = 12, 8
    s = SpPseudoSolver(ctx, H, nev, nex)
    s.Start(); s.initVecs(True)
    k = R.OracleSpPseudo(H, nev, nex)
    k.initVecs(True)
    assert np.array_equal(s.peek_v(), R.widen(k.V1))
    s.QR(0, 1.0); k.QR(0, 1.0)
    ub, idx = s.lanczos_for_H2(10, 20)
    ub_k, idx_k = O.lanczos_for_H2(k, H.shape[0], 10, 20, nev + nex, k.ritzv)
    print(f"lanczos_for_H2 {kind}: upperb {ub:.9e} (emulation {ub_k:.9e}), idx {idx} ({idx_k})")
    lmax = float(np.max(R.positive_spectrum(H)))
    assert 0 < ub <= lmax * lmax * (1 + 1e-3) and 0 <= idx <= 20
    assert np.all(np.isfinite(s.ritzv[:nev + nex])) and np.all(s.ritzv[:nev + nex] <= ub)
    s.close()


# ---- 3. whole solves ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.CASES, ids=["%s-%d-%d" % c for c in R.CASES])
def test_whole_solves_of_the_emulated_cases(ctx, case):
    from chase_amd.capi import SpPseudoSolver
    kind, nev, nex = case
    emu = R.emulated(*case)["sp"]
    H = R.fixture(kind)
    H0 = H.copy()
    pos = R.positive_spectrum(H)
    s = SpPseudoSolver(ctx, H, nev, nex)
    s.set(numlanczos=10, lanczositer=50)
    tol = s.get("tol")
    assert tol == 1e-5
    st = s.solve()
    lam = s.ritzv[:nev].copy()
    own = s.resid()[:nev]
    host = SP.host_residuals(H, lam, s.V[:, :nev])
    pb = SP.resid_product_bound(H, s.V[:, :nev])
    eig_err = float(np.max(np.abs(np.sort(lam) - pos[:nev])))
    print("solve", case, {k: st[k] for k in ("iterations", "filtered_vecs", "locked")}, "emulation",
          {k: emu[k] for k in ("iterations", "filtered_vecs")}, "max own resid", float(np.max(own)), "max host resid",
          float(np.max(host)), "max product bound", float(np.max(pb)), "max eig err", eig_err)
    assert np.array_equal(H, H0)                             # the caller's host matrix is read only
    assert st["locked"] >= nev
    assert np.max(own) <= tol
    assert np.all(host <= tol + pb)
    assert eig_err <= tol
    assert abs(st["iterations"] - emu["iterations"]) <= 1
    assert abs(st["filtered_vecs"] - emu["filtered_vecs"]) <= 0.05 * emu["filtered_vecs"]
    assert s.get("hemm_calls") == 0 and s.get("hemm_sp_vecs") == st["filtered_vecs"]
    st2 = s.solve()                                          # the handle is reusable: same matrix, same counts
    assert (st2["iterations"], st2["filtered_vecs"], st2["locked"]) == (st["iterations"], st["filtered_vecs"], st["locked"])
    s.close()


# ---- 4. the C interface -----------------------------------------------------------------------------------------------------------

def test_single_precision_pseudo_c_interface(ctx):
    from chase_amd.capi import lib
    N, nev, nex = R.N_FIXTURE, 12, 8
    nc = 2 * (nev + nex)
    H = R.fixture("complex")
    pos = R.positive_spectrum(H)[:nev]
    ci = lambda v: C.byref(C.c_int(v))
    args = lambda mode: (ci(10), C.byref(C.c_float(1e-5)), C.c_char_p(mode), C.c_char_p(b"S"), C.c_char_p(b"C"))
    lib.chase_hip_cshim_seq_solver.restype = C.c_void_p
    live = lambda kind: lib.chase_hip_cshim_seq_solver(kind)
    def get(kind, key):
        out = C.c_double(0)
        assert lib.chase_hip_solver_get(C.c_void_p(live(kind)), key.encode(), C.byref(out)) == 0
        return out.value
    V = np.zeros((N, nc), dtype=H.dtype, order="F")
    lam = np.zeros(nc, dtype=np.float32)
    init = C.c_int(0)
    lib.cchase_init_pseudo_(ci(N), ci(nev), ci(nex), C.c_void_p(H.ctypes.data), ci(N), C.c_void_p(V.ctypes.data),
                            C.c_void_p(lam.ctypes.data), C.byref(init))
    assert init.value == 1 and live(5) and not live(4)
    lib.chase_set_num_lanczos_(ci(10)); lib.chase_set_lanczos_iter_(ci(50))      # the unified setters reach the handle
    assert get(5, "numlanczos") == 10 and get(5, "lanczositer") == 50
    lib.cchase_pseudo_(*args(b"R"))
    tol = float(np.float32(1e-5))
    assert get(5, "tol") == tol and get(5, "locked") >= nev and get(5, "hemm_calls") == 0
    its = get(5, "iterations")

    def check(vecs, vals):
        vals = vals.astype(np.float64)
        bound = tol + SP.resid_product_bound(H, vecs) + 4 * U * np.abs(vals)     # the Ritz values crossed the boundary as floats
        assert np.all(SP.host_residuals(H, vals, vecs) <= bound)
        assert np.max(np.abs(np.sort(vals) - pos)) <= tol
    check(V[:, :nev], lam[:nev])
    # cchase_ dispatches to the pseudo solver while that one is live
    V[:] = 0; lam[:] = 0
    lib.cchase_(*args(b"R"))
    assert get(5, "locked") >= nev and get(5, "iterations") == its
    check(V[:, :nev], lam[:nev])
    # get_eigenpairs into a padded block
    ld = N + 3
    out = np.zeros((ld, nev), dtype=H.dtype, order="F")
    lo = np.zeros(nev, dtype=np.float32)
    lib.cchase_get_eigenpairs_(C.c_void_p(out.ctypes.data), ci(ld), C.c_void_p(lo.ctypes.data))
    assert np.array_equal(out[:N], V[:, :nev]) and np.all(out[N:] == 0) and np.array_equal(lo, lam[:nev])
    lib.chase_set_max_iter_(ci(7))
    assert get(5, "maxiter") == 7
    # the internal variant owns its storage
    lib.cchase_init_pseudo_internal_(ci(N), ci(nev), ci(nex), C.c_void_p(H.ctypes.data), ci(N), C.byref(init))
    assert init.value == 1 and live(5)
    lib.chase_set_num_lanczos_(ci(10)); lib.chase_set_lanczos_iter_(ci(50))
    lib.cchase_pseudo_(*args(b"R"))
    out2 = np.zeros((N, nev), dtype=H.dtype, order="F")
    lib.cchase_get_eigenpairs_(C.c_void_p(out2.ctypes.data), ci(N), C.c_void_p(lo.ctypes.data))
    check(out2, lo)
    # the slot rules of z: a Hermitian init empties the pseudo slot, and the other way round
    Hh = np.asfortranarray((np.diag(np.arange(1, 65)) / 64.0).astype(np.complex64))
    Vh = np.zeros((64, 8), dtype=np.complex64, order="F")
    lh = np.zeros(8, dtype=np.float32)
    lib.cchase_init_(ci(64), ci(4), ci(4), C.c_void_p(Hh.ctypes.data), ci(64), C.c_void_p(Vh.ctypes.data), C.c_void_p(lh.ctypes.data),
                     C.byref(init))
    assert init.value == 1 and live(4) and not live(5)
    lib.cchase_init_pseudo_(ci(N), ci(nev), ci(nex), C.c_void_p(H.ctypes.data), ci(N), C.c_void_p(V.ctypes.data),
                            C.c_void_p(lam.ctypes.data), C.byref(init))
    assert init.value == 1 and live(5) and not live(4)
    lib.cchase_init_internal_(ci(64), ci(4), ci(4), C.c_void_p(Hh.ctypes.data), ci(64), C.byref(init))
    assert init.value == 1 and live(4) and not live(5)
    lib.cchase_init_pseudo_internal_(ci(N), ci(nev), ci(nex), C.c_void_p(H.ctypes.data), ci(N), C.byref(init))
    assert init.value == 1 and live(5) and not live(4)
    flag = C.c_int(7)
    lib.cchase_finalize_(C.byref(flag))
    assert flag.value == 0 and not live(4) and not live(5)
    before = V.copy()
    lib.cchase_pseudo_(*args(b"R")); lib.cchase_(*args(b"R"))      # finalised: no-ops
    assert np.array_equal(V, before)


# ---- 5. refusals, environment, memory -----------------------------------------------------------------------------------------------

def _bse1024(cplx):
    """the synthetic BSE matrix of the oracle at N = 1024 (its real part for the real solver: [[A, B], [-B, -A]] with symmetric
    blocks), divided by 16 (exact) and rounded to fp32: spectrum within about +-0.7"""
    N = 1024
    H = O.synthetic_bse_block(np.arange(N), np.arange(N), N) / 16.0
    return np.asfortranarray((H if cplx else H.real).astype(_st(cplx)))


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_refused_switches_ignored_environment_no_fp64_matrix(ctx, cplx, monkeypatch):
    from chase_amd.capi import ChaseHipError, SpPseudoSolver, lib, tape_mode
    N, nev, nex = 1024, 8, 8
    H = _bse1024(cplx)
    for var, val in (("CHASE_HIP_MIXED_PRECISION", "1"), ("CHASE_HIP_SP_PRODUCT", "bf16x3"), ("CHASE_HIP_SP_PREPACK", "1"),
                     ("CHASE_HIP_H2_MIXED_PRECISION", "1")):
        monkeypatch.setenv(var, val)
    s = SpPseudoSolver(ctx, H, nev, nex)
    fp64_matrix = N * N * 8 * (2 if cplx else 1)
    assert 0 < s.get("device_bytes") < fp64_matrix
    assert s.get("device_bytes") >= H.nbytes                 # its own fp32 copy of H is in the figure
    for key in ("mixed_precision", "sp_product", "sp_prepack", "h2_mixed_precision"):
        assert s.get(key) == 0                               # the environment did not reach it
        with pytest.raises(ChaseHipError) as e:
            s.set(**{key: 1})
        assert e.value.code == EINVAL and "single-precision pseudo-Hermitian solver" in str(e.value)
        s.set(**{key: 0})
    for mode in (1, 2):
        with pytest.raises(ChaseHipError) as e:
            tape_mode(s, mode)
        assert e.value.code == EINVAL and "single-precision pseudo-Hermitian solver" in str(e.value)
    tape_mode(s, 0)
    hv = C.c_ulonglong()
    assert lib.chase_hip_solver_hash_v(s.h, ctx.h, 1, C.byref(hv)) == EINVAL
    with pytest.raises(ChaseHipError) as e:
        s.set(device_rng=1)
    assert e.value.code == EINVAL
    s.set(device_rng=0)
    st = s.solve()
    print("N = 1024", "complex" if cplx else "real", {k: st[k] for k in ("iterations", "filtered_vecs", "locked")},
          "device_bytes", s.get("device_bytes"))
    assert s.get("hemm_calls") == 0 and s.get("hemm_sp_split_calls") == 0 and s.get("sp_h_converts") == 0
    assert s.get("hemm_sp_vecs") == st["filtered_vecs"]
    assert s.get("device_bytes") < fp64_matrix               # still no fp64 matrix after a solve
    s.close()
    # a device matrix at ld > N is used in place: nothing of the size of H is allocated, and H comes back bit for bit
    ldh = N + 4
    hH = np.full((ldh, N), SENT, dtype=H.dtype, order="F"); hH[:N] = H
    dH = ctx.empty((ldh, N), H.dtype).upload(hH)
    t = SpPseudoSolver(ctx, None, nev, nex, h_on_device_ptr=dH.ptr, N=N, cplx=cplx, ldh=ldh)
    assert t.get("device_bytes") < H.nbytes
    st2 = t.solve()
    assert t.get("device_bytes") < H.nbytes
    assert (st2["iterations"], st2["filtered_vecs"], st2["locked"]) == (st["iterations"], st["filtered_vecs"], st["locked"])
    assert np.array_equal(dH.download(), hH)
    t.close(); dH.free()
