"""CPU references of the single-precision pseudo-Hermitian solver (ChaseHipSpPseudo, capi.SpPseudoSolver).

* scale_rows_sp_ref / kconj_sp_ref: the two fp32 kernels in numpy, component by component (both are exact by construction, so
  the GPU tests compare bits).
* OracleSpPseudo: the emulation the solver was designed on, a subclass of the oracle's OraclePseudoCPU with the Impl's arithmetic
  and rounding points: H and the vector blocks are fp32; the start block is the host normals rounded to fp32 with the lower half
  times fl32(0.001) in fp32; an H^2 step is two fp32 products and an fp32 axpy; QR runs in fp64 on the exactly widened block with
  the float thresholds 1e4 / 1e1 and is rounded back, the locked columns keep their fp32 bits; Rayleigh-Ritz forms S H Q in fp32,
  forms Q^H (S H Q) and Q2^H Q2 as chase_hip_gemm_sd / _cz do - fp32 operands, the sum accumulated in fp32 on the matrix cores,
  the result and alpha acc + beta C in fp64 (include/chase_hip.h) -, runs the dense core in fp64, rounds the first n/2
  eigenvector columns and multiplies in fp32; residual norms are formed and summed in fp64 from the fp32 product; the Lanczos
  vectors are fp64 and each H v is that fp32-input product of the fp32 matrix with the rounded vector.  A real matrix keeps real
  blocks and real start vectors, as the real Impl does.  oracle/ is untouched.
* emulated(): the four cases of the issue on the reference's float BSE fixtures divided by 64 (exact in fp32; ||H||_2 becomes 0.62,
  so the floor sqrt(N) 2^-24 ||H|| = 5e-7 is below tol 1e-5), numLanczos 10, lanczosIter 50, the float defaults, solved by the fp64
  oracle on the widened fp32 matrix (same start vectors) and by the emulation, once per process.
"""
import functools
import os

import numpy as np
import scipy.linalg as sla
from oracle import chase_oracle as O

U = 2.0 ** -24
FIXTURES = {"complex": ("cfloat_random_BSE.bin", np.complex64), "real": ("float_random_BSE.bin", np.float32)}
TINY = {"complex": ("cfloat_tiny_random_BSE.bin", np.complex64), "real": ("float_tiny_random_BSE.bin", np.float32)}
N_FIXTURE, N_TINY = 200, 10
SCALE = 64.0
CASES = [("complex", 20, 20), ("complex", 12, 8), ("real", 20, 20), ("real", 12, 8)]
FLOAT_DEFAULTS = dict(tol=1e-5, deg=10, max_deg=18, lanczos_iter=12)
_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_fixtures")


def widen(A):
    return A.astype(np.complex128 if np.iscomplexobj(A) else np.float64)


def narrow(A):
    return A.astype(np.complex64 if np.iscomplexobj(A) else np.float32)


def read_fp32(name, N, dtype):
    """an N x N column-major fp32 / complex fp32 file of the reference's tests (tests/conftest.py reads the fp64 ones only)"""
    a = np.fromfile(os.path.join(_DIR, name), dtype=dtype)
    assert a.size == N * N, (name, a.size)
    return np.asfortranarray(a.reshape((N, N), order="F"))


def fixture(kind, tiny=False):
    """the float fixture divided by 64 (a power of two: exact), Fortran order"""
    name, dt = (TINY if tiny else FIXTURES)[kind]
    H = read_fp32(name, N_TINY if tiny else N_FIXTURE, dt)
    out = np.asfortranarray(H / dt(SCALE))
    assert out.dtype == dt and np.array_equal(widen(out) * SCALE, widen(H))
    return out


def positive_spectrum(H32):
    """smallest-first positive half of the dense spectrum of the widened matrix"""
    ev = np.linalg.eigvals(widen(H32)).real
    return np.sort(ev[ev > 0])


# ---- the two kernels ---------------------------------------------------------------------------------------------------

def scale_rows_sp_ref(X, row0, s):
    """X[row0:, :] *= s, one fp32 multiply per component (both components of a complex entry times the real s)"""
    out = np.array(X, order="F", copy=True)
    s = np.float32(s)
    if np.iscomplexobj(out):
        out.real[row0:, :] = out.real[row0:, :] * s
        out.imag[row0:, :] = out.imag[row0:, :] * s
    else:
        out[row0:, :] = out[row0:, :] * s
    assert out.dtype == X.dtype
    return out


def kconj_sp_ref(first):
    """the K-conjugate of the columns: halves swapped, complex entries conjugated"""
    h = first.shape[0] // 2
    out = np.empty_like(first, order="F")
    out[h:, :] = np.conj(first[:h, :])
    out[:h, :] = np.conj(first[h:, :])
    return out


# ---- the emulation -----------------------------------------------------------------------------------------------------

def gemm32w(A32, B32):
    """chase_hip_gemm_sd / _cz: fp32 operands, the accumulation in fp32 as in gemm_s / _c, the result handed over in fp64"""
    assert A32.dtype == B32.dtype and A32.dtype in (np.float32, np.complex64)
    return widen(A32 @ B32)


class _RoundedOperand:
    """H as Lanczos sees it: H @ v is the fp32-input product of the fp32 matrix with the vector rounded to fp32 (the Impl
    converts the block and calls chase_hip_gemm_sd / _cz)"""

    def __init__(self, H32):
        self.H32 = H32
        self.shape = H32.shape

    def __matmul__(self, v):
        v32 = narrow(v)
        return gemm32w(self.H32, v32 if np.iscomplexobj(self.H32) else v32.real).astype(v.dtype)


def rr_small(A, M):
    """the dense core of cpu::rayleighRitz_v2 (oracle.rayleighRitz_v2 from its Cholesky factorisation on): A = Q^H S H Q,
    M = I - 2 Q2^H Q2 -> (ritzv[n], Z[:, :n/2] normalised)"""
    n = A.shape[0]
    L = sla.cholesky(A, lower=True, check_finite=False)
    M = sla.solve_triangular(L, M, lower=True, check_finite=False)
    M = sla.solve_triangular(L, M.conj().T, lower=True, check_finite=False).conj().T
    M = -M
    w, Z = sla.eigh(M, lower=True, driver="evd", check_finite=False)
    w = -w
    Z = sla.solve_triangular(L, Z, lower=True, trans="C", check_finite=False)
    half = n // 2
    Z = Z[:, :half] / np.linalg.norm(Z[:, :half], axis=0)[None, :]
    return 1.0 / w, Z


class Oracle64(O.OraclePseudoCPU):
    """the fp64 oracle with the start vectors of the Impl under test: real normals for a real matrix"""

    def __init__(self, H, nev, nex):
        super().__init__(H, nev, nex)
        self.real_matrix = not np.iscomplexobj(H)

    def initVecs(self, random):
        if random:
            self.V1 = np.asfortranarray(O.random_start_vectors(self.N, self.ncol, not self.real_matrix).astype(self.dt))
            self.V1[self.N // 2:, :] *= 0.001
        self.V2 = self.V1.copy(order="F")


class OracleSpPseudo(O.OraclePseudoCPU):
    """OraclePseudoCPU with the arithmetic of ChaseHipSpPseudo.  self.H, self.V1, self.V2 are fp32; self.dt is the fp64 type."""

    def __init__(self, H32, nev, nex):
        assert H32.dtype in (np.float32, np.complex64)
        super().__init__(widen(H32), nev, nex)
        self.st = H32.dtype
        self.cplx = H32.dtype == np.complex64
        self.dt = np.complex128 if self.cplx else np.float64
        self.H = np.array(H32, order="F", copy=True)
        self.V1 = np.zeros((self.N, self.ncol), dtype=self.st, order="F")
        self.V2 = np.zeros_like(self.V1)
        for key, v in FLOAT_DEFAULTS.items():
            setattr(self.config, key, v)
        self.hemm_sp_calls = self.hemm_sp_vecs = 0

    def initVecs(self, random):
        if random:
            V = np.asfortranarray(narrow(O.random_start_vectors(self.N, self.ncol, self.cplx)))
            self.V1 = scale_rows_sp_ref(V, self.N // 2, np.float32(0.001))
        self.V2 = self.V1.copy(order="F")

    def HEMM_H2(self, block, alpha, beta, gamma, offset_left, offset_right=0):
        ncols = block - offset_right if offset_right < block else 0
        c0 = offset_left + self.locked
        if ncols and c0 < self.nevex:
            sl = slice(c0, min(c0 + ncols, self.nevex))
            a, b, g = self.st.type(alpha), self.st.type(beta), self.st.type(gamma)
            tmp = self.H @ self.V1[:, sl]
            out = a * (self.H @ tmp)
            if b != 0:
                out = out + b * self.V2[:, sl]
            out = out + g * self.V1[:, sl]
            assert out.dtype == self.st
            self.V2[:, sl] = out
            self.hemm_sp_calls += 2
            self.hemm_sp_vecs += 2 * (sl.stop - sl.start)
        self.V1, self.V2 = self.V2, self.V1

    def ApplyKconjugate(self, block):
        L = self.locked
        c2 = self.ncol - L - block
        self.V1[:, c2:c2 + block] = kconj_sp_ref(self.V1[:, L:L + block])

    def QR(self, fixednev, cond):
        L, nc = self.locked, self.ncol
        self.V2[:, :L] = self.V1[:, :L]
        self.V2[:, L:2 * L] = self.V1[:, nc - L:]
        self.V2[:, 2 * L:] = self.V1[:, L:nc - L]
        self.V1, self.V2 = self.V2, self.V1
        W = widen(self.V1)
        W[self.N // 2:, :2 * L] *= -1                           # S-orthogonality against the locked vectors, in fp64
        hi, lo = 1e4, 1e1                                       # the reference's single-precision thresholds
        if not self.config.cholqr and cond != 1.0:
            Q = O.houseQR(W); self.qr_variant = 0
        else:
            if cond > hi:
                Q, info = O.shiftedcholQR2(W); self.qr_variant = 3
            elif cond < lo:
                Q, info = O.cholQR1(W); self.qr_variant = 1
            else:
                Q, info = O.cholQR2(W); self.qr_variant = 2
            if info != 0:
                Q = O.houseQR(W); self.qr_variant = 0
        self.V1 = np.asfortranarray(narrow(Q))
        self.V2[:, L:nc - L] = self.V1[:, 2 * L:]
        self.V1, self.V2 = self.V2, self.V1                     # the locked columns here are the saved fp32 ones
        self.V2[:, :L] = self.V1[:, :L]
        self.V2[:, nc - L:] = self.V1[:, nc - L:]

    def RR(self, ritzv_view, block):
        L, n, k = self.locked, 2 * block, self.N // 2
        Q = self.V1[:, L:L + n]
        W = scale_rows_sp_ref(self.H @ Q, k, -1.0)               # S (H Q): fp32 product, exact flip
        Qh = np.ascontiguousarray(Q.conj().T)
        A = gemm32w(Qh, W)
        M = np.eye(n, dtype=self.dt) - 2.0 * gemm32w(np.ascontiguousarray(Q[k:, :].conj().T), np.ascontiguousarray(Q[k:, :]))
        w, Z = rr_small(A, M)
        ritzv_view[:n] = w
        self.V2[:, L:L + block] = Q @ narrow(Z)
        self.V1, self.V2 = self.V2, self.V1

    def Resd(self, ritzv_view, resid_view, fixednev):
        L = self.locked
        sub = self.nevex - L
        V = self.V1[:, L:L + sub]
        W = self.H @ V
        self.V2[:, L:L + sub] = W
        resid_view[:sub] = np.linalg.norm(widen(W) - widen(V) * np.asarray(ritzv_view[:sub])[None, :], axis=0)

    def Lanczos(self, M, numvec=None):
        op = _RoundedOperand(self.H)
        V64 = widen(self.V1).astype(np.complex128)
        if numvec is None:
            Theta, _, _ = O.lanczos_pseudo_multi(op, V64, M, 1)
            return float(Theta[M - 1])
        Theta, Tau, ritzV = O.lanczos_pseudo_multi(op, V64, M, numvec)
        cols = max(M, numvec)
        back = V64[:, :cols] if self.cplx else V64[:, :cols].real
        self.V1[:, :cols] = narrow(back)
        return float(Theta[M - 1]), Theta, Tau, ritzV

    def LanczosDos(self, idx, m, ritzVc):
        self.V1[:, :idx] = narrow(gemm32w(np.ascontiguousarray(self.V1[:, :m]), narrow(np.asarray(ritzVc)[:, :idx].astype(self.dt))))
        self.V1[:, idx:m] = self.V2[:, idx:m]


def host_residuals(H32, lam, V):
    """fp64 residual norms || H v - lambda v ||_2 against the fp32 matrix (V fp32 or fp64)"""
    H, V = widen(H32), widen(np.asarray(V))
    return np.linalg.norm(H @ V - V * np.asarray(lam)[None, :], axis=0)


def configure(k):
    k.config.num_lanczos, k.config.lanczos_iter = 10, 50
    for key in ("tol", "deg", "max_deg"):
        setattr(k.config, key, FLOAT_DEFAULTS[key])


@functools.lru_cache(maxsize=None)
def emulated(kind, nev, nex):
    """One case solved by the fp64 oracle (widened fp32 matrix) and by the emulation: counts, locked pairs, the emulation's own
    residuals, the largest fp64 residual of its wanted pairs against the fp32 matrix and the eigenvalue error against the dense
    spectrum"""
    H32 = fixture(kind)
    pos = positive_spectrum(H32)
    k64 = Oracle64(widen(H32), nev, nex)
    configure(k64)
    s64 = O.solve_pseudo(k64)
    k = OracleSpPseudo(H32, nev, nex)
    configure(k)
    st = O.solve_pseudo(k)
    lam = k.ritzv[:nev].copy()
    return dict(
        fp64=dict(iterations=s64["iterations"], filtered_vecs=s64["filtered_vecs"], locked=s64["locked"],
                  eig_err=float(np.max(np.abs(np.sort(k64.ritzv[:nev]) - pos[:nev])))),
        sp=dict(iterations=st["iterations"], filtered_vecs=st["filtered_vecs"], locked=st["locked"],
                hemm_sp_vecs=k.hemm_sp_vecs, own_resid=k.resid[:nev].copy(), ritzv=lam,
                max_resid=float(np.max(host_residuals(H32, lam, k.V1[:, :nev]))),
                eig_err=float(np.max(np.abs(np.sort(lam) - pos[:nev])))))
