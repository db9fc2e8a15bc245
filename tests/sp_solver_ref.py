"""CPU references of the single-precision Hermitian solver (ChaseHipSp, capi.SpSolver).

* OracleSp: the emulation the solver was designed on, a subclass of the oracle's OracleCPU with the Impl's arithmetic: H and the
  vector blocks are fp32 and every H-times-block product is an fp32 product; QR, the projected matrix and its eigensolver run in
  fp64 on exactly widened data and their results are rounded to fp32 where the Impl rounds; the shifted diagonal is always
  fl32(saved entry + accumulated shift); the Lanczos vectors are fp64 and each H v multiplies the fp32 matrix with the rounded
  vector; residual norms are formed and summed in fp64 from the fp32 product.  oracle/ is untouched.
* emulated(): the four cases of the issue - Clement matrices clement(N, cplx, 1e-6) / N rounded to fp32, the reference's float
  defaults (tol 1e-5, deg 10, maxDeg 18, lanczosIter 12) - solved by the fp64 oracle (on the widened fp32 matrix) and by the
  emulation, once per process: counts and the largest fp64 residual against the fp32 matrix.
* bounds, u = 2^-24 (derived, not tuned):
    product_gamma       (N + 8) u real / (2N + 16) u complex: the fma-chain bound of one fp32 product that
                        tests/test_gpu_mixed_precision.py derives (Higham (3.5); complex from four real products)
    resid_product_bound || gamma |H| |v_j| ||_2: what an fp32 H v_j can be off by, in the 2-norm of a residual
    ritz_margin         the Ritz values are eigenvalues of A = Q^H fl32(H Q), formed by a second fp32-accumulated product: A is
                        off by at most E = gamma |Q|^H (|H| |Q|) (2 + gamma) entry by entry, and eigenvalues move by at most
                        ||E||_2 <= ||E||_F (Weyl)
    resid_norms_bound   the kernel's own rounding: every fp32 entry widens exactly; r_i = w_i - lambda v_i is formed in fp64 with
                        at most two roundings (one with an fma): |e_i| <= 2 u64 (|w_i| + |lambda v_i|); n squares summed in any
                        order and a square root add (n + 3) u64 relative; | ||r + e|| - ||r|| | <= ||e||:
                        |computed - exact| <= ||e||_2 + (n + 3) u64 (||r||_2 + ||e||_2), u64 = 2^-53, n floats per column
"""
import functools

import numpy as np
import scipy.linalg as sla
from oracle import chase_oracle as O

U = 2.0 ** -24
U64 = 2.0 ** -53
# (N, nev, nex, complex): the issue's cases with iterations / filtered vectors / residual ceiling of its author's emulation run
CASES = [(256, 24, 16, False), (256, 24, 16, True), (301, 30, 20, True), (1001, 100, 60, False)]
FLOAT_DEFAULTS = dict(tol=1e-5, deg=10, max_deg=18, lanczos_iter=12)


def case_matrix(N, cplx):
    """clement(N, cplx, 1e-6) / N rounded to fp32 (Fortran order): norm of order 1, as tol 1e-5 needs"""
    return np.asfortranarray((O.clement(N, cplx, 1e-6) / N).astype(np.complex64 if cplx else np.float32))


def widen(A):
    return A.astype(np.complex128 if np.iscomplexobj(A) else np.float64)


def narrow(A):
    return A.astype(np.complex64 if np.iscomplexobj(A) else np.float32)


class _RoundedOperand:
    """H as Lanczos sees it: (H^H) @ v multiplies the widened fp32 matrix with the vector rounded to fp32 (the Impl converts the
    block and calls the fp32-input product).  H is Hermitian, so conj() and T return the operator itself."""

    def __init__(self, H32):
        self.H64 = widen(H32)
        self.shape = H32.shape

    def conj(self): return self
    @property
    def T(self): return self
    def __matmul__(self, v): return self.H64 @ widen(narrow(v))


class OracleSp(O.OracleCPU):
    """OracleCPU with the arithmetic of ChaseHipSp.  self.H, self.V1, self.V2 are fp32; self.dt stays the fp64 type (what the
    driver's scalars and the projected eigenvectors are)."""

    def __init__(self, H32, nev, nex):
        assert H32.dtype in (np.float32, np.complex64)
        super().__init__(widen(H32), nev, nex)
        self.st = H32.dtype
        self.H = np.array(H32, order="F", copy=True)
        self.V1 = np.zeros((self.N, self.nevex), dtype=self.st, order="F")
        self.V2 = np.zeros_like(self.V1)
        for key, v in FLOAT_DEFAULTS.items():
            setattr(self.config, key, v)
        self.shift = 0.0
        self.d0 = None
        self.hemm_sp_calls = self.hemm_sp_vecs = 0

    def initVecs(self, random):
        if random:
            self.V1 = np.asfortranarray(narrow(O.random_start_vectors(self.N, self.nevex, self.cplx)))
        self.V2 = self.V1.copy(order="F")

    def Shift(self, c, isunshift=False):
        idx = np.arange(self.N)
        if self.shift == 0.0:
            self.d0 = self.H[idx, idx].copy()
        self.shift = 0.0 if isunshift else self.shift + float(np.real(c))
        re = (self.d0.real.astype(np.float64) + self.shift).astype(np.float32)
        self.H[idx, idx] = (re + 1j * self.d0.imag).astype(self.st) if self.cplx else re

    def HEMM(self, block, alpha, beta, offset_left, offset_right=0):
        ncols = block - offset_right if offset_right < block else 0
        if ncols:
            c0 = self.locked + offset_left
            sl = slice(c0, c0 + ncols)
            a, b = self.st.type(alpha), self.st.type(beta)
            out = a * (self.H @ self.V1[:, sl])
            if b != 0:
                out = out + b * self.V2[:, sl]
            assert out.dtype == self.st
            self.V2[:, sl] = out
            self.counters["hemm_cols"] += ncols
            self.hemm_sp_calls += 1
            self.hemm_sp_vecs += ncols
        self.V1, self.V2 = self.V2, self.V1

    def QR(self, fixednev, cond):
        L = self.locked
        self.V2[:, :L] = self.V1[:, :L]
        W = widen(self.V1)
        hi, lo = 1e4, 1e1                                    # the reference's single-precision thresholds
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
        self.V1[:, :L] = self.V2[:, :L]

    def RR(self, ritzv_view, block):
        L = self.locked
        Q = self.V1[:, L:L + block]
        W = self.H @ Q
        A = widen(Q).conj().T @ widen(W)
        w, Z = sla.eigh(A, lower=True, driver="evd", check_finite=False)
        ritzv_view[:block] = w
        self.V2[:, L:L + block] = Q @ narrow(Z)
        self.V1, self.V2 = self.V2, self.V1

    def Resd(self, ritzv_view, resid_view, fixednev):
        L = self.locked
        sub = self.nevex - L
        V = self.V1[:, L:]
        W = self.H @ V
        self.V2[:, L:] = W
        resid_view[:sub] = np.linalg.norm(widen(W) - widen(V) * np.asarray(ritzv_view[:sub])[None, :], axis=0)

    def Lanczos(self, M, numvec=None):
        op = _RoundedOperand(self.H)
        V64 = widen(self.V1)
        if numvec is None:
            return O.lanczos_multi(op, V64, M, 1)[0]
        out = O.lanczos_multi(op, V64, M, numvec)
        cols = max(M, numvec)
        self.V1[:, :cols] = narrow(V64[:, :cols])
        return out

    def LanczosDos(self, idx, m, ritzVc):
        self.V1[:, :idx] = narrow(widen(self.V1[:, :m]) @ widen(narrow(ritzVc[:, :idx])))
        self.V1[:, idx:m] = self.V2[:, idx:m]


def host_residuals(H32, lam, V):
    """fp64 residual norms || H v - lambda v ||_2 against the fp32 matrix (V fp32 or fp64)"""
    H, V = widen(H32), widen(np.asarray(V))
    return np.linalg.norm(H @ V - V * np.asarray(lam)[None, :], axis=0)


def product_gamma(N, cplx):
    return ((2 * N + 16) if cplx else (N + 8)) * U


def resid_product_bound(H32, V):
    """per column: || gamma |H| |v_j| ||_2"""
    g = product_gamma(H32.shape[0], np.iscomplexobj(H32))
    return g * np.linalg.norm(np.abs(widen(H32)) @ np.abs(widen(np.asarray(V))), axis=0)


def ritz_margin(H32, Q):
    g = product_gamma(H32.shape[0], np.iscomplexobj(H32))
    aQ = np.abs(widen(np.asarray(Q)))
    return float(np.linalg.norm(g * (2 + g) * (aQ.T @ (np.abs(widen(H32)) @ aQ)), "fro"))


def resid_norms_exact(W32, V32, lam):
    """|| W_j - lambda_j V_j ||_2 in extended precision on the exactly widened fp32 entries"""
    ld = np.clongdouble if np.iscomplexobj(W32) else np.longdouble
    R = W32.astype(ld) - V32.astype(ld) * np.asarray(lam, dtype=np.longdouble)[None, :]
    return np.sqrt(np.sum(np.abs(R) ** 2, axis=0)).astype(np.float64)


def resid_norms_bound(W32, V32, lam):
    n = W32.shape[0] * (2 if np.iscomplexobj(W32) else 1)
    lam = np.abs(np.asarray(lam, dtype=np.float64))[None, :]
    parts = lambda A: (np.abs(A.real).astype(np.float64), np.abs(A.imag).astype(np.float64)) if np.iscomplexobj(A) \
        else (np.abs(A).astype(np.float64),)
    e2 = 0.0
    for w, v in zip(parts(W32), parts(V32)):
        e2 = e2 + np.sum((2 * U64 * (w + lam * v)) ** 2, axis=0)
    e = np.sqrt(e2)
    return e + (n + 3) * U64 * (_norm_upper(W32, V32, lam) + e)      # ||r|| <= || |w| + |lambda| |v| ||


def _norm_upper(W32, V32, lam):
    """an upper bound of ||r||_2 that does not depend on the signs: || |w| + |lambda| |v| ||_2"""
    return np.linalg.norm(np.abs(widen(W32)) + lam * np.abs(widen(V32)), axis=0)


@functools.lru_cache(maxsize=None)
def emulated(N, nev, nex, cplx):
    """One case solved by the fp64 oracle and by the emulation: counts, locked pairs, the emulation's own residuals and the
    largest fp64 residual of its wanted pairs against the fp32 matrix"""
    H32 = case_matrix(N, cplx)
    k64 = O.OracleCPU(widen(H32), nev, nex)
    for key, v in FLOAT_DEFAULTS.items():
        setattr(k64.config, key, v)
    s64 = O.solve(k64)
    k = OracleSp(H32, nev, nex)
    st = O.solve(k)
    lam = k.ritzv[:nev].copy()
    return dict(
        fp64=dict(iterations=s64["iterations"], filtered_vecs=s64["filtered_vecs"], locked=s64["locked"]),
        sp=dict(iterations=st["iterations"], filtered_vecs=st["filtered_vecs"], locked=st["locked"],
                hemm_sp_vecs=k.hemm_sp_vecs, own_resid=k.resid[:nev].copy(), ritzv=lam,
                max_resid=float(np.max(host_residuals(H32, lam, k.V1[:, :nev]))),
                h_restored=bool(np.array_equal(k.H, H32))))
