"""CPU references of the pseudo-Hermitian solver's opt-in fp32 H^2 filter (h2_mixed_precision).

* axpy_sp: Y += gamma X in fp32 / complex fp32 evaluated component by component in numpy, and the componentwise bound that
  holds for ANY evaluation order with or without fused multiply-add, u = 2^-24:
      real        |err| <= 2u / (1 - 2u) (|gamma| |x| + |y|)                          (a product and a sum: two roundings at most)
      complex re  |err| <= 3u / (1 - 3u) (|g_r x_r| + |g_i x_i| + |y_r|)              (two products and two sums: every term
      complex im  |err| <= 3u / (1 - 3u) (|g_r x_i| + |g_i x_r| + |y_i|)               passes through three roundings at most)
* OraclePseudoMixed: the emulation the switch was designed on, a subclass of the oracle's OraclePseudoCPU.  A filter call that
  starts while the smallest residual of the unlocked wanted pairs is above 1e-3 rounds H (once) and the unlocked first-half
  columns to fp32, runs its H^2 steps in fp32 and widens the result when the call ends.  oracle/ is untouched: solve_pseudo()
  below brackets the oracle's filter_H2 for the duration of one solve.
* emulated(): both reference fixtures solved in fp64 and mixed, once per process; the iteration and filtered-vector counts the
  GPU tests compare against.
"""
import functools
import os

import numpy as np
from oracle import chase_oracle as O

U = 2.0 ** -24
THRESHOLD = 1e-3
FIXTURES = {"complex": ("cdouble_random_BSE.bin", True), "real": ("double_random_BSE.bin", False)}
N_FIXTURE = 200
CASES = [("complex", 20, 20), ("complex", 12, 8), ("real", 20, 20), ("real", 12, 8)]


# ---- axpy_sp -----------------------------------------------------------------------------------------------------------

def axpy_sp_ref(gamma, X, Y):
    """Y + gamma X in the arithmetic of the operands (float32 or complex64), products first, then the sums left to right"""
    if np.iscomplexobj(X):
        g = np.complex64(gamma)
        gr, gi = np.float32(g.real), np.float32(g.imag)
        xr, xi, yr, yi = (np.ascontiguousarray(a, dtype=np.float32) for a in (X.real, X.imag, Y.real, Y.imag))
        re = yr + (gr * xr - gi * xi)
        im = yi + (gr * xi + gi * xr)
        assert re.dtype == np.float32 and im.dtype == np.float32
        return (re + 1j * im).astype(np.complex64)
    out = Y + np.float32(gamma) * X
    assert out.dtype == np.float32
    return out


def axpy_sp_exact(gamma, X, Y):
    """The same update in fp64 on the fp32 operands (products of two floats are exact there; the sums err by 2^-53 relative,
    2^-28 of the bounds below)"""
    if np.iscomplexobj(X):
        return Y.astype(np.complex128) + np.complex128(np.complex64(gamma)) * X.astype(np.complex128)
    return Y.astype(np.float64) + np.float64(np.float32(gamma)) * X.astype(np.float64)


def axpy_sp_bound(gamma, X, Y):
    """Componentwise bound of |computed - exact|: one array (real) or the pair (real part, imaginary part)"""
    if np.iscomplexobj(X):
        g = np.complex128(np.complex64(gamma))
        gr, gi = abs(g.real), abs(g.imag)
        xr, xi = np.abs(X.real).astype(np.float64), np.abs(X.imag).astype(np.float64)
        yr, yi = np.abs(Y.real).astype(np.float64), np.abs(Y.imag).astype(np.float64)
        f = 3 * U / (1 - 3 * U)
        return f * (gr * xr + gi * xi + yr), f * (gr * xi + gi * xr + yi)
    g = abs(np.float64(np.float32(gamma)))
    return 2 * U / (1 - 2 * U) * (g * np.abs(X).astype(np.float64) + np.abs(Y).astype(np.float64))


def axpy_sp_within_bound(gamma, X, Y, got):
    """max over the components of |got - exact| / bound (0 / 0 counts as 0): <= 1 means within the bound"""
    err = got.astype(np.complex128 if np.iscomplexobj(X) else np.float64) - axpy_sp_exact(gamma, X, Y)
    b = axpy_sp_bound(gamma, X, Y)
    pairs = [(np.abs(err.real), b[0]), (np.abs(err.imag), b[1])] if np.iscomplexobj(X) else [(np.abs(err), b)]
    worst = 0.0
    for e, bound in pairs:
        assert np.all(e[bound == 0] == 0)
        nz = bound > 0
        if np.any(nz):
            worst = max(worst, float(np.max(e[nz] / bound[nz])))
    return worst


# ---- the emulation -----------------------------------------------------------------------------------------------------

class OraclePseudoMixed(O.OraclePseudoCPU):
    """OraclePseudoCPU with the fp32 H^2 filter of ChaseHipPseudo: decision at FilterPhaseStart, fp32 steps on shadows of the
    unlocked first-half columns [locked, nev + nex), the result widened at FilterPhaseEnd"""

    def __init__(self, H, nev, nex, mixed=True):
        super().__init__(H, nev, nex)
        self.mixed = mixed
        self.Hs = None
        self.sp_active = self.sp_synced = False
        self.S1 = self.S2 = None
        self.hemm_calls = self.hemm_sp_calls = self.hemm_sp_vecs = self.sp_filters = self.sp_h_converts = 0

    def FilterPhaseStart(self):
        L = self.locked
        if self.mixed and L < self.nev and np.min(self.resid[L:self.nev]) > THRESHOLD:
            if self.Hs is None:
                self.Hs = self.H.astype(np.complex64)
                self.sp_h_converts += 1
            self.sp_active, self.sp_synced = True, False

    def FilterPhaseEnd(self):
        if self.sp_active and self.sp_synced:
            sl = slice(self.locked, self.nevex)
            self.V1[:, sl] = self.S1[:, sl].astype(np.complex128)
        self.sp_active = self.sp_synced = False

    def HEMM_H2(self, block, alpha, beta, gamma, offset_left, offset_right=0):
        ncols = block - offset_right if offset_right < block else 0
        c0 = offset_left + self.locked
        if not self.sp_active:
            if ncols and c0 < self.nevex:
                self.hemm_calls += 2
            return super().HEMM_H2(block, alpha, beta, gamma, offset_left, offset_right)
        if ncols and c0 < self.nevex:
            sl = slice(c0, min(c0 + ncols, self.nevex))
            if not self.sp_synced:
                un = slice(self.locked, self.nevex)
                self.S1 = np.zeros((self.N, self.nevex), dtype=np.complex64, order="F")
                self.S2 = np.zeros_like(self.S1)
                self.S1[:, un] = self.V1[:, un].astype(np.complex64)
                self.S2[:, un] = self.V2[:, un].astype(np.complex64)
                self.sp_synced = True
                self.sp_filters += 1
            a, b, g = np.complex64(alpha), np.complex64(beta), np.complex64(gamma)
            tmp = self.Hs @ self.S1[:, sl]
            out = a * (self.Hs @ tmp)
            if b != 0:
                out = out + b * self.S2[:, sl]
            out = out + g * self.S1[:, sl]
            assert out.dtype == np.complex64
            self.S2[:, sl] = out
            self.hemm_sp_calls += 2
            self.hemm_sp_vecs += 2 * (sl.stop - sl.start)
        self.V1, self.V2 = self.V2, self.V1
        self.S1, self.S2 = self.S2, self.S1


def solve_pseudo(k, trace=None):
    """oracle.solve_pseudo with the filter call bracketed by k.FilterPhaseStart() / k.FilterPhaseEnd(), as the HIP driver does"""
    inner = O.filter_H2

    def bracketed(kk, *args):
        kk.FilterPhaseStart()
        try:
            return inner(kk, *args)
        finally:
            kk.FilterPhaseEnd()
    O.filter_H2 = bracketed
    try:
        return O.solve_pseudo(k, trace)
    finally:
        O.filter_H2 = inner


def fixture(kind):
    """(H, smallest-first positive half of the dense spectrum) of a reference BSE fixture"""
    from conftest import read_ref_matrix
    name, cplx = FIXTURES[kind]
    H = read_ref_matrix(name, N_FIXTURE, N_FIXTURE, cplx)
    ev = np.linalg.eigvals(H).real
    return H, np.sort(ev[ev > 0])


@functools.lru_cache(maxsize=None)
def emulated(kind, nev, nex):
    """One fixture solved by the oracle in fp64 and by the emulation (numLanczos 10, lanczosIter 50, tol 1e-10): the counts and
    the accuracy of the mixed solve"""
    H, pos = fixture(kind)
    Hc = np.asfortranarray(H.astype(np.complex128))
    out = {}
    for mixed in (False, True):
        k = OraclePseudoMixed(Hc, nev, nex, mixed=mixed)
        k.config.num_lanczos, k.config.lanczos_iter, k.config.tol = 10, 50, 1e-10
        st = solve_pseudo(k)
        lam = k.ritzv[:nev].copy()
        V = k.V1[:, :nev]
        out["mixed" if mixed else "fp64"] = dict(
            iterations=st["iterations"], filtered_vecs=st["filtered_vecs"], locked=st["locked"],
            hemm_calls=k.hemm_calls, hemm_sp_calls=k.hemm_sp_calls, sp_filters=k.sp_filters, sp_h_converts=k.sp_h_converts,
            max_resid=float(np.max(np.linalg.norm(Hc @ V - V * lam[None, :], axis=0))),
            eig_err=float(np.max(np.abs(np.sort(lam) - pos[:nev]))))
    return out
