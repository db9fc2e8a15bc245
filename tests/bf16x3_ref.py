"""numpy emulation of the bf16x3 operand split (chase_amd/csrc/gemm_mfma_bf16x3.hip) and the error bound of the split product,
shared by tests/test_sp_bf16x3_cpu.py and the GPU tests.

Split: x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2), round to nearest even, the subtractions in fp32.  bf16 has 8
significant bits and the exponent range of fp32, so |x - x1| <= 2^-8 |x| is a multiple of ulp24(x) with at most 16 bits,
|x - x1 - x2| <= 2^-16 |x| one with at most 8 bits: x3 is exact and x = x1 + x2 + x3 (for |x| >= 2^-110: bf16 subnormals end at
2^-133).  The product keeps the six a_i b_j with i + j <= 4; the dropped a2 b3 + a3 b2 + a3 b3 are below
(2 * 2^-24 + 2^-32) |a||b| in the worst case and far below that on data without structure (random signs).

Bound of the device product against the fp64 one, u = 2^-24: six exact partial products per k enter ONE fp32 accumulation of at
most 6k additions, each erring by at most u (relative to the partial sums, which |A||B| bounds); the dropped terms and the
scalars add a handful more: g = (6k + 16) u for real, (12k + 32) u for complex operands (four real products, moduli)."""
import numpy as np

U = 2.0 ** -24
V64 = 2.0 ** -53


def bf16_rne(x):
    """fp32 array -> the nearest bf16 (ties to even), returned as fp32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def split3(x):
    """the three bf16 parts of an fp32 array, as fp32 arrays"""
    x = np.asarray(x, dtype=np.float32)
    a1 = bf16_rne(x)
    r1 = (x - a1).astype(np.float32)
    a2 = bf16_rne(r1)
    r2 = (r1 - a2).astype(np.float32)
    a3 = bf16_rne(r2)
    return a1, a2, a3


def dropped_terms(A, B):
    """sum over k of a2 b3 + a3 b2 + a3 b3 for real fp32 A (m x k), B (k x n), in fp64 (every product is exact there)"""
    (_, a2, a3), (_, b2, b3) = [tuple(p.astype(np.float64) for p in split3(X)) for X in (A, B)]
    return a2 @ b3 + a3 @ b2 + a3 @ b3


def gamma(k, cplx):
    return ((12 * k + 32) if cplx else (6 * k + 16)) * U


def product_bound(k, cplx, alpha, absAB, beta=0, absC0=None, wide=False):
    """g (|alpha| |A||B| + |beta| |C0|); the wide form (fp64 C, alpha, beta) adds 8 * 2^-53 for its epilogue"""
    g = gamma(k, cplx) + (8 * V64 if wide else 0.0)
    b = abs(alpha) * absAB
    if beta != 0:
        b = b + abs(beta) * absC0
    return g * b
