// gev_kernels.hip — the scalar cores of the reduction H x = lambda S x -> C y = lambda y with S = U^H U, C = U^{-H} H U^{-1}
// (capi_gev.hip): the LDS-resident two-sided reduction of one diagonal block and the triangle-only copies the blocked
// drivers need so that a strictly lower triangle is neither read nor written.
//
// Reference call site replaced: the p?hegst of docs/example/gev.rst (LAPACK xHEGS2, itype = 1, uplo = 'U', for one block).
//
// hegs2_diag: one 256-thread workgroup, one nb x nb block (nb <= 64).  Two tiles live in LDS (128 KiB complex, 64 KiB real):
//   W, column-major with ld = 64, starts as the full Hermitian A_jj rebuilt from its upper triangle (the diagonal's imaginary
//     parts are ignored, as LAPACK does);
//   UT, the TRANSPOSE of the upper triangle of U_jj: UT[c + 64 r] = U[r, c].
// Step 1 solves U^H W' = W by rows (forward substitution, right-looking), step 2 solves C U = W' by columns.  In both the
// thread (i = tid & 63, j) walks a column of W with consecutive lanes on consecutive rows - 16 B (8 B real) apart, every
// bank row used once - and W[k, j] / U[k, j] are wave-uniform broadcasts.  The one strided operand would be the row
// U[k, k+1 : nb] of step 1, 64 elements 1 KiB apart in a column-major tile, all on one bank; stored transposed it is contiguous.
// The upper triangle of the result is written back together with its conjugate below the diagonal, and the diagonal with an
// imaginary part of +0: the block is Hermitian bit for bit, which two products with an inverted block would not give.

#include <hip/hip_runtime.h>
#include <type_traits>
#include "kernels.h"

namespace chase_hip {

namespace {
constexpr int GNB = 64;
struct gcd { double x, y; };
__device__ __forceinline__ gcd g_zero(gcd) { return gcd{0.0, 0.0}; }
__device__ __forceinline__ double g_zero(double) { return 0.0; }
__device__ __forceinline__ gcd g_conj(gcd a) { return gcd{a.x, -a.y}; }
__device__ __forceinline__ double g_conj(double a) { return a; }
__device__ __forceinline__ gcd g_scale(gcd a, double s) { return gcd{a.x * s, a.y * s}; }
__device__ __forceinline__ double g_scale(double a, double s) { return a * s; }
__device__ __forceinline__ double g_real(gcd a) { return a.x; }
__device__ __forceinline__ double g_real(double a) { return a; }
__device__ __forceinline__ gcd g_from_real(double r, gcd) { return gcd{r, 0.0}; }
__device__ __forceinline__ double g_from_real(double r, double) { return r; }
// c - a * b
__device__ __forceinline__ gcd g_nfma(gcd a, gcd b, gcd c) { return gcd{c.x - (a.x * b.x - a.y * b.y), c.y - (a.x * b.y + a.y * b.x)}; }
__device__ __forceinline__ double g_nfma(double a, double b, double c) { return c - a * b; }
} // namespace

template <bool CPLX>
__global__ __launch_bounds__(256) void hegs2_diag_kernel(double* __restrict__ A, long lda, const double* __restrict__ U, long ldu,
                                                         int nb)
{
    using E = typename std::conditional<CPLX, gcd, double>::type;
    __shared__ E W[GNB * GNB];
    __shared__ E UT[GNB * GNB];
    __shared__ double dinv[GNB];
    const int tid = threadIdx.x;
    const int li = tid & 63, lj = tid >> 6;
    E* Ag = (E*)A;
    const E* Ug = (const E*)U;

    for (int j = lj; j < GNB; j += 4) {
        const int i = li;
        E a = g_zero(E{}), u = g_zero(E{});
        if (i < nb && j < nb) {
            if (i < j) { a = Ag[(long)j * lda + i]; u = Ug[(long)j * ldu + i]; }
            else if (i == j) { a = g_from_real(g_real(Ag[(long)j * lda + i]), E{}); u = g_from_real(g_real(Ug[(long)j * ldu + i]), E{}); }
            else a = g_conj(Ag[(long)i * lda + j]);
        }
        W[i + j * GNB] = a;
        UT[j + i * GNB] = u;                                   // U[i, j] at UT[j + 64 i]
    }
    __syncthreads();
    if (tid < GNB) dinv[tid] = (tid < nb) ? 1.0 / g_real(UT[tid + tid * GNB]) : 0.0;
    __syncthreads();

    // ---- step 1: W <- U^{-H} W.  Row k is final after its scaling; rows i > k lose conj(U[k, i]) W[k, :] ----
    for (int k = 0; k < nb; ++k) {
        if (tid < nb) W[k + tid * GNB] = g_scale(W[k + tid * GNB], dinv[k]);
        __syncthreads();
        if (li > k && li < nb) {
            const E uki = g_conj(UT[li + k * GNB]);
            for (int j = lj; j < nb; j += 4) W[li + j * GNB] = g_nfma(uki, W[k + j * GNB], W[li + j * GNB]);
        }
        __syncthreads();
    }

    // ---- step 2: W <- W U^{-1}.  Column k is final after its scaling; columns j > k lose W[:, k] U[k, j] ----
    for (int k = 0; k < nb; ++k) {
        if (tid < nb) W[tid + k * GNB] = g_scale(W[tid + k * GNB], dinv[k]);
        __syncthreads();
        if (li < nb) {
            const E wik = W[li + k * GNB];
            for (int j = k + 1 + lj; j < nb; j += 4) W[li + j * GNB] = g_nfma(wik, UT[j + k * GNB], W[li + j * GNB]);
        }
        __syncthreads();
    }

    // ---- write back: upper triangle, its conjugate below, a real diagonal ----
    for (int j = lj; j < nb; j += 4) {
        const int i = li;
        if (i > j) continue;
        E v = W[i + j * GNB];
        if (i == j) Ag[(long)j * lda + i] = g_from_real(g_real(v), E{});
        else { Ag[(long)j * lda + i] = v; Ag[(long)i * lda + j] = g_conj(v); }
    }
}

int hegs2_diag(hipStream_t st, bool cplx, double* A, long lda, const double* U, long ldu, int nb)
{
    if (nb <= 0) return 0;
    if (nb > GNB) return (int)hipErrorInvalidValue;
    if (cplx) hipLaunchKernelGGL(hegs2_diag_kernel<true>, dim3(1), dim3(256), 0, st, A, lda, U, ldu, nb);
    else      hipLaunchKernelGGL(hegs2_diag_kernel<false>, dim3(1), dim3(256), 0, st, A, lda, U, ldu, nb);
    return (int)hipGetLastError();
}

// dst[i, j] (+)= src[i, j] for i <= j < n, ept doubles per element; nothing below the diagonal is read or written.
// One workgroup per column.
template <bool ADD>
__global__ __launch_bounds__(256) void upper_copy_kernel(const double* __restrict__ src, long lds_, double* __restrict__ dst,
                                                         long ldd, int n, int ept)
{
    const int j = blockIdx.x;
    const double* s = src + (long)j * lds_ * ept;
    double* d = dst + (long)j * ldd * ept;
    const int cnt = (j + 1) * ept;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        if constexpr (ADD) d[i] += s[i]; else d[i] = s[i];
    }
}

int copy_upper(hipStream_t st, const double* src, long ld_src, double* dst, long ld_dst, int n, int ept)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(upper_copy_kernel<false>, dim3(n), dim3(256), 0, st, src, ld_src, dst, ld_dst, n, ept);
    return (int)hipGetLastError();
}

int add_upper(hipStream_t st, const double* src, long ld_src, double* dst, long ld_dst, int n, int ept)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(upper_copy_kernel<true>, dim3(n), dim3(256), 0, st, src, ld_src, dst, ld_dst, n, ept);
    return (int)hipGetLastError();
}

} // namespace chase_hip
