// gev_kernels.hip — the scalar cores of the reduction H x = lambda S x -> C y = lambda y with S = U^H U, C = U^{-H} H U^{-1}
// (capi_gev.hip): the LDS-resident two-sided reduction of one diagonal block, the triangle-only copies the blocked drivers
// need so that a strictly lower triangle is neither read nor written, and - for sequences and itype 2 / 3 - the MFMA diagonal
// step of the triangular product X <- op(U) X (trmm_diag) and the in-place conjugate transpose.
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
struct gcf { float x, y; };
__device__ __forceinline__ gcf g_conj(gcf a) { return gcf{a.x, -a.y}; }
__device__ __forceinline__ float g_conj(float a) { return a; }
__device__ __forceinline__ gcd g_scale(gcd a, double s) { return gcd{a.x * s, a.y * s}; }
__device__ __forceinline__ double g_scale(double a, double s) { return a * s; }
__device__ __forceinline__ double g_real(gcd a) { return a.x; }
__device__ __forceinline__ double g_real(double a) { return a; }
__device__ __forceinline__ gcd g_from_real(double r, gcd) { return gcd{r, 0.0}; }
__device__ __forceinline__ double g_from_real(double r, double) { return r; }
// c - a * b
__device__ __forceinline__ gcd g_nfma(gcd a, gcd b, gcd c) { return gcd{c.x - (a.x * b.x - a.y * b.y), c.y - (a.x * b.y + a.y * b.x)}; }
__device__ __forceinline__ double g_nfma(double a, double b, double c) { return c - a * b; }
// Element i of a matrix stored as S = double (the plain access) or S = float (the single-precision drivers of capi_gev.hip):
// widened on the way into LDS, rounded once on the way out; the arithmetic of hegs2_diag is fp64 for both.
template <class E, class S>
__device__ __forceinline__ E g_load(const S* p, long i)
{
    if constexpr (std::is_same<E, double>::value) return (double)p[i];
    else if constexpr (std::is_same<S, double>::value) return ((const gcd*)p)[i];
    else return gcd{(double)p[2 * i], (double)p[2 * i + 1]};
}
template <class S>
__device__ __forceinline__ void g_store(S* p, long i, double v) { p[i] = (S)v; }
template <class S>
__device__ __forceinline__ void g_store(S* p, long i, gcd v)
{
    if constexpr (std::is_same<S, double>::value) ((gcd*)p)[i] = v;
    else { p[2 * i] = (S)v.x; p[2 * i + 1] = (S)v.y; }
}
} // namespace

template <bool CPLX, class S>
__global__ __launch_bounds__(256) void hegs2_diag_kernel(S* __restrict__ A, long lda, const S* __restrict__ U, long ldu, int nb)
{
    using E = typename std::conditional<CPLX, gcd, double>::type;
    __shared__ E W[GNB * GNB];
    __shared__ E UT[GNB * GNB];
    __shared__ double dinv[GNB];
    const int tid = threadIdx.x;
    const int li = tid & 63, lj = tid >> 6;

    for (int j = lj; j < GNB; j += 4) {
        const int i = li;
        E a = g_zero(E{}), u = g_zero(E{});
        if (i < nb && j < nb) {
            if (i < j) { a = g_load<E>(A, (long)j * lda + i); u = g_load<E>(U, (long)j * ldu + i); }
            else if (i == j) { a = g_from_real(g_real(g_load<E>(A, (long)j * lda + i)), E{}); u = g_from_real(g_real(g_load<E>(U, (long)j * ldu + i)), E{}); }
            else a = g_conj(g_load<E>(A, (long)i * lda + j));
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
        if (i == j) g_store(A, (long)j * lda + i, g_from_real(g_real(v), E{}));
        else { g_store(A, (long)j * lda + i, v); g_store(A, (long)i * lda + j, g_conj(v)); }
    }
}

template <class S>
static int hegs2_diag_t(hipStream_t st, bool cplx, S* A, long lda, const S* U, long ldu, int nb)
{
    if (nb <= 0) return 0;
    if (nb > GNB) return (int)hipErrorInvalidValue;
    if (cplx) hipLaunchKernelGGL((hegs2_diag_kernel<true, S>), dim3(1), dim3(256), 0, st, A, lda, U, ldu, nb);
    else      hipLaunchKernelGGL((hegs2_diag_kernel<false, S>), dim3(1), dim3(256), 0, st, A, lda, U, ldu, nb);
    return (int)hipGetLastError();
}
int hegs2_diag(hipStream_t st, bool cplx, double* A, long lda, const double* U, long ldu, int nb) { return hegs2_diag_t(st, cplx, A, lda, U, ldu, nb); }
int hegs2_diag(hipStream_t st, bool cplx, float* A, long lda, const float* U, long ldu, int nb) { return hegs2_diag_t(st, cplx, A, lda, U, ldu, nb); }

// ---- trmm_diag: X_j <- op(U_jj) X_j for one 64-row step of chase_hip_trmm_left_upper ------------------------------------------------
// One 256-thread workgroup per 64-column tile of X; wave w owns the tile's columns 16 w ... 16 w + 15 and all four 16-row groups
// of the result, so the triangle's uneven work per row group is the same for every wave.  Both operands live in LDS on split
// planes (real, imaginary): the upper triangle of U_jj as stored - everything below the diagonal and beyond nb is BUILT as zeros,
// never read, and for op C the imaginary plane is negated while staging - and the X tile, rows beyond nb zero.  The product runs
// on v_mfma_f64_16x16x4_f64 with the roles swapped as in gemm_mfma_f64.hip (first operand the X fragment, second the U fragment),
// so that the accumulator's lanes run along the rows of the result and a 16-lane group stores 128 (complex 256) contiguous
// bytes.  k-blocks of 4 that lie wholly on the zero side of the diagonal of a 16-row group are skipped.  Complex: four real
// products, Re = Ur Xr - Ui Xi, Im = Ur Xi + Ui Xr.
//
// LDS layout: consecutive lanes on consecutive doubles everywhere.  Staging: lane i writes row i of a column (ds_write_b64, 16
// lanes = 32 banks).  Fragment reads are ds_read_b64 in two groups of 32 lanes = 16 values of the non-k index x 2 values of k
// on 64 banks, so the 32 doubles must fall on distinct double-slots mod 32:
//   X[k, col]       at k + 66 col  ->  2 col + k          (ld 66 = 2 mod 32)
//   op N: U[i, k]   at i + 80 k    ->  i + 16 k           (ld 80 = 16 mod 32)
//   op C: U[k, i]^* at k + 66 i    ->  2 i + k            (ld 66; the block is stored as it lies and read across)
// No operand is read at a stride that is a multiple of the bank width; the transposed copy hegs2_diag keeps is not needed.
namespace {
typedef double gd4 __attribute__((ext_vector_type(4)));
constexpr int TLX = 66;
}

template <bool CPLX, bool OPC>
__global__ __launch_bounds__(256) void trmm_diag_kernel(const double* __restrict__ U, long ldu, double* __restrict__ X, long ldx,
                                                        int nb, int ncols)
{
    constexpr int LU = OPC ? 66 : 80, NP = CPLX ? 2 : 1, EPT = CPLX ? 2 : 1;
    __shared__ double Us[NP * LU * GNB];
    __shared__ double Xs[NP * TLX * GNB];
    double* const Ui = Us + (CPLX ? LU * GNB : 0);
    double* const Xi = Xs + (CPLX ? TLX * GNB : 0);
    const int tid = threadIdx.x;
    const int li = tid & 63, lj = tid >> 6;
    const int c0 = blockIdx.x * GNB;
    const int cw = ncols - c0 < GNB ? ncols - c0 : GNB;

    for (int j = lj; j < GNB; j += 4) {
        double ur = 0.0, ui = 0.0, xr = 0.0, xi = 0.0;
        if (li <= j && j < nb) {
            const double* u = U + ((long)j * ldu + li) * EPT;
            ur = u[0];
            if (CPLX) ui = OPC ? -u[1] : u[1];
        }
        if (li < nb && j < cw) {
            const double* x = X + ((long)(c0 + j) * ldx + li) * EPT;
            xr = x[0];
            if (CPLX) xi = x[1];
        }
        Us[li + j * LU] = ur;
        Xs[li + j * TLX] = xr;
        if (CPLX) { Ui[li + j * LU] = ui; Xi[li + j * TLX] = xi; }
    }
    __syncthreads();

    const int w = tid >> 6, lr = tid & 15, lk = (tid & 63) >> 4;
    gd4 acc[4][NP];
    #pragma unroll
    for (int ib = 0; ib < 4; ++ib)
        #pragma unroll
        for (int p = 0; p < NP; ++p) acc[ib][p] = gd4{0.0, 0.0, 0.0, 0.0};
    const int kend = (nb + 3) >> 2;
    const int xo = TLX * (16 * w + lr);
    for (int k4 = 0; k4 < kend; ++k4) {
        const int k = 4 * k4 + lk;
        const double xr = Xs[k + xo];
        double xi = 0.0, nxi = 0.0;
        if (CPLX) { xi = Xi[k + xo]; nxi = -xi; }
        #pragma unroll
        for (int ib = 0; ib < 4; ++ib) {
            // rows 16 ib ... 16 ib + 15 of op(U): op N is zero for k < 16 ib, op C for k >= 16 (ib + 1); rows beyond nb are not stored
            const bool live = (16 * ib < nb) && (OPC ? k4 < 4 * (ib + 1) : k4 >= 4 * ib);
            if (!live) continue;
            const int uo = OPC ? k + LU * (16 * ib + lr) : (16 * ib + lr) + LU * k;
            const double ur = Us[uo];
            if (CPLX) {
                const double ui = Ui[uo];
                acc[ib][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(xr, ur, acc[ib][0], 0, 0, 0);
                acc[ib][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(nxi, ui, acc[ib][0], 0, 0, 0);
                acc[ib][NP - 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(xi, ur, acc[ib][NP - 1], 0, 0, 0);
                acc[ib][NP - 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(xr, ui, acc[ib][NP - 1], 0, 0, 0);
            } else {
                acc[ib][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(xr, ur, acc[ib][0], 0, 0, 0);
            }
        }
    }

    // accumulator register r of lane (lr, lk): row 16 ib + lr of the result, column 16 w + lk + 4 r of the tile.  Every read of
    // the tile happened before the barrier above, so the result goes over it in place.
    #pragma unroll
    for (int ib = 0; ib < 4; ++ib) {
        const int row = 16 * ib + lr;
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int col = 16 * w + lk + 4 * r;
            if (row < nb && col < cw) {
                double* x = X + ((long)(c0 + col) * ldx + row) * EPT;
                if (CPLX) { double2 v; v.x = acc[ib][0][r]; v.y = acc[ib][NP - 1][r]; *(double2*)x = v; }
                else x[0] = acc[ib][0][r];
            }
        }
    }
}

int trmm_diag(hipStream_t st, bool cplx, bool op_c, const double* U, long ldu, double* X, long ldx, int nb, int ncols)
{
    if (nb <= 0 || ncols <= 0) return 0;
    if (nb > GNB) return (int)hipErrorInvalidValue;
    const dim3 grid((ncols + GNB - 1) / GNB), block(256);
    if (cplx) {
        if (op_c) hipLaunchKernelGGL((trmm_diag_kernel<true, true>), grid, block, 0, st, U, ldu, X, ldx, nb, ncols);
        else      hipLaunchKernelGGL((trmm_diag_kernel<true, false>), grid, block, 0, st, U, ldu, X, ldx, nb, ncols);
    } else {
        if (op_c) hipLaunchKernelGGL((trmm_diag_kernel<false, true>), grid, block, 0, st, U, ldu, X, ldx, nb, ncols);
        else      hipLaunchKernelGGL((trmm_diag_kernel<false, false>), grid, block, 0, st, U, ldu, X, ldx, nb, ncols);
    }
    return (int)hipGetLastError();
}

// ---- trmm_diag_sp: the same step on fp32 data (chase_hip_trmm_left_upper_sp) -------------------------------------------------------
// The scheme of trmm_diag - one workgroup per 64 columns of X, wave w on columns 16 w ... 16 w + 15, triangle and tile on split
// planes in LDS, the zero side of the diagonal built and skipped, roles swapped - on v_mfma_f32_16x16x4_f32.  Its operands sit as
// the f64 form's do (lane l: non-k index l & 15, k = l >> 4), its accumulator does not: register r of lane l is row
// 4 (l >> 4) + r, column l & 15 of the MFMA's D.  With the roles swapped D is the transposed result tile, so lane (lr, lk) holds
// result row 16 ib + lr and the tile's columns 16 w + 4 lk + r: a 16-lane group still stores 64 (complex 128) contiguous bytes.
//
// LDS layout.  ds_read_b32 and ds_write_b32 work in two 32-lane halves on 32 banks of one dword: the 32 floats of a half - 16
// values of the non-k index x 2 consecutive k - must fall on 32 distinct dwords mod 32:
//   X[k, col]       at k + LX col    ->  LX lr + dk, dk in {0, 1}:  LX = 2 mod 32 gives 2 lr + dk, all of 0 ... 31
//   op N: U[i, k]   at i + LUN k     ->  lr + LUN dk:               LUN = 16 mod 32 gives lr + 16 dk
//   op C: U[k, i]^* at k + LUC i     ->  as X:                      LUC = 2 mod 32
// and every leading dimension is at least 64: the smallest are LX = LUC = 66 and LUN = 80.  (The f64 kernel's 66 / 80 answer
// another condition - 32 doubles on 32 distinct 8-byte slots of 64 banks - that happens to have the same residues.)  Staging:
// lane i writes row i of a column, 32 consecutive dwords per half.  48.7 KiB complex, 24.3 KiB real.
namespace {
typedef float gf4 __attribute__((ext_vector_type(4)));
constexpr int SLX = 66;
}

template <bool CPLX, bool OPC>
__global__ __launch_bounds__(256) void trmm_diag_sp_kernel(const float* __restrict__ U, long ldu, float* __restrict__ X, long ldx,
                                                           int nb, int ncols)
{
    constexpr int LU = OPC ? 66 : 80, NP = CPLX ? 2 : 1, EPT = CPLX ? 2 : 1;
    __shared__ float Us[NP * LU * GNB];
    __shared__ float Xs[NP * SLX * GNB];
    float* const Ui = Us + (CPLX ? LU * GNB : 0);
    float* const Xi = Xs + (CPLX ? SLX * GNB : 0);
    const int tid = threadIdx.x;
    const int li = tid & 63, lj = tid >> 6;
    const int c0 = blockIdx.x * GNB;
    const int cw = ncols - c0 < GNB ? ncols - c0 : GNB;

    for (int j = lj; j < GNB; j += 4) {
        float ur = 0.f, ui = 0.f, xr = 0.f, xi = 0.f;
        if (li <= j && j < nb) {
            const float* u = U + ((long)j * ldu + li) * EPT;
            ur = u[0];
            if (CPLX) ui = OPC ? -u[1] : u[1];
        }
        if (li < nb && j < cw) {
            const float* x = X + ((long)(c0 + j) * ldx + li) * EPT;
            xr = x[0];
            if (CPLX) xi = x[1];
        }
        Us[li + j * LU] = ur;
        Xs[li + j * SLX] = xr;
        if (CPLX) { Ui[li + j * LU] = ui; Xi[li + j * SLX] = xi; }
    }
    __syncthreads();

    const int w = tid >> 6, lr = tid & 15, lk = (tid & 63) >> 4;
    gf4 acc[4][NP];
    #pragma unroll
    for (int ib = 0; ib < 4; ++ib)
        #pragma unroll
        for (int p = 0; p < NP; ++p) acc[ib][p] = gf4{0.f, 0.f, 0.f, 0.f};
    const int kend = (nb + 3) >> 2;
    const int xo = SLX * (16 * w + lr);
    for (int k4 = 0; k4 < kend; ++k4) {
        const int k = 4 * k4 + lk;
        const float xr = Xs[k + xo];
        float xi = 0.f, nxi = 0.f;
        if (CPLX) { xi = Xi[k + xo]; nxi = -xi; }
        #pragma unroll
        for (int ib = 0; ib < 4; ++ib) {
            // rows 16 ib ... 16 ib + 15 of op(U): op N is zero for k < 16 ib, op C for k >= 16 (ib + 1); rows beyond nb are not stored
            const bool live = (16 * ib < nb) && (OPC ? k4 < 4 * (ib + 1) : k4 >= 4 * ib);
            if (!live) continue;
            const int uo = OPC ? k + LU * (16 * ib + lr) : (16 * ib + lr) + LU * k;
            const float ur = Us[uo];
            if (CPLX) {
                const float ui = Ui[uo];
                acc[ib][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(xr, ur, acc[ib][0], 0, 0, 0);
                acc[ib][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(nxi, ui, acc[ib][0], 0, 0, 0);
                acc[ib][NP - 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(xi, ur, acc[ib][NP - 1], 0, 0, 0);
                acc[ib][NP - 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(xr, ui, acc[ib][NP - 1], 0, 0, 0);
            } else {
                acc[ib][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(xr, ur, acc[ib][0], 0, 0, 0);
            }
        }
    }

    // accumulator register r of lane (lr, lk): row 16 ib + lr of the result, column 16 w + 4 lk + r of the tile (the f32 C/D map).
    // Every read of the tile happened before the barrier above, so the result goes over it in place.
    #pragma unroll
    for (int ib = 0; ib < 4; ++ib) {
        const int row = 16 * ib + lr;
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int col = 16 * w + 4 * lk + r;
            if (row < nb && col < cw) {
                float* x = X + ((long)(c0 + col) * ldx + row) * EPT;
                if (CPLX) { float2 v; v.x = acc[ib][0][r]; v.y = acc[ib][NP - 1][r]; *(float2*)x = v; }
                else x[0] = acc[ib][0][r];
            }
        }
    }
}

int trmm_diag_sp(hipStream_t st, bool cplx, bool op_c, const float* U, long ldu, float* X, long ldx, int nb, int ncols)
{
    if (nb <= 0 || ncols <= 0) return 0;
    if (nb > GNB) return (int)hipErrorInvalidValue;
    const dim3 grid((ncols + GNB - 1) / GNB), block(256);
    if (cplx) {
        if (op_c) hipLaunchKernelGGL((trmm_diag_sp_kernel<true, true>), grid, block, 0, st, U, ldu, X, ldx, nb, ncols);
        else      hipLaunchKernelGGL((trmm_diag_sp_kernel<true, false>), grid, block, 0, st, U, ldu, X, ldx, nb, ncols);
    } else {
        if (op_c) hipLaunchKernelGGL((trmm_diag_sp_kernel<false, true>), grid, block, 0, st, U, ldu, X, ldx, nb, ncols);
        else      hipLaunchKernelGGL((trmm_diag_sp_kernel<false, false>), grid, block, 0, st, U, ldu, X, ldx, nb, ncols);
    }
    return (int)hipGetLastError();
}

// A <- A^H in place (n x n): one workgroup per pair of 32 x 32 tiles (bi <= bj), both staged in LDS (ld 33) and written to each
// other's place conjugated, so reads and writes both run down columns.
template <class E>
__global__ __launch_bounds__(256) void conj_transpose_kernel(E* __restrict__ Ag, long lda, int n)
{
    constexpr int T = 32, LT = T + 1;
    __shared__ E t1[T * LT];
    __shared__ E t2[T * LT];
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bi > bj) return;
    const int r0 = bi * T, c0 = bj * T;
    const int li = threadIdx.x & 31, lj = threadIdx.x >> 5;
    for (int j = lj; j < T; j += 8) {
        if (r0 + li < n && c0 + j < n) t1[li + j * LT] = Ag[(long)(c0 + j) * lda + r0 + li];              // t1[a, b] = A[r0 + a, c0 + b]
        if (bi != bj && c0 + li < n && r0 + j < n) t2[li + j * LT] = Ag[(long)(r0 + j) * lda + c0 + li];  // t2[a, b] = A[c0 + a, r0 + b]
    }
    __syncthreads();
    for (int j = lj; j < T; j += 8) {
        if (r0 + li < n && c0 + j < n) Ag[(long)(c0 + j) * lda + r0 + li] = g_conj(bi == bj ? t1[j + li * LT] : t2[j + li * LT]);
        if (bi != bj && c0 + li < n && r0 + j < n) Ag[(long)(r0 + j) * lda + c0 + li] = g_conj(t1[j + li * LT]);
    }
}

int conj_transpose_inplace(hipStream_t st, bool cplx, double* A, long lda, int n)
{
    if (n <= 0) return 0;
    const int nt = (n + 31) / 32;
    if (cplx) hipLaunchKernelGGL(conj_transpose_kernel<gcd>, dim3(nt, nt), dim3(256), 0, st, (gcd*)A, lda, n);
    else      hipLaunchKernelGGL(conj_transpose_kernel<double>, dim3(nt, nt), dim3(256), 0, st, A, lda, n);
    return (int)hipGetLastError();
}

int conj_transpose_inplace(hipStream_t st, bool cplx, float* A, long lda, int n)
{
    if (n <= 0) return 0;
    const int nt = (n + 31) / 32;
    if (cplx) hipLaunchKernelGGL(conj_transpose_kernel<gcf>, dim3(nt, nt), dim3(256), 0, st, (gcf*)A, lda, n);
    else      hipLaunchKernelGGL(conj_transpose_kernel<float>, dim3(nt, nt), dim3(256), 0, st, A, lda, n);
    return (int)hipGetLastError();
}

// dst[i, j] (+)= src[i, j] for i <= j < n, ept scalars (double or float) per element; nothing below the diagonal is read or
// written.  One workgroup per column.
template <bool ADD, class T>
__global__ __launch_bounds__(256) void upper_copy_kernel(const T* __restrict__ src, long lds_, T* __restrict__ dst,
                                                         long ldd, int n, int ept)
{
    const int j = blockIdx.x;
    const T* s = src + (long)j * lds_ * ept;
    T* d = dst + (long)j * ldd * ept;
    const int cnt = (j + 1) * ept;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        if constexpr (ADD) d[i] += s[i]; else d[i] = s[i];
    }
}

int copy_upper(hipStream_t st, const double* src, long ld_src, double* dst, long ld_dst, int n, int ept)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL((upper_copy_kernel<false, double>), dim3(n), dim3(256), 0, st, src, ld_src, dst, ld_dst, n, ept);
    return (int)hipGetLastError();
}

int add_upper(hipStream_t st, const double* src, long ld_src, double* dst, long ld_dst, int n, int ept)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL((upper_copy_kernel<true, double>), dim3(n), dim3(256), 0, st, src, ld_src, dst, ld_dst, n, ept);
    return (int)hipGetLastError();
}

int add_upper(hipStream_t st, const float* src, long ld_src, float* dst, long ld_dst, int n, int ept)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL((upper_copy_kernel<true, float>), dim3(n), dim3(256), 0, st, src, ld_src, dst, ld_dst, n, ept);
    return (int)hipGetLastError();
}

} // namespace chase_hip
