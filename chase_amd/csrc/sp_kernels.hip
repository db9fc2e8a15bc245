// sp_kernels.hip — the O(N n) kernels of the single-precision solver (chase_hip_sp_impl.hpp) and their C ABI (include/chase_hip.h).
//
// The fp64 kernels of vec_kernels.hip address 8-byte scalars; a real fp32 block has 4-byte elements, so copies, column swaps and
// transfers get twins here that address floats (a complex fp32 element is two of them).  Every kernel takes `mf` floats per column
// and leading dimensions in floats, moves 16 bytes per access where `vec` says that base pointers and leading dimensions allow
// (the rest of a column, or all of it, float by float), and touches nothing outside the m x n window.  New arithmetic:
//   shift_diag_sp   H_ii = fl32(d0_i + s) from the saved diagonal d0: the shifted diagonal never accumulates fp32 roundings, and
//                   s = 0 gives the saved bits back
//   resid_norms_sp  || W_j - lambda_j V_j ||_2 of fp32 columns: every term widened exactly, formed and summed in fp64, wave64
//                   shuffle reduction in a fixed order (bitwise reproducible)
// and, for the single-precision pseudo-Hermitian solver (chase_hip_sp_pseudo_impl.hpp), both exact by construction:
//   scale_rows_sp   X[row0:, :] *= s, one fp32 multiply per component (s = -1: the S flip, s = fl32(0.001): the start-vector damping)
//   kconj_sp        second half of the block = K-conjugate of the first: the two half-column copies and the conjugation in one pass
#include <hip/hip_runtime.h>
#include <cstdint>
#include "ctx.h"
#include "kernels.h"
#include "../../include/chase_hip.h"

using namespace chase_hip;

#define HIPCHK(x)                                                                                                      \
    do {                                                                                                               \
        hipError_t e_ = (x);                                                                                           \
        if (e_ != hipSuccess) return hip_fail(e_, #x);                                                                 \
    } while (0)
#define LAUNCHED(what)                                                                                                 \
    do {                                                                                                               \
        hipError_t e_ = hipGetLastError();                                                                             \
        if (e_ != hipSuccess) return hip_fail(e_, what);                                                               \
    } while (0)

namespace {

__device__ __forceinline__ double wave_sum(double v)
{
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// strided 2-D copy of float columns
__global__ __launch_bounds__(256) void copy2d_sp_kernel(const float* __restrict__ src, long lds_f, float* __restrict__ dst,
                                                        long ldd_f, long mf, int ncols, int vec)
{
    for (int j = blockIdx.y; j < ncols; j += gridDim.y) {
        const float* s = src + (long)j * lds_f;
        float* d = dst + (long)j * ldd_f;
        const long n4 = vec ? (mf >> 2) : 0;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256)
            ((float4*)d)[i] = ((const float4*)s)[i];
        for (long i = 4 * n4 + (long)blockIdx.x * 256 + threadIdx.x; i < mf; i += (long)gridDim.x * 256) d[i] = s[i];
    }
}

// dst[:, didx[c]] = src[:, sidx[c]], c < cnt (the two halves of a column permutation)
__global__ __launch_bounds__(256) void copy_cols_indexed_sp_kernel(const float* __restrict__ src, long lds_f, float* __restrict__ dst,
                                                                   long ldd_f, long mf, const int* __restrict__ sidx,
                                                                   const int* __restrict__ didx, int cnt, int vec)
{
    for (int c = blockIdx.y; c < cnt; c += gridDim.y) {
        const float* s = src + (long)sidx[c] * lds_f;
        float* d = dst + (long)didx[c] * ldd_f;
        const long n4 = vec ? (mf >> 2) : 0;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256)
            ((float4*)d)[i] = ((const float4*)s)[i];
        for (long i = 4 * n4 + (long)blockIdx.x * 256 + threadIdx.x; i < mf; i += (long)gridDim.x * 256) d[i] = s[i];
    }
}

__global__ __launch_bounds__(256) void swap_sp_kernel(float* __restrict__ a, float* __restrict__ b, long mf, int vec)
{
    const long n4 = vec ? (mf >> 2) : 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 t = ((float4*)a)[i];
        ((float4*)a)[i] = ((float4*)b)[i];
        ((float4*)b)[i] = t;
    }
    for (long i = 4 * n4 + (long)blockIdx.x * 256 + threadIdx.x; i < mf; i += (long)gridDim.x * 256) {
        const float t = a[i]; a[i] = b[i]; b[i] = t;
    }
}

// H[i,i] = fl32(d0[i] + s): real part from the saved entry and the accumulated shift (one rounding of the fp64 sum), the
// imaginary part of a complex entry as saved
__global__ void shift_diag_sp_kernel(float* __restrict__ H, long ldh, int n, int ept, const float* __restrict__ d0, double s)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float* h = H + ((long)i * ldh + i) * ept;
    h[0] = (float)((double)d0[(long)i * ept] + s);
    if (ept == 2) h[1] = d0[(long)i * ept + 1];
}

// out[j] = sqrt(sum_i (W[i,j] - lambda[j] V[i,j])^2) over the mf floats of column j, one block per column
__global__ __launch_bounds__(256) void resid_norms_sp_kernel(const float* __restrict__ W, long ldw_f, const float* __restrict__ V,
                                                             long ldv_f, const double* __restrict__ lambda, long mf,
                                                             double* __restrict__ out, int vec)
{
    __shared__ double sm[4];
    const int j = blockIdx.x;
    const float* w = W + (long)j * ldw_f;
    const float* v = V + (long)j * ldv_f;
    const double lam = lambda[j];
    double s = 0.0;
    const long n4 = vec ? (mf >> 2) : 0;
    for (long i = threadIdx.x; i < n4; i += 256) {
        const float4 a = ((const float4*)w)[i], b = ((const float4*)v)[i];
        const double r0 = (double)a.x - lam * (double)b.x, r1 = (double)a.y - lam * (double)b.y;
        const double r2 = (double)a.z - lam * (double)b.z, r3 = (double)a.w - lam * (double)b.w;
        s += r0 * r0; s += r1 * r1; s += r2 * r2; s += r3 * r3;
    }
    for (long i = 4 * n4 + threadIdx.x; i < mf; i += 256) {
        const double r = (double)w[i] - lam * (double)v[i];
        s += r * r;
    }
    s = wave_sum(s);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) sm[wv] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[j] = sqrt((sm[0] + sm[1]) + (sm[2] + sm[3]));
}

// X[i, j] *= s over the len floats of each column that start at p0 (the caller's row0): one fp32 multiply per float
__global__ __launch_bounds__(256) void scale_rows_sp_kernel(float* __restrict__ p0, long ldx_f, long len, int ncols, float s, int vec)
{
    for (int j = blockIdx.y; j < ncols; j += gridDim.y) {
        float* p = p0 + (long)j * ldx_f;
        const long n4 = vec ? (len >> 2) : 0;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
            float4 v = ((float4*)p)[i];
            v.x *= s; v.y *= s; v.z *= s; v.w *= s;
            ((float4*)p)[i] = v;
        }
        for (long i = 4 * n4 + (long)blockIdx.x * 256 + threadIdx.x; i < len; i += (long)gridDim.x * 256) p[i] *= s;
    }
}

// dst[hf + i] = conj(src[i]), dst[i] = conj(src[hf + i]) for the i < hf floats of each half column; CP: the odd floats are the
// imaginary parts (hf is even then) and change sign
template <bool CP>
__global__ __launch_bounds__(256) void kconj_sp_kernel(const float* __restrict__ src, long ldf_f, float* __restrict__ dst, long lds_f,
                                                       long hf, int ncols, int vec)
{
    for (int j = blockIdx.y; j < ncols; j += gridDim.y) {
        const float* s = src + (long)j * ldf_f;
        float* d = dst + (long)j * lds_f;
        const long n4 = vec ? (hf >> 2) : 0;                 // vec: hf is a multiple of 4, both halves start on 16 bytes
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
            float4 a = ((const float4*)s)[i], b = ((const float4*)(s + hf))[i];
            if (CP) { a.y = -a.y; a.w = -a.w; b.y = -b.y; b.w = -b.w; }
            ((float4*)(d + hf))[i] = a;
            ((float4*)d)[i] = b;
        }
        for (long i = 4 * n4 + (long)blockIdx.x * 256 + threadIdx.x; i < hf; i += (long)gridDim.x * 256) {
            const float a = s[i], b = s[hf + i];
            const bool im = CP && (i & 1);
            d[hf + i] = im ? -a : a;
            d[i] = im ? -b : b;
        }
    }
}

// Hermitian completion from the stored triangle: up != 0: A[i,j] = conj(A[j,i]) for i > j, else for i < j; the diagonal stays
__global__ __launch_bounds__(256) void complete_hermitian_sp_kernel(float* __restrict__ A, long lda, int n, int ept, int up)
{
    const int i = blockIdx.x * 16 + (threadIdx.x & 15), j = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (i >= n || j >= n || i == j) return;
    if (up ? (i < j) : (i > j)) return;               // (i, j) is in the stored triangle
    const float* s = A + ((long)i * lda + j) * ept;   // A[j, i]
    float* d = A + ((long)j * lda + i) * ept;         // A[i, j]
    d[0] = s[0];
    if (ept == 2) d[1] = -s[1];
}

inline unsigned cdiv(long a, long b) { return (unsigned)((a + b - 1) / b); }
inline dim3 grid2(long mf, int ncols)
{
    unsigned gx = cdiv(mf, 256 * 4); if (gx < 1) gx = 1; if (gx > 64) gx = 64;
    return dim3(gx, ncols > 1024 ? 1024u : (unsigned)ncols);
}
inline bool a16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int ept_of(int cplx) { return cplx ? 2 : 1; }

} // namespace

namespace chase_hip {

int copy2d_sp(hipStream_t st, const float* src, long ld_src_f, float* dst, long ld_dst_f, long mf, int ncols)
{
    if (mf <= 0 || ncols <= 0) return 0;
    const int vec = (ld_src_f & 3) == 0 && (ld_dst_f & 3) == 0 && a16(src) && a16(dst);
    hipLaunchKernelGGL(copy2d_sp_kernel, grid2(mf, ncols), dim3(256), 0, st, src, ld_src_f, dst, ld_dst_f, mf, ncols, vec);
    return (int)hipGetLastError();
}

int scale_rows_sp(hipStream_t st, float* X, long ldx_f, long row0_f, long mf, int ncols, float s)
{
    if (row0_f >= mf || ncols <= 0) return 0;
    float* p0 = X + row0_f;
    const int vec = (ldx_f & 3) == 0 && a16(p0);
    hipLaunchKernelGGL(scale_rows_sp_kernel, grid2(mf - row0_f, ncols), dim3(256), 0, st, p0, ldx_f, mf - row0_f, ncols, s, vec);
    return (int)hipGetLastError();
}

int kconj_sp(hipStream_t st, bool cplx, const float* first, long ldf_f, float* second, long lds_f, long hf, int ncols)
{
    if (hf <= 0 || ncols <= 0) return 0;
    const int vec = (ldf_f & 3) == 0 && (lds_f & 3) == 0 && (hf & 3) == 0 && a16(first) && a16(second);
    if (cplx) hipLaunchKernelGGL(kconj_sp_kernel<true>, grid2(hf, ncols), dim3(256), 0, st, first, ldf_f, second, lds_f, hf, ncols, vec);
    else      hipLaunchKernelGGL(kconj_sp_kernel<false>, grid2(hf, ncols), dim3(256), 0, st, first, ldf_f, second, lds_f, hf, ncols, vec);
    return (int)hipGetLastError();
}

} // namespace chase_hip

extern "C" {

int chase_hip_scale_rows_sp(chase_hip_ctx* c, int cplx, int m, int n, void* X, long ldx, int row0, float s)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "scale_rows_sp: NULL ctx");
    (void)hipSetDevice(c->device);
    if (c->oplog_on) c->oplog_add("scale_rows_sp", m, n, 0, 0);
    if (m < 0 || n < 0 || ldx < m || row0 < 0 || row0 > m) return set_error(CHASE_HIP_EINVAL, "scale_rows_sp: bad shape");
    if (m == 0 || n == 0 || row0 == m) return 0;
    if (!X) return set_error(CHASE_HIP_EINVAL, "scale_rows_sp: NULL matrix");
    const int e = ept_of(cplx);
    HIPCHK((hipError_t)scale_rows_sp(c->stream, (float*)X, ldx * e, (long)row0 * e, (long)m * e, n, s));
    return 0;
}

int chase_hip_kconj_sp(chase_hip_ctx* c, int cplx, int N, int n, const void* first, long ldf, void* second, long lds_)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "kconj_sp: NULL ctx");
    (void)hipSetDevice(c->device);
    if (c->oplog_on) c->oplog_add("kconj_sp", N, n, 0, 0);
    if (N < 0 || (N & 1) || n < 0 || ldf < N || lds_ < N) return set_error(CHASE_HIP_EINVAL, "kconj_sp: bad shape (N even, ld >= N)");
    if (N == 0 || n == 0) return 0;
    if (!first || !second) return set_error(CHASE_HIP_EINVAL, "kconj_sp: NULL matrix");
    const int e = ept_of(cplx);
    HIPCHK((hipError_t)kconj_sp(c->stream, cplx != 0, (const float*)first, ldf * e, (float*)second, lds_ * e, (long)(N / 2) * e, n));
    return 0;
}

int chase_hip_shift_diag_sp(chase_hip_ctx* c, int cplx, int n, void* H, long ldh, const void* d0, double shift)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "shift_diag_sp: NULL ctx");
    (void)hipSetDevice(c->device);
    if (c->oplog_on) c->oplog_add("shift_diag_sp", n, 0, 0, 0);
    if (n < 0 || ldh < n) return set_error(CHASE_HIP_EINVAL, "shift_diag_sp: bad shape");
    if (n == 0) return 0;
    if (!H || !d0) return set_error(CHASE_HIP_EINVAL, "shift_diag_sp: NULL argument");
    hipLaunchKernelGGL(shift_diag_sp_kernel, dim3(cdiv(n, 256)), dim3(256), 0, c->stream, (float*)H, ldh, n, ept_of(cplx),
                       (const float*)d0, shift);
    LAUNCHED("shift_diag_sp");
    return 0;
}

int chase_hip_resid_norms_sp(chase_hip_ctx* c, int cplx, int m, int n, const void* W, long ldw, const void* V, long ldv,
                             const double* lambda_host, double* resid_host)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "resid_norms_sp: NULL ctx");
    (void)hipSetDevice(c->device);
    if (c->oplog_on) c->oplog_add("resid_norms_sp", m, n, 0, 0);
    if (m < 0 || n < 0) return set_error(CHASE_HIP_EINVAL, "resid_norms_sp: negative extent");
    if (n == 0) return 0;
    if (ldw < m || ldv < m) return set_error(CHASE_HIP_EINVAL, "resid_norms_sp: leading dimension smaller than m");
    if (!lambda_host || !resid_host || (m > 0 && (!W || !V))) return set_error(CHASE_HIP_EINVAL, "resid_norms_sp: NULL argument");
    const int e = ept_of(cplx);
    int rc = c->ensure_buf(chase_hip_ctx::BUF_LAMBDA, (size_t)2 * n * sizeof(double));
    if (rc) return rc;
    double* dl = (double*)c->bufs[chase_hip_ctx::BUF_LAMBDA];
    double* dr = dl + n;
    HIPCHK(hipMemcpyAsync(dl, lambda_host, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const long ldw_f = ldw * e, ldv_f = ldv * e;
    const int vec = (ldw_f & 3) == 0 && (ldv_f & 3) == 0 && a16(W) && a16(V);
    hipLaunchKernelGGL(resid_norms_sp_kernel, dim3(n), dim3(256), 0, c->stream, (const float*)W, ldw_f, (const float*)V, ldv_f, dl,
                       (long)m * e, dr, vec);
    LAUNCHED("resid_norms_sp");
    HIPCHK(hipMemcpyAsync(resid_host, dr, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int chase_hip_lacpy_sp(chase_hip_ctx* c, int cplx, int m, int n, const void* A, long lda, void* B, long ldb)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "lacpy_sp: NULL ctx");
    (void)hipSetDevice(c->device);
    if (c->oplog_on) c->oplog_add("lacpy_sp", m, n, 0, 0);
    if (m < 0 || n < 0 || lda < m || ldb < m) return set_error(CHASE_HIP_EINVAL, "lacpy_sp: bad shape");
    if (m == 0 || n == 0) return 0;
    if (!A || !B) return set_error(CHASE_HIP_EINVAL, "lacpy_sp: NULL matrix");
    const int e = ept_of(cplx);
    const long lda_f = lda * e, ldb_f = ldb * e, mf = (long)m * e;
    const int vec = (lda_f & 3) == 0 && (ldb_f & 3) == 0 && a16(A) && a16(B);
    hipLaunchKernelGGL(copy2d_sp_kernel, grid2(mf, n), dim3(256), 0, c->stream, (const float*)A, lda_f, (float*)B, ldb_f, mf, n, vec);
    LAUNCHED("lacpy_sp");
    return 0;
}

int chase_hip_swap_cols_sp(chase_hip_ctx* c, int cplx, int m, void* V, long ldv, long i, long j)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "swap_cols_sp: NULL ctx");
    (void)hipSetDevice(c->device);
    if (c->oplog_on) c->oplog_add("swap_cols_sp", m, 0, 0, 0);
    if (m < 0 || ldv < m || i < 0 || j < 0) return set_error(CHASE_HIP_EINVAL, "swap_cols_sp: bad shape");
    if (m == 0 || i == j) return 0;
    if (!V) return set_error(CHASE_HIP_EINVAL, "swap_cols_sp: NULL matrix");
    const int e = ept_of(cplx);
    const long ld_f = ldv * e, mf = (long)m * e;
    float* a = (float*)V + i * ld_f;
    float* b = (float*)V + j * ld_f;
    const int vec = a16(a) && a16(b);
    hipLaunchKernelGGL(swap_sp_kernel, grid2(mf, 1), dim3(256), 0, c->stream, a, b, mf, vec);
    LAUNCHED("swap_cols_sp");
    return 0;
}

int chase_hip_permute_cols_sp(chase_hip_ctx* c, int cplx, int m, void* V, long ldv, void* scratch, long lds_, const int* src_host,
                              const int* dst_host, int cnt)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "permute_cols_sp: NULL ctx");
    (void)hipSetDevice(c->device);
    if (c->oplog_on) c->oplog_add("permute_cols_sp", m, cnt, 0, 0);
    if (m < 0 || cnt < 0 || ldv < m || lds_ < m) return set_error(CHASE_HIP_EINVAL, "permute_cols_sp: bad shape");
    if (m == 0 || cnt == 0) return 0;
    if (!V || !scratch || !src_host || !dst_host) return set_error(CHASE_HIP_EINVAL, "permute_cols_sp: NULL argument");
    for (int k = 0; k < cnt; ++k)
        if (src_host[k] < 0 || dst_host[k] < 0) return set_error(CHASE_HIP_EINVAL, "permute_cols_sp: negative column index");
    const int e = ept_of(cplx);
    int rc = c->ensure_buf(chase_hip_ctx::BUF_LAMBDA, (size_t)2 * cnt * sizeof(int) + 64);
    if (rc) return rc;
    int* ds = (int*)c->bufs[chase_hip_ctx::BUF_LAMBDA];
    int* dd = ds + cnt;
    HIPCHK(hipMemcpyAsync(ds, src_host, (size_t)cnt * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dd, dst_host, (size_t)cnt * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));          // the host index arrays may be reused right after we return
    const long ldv_f = ldv * e, lds_f = lds_ * e, mf = (long)m * e;
    const int vec = (ldv_f & 3) == 0 && (lds_f & 3) == 0 && a16(V) && a16(scratch);
    hipLaunchKernelGGL(copy_cols_indexed_sp_kernel, grid2(mf, cnt), dim3(256), 0, c->stream, (const float*)V, ldv_f, (float*)scratch,
                       lds_f, mf, ds, dd, cnt, vec);
    LAUNCHED("permute_cols_sp gather");
    hipLaunchKernelGGL(copy_cols_indexed_sp_kernel, grid2(mf, cnt), dim3(256), 0, c->stream, (const float*)scratch, lds_f, (float*)V,
                       ldv_f, mf, dd, dd, cnt, vec);
    LAUNCHED("permute_cols_sp scatter");
    return 0;
}

int chase_hip_upload_matrix_sp(chase_hip_ctx* c, int cplx, int m, int n, const void* host, long ldh, void* dev, long ldd)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "upload_matrix_sp: NULL ctx");
    (void)hipSetDevice(c->device);
    if (c->oplog_on) c->oplog_add("upload_matrix_sp", m, n, 0, 0);
    if (m < 0 || n < 0 || ldh < m || ldd < m) return set_error(CHASE_HIP_EINVAL, "upload_matrix_sp: bad shape");
    if (m == 0 || n == 0) return 0;
    if (!host || !dev) return set_error(CHASE_HIP_EINVAL, "upload_matrix_sp: NULL matrix");
    const size_t es = sizeof(float) * ept_of(cplx);
    HIPCHK(hipMemcpy2DAsync(dev, (size_t)ldd * es, host, (size_t)ldh * es, (size_t)m * es, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int chase_hip_download_matrix_sp(chase_hip_ctx* c, int cplx, int m, int n, const void* dev, long ldd, void* host, long ldh)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "download_matrix_sp: NULL ctx");
    (void)hipSetDevice(c->device);
    if (c->oplog_on) c->oplog_add("download_matrix_sp", m, n, 0, 0);
    if (m < 0 || n < 0 || ldh < m || ldd < m) return set_error(CHASE_HIP_EINVAL, "download_matrix_sp: bad shape");
    if (m == 0 || n == 0) return 0;
    if (!host || !dev) return set_error(CHASE_HIP_EINVAL, "download_matrix_sp: NULL matrix");
    const size_t es = sizeof(float) * ept_of(cplx);
    HIPCHK(hipMemcpy2DAsync(host, (size_t)ldh * es, dev, (size_t)ldd * es, (size_t)m * es, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int chase_hip_complete_hermitian_sp(chase_hip_ctx* c, int cplx, char uplo, int n, void* A, long lda)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "complete_hermitian_sp: NULL ctx");
    (void)hipSetDevice(c->device);
    if (c->oplog_on) c->oplog_add("complete_hermitian_sp", n, 0, 0, 0);
    const bool up = uplo == 'U' || uplo == 'u';
    if (!up && uplo != 'L' && uplo != 'l') return set_error(CHASE_HIP_EINVAL, "complete_hermitian_sp: uplo must be 'U' or 'L'");
    if (n < 0 || lda < n) return set_error(CHASE_HIP_EINVAL, "complete_hermitian_sp: bad shape");
    if (n == 0) return 0;
    if (!A) return set_error(CHASE_HIP_EINVAL, "complete_hermitian_sp: NULL matrix");
    hipLaunchKernelGGL(complete_hermitian_sp_kernel, dim3(cdiv(n, 16), cdiv(n, 16)), dim3(256), 0, c->stream, (float*)A, lda, n,
                       ept_of(cplx), up ? 1 : 0);
    LAUNCHED("complete_hermitian_sp");
    return 0;
}

} // extern "C"
