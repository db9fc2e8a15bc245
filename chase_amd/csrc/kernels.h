// kernels.h — internal C++ declarations of the HIP kernel launchers (not part of the C ABI; see include/chase_hip.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

struct chase_hip_gemm_launch;     // include/chase_hip.h

namespace chase_hip {

// C = alpha*op(A)*B + beta*C, column-major, device pointers. cplx: elements are interleaved (re,im) doubles.
// lda/ldb/ldc in elements. alpha/beta point to 1 (real) or 2 (complex) host doubles.
// ws/ws_bytes: optional device workspace for deterministic split-K.
// tag: 1 = Chebyshev-filter product (own kernel symbol; complex products may take the three-multiplication scheme),
// 2 = H-times-block product outside the filter, 0 = everything else.  device: ordinal the stream lives on (per-device
// kernel attributes).  exec_flops (optional): += the flops the matrix cores execute for this product.  min_rounds > 0: the
// launch shares the chip with a collective - products with fewer tiles than min_rounds per workgroup slot are cut along K.
int gemm_f64(hipStream_t st, bool cplx, char opA, int m, int n, int k, const double* alpha, const double* A, long lda,
             const double* B, long ldb, const double* beta, double* C, long ldc, double* ws, size_t ws_bytes,
             int num_cu, int tag = 0, int device = 0, double* exec_flops = nullptr, int min_rounds = 0);
constexpr size_t GEMM_WS_CAP = (size_t)640 << 20;         // upper bound of the split-K workspace
size_t gemm_f64_ws_need(bool cplx, char opA, int m, int n, int k, int num_cu, int min_rounds = 0);
// gemm_f64's status when the caller's split-K workspace is smaller than gemm_f64_ws_need says for the shape (the launcher
// never picks another split to fit: the summation order of a shape must not depend on allocation history)
constexpr int GEMM_F64_EWORKSPACE = -77001;
int gemm3m_enabled();
void gemm3m_set(int on);
// the launches gemm_f64 makes for a product (chase_hip_gemm_plan): their count; the first max_out are written to out
int gemm_f64_plan(bool cplx, char opA, int m, int n, int k, long lda, long ldb, bool aligned16, int tag, int num_cu, int min_rounds,
                  chase_hip_gemm_launch* out, int max_out);

// ---- single precision (gemm_mfma_f32.hip): the product of the mixed-precision filter.  op(A) = N only (anything else returns
// GEMM_F32_EOP), any m, n, k and leading dimensions, operands 4-byte (real) / 8-byte (complex) aligned.  One workgroup per output
// tile over the whole K: bitwise reproducible.  alpha / beta point to 1 (real) or 2 (complex) host floats.  tag 1: the filter's
// own kernel symbol.
constexpr int GEMM_F32_EOP = -77002;
int gemm_f32(hipStream_t st, bool cplx, char opA, int m, int n, int k, const float* alpha, const float* A, long lda, const float* B,
             long ldb, const float* beta, float* C, long ldc, int num_cu, int tag = 0);
// gemm_f32 with op(A) = N or C (real: T as well), A for op = C a k x m array: op N is gemm_f32 bit for bit, op C is op N on the
// explicitly formed A^H bit for bit.  The product of the single-precision generalized problem (capi_gev.hip).
int gemm_f32_op(hipStream_t st, bool cplx, char opA, int m, int n, int k, const float* alpha, const float* A, long lda,
                const float* B, long ldb, const float* beta, float* C, long ldc, int num_cu, int tag = 0);
// the same product written and scaled in fp64: C64 = alpha op(A32) B32 + beta C64, op(A) = N or C (real: T as well), A for
// op = C a k x m array.  alpha / beta point to 1 or 2 host doubles.  The product of the filter on a grid: the partial products
// of the ranks are summed in fp64.  Whole K unless gemm_min_rounds asks for pieces; bitwise reproducible either way:
// min_rounds > 0 (the launch shares the chip with a collective) cuts a product with fewer tiles than workgroup slots into
// K pieces (sp_frame::split_plan, a function of shape, chip and min_rounds only), each an ordinary product
// into an fp64 slab of its own in ws, and sp_slab_reduce sums the slabs in piece order.  ws_bytes below gemm_sp_ws_need:
// GEMM_F64_EWORKSPACE.  pieces (optional): the K pieces of this product (1: whole K).
int gemm_f32w(hipStream_t st, bool cplx, char opA, int m, int n, int k, const double* alpha, const float* A, long lda,
              const float* B, long ldb, const double* beta, double* C, long ldc, int num_cu, int tag = 0, double* ws = nullptr,
              size_t ws_bytes = 0, int min_rounds = 0, int* pieces = nullptr);
// the same two products on the bf16 matrix cores with every fp32 operand split into three bf16 parts in the kernel
// (gemm_mfma_bf16x3.hip): six partial products per k in the fp32 accumulator.  Interfaces, statuses and reproducibility as above.
int gemm_bf16x3(hipStream_t st, bool cplx, char opA, int m, int n, int k, const float* alpha, const float* A, long lda, const float* B,
                long ldb, const float* beta, float* C, long ldc, int num_cu, int tag = 0);
int gemm_bf16x3w(hipStream_t st, bool cplx, char opA, int m, int n, int k, const double* alpha, const float* A, long lda,
                 const float* B, long ldb, const double* beta, double* C, long ldc, int num_cu, int tag = 0, double* ws = nullptr,
                 size_t ws_bytes = 0, int min_rounds = 0, int* pieces = nullptr);
// the narrow bf16x3 product with A split and tiled once (gemm_mfma_bf16x3p.hip): pack writes all pack_bytes(m, k) bytes of the
// packed image of an m x k fp32 (src_f64: fp64, rounded to fp32 first) A, pack_diag the n diagonal entries of an n x n pack from
// an fp64 H, and gemm_bf16x3p is gemm_bf16x3('N', ...) on the pack, bit for bit.
size_t bf16x3_pack_bytes(bool cplx, int m, int k);
int bf16x3_pack(hipStream_t st, bool cplx, bool src_f64, int m, int k, const void* A, long lda, void* packed);
int bf16x3_pack_diag(hipStream_t st, bool cplx, int n, const double* H, long ldh, void* packed);
int gemm_bf16x3p(hipStream_t st, bool cplx, int m, int n, int k, const float* alpha, const void* packedA, const float* B, long ldb,
                 const float* beta, float* C, long ldc, int num_cu, int tag = 0);
// C = alpha (S_0 + S_1 + ... + S_{sk-1}) + beta C in fp64, the slabs summed in index order (vec_kernels.hip): slab p is the dense
// lds x (columns) block at S + p * slab_stride (doubles; lds in elements, even), of which rows < m and columns < n are read.
// alpha / beta point to 1 (real) or 2 (complex) host doubles; beta == 0: C is not read.
int sp_slab_reduce(hipStream_t st, bool cplx, int m, int n, int sk, const double* S, long lds, long slab_stride, const double* alpha,
                   const double* beta, double* C, long ldc);

int mfma_f64_peak(hipStream_t st, double* out, int blocks, int iters);
int stream_copy(hipStream_t st, void* dst, const void* src, size_t bytes);

// ---- streaming / reduction kernels (vec_kernels.hip); *_d arguments are in doubles (m*ept, ld*ept) ----
int shift_diag(hipStream_t st, double* H, long ld, int n, int ept, double shift);
int shift_list(hipStream_t st, double* H, long ld, const int* rows, const int* cols, int cnt, int ept, double shift);
int shift_diag_dev(hipStream_t st, double* A, long ld, int n, int ept, const double* nrmf_dev, double factor);
int abs_trace(hipStream_t st, const double* A, long ld, int n, int ept, double* out_dev);
int copy2d(hipStream_t st, const double* src, long ld_src_d, double* dst, long ld_dst_d, long md, int ncols);
int swap_cols(hipStream_t st, double* a, double* b, long md);
int rows_indexed(hipStream_t st, bool cplx, const double* in, long ld_in, double* out, long ld_out, const int* idx_dev,
                 int np, int ncols, int scatter);
int hash64(hipStream_t st, const double* x, long ld_d, long md, int ncols, unsigned long long* out_dev);
int tri_mask_bc(hipStream_t st, bool cplx, double* H, long ldh, int mloc, int nloc, long mb, int pr, int pi, long nb, int pc,
                int pj, int keep_upper);
int conj_transpose_add(hipStream_t st, bool cplx, const double* P, long ldp, int nr, int nc, const int* rowmap_dev,
                       const int* colmap_dev, double* H, long ldh);
int copy_cols_indexed(hipStream_t st, const double* src, long ld_src_d, double* dst, long ld_dst_d, long md,
                      const int* src_idx_dev, const int* dst_idx_dev, int cnt);
// dst column dst0 + c <- src column src_idx[c], c < cnt (md doubles per column)
int copy_cols_indexed_range(hipStream_t st, const double* src, long ld_src_d, double* dst, long ld_dst_d, long md,
                            const int* src_idx_dev, int dst0, int cnt);
int resid_norms(hipStream_t st, const double* W, long ldw_d, const double* V, long ldv_d, const double* lambda_dev,
                long md, int ncols, double* out_dev, int do_sqrt);
int sqrt_inplace(hipStream_t st, double* x, int n);
int col_dot(hipStream_t st, bool cplx, const double* X, long ldx_d, const double* Y, long ldy_d, int m, int ncols,
            double* out_dev);
int col_axpy(hipStream_t st, bool cplx, const double* a_dev, int a_is_real, int a_stride, double sgn, const double* X,
             long ldx_d, double* Y, long ldy_d, int m, int ncols);
int col_scal(hipStream_t st, const double* a_dev, int inv, double* X, long ldx_d, long md, int ncols);
int scale_rows(hipStream_t st, double* X, long ldx_d, long row0_d, long md, int ncols, double s);
int scale_rows_bc(hipStream_t st, double* X, long ldx_d, long m, int ncols, int ept, long g0, long nb, int p, int q, double s);
int conj_inplace(hipStream_t st, double* X, long ldx_d, int m, int ncols);
int pack_upper(hipStream_t st, const double* A, long lda, int n, int ept, double* P);
int unpack_upper(hipStream_t st, double* P, int n, int ept, double* A, long lda);
int mirror_upper(hipStream_t st, double* A, long lda, int n, int ept);
int mirror_lower(hipStream_t st, double* A, long lda, int n, int ept, int zero_diag_imag = 1);
// precision conversion, ms scalars per column (m * ept), leading dimensions in scalars of their own type
int convert_d2s(hipStream_t st, const double* src, long ld_src, float* dst, long ld_dst, long ms, int ncols);   // round to nearest
int convert_s2d(hipStream_t st, const float* src, long ld_src, double* dst, long ld_dst, long ms, int ncols);   // exact
int diag_d2s(hipStream_t st, const double* H, long ldh, float* Hs, long ldhs, int n, int ept);                  // Hs[i,i] = (float)H[i,i]
// Y_j += (gr + i gi) X_j on fp32 columns of ms floats (m * ept), leading dimensions in floats; gamma by value
int axpy_sp(hipStream_t st, bool cplx, float gr, float gi, const float* X, long ldx_f, float* Y, long ldy_f, long ms, int ncols);
// sp_kernels.hip: X[i, j] *= s for the floats i >= row0_f of the mf floats of each column (one fp32 multiply per float)
int scale_rows_sp(hipStream_t st, float* X, long ldx_f, long row0_f, long mf, int ncols, float s);
// sp_kernels.hip: second[hf + i, j] = conj(first[i, j]), second[i, j] = conj(first[hf + i, j]), i < hf floats (hf = N/2 * ept);
// cplx: the odd floats (imaginary parts) change sign, real: the plain half swap.  first and second must not overlap
int kconj_sp(hipStream_t st, bool cplx, const float* first, long ldf_f, float* second, long lds_f, long hf, int ncols);
// Hs[rows[i], cols[i]] = (float)H[rows[i], cols[i]], i < cnt (device lists: the diagonal inside a rank's block)
int diag_list_d2s(hipStream_t st, const double* H, long ldh, float* Hs, long ldhs, const int* rows, const int* cols, int cnt, int ept);

// ---- generators (gen_kernels.hip) ----
int fill_normal(hipStream_t st, bool cplx, double* X, long ldx, int m, int n, long grow0, long gcol0, long gld,
                unsigned long long seed, int mb = 0, int pr = 1, int pi = 0);
int gen_clement(hipStream_t st, bool cplx, double* H, long ldh, int mloc, int nloc, long N, int mb, int pr, int pi,
                long roff, int nb, int pc, int pj, long coff, double scale, double perturb, unsigned long long seed);
int gen_bse(hipStream_t st, bool cplx, double* H, long ldh, int mloc, int nloc, long N, int mb, int pr, int pi, int nb,
            int pc, int pj, double dmin, double dmax, double offdiag, unsigned long long seed);

// ---- tridiagonal divide & conquer with the O(n^2) / O(n^3) parts on the device (stedc_gpu.hip); d, e on the host ----
}
struct chase_hip_ctx;
namespace chase_hip {
int stedc_gpu(chase_hip_ctx* c, int n, const double* d, const double* e, double* w_host, double* Z_dev, long ldz);

// ---- factorisation cores (factor_kernels.hip) ----
int potf2_trtri(hipStream_t st, bool cplx, double* A, long lda, int nb, int joff, double* Tinv, int* info_dev);
int trtri_diag(hipStream_t st, bool cplx, const double* R, long ldr, int n, double* Tinv);

// ---- generalized problem (gev_kernels.hip) ----
// A_jj <- U_jj^{-H} A_jj U_jj^{-1} for one nb x nb block (nb <= 64, one workgroup) from the upper triangles of both; both
// triangles of A_jj are written, the lower one the bitwise conjugate of the upper one, imaginary diagonal +0
int hegs2_diag(hipStream_t st, bool cplx, double* A, long lda, const double* U, long ldu, int nb);
// dst[i, j] = src[i, j] / dst[i, j] += src[i, j] for i <= j < n (leading dimensions in elements, ept doubles per element)
int copy_upper(hipStream_t st, const double* src, long ld_src, double* dst, long ld_dst, int n, int ept);
int add_upper(hipStream_t st, const double* src, long ld_src, double* dst, long ld_dst, int n, int ept);
// X (nb x ncols, nb <= 64) <- op(U) X in place, U the upper triangle of an nb x nb block (nothing below its diagonal is read),
// op_c: op = conjugate transpose; one workgroup per 64 columns, f64 MFMA, four multiplications per complex product
int trmm_diag(hipStream_t st, bool cplx, bool op_c, const double* U, long ldu, double* X, long ldx, int nb, int ncols);
// A (n x n) <- A^H in place
int conj_transpose_inplace(hipStream_t st, bool cplx, double* A, long lda, int n);

// ---- the same cores on fp32 storage (the _sp entry points of capi_gev.hip) ----
// potf2_trtri / trtri_diag / hegs2_diag: the kernels above instantiated for float matrices - loads widened, all arithmetic in
// fp64 registers and LDS, one rounding on the way out (Tinv is fp32 too: it feeds the fp32 product).  The helpers address floats.
int potf2_trtri(hipStream_t st, bool cplx, float* A, long lda, int nb, int joff, float* Tinv, int* info_dev);
int trtri_diag(hipStream_t st, bool cplx, const float* R, long ldr, int n, float* Tinv);
int hegs2_diag(hipStream_t st, bool cplx, float* A, long lda, const float* U, long ldu, int nb);
int add_upper(hipStream_t st, const float* src, long ld_src, float* dst, long ld_dst, int n, int ept);
int conj_transpose_inplace(hipStream_t st, bool cplx, float* A, long lda, int n);
int mirror_upper(hipStream_t st, float* A, long lda, int n, int ept);
int mirror_lower(hipStream_t st, float* A, long lda, int n, int ept, int zero_diag_imag = 1);
int copy2d_sp(hipStream_t st, const float* src, long ld_src_f, float* dst, long ld_dst_f, long mf, int ncols);   // sp_kernels.hip
// trmm_diag on fp32 data: v_mfma_f32_16x16x4_f32, fp32 accumulation
int trmm_diag_sp(hipStream_t st, bool cplx, bool op_c, const float* U, long ldu, float* X, long ldx, int nb, int ncols);
// the two under the names of their fp64 forms, for the drivers of capi_gev.hip that are written once for both precisions
inline int copy2d(hipStream_t st, const float* src, long ld_src_f, float* dst, long ld_dst_f, long mf, int ncols)
{
    return copy2d_sp(st, src, ld_src_f, dst, ld_dst_f, mf, ncols);
}
inline int trmm_diag(hipStream_t st, bool cplx, bool op_c, const float* U, long ldu, float* X, long ldx, int nb, int ncols)
{
    return trmm_diag_sp(st, cplx, op_c, U, ldu, X, ldx, nb, ncols);
}

} // namespace chase_hip
