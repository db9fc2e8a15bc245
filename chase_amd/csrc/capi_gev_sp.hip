// capi_gev_sp.hip — the generalized Hermitian-definite problem H x = lambda S x (itype 1) on fp32 data, one GPU: the drivers of
// capi_gev.hip with the product swapped.  H, S, the factor and the vector blocks stay fp32 (real, or interleaved complex) from
// start to end; nothing of size N^2 is ever widened.  Every O(n^3) flop goes through gemm_f32_op (gemm_mfma_f32_op.hip,
// v_mfma_f32_32x32x2_f32, whole K, no atomics: four-multiplication complex products, bitwise reproducible); the cores are the
// fp32-storage forms of potf2_trtri / trtri_diag (factor_kernels.hip) and hegs2_diag, which compute in fp64 and round once, and
// trmm_diag_sp, the 64-row step of the triangular product on v_mfma_f32_16x16x4_f32 (gev_kernels.hip).
//
// Same block sizes as capi_gev.hip (64 / 256 / 256 / 2048), same rule that the strictly lower triangle of S is neither read nor
// written, same info convention.  Two things differ from the fp64 drivers:
//  * the Cholesky factorises an outer diagonal block in place in fp32 storage (64-wide potf2 steps with trapezoid updates inside
//    the block) instead of on a scratch copy by chase_hip_potrf_upper: no fp64 copy of the block, and nothing below the diagonal
//    is touched to begin with;
//  * the two-sided reduction has the two-full-solve form only, and its right solve A U^{-1} is a left solve on the conjugate
//    transpose, U^{-H} (U^{-H} A)^H = U^{-H} A U^{-1} for Hermitian A: one solve routine instead of two, and both solves run the
//    op C product whose operands are read k-contiguous.
// The scratch is the context's BUF_GEV_* (sized in bytes; these drivers never run inside an fp64 one).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include "../../include/chase_hip.h"
#include "ctx.h"
#include "kernels.h"

using namespace chase_hip;

#define HIPCHK(x)                                                                                                      \
    do {                                                                                                               \
        hipError_t e_ = (x);                                                                                           \
        if (e_ != hipSuccess) return hip_fail(e_, #x);                                                                 \
    } while (0)
#define KCHK(x, what)                                                                                                  \
    do {                                                                                                               \
        int e_ = (x);                                                                                                  \
        if (e_) return hip_fail((hipError_t)e_, what);                                                                 \
    } while (0)
#define RCCHK(x)                                                                                                       \
    do {                                                                                                               \
        int r_ = (x);                                                                                                  \
        if (r_) return r_;                                                                                             \
    } while (0)

namespace {
constexpr int NB = 64;
constexpr int SOLVE_WB = 256;        // rows per left-looking step of the left solve (64-row steps inside)
constexpr int TRAP_CB = 256;         // column block of the trapezoid updates
constexpr int POTRF_OUTER_NB = 2048; // the fp64 driver's default (profiles/gev.txt)

inline int ept_of(int cplx) { return cplx ? 2 : 1; }
inline int imin(int a, int b) { return a < b ? a : b; }

int gemm(chase_hip_ctx* c, int cplx, char op, int m, int n, int k, float ar, const float* A, long lda, const float* B, long ldb,
         float br, float* C, long ldc)
{
    if (m <= 0 || n <= 0) return 0;
    const float alpha[2] = {ar, 0.f}, beta[2] = {br, 0.f};
    if (c->oplog_on) c->oplog_add(cplx ? (op == 'N' ? "gemm_c_opN" : "gemm_c_opC") : (op == 'N' ? "gemm_s_opN" : "gemm_s_opC"), m, n, k, 0);
    KCHK(gemm_f32_op(c->stream, cplx != 0, op, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, c->num_cu, 0), "gemm_f32_op launch");
    return 0;
}

// B (n x nrhs) <- op(R)^{-1} B: trsm_left of capi_gev.hip on floats
int trsm_left(chase_hip_ctx* c, int cplx, char op, int n, int nrhs, const float* R, long ldr, float* B, long ldb)
{
    if (n <= 0 || nrhs <= 0) return 0;
    const int e = ept_of(cplx);
    const int nblk = (n + NB - 1) / NB;
    RCCHK(c->ensure_buf(chase_hip_ctx::BUF_GEV_TINV, (size_t)nblk * NB * NB * sizeof(float) * e));
    RCCHK(c->ensure_buf(chase_hip_ctx::BUF_GEV_PANEL, (size_t)NB * nrhs * sizeof(float) * e));
    float* Tinv = (float*)c->bufs[chase_hip_ctx::BUF_GEV_TINV];
    float* P = (float*)c->bufs[chase_hip_ctx::BUF_GEV_PANEL];
    KCHK(trtri_diag(c->stream, cplx != 0, R, ldr, n, Tinv), "trtri_diag");
    if (op == 'C') {
        for (int J0 = 0; J0 < n; J0 += SOLVE_WB) {
            const int Jend = imin(n, J0 + SOLVE_WB), wb = Jend - J0;
            if (J0 > 0)          // B_J -= R[0:J0, J]^H X[0:J0, :]
                RCCHK(gemm(c, cplx, 'C', wb, nrhs, J0, -1.f, R + (long)J0 * ldr * e, ldr, B, ldb, 1.f, B + (long)J0 * e, ldb));
            for (int j0 = J0; j0 < Jend; j0 += NB) {
                const int nb = imin(NB, Jend - j0);
                float* Bj = B + (long)j0 * e;
                RCCHK(gemm(c, cplx, 'C', nb, nrhs, nb, 1.f, Tinv + (long)(j0 / NB) * NB * NB * e, NB, Bj, ldb, 0.f, P, nb));
                KCHK(copy2d_sp(c->stream, P, (long)nb * e, Bj, ldb * e, (long)nb * e, nrhs), "trsm_left_sp panel copy");
                const int rest = Jend - j0 - nb;               // the block's remaining rows only
                if (rest > 0)
                    RCCHK(gemm(c, cplx, 'C', rest, nrhs, nb, -1.f, R + ((long)(j0 + nb) * ldr + j0) * e, ldr, P, nb, 1.f,
                               B + (long)(j0 + nb) * e, ldb));
            }
        }
    } else {
        for (int J0 = (n - 1) / SOLVE_WB * SOLVE_WB; J0 >= 0; J0 -= SOLVE_WB) {
            const int Jend = imin(n, J0 + SOLVE_WB), wb = Jend - J0;
            if (Jend < n)        // B_J -= R[J, Jend:n] X[Jend:n, :]
                RCCHK(gemm(c, cplx, 'N', wb, nrhs, n - Jend, -1.f, R + ((long)Jend * ldr + J0) * e, ldr, B + (long)Jend * e, ldb, 1.f,
                           B + (long)J0 * e, ldb));
            for (int j0 = J0 + (wb - 1) / NB * NB; j0 >= J0; j0 -= NB) {
                const int nb = imin(NB, Jend - j0);
                float* Bj = B + (long)j0 * e;
                RCCHK(gemm(c, cplx, 'N', nb, nrhs, nb, 1.f, Tinv + (long)(j0 / NB) * NB * NB * e, NB, Bj, ldb, 0.f, P, nb));
                KCHK(copy2d_sp(c->stream, P, (long)nb * e, Bj, ldb * e, (long)nb * e, nrhs), "trsm_left_sp panel copy");
                const int above = j0 - J0;                     // the block's rows above this step only
                if (above > 0)
                    RCCHK(gemm(c, cplx, 'N', above, nrhs, nb, -1.f, R + ((long)j0 * ldr + J0) * e, ldr, P, nb, 1.f,
                               B + (long)J0 * e, ldb));
            }
        }
    }
    return 0;
}

// X (n x ncols) <- op(U) X in place: trmm_left of capi_gev.hip on floats, the 64-row step by trmm_diag_sp
int trmm_left(chase_hip_ctx* c, int cplx, char op, int n, int ncols, const float* U, long ldu, float* X, long ldx)
{
    if (n <= 0 || ncols <= 0) return 0;
    const int e = ept_of(cplx);
    if (op == 'N') {
        for (int J0 = 0; J0 < n; J0 += SOLVE_WB) {
            const int Jend = imin(n, J0 + SOLVE_WB), wb = Jend - J0;
            for (int j0 = J0; j0 < Jend; j0 += NB) {
                const int nb = imin(NB, Jend - j0);
                float* Xj = X + (long)j0 * e;
                KCHK(trmm_diag_sp(c->stream, cplx != 0, false, U + ((long)j0 * ldu + j0) * e, ldu, Xj, ldx, nb, ncols), "trmm_diag_sp");
                const int rest = Jend - j0 - nb;               // X_j += U[j, j0+nb : Jend] X[j0+nb : Jend], rows not yet overwritten
                if (rest > 0)
                    RCCHK(gemm(c, cplx, 'N', nb, ncols, rest, 1.f, U + ((long)(j0 + nb) * ldu + j0) * e, ldu,
                               X + (long)(j0 + nb) * e, ldx, 1.f, Xj, ldx));
            }
            if (Jend < n)        // X_J += U[J, Jend:n] X[Jend:n, :]
                RCCHK(gemm(c, cplx, 'N', wb, ncols, n - Jend, 1.f, U + ((long)Jend * ldu + J0) * e, ldu, X + (long)Jend * e, ldx, 1.f,
                           X + (long)J0 * e, ldx));
        }
    } else {
        for (int J0 = (n - 1) / SOLVE_WB * SOLVE_WB; J0 >= 0; J0 -= SOLVE_WB) {
            const int Jend = imin(n, J0 + SOLVE_WB), wb = Jend - J0;
            for (int j0 = J0 + (wb - 1) / NB * NB; j0 >= J0; j0 -= NB) {
                const int nb = imin(NB, Jend - j0);
                float* Xj = X + (long)j0 * e;
                KCHK(trmm_diag_sp(c->stream, cplx != 0, true, U + ((long)j0 * ldu + j0) * e, ldu, Xj, ldx, nb, ncols), "trmm_diag_sp");
                const int above = j0 - J0;                     // X_j += U[J0 : j0, j]^H X[J0 : j0], rows not yet overwritten
                if (above > 0)
                    RCCHK(gemm(c, cplx, 'C', nb, ncols, above, 1.f, U + ((long)j0 * ldu + J0) * e, ldu, X + (long)J0 * e, ldx, 1.f,
                               Xj, ldx));
            }
            if (J0 > 0)          // X_J += U[0:J0, J]^H X[0:J0, :]
                RCCHK(gemm(c, cplx, 'C', wb, ncols, J0, 1.f, U + (long)J0 * ldu * e, ldu, X, ldx, 1.f, X + (long)J0 * e, ldx));
        }
    }
    return 0;
}

// A[r0 : r1, r0 : r1] -= P^H P on the upper block trapezoid, P = A[p0 : p0 + k, r0 : r1] (the rows of a finished panel), in
// column blocks: the rectangle above each diagonal block in place, the diagonal block itself through the scratch product G of
// which only the upper triangle is added - nothing below the diagonal is read or written.
int trapezoid_update(chase_hip_ctx* c, int cplx, float* A, long lda, int p0, int k, int r0, int r1, float* G)
{
    const int e = ept_of(cplx);
    const float* Pr = A + ((long)r0 * lda + p0) * e;
    for (int c0 = r0; c0 < r1; c0 += TRAP_CB) {
        const int cw = imin(TRAP_CB, r1 - c0);
        const float* Pc = A + ((long)c0 * lda + p0) * e;             // the panel's columns of this block
        RCCHK(gemm(c, cplx, 'C', c0 - r0, cw, k, -1.f, Pr, lda, Pc, lda, 1.f, A + ((long)c0 * lda + r0) * e, lda));
        RCCHK(gemm(c, cplx, 'C', cw, cw, k, -1.f, Pc, lda, Pc, lda, 0.f, G, cw));
        KCHK(add_upper(c->stream, G, cw, A + ((long)c0 * lda + c0) * e, lda, cw, e), "potrf_blocked_sp diagonal update");
    }
    return 0;
}

// Upper Cholesky in two levels, in place in fp32 storage.  Per outer block of ob columns: the diagonal block is factorised by
// 64-wide steps (potf2_trtri, row panel with the inverted block, trapezoid update inside the outer block), then the row panel
// behind it is solved with U_JJ^H from the left and the trailing trapezoid is updated with an inner dimension of ob.  The
// pivot flag is read once per outer block: a failure ends the factorisation there.
int potrf_blocked(chase_hip_ctx* c, int cplx, int n, float* A, long lda, int ob)
{
    const int e = ept_of(cplx);
    RCCHK(c->ensure_buf(chase_hip_ctx::BUF_GEV_DIAG, ((size_t)NB * NB + (size_t)TRAP_CB * TRAP_CB) * sizeof(float) * e + 64));
    RCCHK(c->ensure_buf(chase_hip_ctx::BUF_GEV_PANEL, (size_t)NB * n * sizeof(float) * e));       // trsm_left asks for no more
    float* Tinv = (float*)c->bufs[chase_hip_ctx::BUF_GEV_DIAG];
    float* G = Tinv + (size_t)NB * NB * e;
    int* info_dev = (int*)(G + (size_t)TRAP_CB * TRAP_CB * e);
    HIPCHK(hipMemsetAsync(info_dev, 0, sizeof(int), c->stream));
    for (int J0 = 0; J0 < n; J0 += ob) {
        const int w = imin(ob, n - J0), T0 = J0 + w;
        for (int j0 = J0; j0 < T0; j0 += NB) {
            const int nb = imin(NB, T0 - j0), rest = T0 - j0 - nb;
            float* Ajj = A + ((long)j0 * lda + j0) * e;
            KCHK(potf2_trtri(c->stream, cplx != 0, Ajj, lda, nb, j0, Tinv, info_dev), "potf2_trtri");
            if (rest > 0) {
                float* P = (float*)c->bufs[chase_hip_ctx::BUF_GEV_PANEL];
                float* Ajr = A + ((long)(j0 + nb) * lda + j0) * e;         // A[j0 : j0 + nb, j0 + nb : T0]
                RCCHK(gemm(c, cplx, 'C', nb, rest, nb, 1.f, Tinv, NB, Ajr, lda, 0.f, P, nb));
                KCHK(copy2d_sp(c->stream, P, (long)nb * e, Ajr, lda * e, (long)nb * e, rest), "potrf_blocked_sp panel copy");
                RCCHK(trapezoid_update(c, cplx, A, lda, j0, nb, j0 + nb, T0, G));
            }
        }
        int info = 0;
        HIPCHK(hipMemcpyAsync(&info, info_dev, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (info != 0) return info;
        if (T0 >= n) break;
        float* Ajr = A + ((long)T0 * lda + J0) * e;                        // A[J0 : T0, T0 : n]
        RCCHK(trsm_left(c, cplx, 'C', w, n - T0, A + ((long)J0 * lda + J0) * e, lda, Ajr, lda));
        RCCHK(trapezoid_update(c, cplx, A, lda, J0, w, T0, n, G));
    }
    return 0;
}

int block_size(int asked, int dflt) { return asked == 0 ? dflt : asked; }
char norm_op(char op) { return op == 'n' ? 'N' : op == 'c' ? 'C' : op; }
} // namespace

extern "C" {

/* chase_hip_trsm_left_upper on fp32 data */
int chase_hip_trsm_left_upper_sp(chase_hip_ctx* c, int cplx, char op, int n, int nrhs, const void* R, long ldr, void* B, long ldb)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "trsm_left_upper_sp: NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add("trsm_left_upper_sp", n, nrhs, op, 0);
    op = norm_op(op);
    if (op != 'N' && op != 'C') return set_error(CHASE_HIP_EINVAL, "trsm_left_upper_sp: op must be 'N' or 'C'");
    if (n < 0 || nrhs < 0 || ldr < n || ldb < n) return set_error(CHASE_HIP_EINVAL, "trsm_left_upper_sp: bad shape");
    if (n == 0 || nrhs == 0) return 0;
    if (!R || !B) return set_error(CHASE_HIP_EINVAL, "trsm_left_upper_sp: NULL matrix");
    return trsm_left(c, cplx, op, n, nrhs, (const float*)R, ldr, (float*)B, ldb);
}

/* chase_hip_trmm_left_upper on fp32 data */
int chase_hip_trmm_left_upper_sp(chase_hip_ctx* c, int cplx, char op, int n, int ncols, const void* U, long ldu, void* X, long ldx)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "trmm_left_upper_sp: NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add("trmm_left_upper_sp", n, ncols, op, 0);
    op = norm_op(op);
    if (op != 'N' && op != 'C') return set_error(CHASE_HIP_EINVAL, "trmm_left_upper_sp: op must be 'N' or 'C'");
    if (n < 0 || ncols < 0 || ldu < n || ldx < n) return set_error(CHASE_HIP_EINVAL, "trmm_left_upper_sp: bad shape");
    if (n == 0 || ncols == 0) return 0;
    if (!U || !X) return set_error(CHASE_HIP_EINVAL, "trmm_left_upper_sp: NULL matrix");
    return trmm_left(c, cplx, op, n, ncols, (const float*)U, ldu, (float*)X, ldx);
}

/* In-place upper Cholesky A = U^H U of an fp32 matrix with the contract and info of chase_hip_potrf_upper_blocked: the strictly
 * lower triangle is neither read nor written; info > 0 is the first non-positive pivot.  The outer diagonal blocks are
 * factorised in place (64-wide steps whose cores compute in fp64), not on an fp64 scratch copy. */
int chase_hip_potrf_upper_blocked_sp(chase_hip_ctx* c, int cplx, int n, void* A, long lda, int outer_nb)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "potrf_upper_blocked_sp: NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add("potrf_upper_blocked_sp", n, outer_nb, 0, 0);
    if (n < 0 || lda < n) return set_error(CHASE_HIP_EINVAL, "potrf_upper_blocked_sp: bad shape");
    if (outer_nb < 0 || outer_nb % NB) return set_error(CHASE_HIP_EINVAL, "potrf_upper_blocked_sp: outer_nb must be 0 or a multiple of 64");
    if (n == 0) return 0;
    if (!A) return set_error(CHASE_HIP_EINVAL, "potrf_upper_blocked_sp: NULL matrix");
    return potrf_blocked(c, cplx, n, (float*)A, lda, block_size(outer_nb, POTRF_OUTER_NB));
}

/* A <- U^{-H} A U^{-1} on fp32 data with the argument and result contract of chase_hip_hegst_upper (nb = 0): A is read from its
 * upper triangle only, the strictly lower triangle of U never; on return A is Hermitian bit for bit, imaginary diagonal +0.
 * n <= 64: hegs2_diag.  Above: two left solves with U^H on the completed matrix and an in-place conjugate transpose between. */
int chase_hip_hegst_upper_sp(chase_hip_ctx* c, int cplx, int n, void* A, long lda, const void* U, long ldu)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "hegst_upper_sp: NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add("hegst_upper_sp", n, 0, 0, 0);
    if (n < 0 || lda < n || ldu < n) return set_error(CHASE_HIP_EINVAL, "hegst_upper_sp: bad shape");
    if (n == 0) return 0;
    if (!A || !U) return set_error(CHASE_HIP_EINVAL, "hegst_upper_sp: NULL matrix");
    const int e = ept_of(cplx);
    if (n <= NB) {
        KCHK(hegs2_diag(c->stream, cplx != 0, (float*)A, lda, (const float*)U, ldu, n), "hegs2_diag");
        return 0;
    }
    KCHK(mirror_upper(c->stream, (float*)A, lda, n, e), "mirror_upper");
    RCCHK(trsm_left(c, cplx, 'C', n, n, (const float*)U, ldu, (float*)A, lda));                      // W = U^{-H} A
    KCHK(conj_transpose_inplace(c->stream, cplx != 0, (float*)A, lda, n), "conj_transpose_inplace");  // W^H = A U^{-1}
    RCCHK(trsm_left(c, cplx, 'C', n, n, (const float*)U, ldu, (float*)A, lda));                      // U^{-H} A U^{-1}
    KCHK(mirror_lower(c->stream, (float*)A, lda, n, e, 1), "mirror_lower");
    return 0;
}

/* chase_hip_gev_reduce_itype (itype 1) on fp32 data: factor = 1, S <- U first; factor = 0, S already holds U.  Returns the
 * potrf info > 0 when S is not positive definite; A is then untouched. */
int chase_hip_gev_reduce_sp(chase_hip_ctx* c, int cplx, int factor, int n, void* A, long lda, void* S, long lds_)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "gev_reduce_sp: NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add("gev_reduce_sp", n, 0, 0, factor);
    if (factor != 0 && factor != 1) return set_error(CHASE_HIP_EINVAL, "gev_reduce_sp: factor must be 0 or 1");
    if (n < 0 || lda < n || lds_ < n) return set_error(CHASE_HIP_EINVAL, "gev_reduce_sp: bad shape");
    if (n == 0) return 0;
    if (!A || !S) return set_error(CHASE_HIP_EINVAL, "gev_reduce_sp: NULL matrix");
    if (factor) {
        const int info = chase_hip_potrf_upper_blocked_sp(c, cplx, n, S, lds_, 0);
        if (info != 0) return info;
    }
    return chase_hip_hegst_upper_sp(c, cplx, n, A, lda, S, lds_);
}

/* X (n x ncols, fp32) <- U^{-1} X */
int chase_hip_gev_backtransform_sp(chase_hip_ctx* c, int cplx, int n, int ncols, const void* U, long ldu, void* X, long ldx)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "gev_backtransform_sp: NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add("gev_backtransform_sp", n, ncols, 0, 0);
    if (n < 0 || ncols < 0 || ldu < n || ldx < n) return set_error(CHASE_HIP_EINVAL, "gev_backtransform_sp: bad shape");
    if (n == 0 || ncols == 0) return 0;
    if (!U || !X) return set_error(CHASE_HIP_EINVAL, "gev_backtransform_sp: NULL matrix");
    return trsm_left(c, cplx, 'N', n, ncols, (const float*)U, ldu, (float*)X, ldx);
}

/* X (n x ncols, fp32) <- U X: the inverse of chase_hip_gev_backtransform_sp */
int chase_hip_gev_starttransform_sp(chase_hip_ctx* c, int cplx, int n, int ncols, const void* U, long ldu, void* X, long ldx)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "gev_starttransform_sp: NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add("gev_starttransform_sp", n, ncols, 0, 0);
    if (n < 0 || ncols < 0 || ldu < n || ldx < n) return set_error(CHASE_HIP_EINVAL, "gev_starttransform_sp: bad shape");
    if (n == 0 || ncols == 0) return 0;
    if (!U || !X) return set_error(CHASE_HIP_EINVAL, "gev_starttransform_sp: NULL matrix");
    return trmm_left(c, cplx, 'N', n, ncols, (const float*)U, ldu, (float*)X, ldx);
}

} // extern "C"
