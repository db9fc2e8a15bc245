// capi_gev.hip — C ABI entry points of the generalized Hermitian-definite problem H x = lambda S x on one GPU
// (include/chase_hip.h), on fp64 data and - the _sp entry points, itype 1 - on fp32 data: the left triangular solve, the two-level
// Cholesky that leaves the strictly lower triangle alone, the two-sided reduction C = U^{-H} H U^{-1} and the back-transformation
// X = U^{-1} Y.  They replace the three ScaLAPACK calls (ppotrf, phegst, ptrtrs) the reference's docs/example/gev.rst puts around
// chase::Solve.  For sequences of pencils and LAPACK's problem types 2 and 3: the triangular product X <- op(U) X, C = U H U^H,
// the itype-aware reduction and back-transformation and the start transform that makes the previous pencil's eigenvectors the
// start block of the next reduced problem.
//
// The blocked drivers (trsm_left, trmm_left, trapezoid_update) are written once, as templates over the scalar type; what the two
// precisions do differently they do through overloads: gemm below, copy2d, trmm_diag and the cores of kernels.h.
//  * fp64: every O(n^3) flop goes through the context's MFMA GEMM; the cores are potf2_trtri / trtri_diag (factor_kernels.hip),
//    hegs2_diag and the 64-row MFMA step of the triangular product, trmm_diag (gev_kernels.hip).
//  * fp32: H, S, the factor and the vector blocks stay fp32 (real, or interleaved complex) from start to end; nothing of size N^2
//    is ever widened.  Every O(n^3) flop goes through gemm_f32_op (gemm_mfma_f32_op.hip, v_mfma_f32_32x32x2_f32, whole K, no
//    atomics: bitwise reproducible); the cores are the fp32-storage forms of potf2_trtri / trtri_diag and hegs2_diag, which
//    compute in fp64 and round once, and trmm_diag on v_mfma_f32_16x16x4_f32.
// Same block sizes (64 / 256 / 256 / 2048), same rule that the strictly lower triangle of S is neither read nor written, same
// info convention.  The context's phase is 0 while these run: complex products take four multiplications, which is what the
// componentwise bounds of tests/gev_refs.py and tests/gev_sp_refs.py assume.  The scratch is the context's BUF_GEV_*, sized in
// bytes (an fp32 driver never runs inside an fp64 one).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <string>
#include "../../include/chase_hip.h"
#include "ctx.h"
#include "kernels.h"

using namespace chase_hip;

namespace {
constexpr int NB = 64;
constexpr int SOLVE_WB = 256;        // rows per left-looking step of the left solve (64-row steps inside)
constexpr int TRAP_CB = 256;         // column block of the trapezoid updates
constexpr int POTRF_OUTER_NB = 2048; // outer_nb = 0: the fastest of 256 ... 2048 at N = 16384 (profiles/gev.txt)

inline int ept_of(int cplx) { return cplx ? 2 : 1; }
inline int imin(int a, int b) { return a < b ? a : b; }
int block_size(int asked, int dflt) { return asked == 0 ? dflt : asked; }
char norm_op(char op) { return op == 'n' ? 'N' : op == 'c' ? 'C' : op; }

struct phase_zero {                  // four-multiplication complex products while a driver of this file runs (gemm_f32_op never asks)
    chase_hip_ctx* c;
    int saved;
    explicit phase_zero(chase_hip_ctx* c_) : c(c_), saved(c_->phase) { c->phase = 0; }
    ~phase_zero() { c->phase = saved; }
};

// C = ar op(A) B + br C: fp64 through the context's GEMM, which logs and keeps the books itself ...
int gemm(chase_hip_ctx* c, int cplx, char op, int m, int n, int k, double ar, const double* A, long lda, const double* B,
         long ldb, double br, double* C, long ldc)
{
    if (m <= 0 || n <= 0) return 0;
    const double alpha[2] = {ar, 0.0}, beta[2] = {br, 0.0};
    return c->gemm(cplx != 0, op, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc);
}

// ... fp32 through gemm_f32_op, logged here under the name of chase_hip_gemm_s_op / _c_op
int gemm(chase_hip_ctx* c, int cplx, char op, int m, int n, int k, float ar, const float* A, long lda, const float* B, long ldb,
         float br, float* C, long ldc)
{
    if (m <= 0 || n <= 0) return 0;
    const float alpha[2] = {ar, 0.f}, beta[2] = {br, 0.f};
    if (c->oplog_on) c->oplog_add(cplx ? (op == 'N' ? "gemm_c_opN" : "gemm_c_opC") : (op == 'N' ? "gemm_s_opN" : "gemm_s_opC"), m, n, k, 0);
    KCHK(gemm_f32_op(c->stream, cplx != 0, op, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, c->num_cu, 0), "gemm_f32_op launch");
    return 0;
}

// B (n x nrhs) <- op(R)^{-1} B, R upper triangular n x n: 64-row steps with the inverted diagonal blocks, grouped in blocks of
// SOLVE_WB rows that first receive everything the finished rows contribute in one product with a long inner dimension
// (the scheme of chase_hip_trsm_right_upper, transposed).  op 'C' runs forward (R^H is lower triangular), op 'N' backward.
template <class T>
int trsm_left(chase_hip_ctx* c, int cplx, char op, int n, int nrhs, const T* R, long ldr, T* B, long ldb)
{
    if (n <= 0 || nrhs <= 0) return 0;
    const int e = ept_of(cplx);
    const int nblk = (n + NB - 1) / NB;
    RCCHK(c->ensure_buf(chase_hip_ctx::BUF_GEV_TINV, (size_t)nblk * NB * NB * sizeof(T) * e));
    RCCHK(c->ensure_buf(chase_hip_ctx::BUF_GEV_PANEL, (size_t)NB * nrhs * sizeof(T) * e));
    T* Tinv = (T*)c->bufs[chase_hip_ctx::BUF_GEV_TINV];
    T* P = (T*)c->bufs[chase_hip_ctx::BUF_GEV_PANEL];
    KCHK(trtri_diag(c->stream, cplx != 0, R, ldr, n, Tinv), "trtri_diag");
    if (op == 'C') {
        for (int J0 = 0; J0 < n; J0 += SOLVE_WB) {
            const int Jend = imin(n, J0 + SOLVE_WB), wb = Jend - J0;
            if (J0 > 0)          // B_J -= R[0:J0, J]^H X[0:J0, :]
                RCCHK(gemm(c, cplx, 'C', wb, nrhs, J0, T(-1), R + (long)J0 * ldr * e, ldr, B, ldb, T(1), B + (long)J0 * e, ldb));
            for (int j0 = J0; j0 < Jend; j0 += NB) {
                const int nb = imin(NB, Jend - j0);
                T* Bj = B + (long)j0 * e;
                RCCHK(gemm(c, cplx, 'C', nb, nrhs, nb, T(1), Tinv + (long)(j0 / NB) * NB * NB * e, NB, Bj, ldb, T(0), P, nb));
                KCHK(copy2d(c->stream, P, (long)nb * e, Bj, ldb * e, (long)nb * e, nrhs), "trsm_left panel copy");
                const int rest = Jend - j0 - nb;               // the block's remaining rows only
                if (rest > 0)
                    RCCHK(gemm(c, cplx, 'C', rest, nrhs, nb, T(-1), R + ((long)(j0 + nb) * ldr + j0) * e, ldr, P, nb, T(1),
                               B + (long)(j0 + nb) * e, ldb));
            }
        }
    } else {
        for (int J0 = (n - 1) / SOLVE_WB * SOLVE_WB; J0 >= 0; J0 -= SOLVE_WB) {
            const int Jend = imin(n, J0 + SOLVE_WB), wb = Jend - J0;
            if (Jend < n)        // B_J -= R[J, Jend:n] X[Jend:n, :]
                RCCHK(gemm(c, cplx, 'N', wb, nrhs, n - Jend, T(-1), R + ((long)Jend * ldr + J0) * e, ldr, B + (long)Jend * e, ldb, T(1),
                           B + (long)J0 * e, ldb));
            for (int j0 = J0 + (wb - 1) / NB * NB; j0 >= J0; j0 -= NB) {
                const int nb = imin(NB, Jend - j0);
                T* Bj = B + (long)j0 * e;
                RCCHK(gemm(c, cplx, 'N', nb, nrhs, nb, T(1), Tinv + (long)(j0 / NB) * NB * NB * e, NB, Bj, ldb, T(0), P, nb));
                KCHK(copy2d(c->stream, P, (long)nb * e, Bj, ldb * e, (long)nb * e, nrhs), "trsm_left panel copy");
                const int above = j0 - J0;                     // the block's rows above this step only
                if (above > 0)
                    RCCHK(gemm(c, cplx, 'N', above, nrhs, nb, T(-1), R + ((long)j0 * ldr + J0) * e, ldr, P, nb, T(1),
                               B + (long)J0 * e, ldb));
            }
        }
    }
    return 0;
}

// X (n x ncols) <- op(U) X in place, U upper triangular: the mirror image of trsm_left.  Blocks of SOLVE_WB rows, op 'N' from
// the top down and op 'C' from the bottom up, so that the rows a block needs from outside itself are still the old ones.
// Inside a block 64-row steps X_j <- op(U_jj) X_j (trmm_diag: the triangle in LDS, MFMA, in place - no panel buffer and no
// copy back), each followed by the rectangle inside the block; then ONE product with a long inner dimension for everything
// outside the block.
template <class T>
int trmm_left(chase_hip_ctx* c, int cplx, char op, int n, int ncols, const T* U, long ldu, T* X, long ldx)
{
    if (n <= 0 || ncols <= 0) return 0;
    const int e = ept_of(cplx);
    if (op == 'N') {
        for (int J0 = 0; J0 < n; J0 += SOLVE_WB) {
            const int Jend = imin(n, J0 + SOLVE_WB), wb = Jend - J0;
            for (int j0 = J0; j0 < Jend; j0 += NB) {
                const int nb = imin(NB, Jend - j0);
                T* Xj = X + (long)j0 * e;
                KCHK(trmm_diag(c->stream, cplx != 0, false, U + ((long)j0 * ldu + j0) * e, ldu, Xj, ldx, nb, ncols), "trmm_diag");
                const int rest = Jend - j0 - nb;               // X_j += U[j, j0+nb : Jend] X[j0+nb : Jend], rows not yet overwritten
                if (rest > 0)
                    RCCHK(gemm(c, cplx, 'N', nb, ncols, rest, T(1), U + ((long)(j0 + nb) * ldu + j0) * e, ldu,
                               X + (long)(j0 + nb) * e, ldx, T(1), Xj, ldx));
            }
            if (Jend < n)        // X_J += U[J, Jend:n] X[Jend:n, :]
                RCCHK(gemm(c, cplx, 'N', wb, ncols, n - Jend, T(1), U + ((long)Jend * ldu + J0) * e, ldu, X + (long)Jend * e, ldx, T(1),
                           X + (long)J0 * e, ldx));
        }
    } else {
        for (int J0 = (n - 1) / SOLVE_WB * SOLVE_WB; J0 >= 0; J0 -= SOLVE_WB) {
            const int Jend = imin(n, J0 + SOLVE_WB), wb = Jend - J0;
            for (int j0 = J0 + (wb - 1) / NB * NB; j0 >= J0; j0 -= NB) {
                const int nb = imin(NB, Jend - j0);
                T* Xj = X + (long)j0 * e;
                KCHK(trmm_diag(c->stream, cplx != 0, true, U + ((long)j0 * ldu + j0) * e, ldu, Xj, ldx, nb, ncols), "trmm_diag");
                const int above = j0 - J0;                     // X_j += U[J0 : j0, j]^H X[J0 : j0], rows not yet overwritten
                if (above > 0)
                    RCCHK(gemm(c, cplx, 'C', nb, ncols, above, T(1), U + ((long)j0 * ldu + J0) * e, ldu, X + (long)J0 * e, ldx, T(1),
                               Xj, ldx));
            }
            if (J0 > 0)          // X_J += U[0:J0, J]^H X[0:J0, :]
                RCCHK(gemm(c, cplx, 'C', wb, ncols, J0, T(1), U + (long)J0 * ldu * e, ldu, X, ldx, T(1), X + (long)J0 * e, ldx));
        }
    }
    return 0;
}

// A[r0 : r1, r0 : r1] -= P^H P on the upper block trapezoid, P = A[p0 : p0 + k, r0 : r1] (the rows of a finished panel), in
// column blocks: the rectangle above each diagonal block in place, the diagonal block itself through the scratch product G of
// which only the upper triangle is added - nothing below the diagonal is read or written.
template <class T>
int trapezoid_update(chase_hip_ctx* c, int cplx, T* A, long lda, int p0, int k, int r0, int r1, T* G)
{
    const int e = ept_of(cplx);
    const T* Pr = A + ((long)r0 * lda + p0) * e;
    for (int c0 = r0; c0 < r1; c0 += TRAP_CB) {
        const int cw = imin(TRAP_CB, r1 - c0);
        const T* Pc = A + ((long)c0 * lda + p0) * e;                 // the panel's columns of this block
        RCCHK(gemm(c, cplx, 'C', c0 - r0, cw, k, T(-1), Pr, lda, Pc, lda, T(1), A + ((long)c0 * lda + r0) * e, lda));
        RCCHK(gemm(c, cplx, 'C', cw, cw, k, T(-1), Pc, lda, Pc, lda, T(0), G, cw));
        KCHK(add_upper(c->stream, G, cw, A + ((long)c0 * lda + c0) * e, lda, cw, e), "trapezoid_update diagonal update");
    }
    return 0;
}

// Upper Cholesky in two levels; the strictly lower triangle of A is neither read nor written.  Per outer block of ob columns:
// the diagonal block is factorised, the row panel behind it is solved with U_JJ^H from the left, and the trailing trapezoid is
// updated with an inner dimension of ob.  The two precisions factorise the diagonal block differently and so stay apart:
// fp64 hands a scratch copy of its upper triangle to chase_hip_potrf_upper, which works on whole squares ...
int potrf_blocked(chase_hip_ctx* c, int cplx, int n, double* A, long lda, int ob)
{
    const int e = ept_of(cplx);
    const int dmax = imin(ob, n);
    RCCHK(c->ensure_buf(chase_hip_ctx::BUF_GEV_DIAG, ((size_t)dmax * dmax + (size_t)TRAP_CB * TRAP_CB) * sizeof(double) * e));
    double* D = (double*)c->bufs[chase_hip_ctx::BUF_GEV_DIAG];
    double* G = D + (size_t)dmax * dmax * e;
    for (int J0 = 0; J0 < n; J0 += ob) {
        const int w = imin(ob, n - J0);
        double* Ajj = A + ((long)J0 * lda + J0) * e;
        KCHK(copy_upper(c->stream, Ajj, lda, D, w, w, e), "potrf_blocked copy in");
        const int info = chase_hip_potrf_upper(c, cplx, w, D, w);
        if (info != 0) return info > 0 ? J0 + info : info;
        KCHK(copy_upper(c->stream, D, w, Ajj, lda, w, e), "potrf_blocked copy out");
        const int T0 = J0 + w;
        if (T0 >= n) break;
        RCCHK(trsm_left(c, cplx, 'C', w, n - T0, D, w, A + ((long)T0 * lda + J0) * e, lda));   // A[J0 : T0, T0 : n]
        RCCHK(trapezoid_update(c, cplx, A, lda, J0, w, T0, n, G));
    }
    return 0;
}

// ... fp32 factorises it in place by 64-wide steps (potf2_trtri, whose cores compute in fp64; row panel with the inverted block;
// trapezoid update inside the outer block): no fp64 copy of the block, and nothing below the diagonal is touched to begin with.
// The pivot flag lives on the device and is read once per outer block: a failure ends the factorisation there.
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
                KCHK(copy2d(c->stream, P, (long)nb * e, Ajr, lda * e, (long)nb * e, rest), "potrf_blocked panel copy");
                RCCHK(trapezoid_update(c, cplx, A, lda, j0, nb, j0 + nb, T0, G));
            }
        }
        int info = 0;
        HIPCHK(hipMemcpyAsync(&info, info_dev, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (info != 0) return info;
        if (T0 >= n) break;
        RCCHK(trsm_left(c, cplx, 'C', w, n - T0, A + ((long)J0 * lda + J0) * e, lda, A + ((long)T0 * lda + J0) * e, lda));
        RCCHK(trapezoid_update(c, cplx, A, lda, J0, w, T0, n, G));
    }
    return 0;
}

// The blocked xHEGST recurrence (itype 1, upper) on the upper triangle of A with panels of nb columns; diagonal blocks of at
// most 64 go through hegs2_diag, wider ones through this routine with nb = 64 and are completed to full Hermitian blocks,
// because the A11 U12 products read them whole.  The trapezoid update writes whole diagonal squares: what it leaves below
// the diagonal is never read again - hegs2_diag and the mirrors rebuild it from the upper triangle.
int hegst_rec(chase_hip_ctx* c, int cplx, int n, double* A, long lda, const double* U, long ldu, int nb)
{
    const int e = ept_of(cplx);
    for (int k0 = 0; k0 < n; k0 += nb) {
        const int kb = imin(nb, n - k0);
        double* A11 = A + ((long)k0 * lda + k0) * e;
        const double* U11 = U + ((long)k0 * ldu + k0) * e;
        if (kb <= NB) {
            KCHK(hegs2_diag(c->stream, cplx != 0, A11, lda, U11, ldu, kb), "hegs2_diag");
        } else {
            RCCHK(hegst_rec(c, cplx, kb, A11, lda, U11, ldu, NB));
            KCHK(mirror_upper(c->stream, A11, lda, kb, e), "mirror_upper");
        }
        const int T0 = k0 + kb, rest = n - T0;
        if (rest <= 0) break;
        double* A12 = A + ((long)T0 * lda + k0) * e;
        const double* U12 = U + ((long)T0 * ldu + k0) * e;
        RCCHK(trsm_left(c, cplx, 'C', kb, rest, U11, ldu, A12, lda));                                  // A12 <- U11^{-H} A12
        RCCHK(gemm(c, cplx, 'N', kb, rest, kb, -0.5, A11, lda, U12, ldu, 1.0, A12, lda));              // A12 -= 1/2 A11 U12
        for (int c0 = T0; c0 < n; c0 += TRAP_CB) {                                                     // A22 -= A12^H U12 + U12^H A12
            const int cw = imin(TRAP_CB, n - c0), rows = c0 + cw - T0;
            double* Ac = A + ((long)c0 * lda + T0) * e;
            RCCHK(gemm(c, cplx, 'C', rows, cw, kb, -1.0, A12, lda, U + ((long)c0 * ldu + k0) * e, ldu, 1.0, Ac, lda));
            RCCHK(gemm(c, cplx, 'C', rows, cw, kb, -1.0, U12, ldu, A + ((long)c0 * lda + k0) * e, lda, 1.0, Ac, lda));
        }
        RCCHK(gemm(c, cplx, 'N', kb, rest, kb, -0.5, A11, lda, U12, ldu, 1.0, A12, lda));              // A12 -= 1/2 A11 U12
        RCCHK(chase_hip_trsm_right_upper(c, cplx, kb, rest, U + ((long)T0 * ldu + T0) * e, ldu, A12, lda));   // A12 <- A12 U22^{-1}
    }
    return 0;
}

// ---- the head every entry point shares, in this order: NULL ctx, the context's device made current, the oplog line, `early`
// (the complaint about op / itype / factor, or nullptr), the shape, `late` (the complaint about a block size, or nullptr), the
// empty problem, NULL matrices.  RUN: the driver is to run; anything else is the entry point's return value.
constexpr int RUN = 1;

int fail(const char* name, const char* what) { return set_error(CHASE_HIP_EINVAL, (std::string(name) + ": " + what).c_str()); }

int enter(chase_hip_ctx* c, const char* name, long l0, long l1, long l2, long l3, const char* early, bool bad_shape, const char* late,
          bool empty, bool null_matrix)
{
    if (!c) return fail(name, "NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add(name, l0, l1, l2, l3);
    if (early) return fail(name, early);
    if (bad_shape) return fail(name, "bad shape");
    if (late) return fail(name, late);
    if (empty) return 0;
    if (null_matrix) return fail(name, "NULL matrix");
    return RUN;
}

// an n x n triangular U and an n x ncols block X; logged as name, n, ncols, l2, l3
int enter_block(chase_hip_ctx* c, const char* name, long l2, long l3, const char* early, int n, int ncols, const void* U, long ldu,
                const void* X, long ldx)
{
    return enter(c, name, n, ncols, l2, l3, early, n < 0 || ncols < 0 || ldu < n || ldx < n, nullptr, n == 0 || ncols == 0, !U || !X);
}

// two n x n matrices (or one, given twice); logged as name, n, l1, 0, l3
int enter_square(chase_hip_ctx* c, const char* name, long l1, long l3, const char* early, const char* late, int n, const void* A,
                 long lda, const void* U, long ldu)
{
    return enter(c, name, n, l1, 0, l3, early, n < 0 || lda < n || ldu < n, late, n == 0, !A || !U);
}

const char* bad_itype(int itype) { return itype < 1 || itype > 3 ? "itype must be 1, 2 or 3" : nullptr; }
const char* bad_factor(int factor) { return factor != 0 && factor != 1 ? "factor must be 0 or 1" : nullptr; }

// chase_hip_trsm_left_upper / chase_hip_trmm_left_upper and their _sp forms: the op is logged as given, then normalised
template <class T>
int left_upper(chase_hip_ctx* c, const char* name, bool product, int cplx, char op, int n, int ncols, const void* U, long ldu, void* X,
               long ldx)
{
    const char o = norm_op(op);
    const int rc = enter_block(c, name, op, 0, o != 'N' && o != 'C' ? "op must be 'N' or 'C'" : nullptr, n, ncols, U, ldu, X, ldx);
    if (rc != RUN) return rc;
    phase_zero pz(c);
    return product ? trmm_left(c, cplx, o, n, ncols, (const T*)U, ldu, (T*)X, ldx)
                   : trsm_left(c, cplx, o, n, ncols, (const T*)U, ldu, (T*)X, ldx);
}

// The back-transformation, X <- U^{-1} X (itype 1 and 2) or U^H X (itype 3), and its inverse, the start transform X <- U X or
// U^{-H} X.  logged: the last number of the oplog line (the itype-free entry points run itype 1 and log 0).
template <class T>
int transform(chase_hip_ctx* c, const char* name, bool start, int itype, int logged, int cplx, int n, int ncols, const void* U,
              long ldu, void* X, long ldx)
{
    const int rc = enter_block(c, name, 0, logged, bad_itype(itype), n, ncols, U, ldu, X, ldx);
    if (rc != RUN) return rc;
    phase_zero pz(c);
    const char op = itype == 3 ? 'C' : 'N';
    return start != (itype == 3) ? trmm_left(c, cplx, op, n, ncols, (const T*)U, ldu, (T*)X, ldx)
                                 : trsm_left(c, cplx, op, n, ncols, (const T*)U, ldu, (T*)X, ldx);
}
} // namespace

extern "C" {

/* B (n x nrhs, device) <- op(R)^{-1} B, R upper triangular n x n (device), op 'N' or 'C' (real data: 'C' is the transpose).
 * The strictly lower triangle of R is never read; rows beyond n are untouched. */
int chase_hip_trsm_left_upper(chase_hip_ctx* c, int cplx, char op, int n, int nrhs, const void* R, long ldr, void* B, long ldb)
{
    return left_upper<double>(c, "trsm_left_upper", false, cplx, op, n, nrhs, R, ldr, B, ldb);
}

/* X (n x ncols, device) <- op(U) X in place, U upper triangular n x n (device), op 'N' or 'C' (real data: 'C' is the transpose).
 * The diagonal is used as stored; the strictly lower triangle of U is never read; rows beyond n are untouched. */
int chase_hip_trmm_left_upper(chase_hip_ctx* c, int cplx, char op, int n, int ncols, const void* U, long ldu, void* X, long ldx)
{
    return left_upper<double>(c, "trmm_left_upper", true, cplx, op, n, ncols, U, ldu, X, ldx);
}

/* the same two on fp32 data */
int chase_hip_trsm_left_upper_sp(chase_hip_ctx* c, int cplx, char op, int n, int nrhs, const void* R, long ldr, void* B, long ldb)
{
    return left_upper<float>(c, "trsm_left_upper_sp", false, cplx, op, n, nrhs, R, ldr, B, ldb);
}

int chase_hip_trmm_left_upper_sp(chase_hip_ctx* c, int cplx, char op, int n, int ncols, const void* U, long ldu, void* X, long ldx)
{
    return left_upper<float>(c, "trmm_left_upper_sp", true, cplx, op, n, ncols, U, ldu, X, ldx);
}

/* In-place upper Cholesky A = U^H U with the result contract and info of chase_hip_potrf_upper, except that the strictly lower
 * triangle is neither read nor written.  outer_nb: columns per outer block, a positive multiple of 64 (0: the default). */
int chase_hip_potrf_upper_blocked(chase_hip_ctx* c, int cplx, int n, void* A, long lda, int outer_nb)
{
    const int rc = enter_square(c, "potrf_upper_blocked", outer_nb, 0, nullptr,
                                outer_nb < 0 || outer_nb % NB ? "outer_nb must be 0 or a multiple of 64" : nullptr, n, A, lda, A, lda);
    if (rc != RUN) return rc;
    phase_zero pz(c);
    return potrf_blocked(c, cplx, n, (double*)A, lda, block_size(outer_nb, POTRF_OUTER_NB));
}

/* The same on an fp32 matrix: info > 0 is the first non-positive pivot.  The outer diagonal blocks are factorised in place
 * (64-wide steps whose cores compute in fp64), not on an fp64 scratch copy. */
int chase_hip_potrf_upper_blocked_sp(chase_hip_ctx* c, int cplx, int n, void* A, long lda, int outer_nb)
{
    const int rc = enter_square(c, "potrf_upper_blocked_sp", outer_nb, 0, nullptr,
                                outer_nb < 0 || outer_nb % NB ? "outer_nb must be 0 or a multiple of 64" : nullptr, n, A, lda, A, lda);
    if (rc != RUN) return rc;
    phase_zero pz(c);
    return potrf_blocked(c, cplx, n, (float*)A, lda, block_size(outer_nb, POTRF_OUTER_NB));
}

/* A <- U^{-H} A U^{-1} (LAPACK xHEGST, itype 1, uplo 'U'): A Hermitian, read from its upper triangle only; U upper triangular,
 * its strictly lower triangle never read.  On return both triangles of A hold the result, the lower one the bitwise conjugate
 * of the upper one, the imaginary diagonal +0.  n <= 64: hegs2_diag.  nb > 0 (a multiple of 64): the blocked xHEGST recurrence
 * with panels of nb columns.  nb = 0: the formulation that measured fastest, two full triangular solves.  (Not shared with the
 * fp32 form below: only this one has the recurrence, and its default solves once from the right.) */
int chase_hip_hegst_upper(chase_hip_ctx* c, int cplx, int n, void* A, long lda, const void* U, long ldu, int nb)
{
    const int rc = enter_square(c, "hegst_upper", nb, 0, nullptr, nb < 0 || nb % NB ? "nb must be 0 or a multiple of 64" : nullptr, n, A,
                                lda, U, ldu);
    if (rc != RUN) return rc;
    phase_zero pz(c);
    const int e = ept_of(cplx);
    if (n <= NB) {
        KCHK(hegs2_diag(c->stream, cplx != 0, (double*)A, lda, (const double*)U, ldu, n), "hegs2_diag");
    } else if (nb == 0) {
        // the default: two full solves on the completed matrix, (A U^{-1}) then U^{-H} (.).  Twice the flops of the recurrence,
        // all of them in products with long inner dimensions: 539 ms against 1056 ms (nb = 512) at N = 16384 complex
        // (profiles/gev.txt).  One triangle of the result is kept and mirrored, so the matrix is Hermitian bit for bit.
        KCHK(mirror_upper(c->stream, (double*)A, lda, n, e), "mirror_upper");
        RCCHK(chase_hip_trsm_right_upper(c, cplx, n, n, U, ldu, A, lda));
        RCCHK(trsm_left(c, cplx, 'C', n, n, (const double*)U, ldu, (double*)A, lda));
        KCHK(mirror_lower(c->stream, (double*)A, lda, n, e, 1), "mirror_lower");
    } else {
        RCCHK(hegst_rec(c, cplx, n, (double*)A, lda, (const double*)U, ldu, nb));
        KCHK(mirror_upper(c->stream, (double*)A, lda, n, e), "mirror_upper");
    }
    return 0;
}

/* A <- U^{-H} A U^{-1} on fp32 data with the argument and result contract of chase_hip_hegst_upper (nb = 0).  n <= 64:
 * hegs2_diag.  Above, the right solve A U^{-1} is a left solve on the conjugate transpose, U^{-H} (U^{-H} A)^H = U^{-H} A U^{-1}
 * for Hermitian A: one solve routine instead of two, and both solves run the op C product whose operands are read k-contiguous. */
int chase_hip_hegst_upper_sp(chase_hip_ctx* c, int cplx, int n, void* A, long lda, const void* U, long ldu)
{
    const int rc = enter_square(c, "hegst_upper_sp", 0, 0, nullptr, nullptr, n, A, lda, U, ldu);
    if (rc != RUN) return rc;
    phase_zero pz(c);
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

/* A <- U A U^H (LAPACK xHEGST, itype 2 / 3, uplo 'U') with the argument and result contract of chase_hip_hegst_upper: two left
 * products on the completed matrix with an in-place conjugate transpose between them, U (U A)^H = U A U^H for Hermitian A;
 * the lower triangle of the result is kept and mirrored. */
int chase_hip_hegst_product_upper(chase_hip_ctx* c, int cplx, int n, void* A, long lda, const void* U, long ldu)
{
    const int rc = enter_square(c, "hegst_product_upper", 0, 0, nullptr, nullptr, n, A, lda, U, ldu);
    if (rc != RUN) return rc;
    phase_zero pz(c);
    const int e = ept_of(cplx);
    KCHK(mirror_upper(c->stream, (double*)A, lda, n, e), "mirror_upper");
    RCCHK(trmm_left(c, cplx, 'N', n, n, (const double*)U, ldu, (double*)A, lda));
    KCHK(conj_transpose_inplace(c->stream, cplx != 0, (double*)A, lda, n), "conj_transpose_inplace");
    RCCHK(trmm_left(c, cplx, 'N', n, n, (const double*)U, ldu, (double*)A, lda));
    KCHK(mirror_lower(c->stream, (double*)A, lda, n, e, 1), "mirror_lower");
    return 0;
}

/* The reduction of A x = lambda S x to standard form: S <- U (upper Cholesky factor, strictly lower triangle untouched), then
 * A <- U^{-H} A U^{-1}.  Returns the potrf info > 0 when S is not positive definite; A is then untouched. */
int chase_hip_gev_reduce(chase_hip_ctx* c, int cplx, int n, void* A, long lda, void* S, long lds_)
{
    const int rc = enter_square(c, "gev_reduce", 0, 0, nullptr, nullptr, n, A, lda, S, lds_);
    if (rc != RUN) return rc;
    const int info = chase_hip_potrf_upper_blocked(c, cplx, n, S, lds_, 0);
    if (info != 0) return info;
    return chase_hip_hegst_upper(c, cplx, n, A, lda, S, lds_, 0);
}

/* gev_reduce for the three LAPACK problem types: itype 1, H x = lambda S x, A <- U^{-H} A U^{-1}; itype 2, H S x = lambda x, and
 * itype 3, S H x = lambda x, A <- U A U^H.  factor = 1: S <- U first, as gev_reduce does (itype 1, factor 1 IS gev_reduce);
 * factor = 0: S already holds U from an earlier call and only the two-sided step runs. */
int chase_hip_gev_reduce_itype(chase_hip_ctx* c, int cplx, int itype, int factor, int n, void* A, long lda, void* S, long lds_)
{
    const char* early = bad_itype(itype);
    if (!early) early = bad_factor(factor);
    const int rc = enter_square(c, "gev_reduce_itype", itype, factor, early, nullptr, n, A, lda, S, lds_);
    if (rc != RUN) return rc;
    if (factor) {
        const int info = chase_hip_potrf_upper_blocked(c, cplx, n, S, lds_, 0);
        if (info != 0) return info;
    }
    return itype == 1 ? chase_hip_hegst_upper(c, cplx, n, A, lda, S, lds_, 0) : chase_hip_hegst_product_upper(c, cplx, n, A, lda, S, lds_);
}

/* chase_hip_gev_reduce_itype (itype 1) on fp32 data: factor = 1, S <- U first; factor = 0, S already holds U.  Returns the
 * potrf info > 0 when S is not positive definite; A is then untouched. */
int chase_hip_gev_reduce_sp(chase_hip_ctx* c, int cplx, int factor, int n, void* A, long lda, void* S, long lds_)
{
    const int rc = enter_square(c, "gev_reduce_sp", 0, factor, bad_factor(factor), nullptr, n, A, lda, S, lds_);
    if (rc != RUN) return rc;
    if (factor) {
        const int info = chase_hip_potrf_upper_blocked_sp(c, cplx, n, S, lds_, 0);
        if (info != 0) return info;
    }
    return chase_hip_hegst_upper_sp(c, cplx, n, A, lda, S, lds_);
}

/* X (n x ncols) <- U^{-1} X: eigenvectors of the reduced problem to those of the generalized one */
int chase_hip_gev_backtransform(chase_hip_ctx* c, int cplx, int n, int ncols, const void* U, long ldu, void* X, long ldx)
{
    return transform<double>(c, "gev_backtransform", false, 1, 0, cplx, n, ncols, U, ldu, X, ldx);
}

/* X (n x ncols) <- U^{-1} X (itype 1 and 2) or U^H X (itype 3): eigenvectors of the reduced problem to those of the pencil */
int chase_hip_gev_backtransform_itype(chase_hip_ctx* c, int cplx, int itype, int n, int ncols, const void* U, long ldu, void* X,
                                      long ldx)
{
    return transform<double>(c, "gev_backtransform_itype", false, itype, itype, cplx, n, ncols, U, ldu, X, ldx);
}

/* The inverse of gev_backtransform_itype, X (n x ncols) <- U X (itype 1 and 2) or U^{-H} X (itype 3): approximate eigenvectors
 * of the pencil become a start block of the reduced problem */
int chase_hip_gev_starttransform(chase_hip_ctx* c, int cplx, int itype, int n, int ncols, const void* U, long ldu, void* X, long ldx)
{
    return transform<double>(c, "gev_starttransform", true, itype, itype, cplx, n, ncols, U, ldu, X, ldx);
}

/* X (n x ncols, fp32) <- U^{-1} X, and its inverse X <- U X */
int chase_hip_gev_backtransform_sp(chase_hip_ctx* c, int cplx, int n, int ncols, const void* U, long ldu, void* X, long ldx)
{
    return transform<float>(c, "gev_backtransform_sp", false, 1, 0, cplx, n, ncols, U, ldu, X, ldx);
}

int chase_hip_gev_starttransform_sp(chase_hip_ctx* c, int cplx, int n, int ncols, const void* U, long ldu, void* X, long ldx)
{
    return transform<float>(c, "gev_starttransform_sp", true, 1, 0, cplx, n, ncols, U, ldu, X, ldx);
}

} // extern "C"
