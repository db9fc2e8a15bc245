// capi_gev.hip — C ABI entry points of the generalized Hermitian-definite problem H x = lambda S x on one GPU
// (include/chase_hip.h): the left triangular solve, the two-level Cholesky that leaves the strictly lower triangle alone, the
// two-sided reduction C = U^{-H} H U^{-1} and the back-transformation X = U^{-1} Y.  They replace the three ScaLAPACK calls
// (ppotrf, phegst, ptrtrs) the reference's docs/example/gev.rst puts around chase::Solve.  For sequences of pencils and LAPACK's
// problem types 2 and 3: the triangular product X <- op(U) X, C = U H U^H, the itype-aware reduction and back-transformation and
// the start transform that makes the previous pencil's eigenvectors the start block of the next reduced problem.
//
// Every O(n^3) flop goes through the context's MFMA GEMM; the cores are potf2_trtri / trtri_diag (factor_kernels.hip), hegs2_diag
// and the 64-row MFMA step of the triangular product, trmm_diag (gev_kernels.hip).  The context's phase is 0 while these run: complex products take four multiplications,
// which is what the componentwise bounds of tests/gev_refs.py assume.
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
constexpr int POTRF_OUTER_NB = 2048; // outer_nb = 0: the fastest of 256 ... 2048 at N = 16384 (profiles/gev.txt)

inline int ept_of(int cplx) { return cplx ? 2 : 1; }
inline int imin(int a, int b) { return a < b ? a : b; }

struct phase_zero {                  // four-multiplication complex products while a driver of this file runs
    chase_hip_ctx* c;
    int saved;
    explicit phase_zero(chase_hip_ctx* c_) : c(c_), saved(c_->phase) { c->phase = 0; }
    ~phase_zero() { c->phase = saved; }
};

int gemm(chase_hip_ctx* c, int cplx, char op, int m, int n, int k, double ar, const double* A, long lda, const double* B,
         long ldb, double br, double* C, long ldc)
{
    if (m <= 0 || n <= 0) return 0;
    const double alpha[2] = {ar, 0.0}, beta[2] = {br, 0.0};
    return c->gemm(cplx != 0, op, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc);
}

// B (n x nrhs) <- op(R)^{-1} B, R upper triangular n x n: 64-row steps with the inverted diagonal blocks, grouped in blocks of
// SOLVE_WB rows that first receive everything the finished rows contribute in one product with a long inner dimension
// (the scheme of chase_hip_trsm_right_upper, transposed).  op 'C' runs forward (R^H is lower triangular), op 'N' backward.
int trsm_left(chase_hip_ctx* c, int cplx, char op, int n, int nrhs, const double* R, long ldr, double* B, long ldb)
{
    if (n <= 0 || nrhs <= 0) return 0;
    const int e = ept_of(cplx);
    const int nblk = (n + NB - 1) / NB;
    RCCHK(c->ensure_buf(chase_hip_ctx::BUF_GEV_TINV, (size_t)nblk * NB * NB * sizeof(double) * e));
    RCCHK(c->ensure_buf(chase_hip_ctx::BUF_GEV_PANEL, (size_t)NB * nrhs * sizeof(double) * e));
    double* Tinv = (double*)c->bufs[chase_hip_ctx::BUF_GEV_TINV];
    double* P = (double*)c->bufs[chase_hip_ctx::BUF_GEV_PANEL];
    KCHK(trtri_diag(c->stream, cplx != 0, R, ldr, n, Tinv), "trtri_diag");
    if (op == 'C') {
        for (int J0 = 0; J0 < n; J0 += SOLVE_WB) {
            const int Jend = imin(n, J0 + SOLVE_WB), wb = Jend - J0;
            if (J0 > 0)          // B_J -= R[0:J0, J]^H X[0:J0, :]
                RCCHK(gemm(c, cplx, 'C', wb, nrhs, J0, -1.0, R + (long)J0 * ldr * e, ldr, B, ldb, 1.0, B + (long)J0 * e, ldb));
            for (int j0 = J0; j0 < Jend; j0 += NB) {
                const int nb = imin(NB, Jend - j0);
                double* Bj = B + (long)j0 * e;
                RCCHK(gemm(c, cplx, 'C', nb, nrhs, nb, 1.0, Tinv + (long)(j0 / NB) * NB * NB * e, NB, Bj, ldb, 0.0, P, nb));
                KCHK(copy2d(c->stream, P, (long)nb * e, Bj, ldb * e, (long)nb * e, nrhs), "trsm_left panel copy");
                const int rest = Jend - j0 - nb;               // the block's remaining rows only
                if (rest > 0)
                    RCCHK(gemm(c, cplx, 'C', rest, nrhs, nb, -1.0, R + ((long)(j0 + nb) * ldr + j0) * e, ldr, P, nb, 1.0,
                               B + (long)(j0 + nb) * e, ldb));
            }
        }
    } else {
        for (int J0 = (n - 1) / SOLVE_WB * SOLVE_WB; J0 >= 0; J0 -= SOLVE_WB) {
            const int Jend = imin(n, J0 + SOLVE_WB), wb = Jend - J0;
            if (Jend < n)        // B_J -= R[J, Jend:n] X[Jend:n, :]
                RCCHK(gemm(c, cplx, 'N', wb, nrhs, n - Jend, -1.0, R + ((long)Jend * ldr + J0) * e, ldr, B + (long)Jend * e, ldb, 1.0,
                           B + (long)J0 * e, ldb));
            for (int j0 = J0 + (wb - 1) / NB * NB; j0 >= J0; j0 -= NB) {
                const int nb = imin(NB, Jend - j0);
                double* Bj = B + (long)j0 * e;
                RCCHK(gemm(c, cplx, 'N', nb, nrhs, nb, 1.0, Tinv + (long)(j0 / NB) * NB * NB * e, NB, Bj, ldb, 0.0, P, nb));
                KCHK(copy2d(c->stream, P, (long)nb * e, Bj, ldb * e, (long)nb * e, nrhs), "trsm_left panel copy");
                const int above = j0 - J0;                     // the block's rows above this step only
                if (above > 0)
                    RCCHK(gemm(c, cplx, 'N', above, nrhs, nb, -1.0, R + ((long)j0 * ldr + J0) * e, ldr, P, nb, 1.0,
                               B + (long)J0 * e, ldb));
            }
        }
    }
    return 0;
}

// X (n x ncols) <- op(U) X in place, U upper triangular: the mirror image of trsm_left.  Blocks of SOLVE_WB rows, op 'N' from
// the top down and op 'C' from the bottom up, so that the rows a block needs from outside itself are still the old ones.
// Inside a block 64-row steps X_j <- op(U_jj) X_j (trmm_diag: the triangle in LDS, f64 MFMA, in place - no panel buffer and no
// copy back), each followed by the rectangle inside the block; then ONE product with a long inner dimension for everything
// outside the block.
int trmm_left(chase_hip_ctx* c, int cplx, char op, int n, int ncols, const double* U, long ldu, double* X, long ldx)
{
    if (n <= 0 || ncols <= 0) return 0;
    const int e = ept_of(cplx);
    if (op == 'N') {
        for (int J0 = 0; J0 < n; J0 += SOLVE_WB) {
            const int Jend = imin(n, J0 + SOLVE_WB), wb = Jend - J0;
            for (int j0 = J0; j0 < Jend; j0 += NB) {
                const int nb = imin(NB, Jend - j0);
                double* Xj = X + (long)j0 * e;
                KCHK(trmm_diag(c->stream, cplx != 0, false, U + ((long)j0 * ldu + j0) * e, ldu, Xj, ldx, nb, ncols), "trmm_diag");
                const int rest = Jend - j0 - nb;               // X_j += U[j, j0+nb : Jend] X[j0+nb : Jend], rows not yet overwritten
                if (rest > 0)
                    RCCHK(gemm(c, cplx, 'N', nb, ncols, rest, 1.0, U + ((long)(j0 + nb) * ldu + j0) * e, ldu,
                               X + (long)(j0 + nb) * e, ldx, 1.0, Xj, ldx));
            }
            if (Jend < n)        // X_J += U[J, Jend:n] X[Jend:n, :]
                RCCHK(gemm(c, cplx, 'N', wb, ncols, n - Jend, 1.0, U + ((long)Jend * ldu + J0) * e, ldu, X + (long)Jend * e, ldx, 1.0,
                           X + (long)J0 * e, ldx));
        }
    } else {
        for (int J0 = (n - 1) / SOLVE_WB * SOLVE_WB; J0 >= 0; J0 -= SOLVE_WB) {
            const int Jend = imin(n, J0 + SOLVE_WB), wb = Jend - J0;
            for (int j0 = J0 + (wb - 1) / NB * NB; j0 >= J0; j0 -= NB) {
                const int nb = imin(NB, Jend - j0);
                double* Xj = X + (long)j0 * e;
                KCHK(trmm_diag(c->stream, cplx != 0, true, U + ((long)j0 * ldu + j0) * e, ldu, Xj, ldx, nb, ncols), "trmm_diag");
                const int above = j0 - J0;                     // X_j += U[J0 : j0, j]^H X[J0 : j0], rows not yet overwritten
                if (above > 0)
                    RCCHK(gemm(c, cplx, 'C', nb, ncols, above, 1.0, U + ((long)j0 * ldu + J0) * e, ldu, X + (long)J0 * e, ldx, 1.0,
                               Xj, ldx));
            }
            if (J0 > 0)          // X_J += U[0:J0, J]^H X[0:J0, :]
                RCCHK(gemm(c, cplx, 'C', wb, ncols, J0, 1.0, U + (long)J0 * ldu * e, ldu, X, ldx, 1.0, X + (long)J0 * e, ldx));
        }
    }
    return 0;
}

// Upper Cholesky in two levels; the strictly lower triangle of A is neither read nor written.  Per outer block of ob columns:
// the diagonal block is factorised by chase_hip_potrf_upper on a scratch copy of its upper triangle, the row panel is solved
// with U_JJ^H from the left, and the trailing update A_rr -= P^H P runs on the upper block trapezoid in column blocks - the
// rectangle above each diagonal block in place, the diagonal block itself through a scratch product of which only the upper
// triangle is added.
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
        const int T0 = J0 + w, rest = n - T0;
        if (rest <= 0) break;
        double* Ajr = A + ((long)T0 * lda + J0) * e;                   // A[J0 : T0, T0 : n]
        RCCHK(trsm_left(c, cplx, 'C', w, rest, D, w, Ajr, lda));
        for (int c0 = T0; c0 < n; c0 += TRAP_CB) {
            const int cw = imin(TRAP_CB, n - c0);
            const double* Pc = A + ((long)c0 * lda + J0) * e;          // the panel's columns of this block
            RCCHK(gemm(c, cplx, 'C', c0 - T0, cw, w, -1.0, Ajr, lda, Pc, lda, 1.0, A + ((long)c0 * lda + T0) * e, lda));
            RCCHK(gemm(c, cplx, 'C', cw, cw, w, -1.0, Pc, lda, Pc, lda, 0.0, G, cw));
            KCHK(add_upper(c->stream, G, cw, A + ((long)c0 * lda + c0) * e, lda, cw, e), "potrf_blocked diagonal update");
        }
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

int block_size(int asked, int dflt) { return asked == 0 ? dflt : asked; }
} // namespace

extern "C" {

/* B (n x nrhs, device) <- op(R)^{-1} B, R upper triangular n x n (device), op 'N' or 'C' (real data: 'C' is the transpose).
 * The strictly lower triangle of R is never read; rows beyond n are untouched. */
int chase_hip_trsm_left_upper(chase_hip_ctx* c, int cplx, char op, int n, int nrhs, const void* R, long ldr, void* B, long ldb)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "trsm_left_upper: NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add("trsm_left_upper", n, nrhs, op, 0);
    if (op == 'n') op = 'N';
    if (op == 'c') op = 'C';
    if (op != 'N' && op != 'C') return set_error(CHASE_HIP_EINVAL, "trsm_left_upper: op must be 'N' or 'C'");
    if (n < 0 || nrhs < 0 || ldr < n || ldb < n) return set_error(CHASE_HIP_EINVAL, "trsm_left_upper: bad shape");
    if (n == 0 || nrhs == 0) return 0;
    if (!R || !B) return set_error(CHASE_HIP_EINVAL, "trsm_left_upper: NULL matrix");
    phase_zero pz(c);
    return trsm_left(c, cplx, op, n, nrhs, (const double*)R, ldr, (double*)B, ldb);
}

/* In-place upper Cholesky A = U^H U with the result contract and info of chase_hip_potrf_upper, except that the strictly lower
 * triangle is neither read nor written.  outer_nb: columns per outer block, a positive multiple of 64 (0: the default). */
int chase_hip_potrf_upper_blocked(chase_hip_ctx* c, int cplx, int n, void* A, long lda, int outer_nb)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "potrf_upper_blocked: NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add("potrf_upper_blocked", n, outer_nb, 0, 0);
    if (n < 0 || lda < n) return set_error(CHASE_HIP_EINVAL, "potrf_upper_blocked: bad shape");
    if (outer_nb < 0 || outer_nb % NB) return set_error(CHASE_HIP_EINVAL, "potrf_upper_blocked: outer_nb must be 0 or a multiple of 64");
    if (n == 0) return 0;
    if (!A) return set_error(CHASE_HIP_EINVAL, "potrf_upper_blocked: NULL matrix");
    phase_zero pz(c);
    return potrf_blocked(c, cplx, n, (double*)A, lda, block_size(outer_nb, POTRF_OUTER_NB));
}

/* A <- U^{-H} A U^{-1} (LAPACK xHEGST, itype 1, uplo 'U'): A Hermitian, read from its upper triangle only; U upper triangular,
 * its strictly lower triangle never read.  On return both triangles of A hold the result, the lower one the bitwise conjugate
 * of the upper one, the imaginary diagonal +0.  n <= 64: hegs2_diag.  nb > 0 (a multiple of 64): the blocked xHEGST recurrence
 * with panels of nb columns.  nb = 0: the formulation that measured fastest, two full triangular solves. */
int chase_hip_hegst_upper(chase_hip_ctx* c, int cplx, int n, void* A, long lda, const void* U, long ldu, int nb)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "hegst_upper: NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add("hegst_upper", n, nb, 0, 0);
    if (n < 0 || lda < n || ldu < n) return set_error(CHASE_HIP_EINVAL, "hegst_upper: bad shape");
    if (nb < 0 || nb % NB) return set_error(CHASE_HIP_EINVAL, "hegst_upper: nb must be 0 or a multiple of 64");
    if (n == 0) return 0;
    if (!A || !U) return set_error(CHASE_HIP_EINVAL, "hegst_upper: NULL matrix");
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

/* The reduction of A x = lambda S x to standard form: S <- U (upper Cholesky factor, strictly lower triangle untouched), then
 * A <- U^{-H} A U^{-1}.  Returns the potrf info > 0 when S is not positive definite; A is then untouched. */
int chase_hip_gev_reduce(chase_hip_ctx* c, int cplx, int n, void* A, long lda, void* S, long lds_)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "gev_reduce: NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add("gev_reduce", n, 0, 0, 0);
    if (n < 0 || lda < n || lds_ < n) return set_error(CHASE_HIP_EINVAL, "gev_reduce: bad shape");
    if (n == 0) return 0;
    if (!A || !S) return set_error(CHASE_HIP_EINVAL, "gev_reduce: NULL matrix");
    const int info = chase_hip_potrf_upper_blocked(c, cplx, n, S, lds_, 0);
    if (info != 0) return info;
    return chase_hip_hegst_upper(c, cplx, n, A, lda, S, lds_, 0);
}

/* X (n x ncols) <- U^{-1} X: eigenvectors of the reduced problem to those of the generalized one */
int chase_hip_gev_backtransform(chase_hip_ctx* c, int cplx, int n, int ncols, const void* U, long ldu, void* X, long ldx)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "gev_backtransform: NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add("gev_backtransform", n, ncols, 0, 0);
    if (n < 0 || ncols < 0 || ldu < n || ldx < n) return set_error(CHASE_HIP_EINVAL, "gev_backtransform: bad shape");
    if (n == 0 || ncols == 0) return 0;
    if (!U || !X) return set_error(CHASE_HIP_EINVAL, "gev_backtransform: NULL matrix");
    phase_zero pz(c);
    return trsm_left(c, cplx, 'N', n, ncols, (const double*)U, ldu, (double*)X, ldx);
}

/* X (n x ncols, device) <- op(U) X in place, U upper triangular n x n (device), op 'N' or 'C' (real data: 'C' is the transpose).
 * The diagonal is used as stored; the strictly lower triangle of U is never read; rows beyond n are untouched. */
int chase_hip_trmm_left_upper(chase_hip_ctx* c, int cplx, char op, int n, int ncols, const void* U, long ldu, void* X, long ldx)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "trmm_left_upper: NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add("trmm_left_upper", n, ncols, op, 0);
    if (op == 'n') op = 'N';
    if (op == 'c') op = 'C';
    if (op != 'N' && op != 'C') return set_error(CHASE_HIP_EINVAL, "trmm_left_upper: op must be 'N' or 'C'");
    if (n < 0 || ncols < 0 || ldu < n || ldx < n) return set_error(CHASE_HIP_EINVAL, "trmm_left_upper: bad shape");
    if (n == 0 || ncols == 0) return 0;
    if (!U || !X) return set_error(CHASE_HIP_EINVAL, "trmm_left_upper: NULL matrix");
    phase_zero pz(c);
    return trmm_left(c, cplx, op, n, ncols, (const double*)U, ldu, (double*)X, ldx);
}

/* A <- U A U^H (LAPACK xHEGST, itype 2 / 3, uplo 'U') with the argument and result contract of chase_hip_hegst_upper: two left
 * products on the completed matrix with an in-place conjugate transpose between them, U (U A)^H = U A U^H for Hermitian A;
 * the lower triangle of the result is kept and mirrored. */
int chase_hip_hegst_product_upper(chase_hip_ctx* c, int cplx, int n, void* A, long lda, const void* U, long ldu)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "hegst_product_upper: NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add("hegst_product_upper", n, 0, 0, 0);
    if (n < 0 || lda < n || ldu < n) return set_error(CHASE_HIP_EINVAL, "hegst_product_upper: bad shape");
    if (n == 0) return 0;
    if (!A || !U) return set_error(CHASE_HIP_EINVAL, "hegst_product_upper: NULL matrix");
    phase_zero pz(c);
    const int e = ept_of(cplx);
    KCHK(mirror_upper(c->stream, (double*)A, lda, n, e), "mirror_upper");
    RCCHK(trmm_left(c, cplx, 'N', n, n, (const double*)U, ldu, (double*)A, lda));
    KCHK(conj_transpose_inplace(c->stream, cplx != 0, (double*)A, lda, n), "conj_transpose_inplace");
    RCCHK(trmm_left(c, cplx, 'N', n, n, (const double*)U, ldu, (double*)A, lda));
    KCHK(mirror_lower(c->stream, (double*)A, lda, n, e, 1), "mirror_lower");
    return 0;
}

/* gev_reduce for the three LAPACK problem types: itype 1, H x = lambda S x, A <- U^{-H} A U^{-1}; itype 2, H S x = lambda x, and
 * itype 3, S H x = lambda x, A <- U A U^H.  factor = 1: S <- U first, as gev_reduce does (itype 1, factor 1 IS gev_reduce);
 * factor = 0: S already holds U from an earlier call and only the two-sided step runs. */
int chase_hip_gev_reduce_itype(chase_hip_ctx* c, int cplx, int itype, int factor, int n, void* A, long lda, void* S, long lds_)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "gev_reduce_itype: NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add("gev_reduce_itype", n, itype, 0, factor);
    if (itype < 1 || itype > 3) return set_error(CHASE_HIP_EINVAL, "gev_reduce_itype: itype must be 1, 2 or 3");
    if (factor != 0 && factor != 1) return set_error(CHASE_HIP_EINVAL, "gev_reduce_itype: factor must be 0 or 1");
    if (n < 0 || lda < n || lds_ < n) return set_error(CHASE_HIP_EINVAL, "gev_reduce_itype: bad shape");
    if (n == 0) return 0;
    if (!A || !S) return set_error(CHASE_HIP_EINVAL, "gev_reduce_itype: NULL matrix");
    if (factor) {
        const int info = chase_hip_potrf_upper_blocked(c, cplx, n, S, lds_, 0);
        if (info != 0) return info;
    }
    return itype == 1 ? chase_hip_hegst_upper(c, cplx, n, A, lda, S, lds_, 0) : chase_hip_hegst_product_upper(c, cplx, n, A, lda, S, lds_);
}

/* X (n x ncols) <- U^{-1} X (itype 1 and 2) or U^H X (itype 3): eigenvectors of the reduced problem to those of the pencil */
int chase_hip_gev_backtransform_itype(chase_hip_ctx* c, int cplx, int itype, int n, int ncols, const void* U, long ldu, void* X,
                                      long ldx)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "gev_backtransform_itype: NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add("gev_backtransform_itype", n, ncols, 0, itype);
    if (itype < 1 || itype > 3) return set_error(CHASE_HIP_EINVAL, "gev_backtransform_itype: itype must be 1, 2 or 3");
    if (n < 0 || ncols < 0 || ldu < n || ldx < n) return set_error(CHASE_HIP_EINVAL, "gev_backtransform_itype: bad shape");
    if (n == 0 || ncols == 0) return 0;
    if (!U || !X) return set_error(CHASE_HIP_EINVAL, "gev_backtransform_itype: NULL matrix");
    phase_zero pz(c);
    return itype == 3 ? trmm_left(c, cplx, 'C', n, ncols, (const double*)U, ldu, (double*)X, ldx)
                      : trsm_left(c, cplx, 'N', n, ncols, (const double*)U, ldu, (double*)X, ldx);
}

/* The inverse of gev_backtransform_itype, X (n x ncols) <- U X (itype 1 and 2) or U^{-H} X (itype 3): approximate eigenvectors
 * of the pencil become a start block of the reduced problem */
int chase_hip_gev_starttransform(chase_hip_ctx* c, int cplx, int itype, int n, int ncols, const void* U, long ldu, void* X, long ldx)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "gev_starttransform: NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add("gev_starttransform", n, ncols, 0, itype);
    if (itype < 1 || itype > 3) return set_error(CHASE_HIP_EINVAL, "gev_starttransform: itype must be 1, 2 or 3");
    if (n < 0 || ncols < 0 || ldu < n || ldx < n) return set_error(CHASE_HIP_EINVAL, "gev_starttransform: bad shape");
    if (n == 0 || ncols == 0) return 0;
    if (!U || !X) return set_error(CHASE_HIP_EINVAL, "gev_starttransform: NULL matrix");
    phase_zero pz(c);
    return itype == 3 ? trsm_left(c, cplx, 'C', n, ncols, (const double*)U, ldu, (double*)X, ldx)
                      : trmm_left(c, cplx, 'N', n, ncols, (const double*)U, ldu, (double*)X, ldx);
}

} // extern "C"
