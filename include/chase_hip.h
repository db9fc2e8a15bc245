/* chase_hip.h — C ABI of the MI355X-native ChASE hot-path backend (libchase_hip.so)
 *
 * Boundary: the reference solver talks to a backend ONLY through the virtuals of
 * chase::ChaseBase<T> (/root/reference algorithm/interface.hpp:46-434).  This header is the thin C ABI the
 * C++ Impl class (chase_amd/host/chase_hip_impl.hpp) calls, and what a ChASE maintainer would bind from an
 * Impl/chase_hip plugin (INTEGRATION.md shows the stub).  Plain pointers and sizes only, no C++/torch types.
 *
 * Conventions
 *   - every entry point returns int: 0 = ok, >0 = LAPACK-style info (potrf), <0 = runtime error
 *     (CHASE_HIP_E* or -(hipError_t)); no exceptions cross the ABI.  chase_hip_last_error() gives text.
 *   - matrices are column-major; complex = interleaved (re,im) doubles ("z" entry points take void* / double[2]).
 *   - "dev" pointers are HIP device pointers; "host" pointers are ordinary host memory.
 *   - all device work is enqueued on the context's HIP stream; entry points that return scalars to the host
 *     synchronise that stream themselves, the others are asynchronous.
 *   - arguments are checked on the host before anything is enqueued: a negative extent, a leading dimension smaller than the
 *     row count or a NULL matrix / index list of a non-empty operand is CHASE_HIP_EINVAL.  An empty operand (n == 0) returns 0
 *     whatever its pointers; the column kernels accept m == 0 with n > 0 (a rank without local rows: dots and norms are 0).
 */
#ifndef CHASE_HIP_H
#define CHASE_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHASE_HIP_OK 0
#define CHASE_HIP_EINVAL (-1001)   /* bad argument (shape, pointer, op) */
#define CHASE_HIP_ENODEV (-1002)   /* no usable HIP device / wrong architecture */
#define CHASE_HIP_ENOMEM (-1003)
#define CHASE_HIP_ENOTCONV (-1004) /* host eigensolver / iteration failed to converge */
#define CHASE_HIP_ECOMM (-1005)    /* RCCL / transport error */
#define CHASE_HIP_ELAPACK (-1006)  /* host LAPACK provider missing */
#define CHASE_HIP_EIO (-1007)      /* matrix file missing, too small or unreadable */

typedef struct chase_hip_ctx chase_hip_ctx;

/* ---- context -------------------------------------------------------------------------------------------------- */
/* device: HIP ordinal.  stream: an existing hipStream_t to enqueue on (e.g. torch's current stream) or NULL to let the
 * context create its own non-blocking stream. */
int chase_hip_ctx_create(chase_hip_ctx** out, int device, void* stream);
int chase_hip_ctx_destroy(chase_hip_ctx* ctx);
int chase_hip_ctx_sync(chase_hip_ctx* ctx);
void* chase_hip_ctx_stream(chase_hip_ctx* ctx);
/* Operator log: with on != 0 every C-ABI operator this context executes afterwards is listed as one line "name a b c d" (its
 * name and shapes; no pointers, no scalars), '\n'-separated in chase_hip_ctx_oplog_text; on == 0 stops listing.  The launches
 * inside the projected eigensolver depend on the data (deflation) and are not listed, only "heevd n".  What the single-rank
 * replay of a multi-GPU solve is compared with, launch for launch (bench.py --replay-rank, tests/test_gpu_replay.py). */
int chase_hip_ctx_oplog(chase_hip_ctx* ctx, int on);
int chase_hip_ctx_oplog_mute(chase_hip_ctx* ctx, int delta); /* > 0: stop listing (nestable), < 0: resume */
const char* chase_hip_ctx_oplog_text(chase_hip_ctx* ctx);
const char* chase_hip_last_error(void);
/* name may be NULL.  clock_khz is the reported max engine clock. */
int chase_hip_device_info(chase_hip_ctx* ctx, int* num_cu, int* clock_khz, size_t* hbm_bytes, char* name,
                          int name_len);
/* PCI bus id ("0000:05:00.0") of the context's device: which physical GPU a rank ended up on, whatever the visibility lists */
int chase_hip_device_bus_id(chase_hip_ctx* ctx, char* out, int len);
const char* chase_hip_version(void);
/* HIP devices visible to this process (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES applied); 0 without a GPU */
int chase_hip_device_count(void);

/* ---- device memory plumbing ----------------------------------------------------------------------------------- */
int chase_hip_malloc(chase_hip_ctx* ctx, void** dev, size_t bytes);
int chase_hip_free(chase_hip_ctx* ctx, void* dev);
int chase_hip_memcpy_h2d(chase_hip_ctx* ctx, void* dev, const void* host, size_t bytes); /* synchronous */
int chase_hip_memcpy_d2h(chase_hip_ctx* ctx, void* host, const void* dev, size_t bytes); /* synchronous */
int chase_hip_memcpy_d2d(chase_hip_ctx* ctx, void* dst, const void* src, size_t bytes);  /* stream-ordered */
int chase_hip_memset(chase_hip_ctx* ctx, void* dev, int value, size_t bytes);            /* stream-ordered */
/* stream-ordered timing helpers: elapsed milliseconds of the work enqueued by fn-free bracketing */
int chase_hip_timer_start(chase_hip_ctx* ctx);
int chase_hip_timer_stop(chase_hip_ctx* ctx, float* ms); /* synchronises */

/* ---- level-3 kernels (device pointers) -------------------------------------------------------------------------
 * C = alpha*op(A)*B + beta*C, opA in {'N','C'} ('T' == 'C' for real).  Replaces the reference's
 * blaspp::t_gemm / cublasTgemm call sites: Impl/chase_cpu/chase_cpu.hpp:497-504, Impl/chase_gpu/chase_gpu.hpp:668-675,
 * linalg/internal/mpi/hemm.hpp:155-167,209-221, linalg/internal/cpu/rayleighRitz.hpp:84-88,110. */
int chase_hip_gemm_d(chase_hip_ctx* ctx, char opA, int m, int n, int k, double alpha, const double* A, long lda,
                     const double* B, long ldb, double beta, double* C, long ldc);
int chase_hip_gemm_z(chase_hip_ctx* ctx, char opA, int m, int n, int k, const double alpha[2], const void* A,
                     long lda, const void* B, long ldb, const double beta[2], void* C, long ldc);
/* The same product in single precision (real fp32 / interleaved complex fp32) on the f32-input matrix cores: the product of the
 * mixed-precision Chebyshev filter (replaces the cublasSgemm / cublasCgemm of the reference's CHASE_ENABLE_MIXED_PRECISION path,
 * Impl/pchase_gpu/pchase_gpu.hpp:785-901).  opA must be 'N' (anything else: CHASE_HIP_EINVAL); any m, n, k and leading dimensions,
 * operands aligned to their element only.  One workgroup per output tile over the whole K - no split, no atomics: results are
 * bitwise reproducible.  beta == 0: C is not read.  Not counted by chase_hip_ctx_gemm_counters (those feed an fp64 roofline);
 * launches in phase 1 carry a kernel symbol of their own. */
int chase_hip_gemm_s(chase_hip_ctx* ctx, char opA, int m, int n, int k, float alpha, const float* A, long lda, const float* B,
                     long ldb, float beta, float* C, long ldc);
int chase_hip_gemm_c(chase_hip_ctx* ctx, char opA, int m, int n, int k, const float alpha[2], const void* A, long lda,
                     const void* B, long ldb, const float beta[2], void* C, long ldc);
/* gemm_s / gemm_c with op(A): C32 = alpha op(A32) B32 + beta C32, opA 'N' or 'C' (real: 'T' as well; anything else:
 * CHASE_HIP_EINVAL); A is m x k for 'N' (lda >= m) and k x m for 'C' (lda >= k).  'N' is gemm_s / gemm_c bit for bit; 'C' is 'N' on
 * the explicitly formed A^H bit for bit (the same LDS image and MFMA order).  The product of the single-precision generalized
 * problem below; gemm_s / gemm_c themselves keep refusing anything but 'N'. */
int chase_hip_gemm_s_op(chase_hip_ctx* ctx, char opA, int m, int n, int k, float alpha, const float* A, long lda, const float* B,
                        long ldb, float beta, float* C, long ldc);
int chase_hip_gemm_c_op(chase_hip_ctx* ctx, char opA, int m, int n, int k, const float alpha[2], const void* A, long lda,
                        const void* B, long ldb, const float beta[2], void* C, long ldc);
/* The fp32-input product with an fp64 result: C64 = alpha op(A32) B32 + beta C64, A and B real fp32 / interleaved complex fp32,
 * C, alpha and beta fp64.  opA is 'N' or 'C' (real: 'T' as well; anything else: CHASE_HIP_EINVAL); A is m x k for 'N' (lda >= m)
 * and k x m for 'C' (lda >= k).  The accumulation runs on the f32-input matrix cores exactly as in gemm_s / _c; alpha acc + beta C
 * is formed in fp64.  This is the filter product of the grid solver: the ranks' partial products are summed in fp64 by the
 * collectives of the fp64 path.  Whole K unless gemm_min_rounds asks for pieces; bitwise reproducible either way: while
 * chase_hip_ctx_set_gemm_min_rounds is > 0, a product with fewer output tiles than workgroup slots is cut into up
 * to 8 K pieces (chase_hip_gemm_sp_plan), each an ordinary product into an fp64 slab of the context's workspace, and the slabs
 * are summed in piece order in fp64 - no atomics, one fixed order per element, a function of shape and chip only.  beta == 0:
 * C is not read; k == 0 gives beta C; not counted by chase_hip_ctx_gemm_counters (chase_hip_ctx_gemm_sp_counters counts them);
 * launches in phase 1 carry a kernel symbol of their own. */
int chase_hip_gemm_sd(chase_hip_ctx* ctx, char opA, int m, int n, int k, double alpha, const float* A, long lda, const float* B,
                      long ldb, double beta, double* C, long ldc);
int chase_hip_gemm_cz(chase_hip_ctx* ctx, char opA, int m, int n, int k, const double alpha[2], const void* A, long lda,
                      const void* B, long ldb, const double beta[2], void* C, long ldc);
/* The four single-precision products above on the bf16 matrix cores with split operands ("bf16x3"): A and B are the same fp32
 * arrays; the kernel writes every operand as the exact sum of three bf16 numbers and accumulates the six partial products
 * a_i b_j, i + j <= 4, in the fp32 accumulator of v_mfma_f32_32x32x16_bf16 - the fp32 product to within u/4 per term, at a
 * matrix-core ceiling of 16/6 of the f32-input instruction's.  Arguments, checks, statuses, tile order and reproducibility are
 * those of gemm_s / _c / _sd / _cz; not counted by chase_hip_ctx_gemm_counters; operator-log names gemm_s3N, gemm_c3N,
 * gemm_sd3N/C, gemm_cz3N/C.  Operands must be finite and below the largest bf16 number (3.39e38) in magnitude. */
int chase_hip_gemm_s_bf16x3(chase_hip_ctx* ctx, char opA, int m, int n, int k, float alpha, const float* A, long lda,
                            const float* B, long ldb, float beta, float* C, long ldc);
int chase_hip_gemm_c_bf16x3(chase_hip_ctx* ctx, char opA, int m, int n, int k, const float alpha[2], const void* A, long lda,
                            const void* B, long ldb, const float beta[2], void* C, long ldc);
int chase_hip_gemm_sd_bf16x3(chase_hip_ctx* ctx, char opA, int m, int n, int k, double alpha, const float* A, long lda,
                             const float* B, long ldb, double beta, double* C, long ldc);
int chase_hip_gemm_cz_bf16x3(chase_hip_ctx* ctx, char opA, int m, int n, int k, const double alpha[2], const void* A, long lda,
                             const void* B, long ldb, const double beta[2], void* C, long ldc);

/* The narrow bf16x3 product with A split and tiled once ("packed"): for an A that stays while B changes - the filter's H.
 * Layout of the packed image of an m x k A (real fp32, or interleaved complex fp32): rows are padded to P = ceil(m / 128) panels
 * of 128, k to T = ceil(k / 16) steps of 16.  Block (panel p, step t) starts at byte ((p T + t) planes 256) 16, the step fastest;
 * planes = 3 (real) or 6 (complex: re p1, p2, p3, then im p1, p2, p3), each plane 256 pieces of 16 bytes.  Piece (row, h),
 * row < 128, h < 2, of plane s sits at piece index 2 row + (h ^ bit 2 of row ^ bit 3 of row) of that plane and holds the eight
 * bf16 numbers x_s[128 p + row, 16 t + 8 h + 0..7] in ascending k, where x = x1 + x2 + x3, x1 = bf16(x), x2 = bf16(x - x1),
 * x3 = bf16(x - x1 - x2), round to nearest even (the split of the _bf16x3 products).  Padding rows and k are zero bytes.
 * pack_bytes: the size, P T planes 4096 (6 bytes per padded real element; 0 when m or k is 0).
 * pack: writes EVERY byte of the image (no caller clears it); src_f64 = 0: A is fp32 / complex fp32, src_f64 = 1: fp64 /
 *   complex fp64, each component rounded to fp32 (nearest even, as convert_d2s) and then split; any lda >= m and any base the
 *   element type allows; packed 16-byte aligned; m == 0 or k == 0: nothing is done.
 * pack_diag: the n diagonal entries of an n x n pack from the fp64 H, nothing else is written: after it the image is byte
 *   for byte a pack of H (the contract diag_d2s has for the fp32 shadow).
 * gemm_s_bf16x3p / gemm_c_bf16x3p: C = alpha A B + beta C with A given as pack(A) of exactly this m and k, op(A) = N, fp32
 *   B, C and scalars: bit for bit chase_hip_gemm_s_bf16x3 / _c_bf16x3('N', ...) on the unpacked operands, for every shape,
 *   leading dimension, alpha and beta (same tiles, same six MFMAs per 16 k in the same order).  beta == 0: C is not read;
 *   k == 0: C = beta C.  Operator-log names bf16x3_pack, bf16x3_pack_diag, gemm_s3pN, gemm_c3pN. */
int chase_hip_bf16x3_pack_bytes(int cplx, int m, int k, size_t* bytes);
int chase_hip_bf16x3_pack(chase_hip_ctx* ctx, int cplx, int src_f64, int m, int k, const void* A, long lda, void* packed);
int chase_hip_bf16x3_pack_diag(chase_hip_ctx* ctx, int cplx, int n, const void* H64, long ldh, void* packed);
int chase_hip_gemm_s_bf16x3p(chase_hip_ctx* ctx, int m, int n, int k, float alpha, const void* packedA, const float* B, long ldb,
                             float beta, float* C, long ldc);
int chase_hip_gemm_c_bf16x3p(chase_hip_ctx* ctx, int m, int n, int k, const float alpha[2], const void* packedA, const void* B,
                             long ldb, const float beta[2], void* C, long ldc);

/* The launch chase_hip_gemm_sd / _cz (bf16x3 != 0: their _bf16x3 twins) make for a product on a device with num_cu compute units
 * while the context's gemm_min_rounds is min_rounds, without making it (host-only: callable without a GPU; a pure function of
 * its arguments).  gm x gn tiles of 128 x bn; sk K pieces per tile of kchunk k each (a multiple of 16; the last piece takes the
 * rest: (sk - 1) kchunk < k <= sk kchunk); sk = 1: whole K, no workspace.  The rule: with min_rounds > 0 a launch of fewer
 * tiles than workgroup slots (2 num_cu: less than one round) is cut; its work is counted in 128 x 64 tiles (a 128-column tile is
 * two), sk = ceil(min_rounds slots / that count), at most 8, at most k / min_piece_k (64 K steps of the kernel: 1024 k, complex
 * fp32 512) and at most what the workspace cap (640 MB) holds.  Returns 0 or CHASE_HIP_EINVAL. */
typedef struct chase_hip_gemm_sp_launch {
    int bn;                   /* tile columns: 128 or 64 */
    int gm, gn;               /* output tiles along M and N */
    int sk, kchunk;           /* K pieces per tile and their length */
    int min_piece_k;          /* no split below 2 min_piece_k */
    size_t slab_bytes;        /* workspace: sk dense fp64 blocks of gm 128 x gn bn elements (0 with sk = 1) */
} chase_hip_gemm_sp_launch;
int chase_hip_gemm_sp_plan(int bf16x3, int cplx, char opA, int m, int n, int k, int num_cu, int min_rounds,
                           chase_hip_gemm_sp_launch* out);
/* slab_bytes of that launch (context-owned, grown on demand) */
size_t chase_hip_gemm_sp_workspace_bytes(int bf16x3, int cplx, char opA, int m, int n, int k, int num_cu, int min_rounds);
/* the wide single-precision products of a context: calls, those of them that ran in K pieces, and the sum of their pieces.  Any
 * output pointer may be NULL. */
int chase_hip_ctx_gemm_sp_counters(chase_hip_ctx* ctx, unsigned long long* wide_calls, unsigned long long* split_calls,
                                   unsigned long long* pieces, int reset);

/* bytes of workspace a product of this shape uses on a device with num_cu compute units (context-owned, grown on
 * demand; min_rounds as in chase_hip_ctx_set_gemm_min_rounds): the split-K slabs and - complex products while the
 * three-multiplication scheme is enabled - the plane of V-side operand sums the 3M kernels read (8 bytes per element of the
 * k x n operand, rounded up to 64-column tiles).  A pure function of the shape (and of the 3M switch), so that the
 * decomposition and with it the summation order never depend on allocation history.  Host-only: callable without a GPU. */
size_t chase_hip_gemm_workspace_bytes(int cplx, char opA, int m, int n, int k, int num_cu, int min_rounds);
/* The launches chase_hip_gemm_{d,z} makes for a product, without making them (host-only: callable without a GPU).  The same
 * decisions as the launcher, from the same code: the pieces of a 3M bulk with 4M rims and of a width in two column launches,
 * and for each launch its tiling, work decomposition, tile order, kernel and workspace.  Arguments as chase_hip_gemm_{d,z}
 * plus: aligned16 = A and B start on 16-byte boundaries, phase = chase_hip_ctx_set_phase's (0-3), num_cu and min_rounds as in
 * chase_hip_gemm_workspace_bytes; the run-time switches (chase_hip_set_gemm3m, CHASE_HIP_GEMM3M_RR, CHASE_HIP_TILE_GROUP,
 * CHASE_HIP_UNIFORM_TILES, CHASE_HIP_REAL_NARROW) apply as they do to a product.  Writes the first max_out records to out (may be
 * NULL) and returns the number of launches (0 when m or n is 0), or CHASE_HIP_EINVAL. */
typedef struct chase_hip_gemm_launch {
    int row0, col0, k0;       /* the launch writes C[row0 : row0+m, col0 : col0+n] from op(A)[., k0 : k0+k] and B[k0 : k0+k, .] */
    int m, n, k;
    int beta_one;             /* 1: adds into C (beta = 1: the K rim of a 3M bulk, launched after it); 0: applies the caller's beta */
    int bn_cols;              /* column stride of its output tiles (< the tile width: "uniform ragged" tiles) */
    int narrow;               /* real 128 x 64 tile */
    int m3;                   /* three-multiplication kernel (0: four) */
    int ragged;               /* the last column tile skips 16-column groups */
    int glds_ok;              /* operands copied global -> LDS directly (0: the register-staged path) */
    int gm, gn;               /* output tiles along M and N */
    long full_tiles;          /* tiles computed whole, one workgroup each */
    long tail_tiles;          /* the rest, each cut into tail_sk K pieces of tail_kchunk and reduced in a fixed order */
    int tail_sk, tail_kchunk;
    int group_rows;           /* tile order: row panels per group */
    int forced_split;         /* the K split is min_rounds' (every tile split), not the automatic one */
    size_t slab_bytes;        /* workspace of the tail's partial tiles */
    size_t plane_bytes;       /* workspace of a 3M launch's operand-sum plane, behind the slabs at a 256-byte boundary */
} chase_hip_gemm_launch;
int chase_hip_gemm_plan(int cplx, char opA, int m, int n, int k, long lda, long ldb, int aligned16, int phase, int num_cu,
                        int min_rounds, chase_hip_gemm_launch* out, int max_out);
/* 1 when complex products issued in phase 1 (chase_hip_ctx_set_phase: the Chebyshev filter) and phase 2 (the H-times-block
 * products of Rayleigh-Ritz / residuals; CHASE_HIP_GEMM3M_RR=0 keeps those on four) use the three-multiplication scheme
 * (default; CHASE_HIP_GEMM3M=0 or chase_hip_set_gemm3m(0) selects the four-multiplication kernel, the arithmetic of the
 * reference's zgemm).  It applies to launches with m a multiple of 128, k a multiple of 8 and 16-byte addressable
 * operands; other shapes, and every other product (Gram matrices, back-transforms, QR, phase 3), take the
 * four-multiplication kernel. */
int chase_hip_gemm3m_enabled(void);
int chase_hip_set_gemm3m(int on); /* process-wide run-time switch */
/* GEMM books of a context, per phase (0 other, 1 filter, 2 H-times-block outside the filter, 3 verification): flops in the reference's
 * model (2*F*m*n*k, F = 4 complex: algorithm/performance.hpp:152,250), flops the matrix cores actually executed (3/4 of
 * the model for three-multiplication launches) and the number of products.  Any output pointer may be NULL. */
int chase_hip_ctx_gemm_counters(chase_hip_ctx* ctx, int phase, double* flops_model, double* flops_executed,
                                unsigned long long* calls, int reset);
/* register-resident v_mfma_f64_16x16x4_f64 issue-rate probe: returns achieved TFLOP/s */
int chase_hip_mfma_f64_peak(chase_hip_ctx* ctx, double* tflops);
/* streaming-copy probe: achieved HBM GB/s for a bytes-sized device-to-device float4 copy */
int chase_hip_hbm_copy_peak(chase_hip_ctx* ctx, size_t bytes, double* gbps);

/* phase 1 = inside FilterPhaseStart/End: GEMMs are launched through the filter-tagged kernel symbol so that rocprofv3
 * reports the Chebyshev-filter HEMM separately; phase 2 = an H-times-block product outside the filter (Rayleigh-Ritz,
 * residuals): ordinary symbol, three multiplications like the filter (CHASE_HIP_GEMM3M_RR=0: four); phase 3 = a
 * verification product (independent residuals, the re-check of residuals that sit on the tolerance): always four
 * multiplications, the arithmetic of the reference's zgemm; 0 = everything else (always four multiplications) */
int chase_hip_ctx_set_phase(chase_hip_ctx* ctx, int phase);
/* Granularity of the following products: rounds > 0 says they share the chip with a collective on another stream (the panel
 * products of the pipelined distributed HEMM) - a product with fewer than `rounds` output tiles per workgroup slot is then cut
 * along K into that many pieces per slot, so that the CUs the collective's kernel takes displace a fraction of a tile and
 * not a whole one; 0 (default) = the automatic decomposition.  Results stay deterministic (fixed-order slab reduction).  The
 * wide single-precision products (gemm_sd / _cz and their bf16x3 twins) are cut by a rule of their own: chase_hip_gemm_sp_plan. */
int chase_hip_ctx_set_gemm_min_rounds(chase_hip_ctx* ctx, int rounds);

/* ---- on-device input generators (global-index addressed, shard-safe) ------------------------------------------ */
/* N(0,1) fill (Philox4x32-10 + Box-Muller).  Replaces cuda/random_normal_distribution.cu:21-95 (initVecs on GPU) */
int chase_hip_fill_normal(chase_hip_ctx* ctx, int cplx, int m, int n, void* X, long ldx, long grow0, long gcol0,
                          long gld, unsigned long long seed);
int chase_hip_fill_normal_bc(chase_hip_ctx* ctx, int cplx, int m, int n, void* X, long ldx, long gld, int mb, int pr,
                             int pi, unsigned long long seed);
/* row gather / scatter by a device index list (column-type <-> row-type multivector redistribution,
 * linalg/distMatrix/distMultiVector.hpp:2444-2720) */
int chase_hip_rows_indexed(chase_hip_ctx* ctx, int cplx, const void* in, long ld_in, void* out, long ld_out,
                           const int* idx_dev, int np, int ncols, int scatter);
/* 64-bit content hash of a device matrix (position-mixed 8-byte words summed modulo 2^64: independent of the order of
 * evaluation, hence reproducible): two holders of what should be the same block compare 8 bytes instead of the block */
int chase_hip_hash64(chase_hip_ctx* ctx, int cplx, int m, int n, const void* A, long lda, unsigned long long* out_host);
/* column gather by a device index list: out[:, c] = in[:, idx[c]], c < ncols */
int chase_hip_cols_indexed(chase_hip_ctx* ctx, int cplx, int m, const void* in, long ld_in, void* out, long ld_out,
                           const int* idx_dev, int ncols);
/* Hermitian completion of a device matrix from its stored triangle ('U': lower <- conj(upper)^T, 'L': the other way round; the
 * diagonal is left alone) - cpu::symOrHermMatrix (linalg/internal/cpu/symOrHerm.hpp:111-134) for a matrix that lives in HBM */
int chase_hip_complete_hermitian(chase_hip_ctx* ctx, int cplx, char uplo, int n, void* A, long lda);
/* the two local steps of the distributed symOrHermMatrix (linalg/internal/mpi/symOrHerm.hpp:127-320): the triangle mask of a
 * block-cyclic shard by global position (kept triangle untouched, the other one zeroed, diagonal halved), and
 * H[colmap[b], rowmap[a]] += conj(P[a, b]) - the conjugate transpose of a received piece added into the shard */
int chase_hip_tri_mask_bc(chase_hip_ctx* ctx, int cplx, char uplo, int mloc, int nloc, void* H, long ldh, long mb, int pr, int pi,
                          long nb, int pc, int pj);
int chase_hip_conj_transpose_add(chase_hip_ctx* ctx, int cplx, int nr, int nc, const void* P, long ldp, const int* rowmap_dev,
                                 const int* colmap_dev, void* H, long ldh);
/* Clement-type test matrix of the reference's solve tests (tests/chase_serial_solve.cpp:52-90), any 2D shard:
 * H = scale * (Clement + perturb * G), G dense Hermitian N(0,1) on the entries the reference perturbs */
int chase_hip_gen_clement(chase_hip_ctx* ctx, int cplx, void* H, long ldh, int mloc, int nloc, long N, int mb, int pr,
                          int pi, long roff, int nb, int pc, int pj, long coff, double scale, double perturb,
                          unsigned long long seed);
/* Synthetic Bethe-Salpeter test matrix H = [[A, B], [-conj(B), -conj(A)]] (A Hermitian with diagonal dmin..dmax spaced uniformly in
 * the square, B symmetric, off-diagonal entries offdiag * N(0,1)), any 2D block-cyclic shard; stands in for the matrix file of
 * examples/5_bse_benchmark/5_bse_benchmark.cpp (BASELINE config 5) */
int chase_hip_gen_bse(chase_hip_ctx* ctx, int cplx, void* H, long ldh, int mloc, int nloc, long N, int mb, int pr, int pi,
                      int nb, int pc, int pj, double dmin, double dmax, double offdiag, unsigned long long seed);
/* Raw column-major binary matrix files (N x N elements of T, no header; the reference's input format):
 * chase_hip_load_matrix_shard reads this rank's (mb x nb block-cyclic; block layout: mb = nb = block length) shard of
 * the file straight into a device block — replaces Matrix::readFromBinaryFile (linalg/matrix/matrix.hpp:313-360) and the
 * BlockBlock / BlockCyclic readFromBinaryFile views (linalg/distMatrix/distMatrix.hpp:2425-2520, 3210-3330).  A file
 * smaller than N*N elements is an error, a larger one is accepted, like the reference.
 * chase_hip_save_matrix writes a device matrix (m x n, ld) as such a file (Matrix::saveToBinaryFile). */
int chase_hip_load_matrix_shard(chase_hip_ctx* ctx, const char* path, int cplx, long N, int mloc, int nloc, int mb,
                                int pr, int pi, int nb, int pc, int pj, void* dev, long ldd);
int chase_hip_save_matrix(chase_hip_ctx* ctx, const char* path, int cplx, int m, int n, const void* dev, long ldd);
/* writes this rank's block-cyclic shard into its byte ranges of the shared N x N file (created if missing, never
 * truncated: all ranks of a grid may write the same path concurrently) — distMatrix.hpp:2241-2300,3117-3200 */
int chase_hip_save_matrix_shard(chase_hip_ctx* ctx, const char* path, int cplx, long N, int mloc, int nloc, int mb,
                                int pr, int pi, int nb, int pc, int pj, const void* dev, long ldd);

/* ---- host LAPACK provider (HEEVD / STEMR stay on the host per the north star) --------------------------------- */
int chase_hip_set_lapack_lib(const char* path);   /* optional explicit LP64 LAPACK shared library */
const char* chase_hip_lapack_provider(void);      /* path of the bound provider ("" if none) */
int chase_hip_set_host_threads(int n);
/* bind the provider and page its compute kernels in (called by the solver constructors; first use of a cold MKL costs
 * seconds, which would otherwise land in the first solve) */
int chase_hip_host_lapack_warmup(void);

/* ---- O(N*n) kernels; cplx = 0 (fp64) or 1 (complex fp64); all matrix pointers are device pointers -------------- */
/* H[i,i] += shift (real part).  Replaces chase_cpu.hpp:384-389 / cuda/shiftDiagonal.cu:23-50 */
int chase_hip_shift_diag(chase_hip_ctx* ctx, int cplx, int n, void* H, long ldh, double shift);
/* H[rows[i], cols[i]] += shift for precomputed local diagonal positions (device int arrays).
 * Replaces cuda/shiftDiagonal.cu:100-149 + Impl/pchase_gpu/pchase_gpu.hpp:340-409 */
int chase_hip_shift_list(chase_hip_ctx* ctx, int cplx, void* H, long ldh, const int* rows_dev, const int* cols_dev,
                         int cnt, double shift);
/* B = A (lacpy 'A').  Replaces cuda/lacpy.cu:503-835 */
int chase_hip_lacpy(chase_hip_ctx* ctx, int cplx, int m, int n, const void* A, long lda, void* B, long ldb);
/* Precision conversion of an m x n matrix (cplx: complex elements), leading dimensions in elements of each side's type.
 * d2s: fp64 -> fp32, round to nearest; s2d: fp32 -> fp64, exact; diag_d2s: Hs[i,i] = (fp32) H[i,i] for i < n, nothing else of
 * Hs is touched.  Replaces linalg/internal/cuda/precision_conversion.cu */
int chase_hip_convert_d2s(chase_hip_ctx* ctx, int cplx, int m, int n, const void* src, long ld_src, void* dst, long ld_dst);
int chase_hip_convert_s2d(chase_hip_ctx* ctx, int cplx, int m, int n, const void* src, long ld_src, void* dst, long ld_dst);
int chase_hip_diag_d2s(chase_hip_ctx* ctx, int cplx, int n, const void* H, long ldh, void* Hs, long ldhs);
/* Y_j += gamma X_j on m x n fp32 (cplx: complex fp32) columns, leading dimensions in elements: the gamma term of the
 * single-precision H^2 filter step.  gamma: 1 float (2 when cplx) on the HOST, handed to the kernel by value - no device-side
 * scalar, no copy.  Rows >= m of a column are neither read nor written; m == 0 or n == 0 does nothing.  X and Y must not overlap */
int chase_hip_axpy_sp(chase_hip_ctx* ctx, int cplx, int m, int n, const float* gamma, const void* X, long ldx, void* Y, long ldy);
/* the list form of diag_d2s: Hs[rows[i], cols[i]] = (fp32) H[rows[i], cols[i]] for i < cnt, nothing else of Hs is touched; rows
 * and cols are DEVICE int arrays (the lists chase_hip_shift_list takes: the global diagonal inside a rank's block) */
int chase_hip_diag_list_d2s(chase_hip_ctx* ctx, int cplx, const void* H, long ldh, void* Hs, long ldhs, const int* rows_dev,
                            const int* cols_dev, int cnt);
/* swap columns i and j of V.  Replaces chase_gpu.hpp:1003-1005 (cublasTswap) */
int chase_hip_swap_cols(chase_hip_ctx* ctx, int cplx, int m, void* V, long ldv, long i, long j);
/* apply a batch of deferred Swap()s: V[:, dst[c]] <- V[:, src[c]] simultaneously; src/dst are host arrays, scratch is a
 * device matrix with at least max(dst)+1 columns (the Impl passes its second vector buffer) */
int chase_hip_permute_cols(chase_hip_ctx* ctx, int cplx, int m, void* V, long ldv, void* scratch, long lds,
                           const int* src_host, const int* dst_host, int cnt);
/* strided host <-> device matrix transfers (synchronous).  Replace Hmat_->H2D() / cublasGetMatrix
 * (chase_gpu.hpp:536,1010-1018) */
int chase_hip_upload_matrix(chase_hip_ctx* ctx, int cplx, int m, int n, const void* host, long ldh, void* dev, long ldd);
int chase_hip_download_matrix(chase_hip_ctx* ctx, int cplx, int m, int n, const void* dev, long ldd, void* host,
                              long ldh);
/* X[row0:, :] *= s.  Replaces cuda/flipSign.cu:19-260 (s = -1) and scaleLowerBlockRows */
int chase_hip_scale_rows(chase_hip_ctx* ctx, int cplx, int m, int n, void* X, long ldx, int row0, double s);
/* the same for a 1D block-cyclic row distribution (block nb over p ranks, this rank q; a block layout is nb = block
 * length): local rows whose global index is >= g0 are scaled.  Replaces the distributed flipLowerHalfMatrixSign
 * (linalg/internal/mpi/flipSign.hpp, cuda_aware_mpi/flipSign.hpp) and the l_half() damping of pchase_cpu.hpp:283-300 */
int chase_hip_scale_rows_bc(chase_hip_ctx* ctx, int cplx, int m, int n, void* X, long ldx, long g0, long nb, int p, int q,
                            double s);
/* in-place conjugate (complex only).  Replaces cuda/conjugate.cu:21-70 */
int chase_hip_conj(chase_hip_ctx* ctx, int m, int n, void* X, long ldx);
/* resid[j] = ||W_j - lambda_j V_j||_2 (squared != 0: sum of squares, for the distributed all-reduce).
 * V == NULL gives plain column norms.  Replaces cuda/residuals.cu:113-296, cpu/residuals.hpp:72-79 */
int chase_hip_resid_norms(chase_hip_ctx* ctx, int cplx, int m, int n, const void* W, long ldw, const void* V, long ldv,
                          const double* lambda_host, double* resid_host, int squared);

/* the same, result left in device memory (out_dev: n doubles) - no host round trip before the distributed all-reduce
 * (linalg/internal/nccl/residuals.hpp:28-88) */
int chase_hip_resid_norms_dev(chase_hip_ctx* ctx, int cplx, int m, int n, const void* W, long ldw, const void* V, long ldv,
                              const double* lambda_host, double* out_dev, int squared);

/* ---- kernels of the single-precision solver (chase_hip_solver_create_sp); cplx = 0 (fp32) or 1 (complex fp32), leading
 * dimensions in elements.  Each moves 16 bytes per access where base pointers and leading dimensions allow and element by element
 * otherwise, and touches nothing outside its m x n window.  A negative extent, a leading dimension smaller than the row count, a
 * negative column index or a NULL matrix of a non-empty operand is CHASE_HIP_EINVAL; empty extents return 0. -------------------- */
/* H[i,i] = fl32(d0[i] + shift), i < n: the real part is the fp64 sum of the saved entry and the ACCUMULATED shift rounded once, the
 * imaginary part of a complex entry is the saved one.  d0: n saved diagonal entries (device, element type of H).  In fp32
 * (h + c) - c need not give h back, so the shifted diagonal is always formed from the saved one: shift == 0 restores it bit for bit */
int chase_hip_shift_diag_sp(chase_hip_ctx* ctx, int cplx, int n, void* H, long ldh, const void* d0, double shift);
/* resid[j] = || W_j - lambda_j V_j ||_2, j < n, on fp32 / complex fp32 columns: every entry is widened exactly, the differences are
 * formed and their squares summed in fp64 (fixed order: bitwise reproducible).  lambda_host, resid_host: n doubles on the host */
int chase_hip_resid_norms_sp(chase_hip_ctx* ctx, int cplx, int m, int n, const void* W, long ldw, const void* V, long ldv,
                             const double* lambda_host, double* resid_host);
/* X[i, j] *= s for row0 <= i < m, j < n on fp32 (cplx: complex fp32) columns: one IEEE fp32 multiply per component (both
 * components of a complex entry times the real s), no other arithmetic: s = -1 is the exact sign flip.  0 <= row0 <= m; row0 == m
 * does nothing.  The fp32 twin of chase_hip_scale_rows */
int chase_hip_scale_rows_sp(chase_hip_ctx* ctx, int cplx, int m, int n, void* X, long ldx, int row0, float s);
/* The K-conjugate of n fp32 (cplx: complex fp32) columns of N rows (N even, h = N/2): second[i + h, j] = conj(first[i, j]) and
 * second[i, j] = conj(first[i + h, j]) for i < h; real: the plain half swap.  Exact.  first and second are disjoint column ranges
 * (they may belong to one block).  Replaces two lacpy calls and a conj (chase_cpu.hpp:557-588) */
int chase_hip_kconj_sp(chase_hip_ctx* ctx, int cplx, int N, int n, const void* first, long ldf, void* second, long lds);
/* the fp32 twins of lacpy, swap_cols, permute_cols, upload_matrix, download_matrix and complete_hermitian (same contracts) */
int chase_hip_lacpy_sp(chase_hip_ctx* ctx, int cplx, int m, int n, const void* A, long lda, void* B, long ldb);
int chase_hip_swap_cols_sp(chase_hip_ctx* ctx, int cplx, int m, void* V, long ldv, long i, long j);
int chase_hip_permute_cols_sp(chase_hip_ctx* ctx, int cplx, int m, void* V, long ldv, void* scratch, long lds,
                              const int* src_host, const int* dst_host, int cnt);
int chase_hip_upload_matrix_sp(chase_hip_ctx* ctx, int cplx, int m, int n, const void* host, long ldh, void* dev, long ldd);
int chase_hip_download_matrix_sp(chase_hip_ctx* ctx, int cplx, int m, int n, const void* dev, long ldd, void* host, long ldh);
int chase_hip_complete_hermitian_sp(chase_hip_ctx* ctx, int cplx, char uplo, int n, void* A, long lda);

/* ---- Cholesky-QR building blocks (replace cublasTsyherk / cusolverDnTpotrf / cublasTtrsm, cuda/cholqr.hpp:110-132) */
int chase_hip_herk(chase_hip_ctx* ctx, int cplx, int n, int k, const void* V, long ldv, void* A, long lda);
/* C (n x n) = A^H B for k x n operands whose product is Hermitian (Gram matrix: A = B; projected matrix of Rayleigh-Ritz:
 * A = H Q, B = Q; linalg/internal/cuda/cholqr.hpp:110-112 cublasTsyherk, nccl/rayleighRitz.hpp:118-129): only the block
 * columns' parts on and above the diagonal are multiplied; mirror != 0 also fills the strictly lower triangle */
int chase_hip_herkx(chase_hip_ctx* ctx, int cplx, int n, int k, const void* A, long lda, const void* B, long ldb, void* C,
                    long ldc, int mirror);
int chase_hip_abs_trace(chase_hip_ctx* ctx, int cplx, int n, const void* A, long lda, double* out_host);
/* in-place upper Cholesky A = R^H R; returns 0 or LAPACK info > 0 (first non-positive or NaN pivot).  The strictly lower
 * triangle is never read and its contents on return are unspecified; rows beyond n (lda > n) are untouched */
int chase_hip_potrf_upper(chase_hip_ctx* ctx, int cplx, int n, void* A, long lda);
int chase_hip_trsm_right_upper(chase_hip_ctx* ctx, int cplx, int m, int n, const void* R, long ldr, void* V, long ldv);

/* ---- generalized Hermitian-definite problem H x = lambda S x, S = U^H U (capi_gev.hip): fp64, one GPU, upper storage.  These
 * are the ppotrf / phegst / ptrtrs of the reference's docs/example/gev.rst.  All products take four multiplications whatever the
 * context's phase; rows beyond n (padded leading dimensions) are never written; op other than 'N' / 'C', a block size that is
 * negative or no multiple of 64, a leading dimension below n: CHASE_HIP_EINVAL. ------------------------------------------- */
/* B (n x nrhs) <- op(R)^{-1} B, R upper triangular, op 'N' or 'C' (real data: the transpose); the strictly lower triangle of R is
 * never read.  64-row steps with inverted diagonal blocks, long products between blocks of 256 rows. */
int chase_hip_trsm_left_upper(chase_hip_ctx* ctx, int cplx, char op, int n, int nrhs, const void* R, long ldr, void* B, long ldb);
/* chase_hip_potrf_upper (same result, same info) in two levels, for matrices of the size of the problem: the strictly lower
 * triangle is neither read nor written and the trailing updates touch the upper block trapezoid only.  outer_nb: columns per
 * outer block (0: default 2048); n <= outer_nb is one chase_hip_potrf_upper on a scratch copy. */
int chase_hip_potrf_upper_blocked(chase_hip_ctx* ctx, int cplx, int n, void* A, long lda, int outer_nb);
/* A <- U^{-H} A U^{-1} (LAPACK xHEGST, itype 1, uplo 'U').  A is read from its upper triangle only, U likewise.  On return both
 * triangles of A hold the result, exactly Hermitian: the lower triangle is the bitwise conjugate of the upper one and the
 * imaginary diagonal is +0.  One block (n <= 64) is reduced in LDS by one workgroup.  nb > 0: the blocked xHEGST recurrence with
 * panels of nb columns (n^3 / 2 multiply-adds).  nb = 0, the default: two full triangular solves on the completed matrix,
 * (A U^{-1}) then U^{-H} (.), one triangle kept and mirrored - n^3 multiply-adds, but all in products with long inner dimensions,
 * and about twice as fast at N = 16384 (profiles/gev.txt). */
int chase_hip_hegst_upper(chase_hip_ctx* ctx, int cplx, int n, void* A, long lda, const void* U, long ldu, int nb);
/* potrf_upper_blocked(S), then hegst_upper(A, S).  Returns the potrf info > 0 when S is not positive definite and leaves A
 * untouched then.  S stays on the device next to A: the reduction needs 2 n^2 elements plus panels. */
int chase_hip_gev_reduce(chase_hip_ctx* ctx, int cplx, int n, void* A, long lda, void* S, long lds);
/* X (n x ncols) <- U^{-1} X: the eigenvectors of the reduced problem become those of (H, S), S-orthonormal */
int chase_hip_gev_backtransform(chase_hip_ctx* ctx, int cplx, int n, int ncols, const void* U, long ldu, void* X, long ldx);
/* X (n x ncols) <- op(U) X in place, U upper triangular, op 'N' or 'C' (real data: the transpose).  The diagonal is used as
 * stored; the strictly lower triangle of U is never read; empty operands are legal.  The mirror image of trsm_left_upper: blocks
 * of 256 rows, op N from the top down and op C from the bottom up; inside a block 64-row steps through trmm_diag (the triangle
 * and the tile of X in LDS, f64 MFMA, written over the tile in place), then one long product for the rows outside the block. */
int chase_hip_trmm_left_upper(chase_hip_ctx* ctx, int cplx, char op, int n, int ncols, const void* U, long ldu, void* X, long ldx);
/* A <- U A U^H (LAPACK xHEGST, itype 2 and 3, uplo 'U') with the contract of chase_hip_hegst_upper: A is read from its upper
 * triangle only, U likewise; on return both triangles of A hold the result, the lower one the bitwise conjugate of the upper
 * one, the imaginary diagonal +0.  Two left products on the completed matrix with an in-place conjugate transpose between them
 * (U (U A)^H = U A U^H), one triangle kept and mirrored: n^3 multiply-adds. */
int chase_hip_hegst_product_upper(chase_hip_ctx* ctx, int cplx, int n, void* A, long lda, const void* U, long ldu);
/* gev_reduce for LAPACK's three problem types.  itype 1: H x = lambda S x, A <- U^{-H} A U^{-1}.  itype 2: H S x = lambda x, and
 * itype 3: S H x = lambda x, A <- U A U^H.  factor = 1: S <- U first (itype 1, factor 1 is chase_hip_gev_reduce bit for bit;
 * info > 0 and A untouched when S is not positive definite).  factor = 0: S already holds U from an earlier call - the overlap
 * matrix of a sequence did not change - and only the two-sided step runs.  Any other itype or factor: CHASE_HIP_EINVAL. */
int chase_hip_gev_reduce_itype(chase_hip_ctx* ctx, int cplx, int itype, int factor, int n, void* A, long lda, void* S, long lds);
/* X (n x ncols) <- U^{-1} X for itype 1 and 2, X <- U^H X for itype 3: eigenvectors y of the reduced problem become those of
 * the pencil (X^H S X = I for itype 1 and 2, X^H S^{-1} X = I for itype 3) */
int chase_hip_gev_backtransform_itype(chase_hip_ctx* ctx, int cplx, int itype, int n, int ncols, const void* U, long ldu, void* X,
                                      long ldx);
/* the inverse of gev_backtransform_itype: X <- U X for itype 1 and 2, X <- U^{-H} X for itype 3.  Approximate eigenvectors of the
 * pencil - the previous step's of a sequence - become the start block of the reduced problem (mode 'A' / approx) */
int chase_hip_gev_starttransform(chase_hip_ctx* ctx, int cplx, int itype, int n, int ncols, const void* U, long ldu, void* X,
                                 long ldx);
/* ---- The generalized problem in single precision: H x = lambda S x (itype 1 only) on real fp32 / interleaved complex fp32 data.
 * The entry points above with float matrices, the same contracts (upper storage, the strictly lower triangle of S / U / R
 * neither read nor written, rows beyond n untouched, info > 0 the first non-positive pivot) and the same block sizes; nothing
 * of size n^2 is widened to fp64.  Products run on the fp32 matrix cores (chase_hip_gemm_s_op / _c_op), the 64-wide diagonal
 * cores compute in fp64 and round once.  hegst_upper_sp has the two-full-solve form only; reduce / backtransform /
 * starttransform are the itype 1 forms: gev_reduce_sp(factor = 0) reuses the U stored in S. */
int chase_hip_trsm_left_upper_sp(chase_hip_ctx* ctx, int cplx, char op, int n, int nrhs, const void* R, long ldr, void* B, long ldb);
int chase_hip_trmm_left_upper_sp(chase_hip_ctx* ctx, int cplx, char op, int n, int ncols, const void* U, long ldu, void* X, long ldx);
int chase_hip_potrf_upper_blocked_sp(chase_hip_ctx* ctx, int cplx, int n, void* A, long lda, int outer_nb);
int chase_hip_hegst_upper_sp(chase_hip_ctx* ctx, int cplx, int n, void* A, long lda, const void* U, long ldu);
int chase_hip_gev_reduce_sp(chase_hip_ctx* ctx, int cplx, int factor, int n, void* A, long lda, void* S, long lds);
int chase_hip_gev_backtransform_sp(chase_hip_ctx* ctx, int cplx, int n, int ncols, const void* U, long ldu, void* X, long ldx);
int chase_hip_gev_starttransform_sp(chase_hip_ctx* ctx, int cplx, int n, int ncols, const void* U, long ldu, void* X, long ldx);
/* variant 1 = cholQR1, 2 = cholQR2, 3 = shiftedcholQR2 (linalg/internal/cpu/cholqr1.hpp:41-189); returns info */
int chase_hip_cholqr(chase_hip_ctx* ctx, int cplx, int m, int n, void* V, long ldv, void* A, long lda, int variant,
                     long m_global);
/* Householder QR fallback: V <- first n columns of Q (cpu/cholqr1.hpp:203-210: geqrf + ungqr) */
int chase_hip_houseqr(chase_hip_ctx* ctx, int cplx, int m, int n, void* V, long ldv);

/* ---- Rayleigh-Ritz: host HEEVD of a device matrix ('V','L'), eigenvectors back on the device -------------------- */
int chase_hip_heevd(chase_hip_ctx* ctx, int cplx, int n, void* A, long lda, double* w_host);
/* same contract; Householder tridiagonalisation + back-transformation on the GPU, tridiagonal stemr on the host
 * (chase_hip_heevd switches to it for n >= 384; env CHASE_HIP_HEEVD_GPU_MIN - sizes below 3, which this entry point refuses,
 * always stay on the host there) */
int chase_hip_heevd_gpu(chase_hip_ctx* ctx, int cplx, int n, void* A, long lda, double* w_host);
/* pseudo-Hermitian (BSE) Rayleigh-Ritz: small dense part of cpu::rayleighRitz_v2 (cpu/rayleighRitz.hpp:316-383) on the host */
int chase_hip_pseudo_rr_small(chase_hip_ctx* ctx, int cplx, int n, void* A_dev, void* M_dev, double* ritzv_host);
int chase_hip_set_identity(chase_hip_ctx* ctx, int cplx, int n, void* A, long lda);
int chase_hip_heevd_host(int cplx, int n, void* A_host, long lda, double* w_host); /* host-only twin (provider check) */
/* host-only: all eigenpairs of a symmetric tridiagonal (Lanczos; lapackpp::t_stemr, cpu/lanczos.hpp:188); non-finite d / e
 * (a Lanczos recurrence that broke down) is CHASE_HIP_EINVAL: LAPACK's MRRR need not terminate on such input */
int chase_hip_stemr_host(int n, double* d, double* e, double* w, double* Z, int ldz);
/* Real symmetric tridiagonal eigenproblem by divide & conquer with the O(n^2) / O(n^3) parts on the device (secular equation,
 * Gu-Eisenstat vectors, merge GEMMs; deflation and the leaves on the host): d (n), e (n-1) on the host, eigenvalues ascending
 * to w_host, eigenvectors (n x n real, ldz) to DEVICE memory.  What chase_hip_heevd_gpu uses between its tridiagonalisation and
 * back-transformation for n >= CHASE_HIP_STEDC_GPU_MIN (512).  Replaces the tridiagonal stage of cusolverDnXheevd
 * (linalg/internal/nccl/rayleighRitz.hpp:170-173). */
int chase_hip_stedc(chase_hip_ctx* ctx, int n, const double* d_host, const double* e_host, double* w_host, double* Z_dev,
                    long ldz);

/* ---- batched multi-vector level-1 kernels with device-resident scalars (Lanczos; cuda/lanczos_kernels.cu) ------- */
/* out_dev[j] = X_j^H Y_j (complex: 2 doubles per column) */
int chase_hip_col_dot(chase_hip_ctx* ctx, int cplx, int m, int n, const void* X, long ldx, const void* Y, long ldy,
                      double* out_dev);
int chase_hip_col_nrm2(chase_hip_ctx* ctx, int cplx, int m, int n, const void* X, long ldx, double* out_dev);
/* partial sums of squares + elementwise sqrt (distributed norms: cuda/lanczos_kernels.cu:433-441 batched_sqrt) */
int chase_hip_col_sumsq(chase_hip_ctx* ctx, int cplx, int m, int n, const void* X, long ldx, double* out_dev);
int chase_hip_sqrt_inplace(chase_hip_ctx* ctx, double* x_dev, int n);
/* Y_j += sgn * a[j*a_stride] * X_j; a is a device array of reals (a_is_real) or of T */
int chase_hip_col_axpy(chase_hip_ctx* ctx, int cplx, int m, int n, const double* a_dev, int a_is_real, int a_stride,
                       double sgn, const void* X, long ldx, void* Y, long ldy);
/* X_j *= a[j] (or 1/a[j] when inverse != 0), a real device array */
int chase_hip_col_scal(chase_hip_ctx* ctx, int cplx, int m, int n, const double* a_dev, int inverse, void* X, long ldx);

/* ---- packed upper triangle (Gram all-reduce payload; cuda/lacpy.cu:837-1094) ------------------------------------ */
int chase_hip_pack_upper(chase_hip_ctx* ctx, int cplx, int n, const void* A, long lda, void* P);
int chase_hip_unpack_upper(chase_hip_ctx* ctx, int cplx, int n, const void* P, void* A, long lda, int mirror);

#ifdef __cplusplus
}
#endif
#endif /* CHASE_HIP_H */
