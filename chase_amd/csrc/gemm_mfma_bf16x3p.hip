// gemm_mfma_bf16x3p.hip — the bf16x3 split product (gemm_mfma_bf16x3.hip) with A split and tiled ONCE: the opt-in sp_prepack = 1 of
// the mixed-precision Chebyshev filter, whose A is the same matrix H in every product of a filter call and, between filter
// calls, moves only on its diagonal.
//
//   packed = pack(A)                        A m x k column-major, fp32 or fp64 (rounded to fp32 first), real or complex   (bf16x3_pack)
//   packed diagonal = pack(diag H)          the n diagonal entries of an n x n pack from the fp64 H                       (bf16x3_pack_diag)
//   C = alpha * A * B + beta * C            A as its pack, B and C fp32 column-major, op(A) = N only                      (gemm_bf16x3p)
//
// Arithmetic: that of gemm_mfma_bf16x3.hip, term for term - x = x1 + x2 + x3, x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2),
// round to nearest even; six MFMAs per 32 x 32 tile and 16 k into one accumulator in the order a3 b1, a2 b2, a1 b3, a2 b1, a1 b2,
// a1 b1, over ascending k, with zeros where a tile or a K step is not whole.  The split is elementwise and the LDS image of A is
// the same, so the product is BITWISE gemm_bf16x3('N', ...) on the unpacked operands, for every shape, leading dimension, alpha
// and beta.  split3 and piece are restated here (twenty lines) so that gemm_mfma_bf16x3.hip and gemm_sp_frame.h stay untouched.
//
// The packed operand is the sequence of the LDS images sA[buf] of that kernel (include/chase_hip.h states it for callers): rows
// padded to 128, k to 16; block (row panel p, K step t) at 16-byte piece (p T + t) * planes * 256, T = ceil(k / 16), the K step
// fastest; a block holds planes = 3 (real) or 6 (complex: re p1, p2, p3, im p1, p2, p3) planes of 256 pieces; piece (row, h) of a
// plane - 8 bf16: k = 16 t + 8 h + 0..7 of row 128 p + row - sits at 2 row + (h ^ bit 2 of row ^ bit 3 of row).  Padding is
// zero.  6 bytes per real element.
//
// Staging.  A: every thread copies planes pieces of 16 bytes, global_load_dwordx4 -> registers -> ds_write_b128, piece tid of
// each plane: a wave reads 1 KB contiguous per instruction and writes LDS linearly (conflict free), and the swizzle is already in
// the image ("swizzle both sides or neither" holds trivially).  The loads of step t + 1 are issued in front of the MFMAs of step t
// like the frame's other loads; registers in flight: 12 (real) / 24 (complex) against the 8 / 16 of the fp32 elements they
// replace, with no conversion or subtraction behind them.  The LDS-DMA (global_load_lds_dwordx4) would spare those registers and the
// ds_write, but B's loads stay in flight across the same barrier and are consumed by VALU code, so the counted vmcnt of
// gemm_mfma_f64.hip would have to tell the two apart: not taken here.  B: split in the kernel as before (choice (a)) - it is
// the N x n block that changes with every product.  K stage: 16 k per barrier, LDS and launch bounds as in gemm_mfma_bf16x3.hip.
#include "gemm_sp_frame.h"

namespace chase_hip {
namespace {

using namespace sp_frame;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int BK = 16;             // k per step: one MFMA
constexpr int PA = 2 * BM;         // 16-byte pieces per plane of a 128-row block

// 16-byte piece (row, h) of a plane, in 16-byte units (gemm_mfma_bf16x3.hip derives the swizzle)
__host__ __device__ __forceinline__ int piece(int row, int h) { return 2 * row + (h ^ (((row >> 2) ^ (row >> 3)) & 1)); }

// the three bf16 parts of one fp32 number
__device__ __forceinline__ void split1(float v, __bf16& a1, __bf16& a2, __bf16& a3)
{
    a1 = (__bf16)v;
    const float r1 = v - (float)a1;
    a2 = (__bf16)r1;
    const float r2 = r1 - (float)a2;
    a3 = (__bf16)r2;
}

// x[0..7] (stride st) -> the three bf16 parts, packed
__device__ __forceinline__ void split3(const float* x, int st, u32x4& p1, u32x4& p2, u32x4& p3)
{
    bf16x8 a1, a2, a3;
    #pragma unroll
    for (int e = 0; e < 8; ++e) {
        __bf16 s1, s2, s3;
        split1(x[st * e], s1, s2, s3);
        a1[e] = s1; a2[e] = s2; a3[e] = s3;
    }
    p1 = __builtin_bit_cast(u32x4, a1); p2 = __builtin_bit_cast(u32x4, a2); p3 = __builtin_bit_cast(u32x4, a3);
}

// ---- pack ------------------------------------------------------------------------------------------------------------------------

// one workgroup per block (K step blockIdx.x, row panel blockIdx.y), one thread per (row, k half): 8 element loads a leading
// dimension apart, 64 consecutive rows per wave instruction; every piece of the block is written, padding as zeros
template <bool CPLX, class S>
__global__ __launch_bounds__(256) void bf16x3_pack_kernel(int m, int k, const S* __restrict__ A, long lda, u32x4* __restrict__ out)
{
    constexpr int E = CPLX ? 2 : 1;
    const int tid = threadIdx.x, r = tid % BM, h = tid / BM;
    const long t = blockIdx.x, T = gridDim.x, p = blockIdx.y;
    const long row = p * BM + r, kg = t * BK + 8 * h;
    float x[8 * E];
    #pragma unroll
    for (int e = 0; e < 8; ++e) {
        #pragma unroll
        for (int c = 0; c < E; ++c) x[E * e + c] = 0.f;
        if (row < m && kg + e < k) {
            const S* q = A + E * (row + (kg + e) * lda);
            #pragma unroll
            for (int c = 0; c < E; ++c) x[E * e + c] = (float)q[c];
        }
    }
    u32x4* d = out + (p * T + t) * (3 * E * PA) + piece(r, h);
    #pragma unroll
    for (int c = 0; c < E; ++c) {
        u32x4 p1, p2, p3;
        split3(x + c, E, p1, p2, p3);
        d[(3 * c) * PA] = p1; d[(3 * c + 1) * PA] = p2; d[(3 * c + 2) * PA] = p3;
    }
}

// diagonal entry i of an n x n pack: 2 bytes per plane
template <bool CPLX>
__global__ __launch_bounds__(256) void bf16x3_pack_diag_kernel(int n, const double* __restrict__ H, long ldh, unsigned short* __restrict__ out)
{
    constexpr int E = CPLX ? 2 : 1;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long T = ((long)n + BK - 1) / BK, p = i / BM, t = i / BK;
    const int r = (int)(i % BM), h = (int)(i % BK) / 8, e = (int)(i % 8);
    unsigned short* d = out + 8 * ((p * T + t) * (3 * E * PA) + piece(r, h)) + e;
    const double* q = H + E * (i + i * ldh);
    #pragma unroll
    for (int c = 0; c < E; ++c) {
        __bf16 s1, s2, s3;
        split1((float)q[c], s1, s2, s3);
        d[8L * (3 * c) * PA] = __builtin_bit_cast(unsigned short, s1);
        d[8L * (3 * c + 1) * PA] = __builtin_bit_cast(unsigned short, s2);
        d[8L * (3 * c + 2) * PA] = __builtin_bit_cast(unsigned short, s3);
    }
}

// ---- product ---------------------------------------------------------------------------------------------------------------------

// gemm_bf16x3_kernel<CPLX, WN, TAG> of gemm_mfma_bf16x3.hip (narrow, op N) with sA[buf] copied from the packed image; a.A is the
// pack, a.lda unused.  TAG: the filter's launches (context phase 1) carry a kernel symbol of their own.
template <bool CPLX, int WN, int TAG, bool WIDE = false>
__global__ __launch_bounds__(256, 2) void gemm_bf16x3p_kernel(const Args a)
{
    static_assert(!WIDE, "narrow form only: fp32 C and scalars");
    constexpr int BN = 64 * WN;
    constexpr int E = CPLX ? 2 : 1;            // floats per element
    static_assert(!CPLX || WN == 1, "complex tiles are 128 x 64");
    constexpr int PB = 2 * BN;                 // 16-byte pieces per plane
    constexpr int HB = 256 / BN;               // threads per column of the B tile: 2 k halves at BN = 128; at BN = 64 the
                                               // first 128 threads carry the B tile
    __shared__ u32x4 sA[2][3 * E * PA];
    __shared__ u32x4 sB[2][3 * E * PB];

    const Place at = place<BN>(a);
    const long n0 = at.n0;
    const int tid = at.tid, wm = at.wm, wn = at.wn, lr = at.lr, lh = at.lh;
    const int jb = tid % BN, hb = tid / BN;                    // this thread's piece of the B tile (hb < 2)
    const bool has_b = HB == 2 || hb < 2;                      // wave-uniform
    // this row panel's blocks: one K step is 3 E planes of PA pieces; this thread copies piece tid of each plane
    const long T = ((long)a.k + BK - 1) / BK;
    const u32x4* Ap = (const u32x4*)a.A + (at.m0 / BM) * T * (3 * E * PA) + tid;

    f32x16 acc[2][WN][E];
    #pragma unroll
    for (int i = 0; i < 2; ++i)
        #pragma unroll
        for (int j = 0; j < WN; ++j)
            #pragma unroll
            for (int p = 0; p < E; ++p)
                #pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][p][r] = 0.f;

    u32x4 pa[3 * E];                           // the pieces of A in flight
    float xb[8 * E];                           // 8 k of one column of B: element e at [E e], (re, im) interleaved
    // the pack is padded: A never needs a guard.  B's fast loads want the tile's columns inside the matrix and 16-byte addressable
    const bool tile_fast = a.vecB && n0 + BN <= a.n;
    auto load_a = [&](long k0) {
        const u32x4* s = Ap + (k0 / BK) * (3 * E * PA);
        #pragma unroll
        for (int q = 0; q < 3 * E; ++q) pa[q] = s[q * PA];
    };
    auto load_k_fast = [&](const float* p, float* x) {
        #pragma unroll
        for (int q = 0; q < 2 * E; ++q) {
            const float4 t = ((const float4*)p)[q];
            x[4 * q] = t.x; x[4 * q + 1] = t.y; x[4 * q + 2] = t.z; x[4 * q + 3] = t.w;
        }
    };
    // the same, of column col (valid: inside the matrix) from k = kg, guarded
    auto load_k_slow = [&](const float* p, bool valid, bool vec, long kg, float* x) {
        constexpr int EPV = 4 / E;             // elements per 16-byte vector
        #pragma unroll
        for (int q = 0; q < 8 * E; ++q) x[q] = 0.f;
        if (!valid) return;
        #pragma unroll
        for (int q = 0; q < 2 * E; ++q) {
            if (vec && kg + (long)(q + 1) * EPV <= a.k) {
                const float4 t = ((const float4*)p)[q];
                x[4 * q] = t.x; x[4 * q + 1] = t.y; x[4 * q + 2] = t.z; x[4 * q + 3] = t.w;
            } else {
                #pragma unroll
                for (int e = 0; e < EPV; ++e)
                    if (kg + (long)q * EPV + e < a.k) {
                        #pragma unroll
                        for (int c = 0; c < E; ++c) x[4 * q + E * e + c] = p[4 * q + E * e + c];
                    }
            }
        }
    };
    auto load_fast = [&](long k0) {
        load_a(k0);
        if (has_b) load_k_fast(a.B + E * (k0 + 8 * hb + (n0 + jb) * a.ldb), xb);
    };
    auto load_slow = [&](long k0) {
        load_a(k0);
        if (has_b) {
            const long col = n0 + jb, kg = k0 + 8 * hb;
            load_k_slow(a.B + E * (kg + col * a.ldb), col < a.n, a.vecB != 0, kg, xb);
        }
    };
    auto store_tiles = [&](int buf) {
        #pragma unroll
        for (int q = 0; q < 3 * E; ++q) sA[buf][q * PA + tid] = pa[q];
        if (has_b) {
            #pragma unroll
            for (int c = 0; c < E; ++c) {
                u32x4 p1, p2, p3;
                split3(xb + c, E, p1, p2, p3);
                u32x4* d = &sB[buf][3 * c * PB + piece(jb, hb)];
                d[0] = p1; d[PB] = p2; d[2 * PB] = p3;
            }
        }
    };

    auto mfma = [](const u32x4& x, const u32x4& y, f32x16& c) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, x), __builtin_bit_cast(bf16x8, y), c, 0, 0, 0);
    };
    // one real product of split fragments into one accumulator, smallest terms first
    auto prod6 = [&](const u32x4* x, const u32x4* y, f32x16& c) {
        mfma(x[2], y[0], c); mfma(x[1], y[1], c); mfma(x[0], y[2], c);
        mfma(x[1], y[0], c); mfma(x[0], y[1], c); mfma(x[0], y[0], c);
    };
    auto compute = [&](int buf) {
        const u32x4* As = sA[buf] + piece(wm * 64 + lr, lh);       // (the swizzle only depends on bits 2 and 3 of the row)
        const u32x4* Bs = sB[buf] + piece(wn * (32 * WN) + lr, lh);
        if constexpr (CPLX) {
            // (the sign flip of Ai in place, after its last use as +Ai)
            #pragma unroll
            for (int j = 0; j < WN; ++j) {
                u32x4 fb[2][3];
                #pragma unroll
                for (int p = 0; p < 2; ++p)
                    #pragma unroll
                    for (int s = 0; s < 3; ++s) fb[p][s] = Bs[(3 * p + s) * PB + 64 * j];
                #pragma unroll
                for (int i = 0; i < 2; ++i) {
                    u32x4 fa[2][3];
                    #pragma unroll
                    for (int p = 0; p < 2; ++p)
                        #pragma unroll
                        for (int s = 0; s < 3; ++s) fa[p][s] = As[(3 * p + s) * PA + 64 * i];
                    prod6(fa[0], fb[0], acc[i][j][0]);
                    prod6(fa[0], fb[1], acc[i][j][1]);
                    prod6(fa[1], fb[0], acc[i][j][1]);
                    #pragma unroll
                    for (int s = 0; s < 3; ++s) fa[1][s] ^= 0x80008000u;          // -Ai
                    prod6(fa[1], fb[1], acc[i][j][0]);
                }
            }
        } else {
            u32x4 fb[WN][3];
            #pragma unroll
            for (int j = 0; j < WN; ++j)
                #pragma unroll
                for (int s = 0; s < 3; ++s) fb[j][s] = Bs[s * PB + 64 * j];
            #pragma unroll
            for (int i = 0; i < 2; ++i) {
                u32x4 fa[3];
                #pragma unroll
                for (int s = 0; s < 3; ++s) fa[s] = As[s * PA + 64 * i];
                #pragma unroll
                for (int j = 0; j < WN; ++j) prod6(fa, fb[j], acc[i][j][0]);
            }
        }
    };
    k_loop<BK>(a.k, tile_fast, load_fast, load_slow, store_tiles, compute);
#include "gemm_sp_epilogue.h"    // the epilogue, as text: uses a, at, acc (the file says why it is no function)
}

template <bool CPLX, int WN>
int launch(hipStream_t st, const Args& a, int tag)
{
    if (tag == 1) hipLaunchKernelGGL((gemm_bf16x3p_kernel<CPLX, WN, 1>), dim3(a.total), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((gemm_bf16x3p_kernel<CPLX, WN, 0>), dim3(a.total), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

template <bool CPLX, class S>
int launch_pack(hipStream_t st, int m, int k, const void* A, long lda, void* packed)
{
    const unsigned T = (unsigned)(((long)k + BK - 1) / BK), P = (unsigned)(((long)m + BM - 1) / BM);
    hipLaunchKernelGGL((bf16x3_pack_kernel<CPLX, S>), dim3(T, P), dim3(256), 0, st, m, k, (const S*)A, lda, (u32x4*)packed);
    return (int)hipGetLastError();
}

} // namespace

size_t bf16x3_pack_bytes(bool cplx, int m, int k)
{
    if (m <= 0 || k <= 0) return 0;
    const size_t T = ((size_t)k + BK - 1) / BK, P = ((size_t)m + BM - 1) / BM;
    return P * T * (size_t)(cplx ? 6 : 3) * PA * 16;
}

int bf16x3_pack(hipStream_t st, bool cplx, bool src_f64, int m, int k, const void* A, long lda, void* packed)
{
    if (m <= 0 || k <= 0) return 0;
    if (((long)m + BM - 1) / BM > 65535) return (int)hipErrorInvalidValue;     // row panels ride on gridDim.y
    if (cplx) return src_f64 ? launch_pack<true, double>(st, m, k, A, lda, packed) : launch_pack<true, float>(st, m, k, A, lda, packed);
    return src_f64 ? launch_pack<false, double>(st, m, k, A, lda, packed) : launch_pack<false, float>(st, m, k, A, lda, packed);
}

int bf16x3_pack_diag(hipStream_t st, bool cplx, int n, const double* H, long ldh, void* packed)
{
    if (n <= 0) return 0;
    const unsigned g = (unsigned)((n + 255) / 256);
    if (cplx) hipLaunchKernelGGL(bf16x3_pack_diag_kernel<true>, dim3(g), dim3(256), 0, st, n, H, ldh, (unsigned short*)packed);
    else hipLaunchKernelGGL(bf16x3_pack_diag_kernel<false>, dim3(g), dim3(256), 0, st, n, H, ldh, (unsigned short*)packed);
    return (int)hipGetLastError();
}

int gemm_bf16x3p(hipStream_t st, bool cplx, int m, int n, int k, const float* alpha, const void* packedA, const float* B, long ldb,
                 const float* beta, float* C, long ldc, int num_cu, int tag)
{
    const int bn = cplx ? 64 : tile_cols(m, n, num_cu);
    return narrow(cplx, 'N', m, n, k, alpha, (const float*)packedA, 0, B, ldb, beta, C, ldc, bn, [&](const Args& a) {
        if (cplx) return launch<true, 1>(st, a, tag);
        return bn == 64 ? launch<false, 1>(st, a, tag) : launch<false, 2>(st, a, tag);
    });
}

} // namespace chase_hip
