// gemm_mfma_bf16x3.hip — the single-precision product of the mixed-precision Chebyshev filter on the gfx950 bf16 matrix cores
// (v_mfma_f32_32x32x16_bf16) with split operands: the opt-in alternative (sp_product = 1) to gemm_mfma_f32.hip, whose
// f32-input MFMA runs at 1/16 of the bf16 rate.
//
//   C = alpha * A * B + beta * C           column-major, op(A) = N, real fp32 or interleaved (re, im) complex fp32   (gemm_bf16x3)
//   C64 = alpha * op(A) * B + beta * C64   op(A) = N or C, A and B fp32, C / alpha / beta fp64                      (gemm_bf16x3w)
//
// Arithmetic.  Every fp32 number x is exactly x1 + x2 + x3 with x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2) (round
// to nearest even, 8 significant bits each; the subtractions are exact in fp32 and bf16 has the exponent range of fp32).  A
// bf16 x bf16 product is exact in fp32.  Of the nine partial products the six with i + j <= 4 are kept - the dropped ones are
// below 2^-26 |a||b| - and accumulated in the MFMA's fp32 accumulator, per 32 x 32 tile and 16 k into ONE accumulator, smallest
// first: a3 b1, a2 b2, a1 b3, a2 b1, a1 b2, a1 b1.  Six MFMAs of 32 cycles replace the eight v_mfma_f32_32x32x2_f32 of 64 cycles
// that 16 k cost in gemm_mfma_f32.hip: a compute ceiling of 16/6 = 2.67 x that kernel's.  Infinities and values that round to a
// bf16 infinity (|x| > 0x7f7f8000) give NaN, not the overflow of an fp32 product: the filter's operands are scaled far below.
//
// A and B stay fp32 in memory; the split happens between the global load and the LDS store (v_cvt_pk_bf16_f32 and v_sub_f32).
// Complex operands become planar on the way in (re | im, three bf16 planes each); one complex tile step is four real products
// Cr += Ar Br + (-Ai) Bi, Ci += Ar Bi + Ai Br, the minus sign being a sign-bit flip of the Ai fragments in registers and the
// conjugation of op = C a sign flip of the imaginary part before it is split (the split commutes with negation).
//
// Launch shape: the frame of gemm_sp_frame.h, which also holds the kernel arguments, the tile order, the K pipeline, the
// tile-width rule and the host setup (the epilogue: gemm_sp_epilogue.h) - one 256-thread workgroup per 128 x BN output tile over the whole K, four
// waves of 64 x BN/2 = 2 x WN MFMA tiles; real: BN = 128 or 64 by the tile-width rule, complex: BN = 64 (see LDS).  K step 16 (one
// MFMA k) for real and complex.  The global loads of step t + 1 are issued in front of the MFMAs of step t and waited for only
// where they are split and stored.
//
// LDS.  One plane is [row][16 k] bf16, 32 bytes per row; a 128-row operand has 3 (real) / 6 (complex) planes of 4 KB.  All
// tiles are double buffered in LDS and run two workgroups per CU, which __launch_bounds__(256, 2) promises (the other
// workgroup's MFMAs cover the barrier and the split): real 2 x 24 KB at BN = 128, 96 KB per CU.  A complex 128 x 128 step needs
// 48 KB, two stages of it would allow one workgroup per CU only, and its 128 accumulator registers beside 48 of fragments and
// 32 of loads in flight do not fit the 256 registers of two workgroups per CU either: complex tiles are always 128 x 64
// (2 x 36 KB, 144 KB per CU of the 160 KB; 64 accumulator registers).
//
// Bank conflicts: none in the K loop, by construction.  Every thread owns one 16-byte piece (one row, 8 consecutive k) per plane,
// which is exactly one lane's MFMA operand: lane l holds A[row l & 31][k = 8 (l >> 5) + j] and B[k = 8 (l >> 5) + j][col l & 31],
// j < 8.  Piece (row, h) of a plane lives at byte 32 row + 16 (h ^ f(row)), f(row) = bit 2 of row ^ bit 3 of row.
//   - fragment read, ds_read_b128: banks are 16-byte slots modulo 16, served in the lane groups {0-3, 12-15, 20-27} and
//     {4-11, 16-19, 28-31} of each half.  Slot = (2 row + (h ^ f)) mod 16 with row = lane & 31: rows 0-3 take the even slots 0-6
//     (f = 0), 12-15 the even slots 8-14 (f = 0), 20-23 the odd slots 9-15 (f = 1), 24-27 the odd slots 1-7 (f = 1); the second
//     group: 4-7 odd 9-15, 8-11 odd 1-7, 16-19 even 0-6, 28-31 even 8-14.  Sixteen lanes, sixteen slots; h = 1 swaps odd and even.
//   - piece store, ds_write_b128: groups of 8 consecutive lanes = 8 consecutive rows aligned to 8, slots modulo 8:
//     rows 8a .. 8a+3 and 8a+4 .. 8a+7 have opposite f, so one quartet takes the even, the other the odd slots.
// That every thread can own a k-contiguous piece is free for B and for A of op = C (k is contiguous in memory: 16-byte loads
// where base pointer and leading dimension allow).  For op = N the transposition is done by the load itself: a thread loads its
// row's 8 k as 8 elements a leading dimension apart, and the 64 lanes of each such load cover 64 consecutive rows (256 / 512
// contiguous bytes per wave instruction) - the same bytes per cache line as 16-byte loads, four times the load instructions,
// beside 24 / 96 MFMAs per wave and step.
//
// Any m, n, k >= 0 and any leading dimensions: guarded element accesses with zero fill wherever a tile is not whole or an
// operand not 16-byte addressable.  beta == 0: C is not read.  k == 0: C = beta C.
#include "gemm_sp_frame.h"

namespace chase_hip {
namespace {

using namespace sp_frame;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int BK = 16;             // k per step: one MFMA

// 16-byte piece (row, h) of a plane, in 16-byte units (the file comment derives the swizzle)
__device__ __forceinline__ int piece(int row, int h) { return 2 * row + (h ^ (((row >> 2) ^ (row >> 3)) & 1)); }

// x[0..7] (stride st) -> the three bf16 parts, packed
__device__ __forceinline__ void split3(const float* x, int st, float sgn, u32x4& p1, u32x4& p2, u32x4& p3)
{
    bf16x8 a1, a2, a3;
    #pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float v = sgn * x[st * e];
        a1[e] = (__bf16)v;
        const float r1 = v - (float)a1[e];
        a2[e] = (__bf16)r1;
        const float r2 = r1 - (float)a2[e];
        a3[e] = (__bf16)r2;
    }
    p1 = __builtin_bit_cast(u32x4, a1); p2 = __builtin_bit_cast(u32x4, a2); p3 = __builtin_bit_cast(u32x4, a3);
}

// TAG only gives the launches of the Chebyshev filter (context phase 1) a kernel symbol of their own (profiles list them apart)
// OPC: op(A) = A^H from a k x m array.  WIDE: epilogue in fp64 on an fp64 C.
template <bool CPLX, int WN, int TAG, bool OPC = false, bool WIDE = false>
__global__ __launch_bounds__(256, 2) void gemm_bf16x3_kernel(const Args launch_args)
{
    const Args a = piece_of<CPLX, OPC, WIDE>(launch_args);     // this workgroup's K piece: the launch itself unless the host cut K
    constexpr int BN = 64 * WN;
    constexpr int E = CPLX ? 2 : 1;            // floats per element
    static_assert(!CPLX || WN == 1, "complex tiles are 128 x 64");
    constexpr int PA = 2 * BM, PB = 2 * BN;    // 16-byte pieces per plane
    constexpr int HB = 256 / BN;               // threads per column of the B tile: 2 k halves at BN = 128; at BN = 64 the
                                               // first 128 threads carry the B tile
    __shared__ u32x4 sA[2][3 * E * PA];
    __shared__ u32x4 sB[2][3 * E * PB];

    const Place at = place<BN>(a);
    const long m0 = at.m0, n0 = at.n0;
    const int tid = at.tid, wm = at.wm, wn = at.wn, lr = at.lr, lh = at.lh;
    const int ja = tid % BM, ha = tid / BM;                    // this thread's piece of the A tile: row, k half
    const int jb = tid % BN, hb = tid / BN;                    // and of the B tile (hb < 2)
    const bool has_b = HB == 2 || hb < 2;                      // wave-uniform

    f32x16 acc[2][WN][E];
    #pragma unroll
    for (int i = 0; i < 2; ++i)
        #pragma unroll
        for (int j = 0; j < WN; ++j)
            #pragma unroll
            for (int p = 0; p < E; ++p)
                #pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][p][r] = 0.f;

    float xa[8 * E], xb[8 * E];                // 8 k of one row / column: element e at [E e], (re, im) interleaved
    // the fast loads want the whole tile inside the matrix and, where they are 16 bytes, 16-byte addressable (k_loop, gemm_sp_frame.h)
    const bool tile_fast = (!OPC || a.vecA) && a.vecB && m0 + BM <= a.m && n0 + BN <= a.n;
    // k-contiguous piece: 8 E floats from p
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
        if constexpr (OPC) {
            load_k_fast(a.A + E * (k0 + 8 * ha + (m0 + ja) * a.lda), xa);
        } else {
            const float* p = a.A + E * (m0 + ja + (k0 + 8 * ha) * a.lda);
            #pragma unroll
            for (int e = 0; e < 8; ++e) {
                if constexpr (CPLX) {
                    const float2 t = *(const float2*)(p + 2 * e * a.lda);
                    xa[2 * e] = t.x; xa[2 * e + 1] = t.y;
                } else {
                    xa[e] = p[e * a.lda];
                }
            }
        }
        if (has_b) load_k_fast(a.B + E * (k0 + 8 * hb + (n0 + jb) * a.ldb), xb);
    };
    auto load_slow = [&](long k0) {
        if constexpr (OPC) {
            const long col = m0 + ja, kg = k0 + 8 * ha;
            load_k_slow(a.A + E * (kg + col * a.lda), col < a.m, a.vecA != 0, kg, xa);
        } else {
            const long row = m0 + ja, kg = k0 + 8 * ha;
            const float* p = a.A + E * (row + kg * a.lda);
            #pragma unroll
            for (int e = 0; e < 8; ++e) {
                #pragma unroll
                for (int c = 0; c < E; ++c) xa[E * e + c] = 0.f;
                if (row < a.m && kg + e < a.k) {
                    #pragma unroll
                    for (int c = 0; c < E; ++c) xa[E * e + c] = p[E * e * a.lda + c];
                }
            }
        }
        if (has_b) {
            const long col = n0 + jb, kg = k0 + 8 * hb;
            load_k_slow(a.B + E * (kg + col * a.ldb), col < a.n, a.vecB != 0, kg, xb);
        }
    };
    auto store_tiles = [&](int buf) {
        #pragma unroll
        for (int c = 0; c < E; ++c) {
            u32x4 p1, p2, p3;
            split3(xa + c, E, (OPC && c == 1) ? -1.f : 1.f, p1, p2, p3);       // conj
            u32x4* d = &sA[buf][3 * c * PA + piece(ja, ha)];
            d[0] = p1; d[PA] = p2; d[2 * PA] = p3;
        }
        if (has_b) {
            #pragma unroll
            for (int c = 0; c < E; ++c) {
                u32x4 p1, p2, p3;
                split3(xb + c, E, 1.f, p1, p2, p3);
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

template <bool CPLX, int WN, bool OPC = false, bool WIDE = false>
int launch(hipStream_t st, const Args& a, int tag)
{
    if (tag == 1) hipLaunchKernelGGL((gemm_bf16x3_kernel<CPLX, WN, 1, OPC, WIDE>), dim3(a.total, a.sk), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((gemm_bf16x3_kernel<CPLX, WN, 0, OPC, WIDE>), dim3(a.total, a.sk), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

} // namespace

int gemm_bf16x3w(hipStream_t st, bool cplx, char opA, int m, int n, int k, const double* alpha, const float* A, long lda,
                 const float* B, long ldb, const double* beta, double* C, long ldc, int num_cu, int tag, double* ws, size_t ws_bytes,
                 int min_rounds, int* pieces)
{
    const int bn = wide_tile_cols(KIND_BF16X3, cplx, m, n, num_cu);
    const SplitPlan sp = split_plan(KIND_BF16X3, cplx, m, n, k, bn, num_cu, min_rounds);
    if (pieces) *pieces = sp.sk;
    return wide(st, cplx, opA, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, bn, sp, ws, ws_bytes, [&](const Args& a, bool opc) {
        if (cplx) {
            if (opc) return launch<true, 1, true, true>(st, a, tag);
            return launch<true, 1, false, true>(st, a, tag);
        }
        if (opc) return bn == 64 ? launch<false, 1, true, true>(st, a, tag) : launch<false, 2, true, true>(st, a, tag);
        return bn == 64 ? launch<false, 1, false, true>(st, a, tag) : launch<false, 2, false, true>(st, a, tag);
    });
}

int gemm_bf16x3(hipStream_t st, bool cplx, char opA, int m, int n, int k, const float* alpha, const float* A, long lda,
                const float* B, long ldb, const float* beta, float* C, long ldc, int num_cu, int tag)
{
    const int bn = cplx ? 64 : tile_cols(m, n, num_cu);
    return narrow(cplx, opA, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, bn, [&](const Args& a) {
        if (cplx) return launch<true, 1>(st, a, tag);
        return bn == 64 ? launch<false, 1>(st, a, tag) : launch<false, 2>(st, a, tag);
    });
}

} // namespace chase_hip
