// gemm_mfma_f32.hip — single-precision GEMM on the gfx950 f32-input matrix cores (v_mfma_f32_32x32x2_f32): the product of the
// mixed-precision Chebyshev filter (ChaseHip::HEMM while the filter call runs in fp32).  Reference: the cublasSgemm / cublasCgemm
// the reference's mixed-precision HEMM issues on its shadow copies (Impl/pchase_gpu/pchase_gpu.hpp:785-901).
//
//   C = alpha * A * B + beta * C           column-major, op(A) = N, real fp32 or interleaved (re, im) complex fp32     (gemm_f32)
//   C64 = alpha * op(A) * B + beta * C64   op(A) = N or C, A and B fp32, C / alpha / beta fp64                        (gemm_f32w)
//   C = alpha * op(A) * B + beta * C       op(A) = C with the fp32 epilogue: instantiated in gemm_mfma_f32_op.hip     (gemm_f32_op)
//
// The second form is the product of the filter on a process grid (pChaseHip): every rank's partial product leaves the kernel in
// fp64 and is summed over the ranks in fp64 by the collectives the fp64 path already has.  OPC reads A as a k x m array
// (contiguous in k: the access pattern of the B tile) and transposes it into the same m-contiguous LDS image the op = N path
// builds: lane l of a 32-lane half stores dword l of an LDS row, one conflict-free ds_write_b32 group, exactly the stores of the
// B tile - the transposition costs no bank conflict that op = N does not have, and the fragment reads are unchanged.  The
// conjugation is the sign of the imaginary plane, applied once at that store, not per MFMA.  WIDE only changes the epilogue.
//
// One 256-thread workgroup owns a 128 x BN output tile (BN = 128 or 64) over the whole K; each of the four waves owns 64 x BN/2
// of the tile as 2 x WN MFMA tiles of 32 x 32: the frame of gemm_sp_frame.h, which holds the kernel arguments, the tile order,
// the K pipeline, the tile-width rule and the host setup (the epilogue: gemm_sp_epilogue.h).  This file is the operand path: HBM -> registers ->
// LDS (double buffered, one barrier per K step of 16 real / 8 complex); complex operands are split into planar (re | im) LDS
// images on the way in, so that one complex tile step is four real MFMAs on planar fragments: Cr += Ar Br - Ai Bi,
// Ci += Ar Bi + Ai Br.
//
// Any m, n, k >= 0 and any leading dimensions: 16-byte loads / stores are taken where base pointer and leading dimension
// allow and the piece lies inside the matrix, element-wise guarded accesses (zero fill) everywhere else.  beta == 0: C is not read.
#include "gemm_sp_frame.h"

namespace chase_hip {
namespace {

using namespace sp_frame;

constexpr int KROWS = 16;          // LDS rows per tile image: 16 k (real) or 2 planes x 8 k (complex)
// (LDS rows are m- / n-contiguous: the 32 lanes of a fragment half read 32 consecutive floats - one conflict-free group of ds_read_b32)

// TAG only gives the launches of the Chebyshev filter (context phase 1) a kernel symbol of their own (profiles list them apart)
// OPC: op(A) = A^H from a k x m array.  WIDE: epilogue in fp64 on an fp64 C.
template <bool CPLX, int WN, int TAG, bool OPC = false, bool WIDE = false>
__global__ __launch_bounds__(256, 2) void gemm_f32_kernel(const Args launch_args)
{
    const Args a = piece_of<CPLX, OPC, WIDE>(launch_args);     // this workgroup's K piece: the launch itself unless the host cut K
    constexpr int BN = 64 * WN;
    constexpr int LDA_T = BM, LDB_T = BN;      // LDS row strides of the two images
    constexpr int E = CPLX ? 2 : 1;            // floats per element
    constexpr int EPV = 4 / E;                 // elements per 16-byte vector
    constexpr int BK = KROWS / E;              // k per step
    constexpr int RG = BM / EPV;               // 16-byte row groups per column of the A tile
    __shared__ __attribute__((aligned(16))) float sA[2][KROWS * LDA_T];
    __shared__ __attribute__((aligned(16))) float sB[2][KROWS * LDB_T];

    const Place at = place<BN>(a);
    const long m0 = at.m0, n0 = at.n0;
    const int tid = at.tid, wm = at.wm, wn = at.wn, lr = at.lr, lh = at.lh;

    f32x16 acc[2][WN][E];
    #pragma unroll
    for (int i = 0; i < 2; ++i)
        #pragma unroll
        for (int j = 0; j < WN; ++j)
            #pragma unroll
            for (int p = 0; p < E; ++p)
                #pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][p][r] = 0.f;

    float4 ga[2], gb[WN];
    // the fast loads want the whole tile inside the matrix and 16-byte addressable (k_loop, gemm_sp_frame.h)
    const bool tile_fast = a.vecA && a.vecB && m0 + BM <= a.m && n0 + BN <= a.n;
    auto load_fast = [&](long k0) {
        #pragma unroll
        for (int r = 0; r < 2; ++r) {
            if constexpr (OPC) {
                const int f = tid + 256 * r, j = f % BM, kq = f / BM;
                ga[r] = *(const float4*)(a.A + E * (k0 + (long)EPV * kq + (m0 + j) * a.lda));
            } else {
                const int f = tid + 256 * r, rg = f % RG, kk = f / RG;
                ga[r] = *(const float4*)(a.A + E * (m0 + (long)EPV * rg + (k0 + kk) * a.lda));
            }
        }
        #pragma unroll
        for (int r = 0; r < WN; ++r) {
            const int f = tid + 256 * r, j = f % BN, kq = f / BN;
            gb[r] = *(const float4*)(a.B + E * (k0 + (long)EPV * kq + (n0 + j) * a.ldb));
        }
    };
    auto load_slow = [&](long k0) {
        #pragma unroll
        for (int r = 0; r < 2; ++r) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (OPC) {
                const int f = tid + 256 * r, j = f % BM, kq = f / BM;
                const long col = m0 + j, kg = k0 + (long)EPV * kq;
                const float* p = a.A + E * (kg + col * a.lda);
                if (col < a.m) {
                    if (a.vecA && kg + EPV <= a.k) {
                        const float4 t = *(const float4*)p;
                        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
                    } else {
                        #pragma unroll
                        for (int e = 0; e < EPV; ++e)
                            if (kg + e < a.k) {
                                #pragma unroll
                                for (int c = 0; c < E; ++c) v[E * e + c] = p[E * e + c];
                            }
                    }
                }
                ga[r] = make_float4(v[0], v[1], v[2], v[3]);
                continue;
            }
            const int f = tid + 256 * r, rg = f % RG, kk = f / RG;
            const long row = m0 + (long)EPV * rg, kg = k0 + kk;
            const float* p = a.A + E * (row + kg * a.lda);
            if (kg < a.k) {
                if (a.vecA && row + EPV <= a.m) {
                    const float4 t = *(const float4*)p;
                    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
                } else {
                    #pragma unroll
                    for (int e = 0; e < EPV; ++e)
                        if (row + e < a.m) {
                            #pragma unroll
                            for (int c = 0; c < E; ++c) v[E * e + c] = p[E * e + c];
                        }
                }
            }
            ga[r] = make_float4(v[0], v[1], v[2], v[3]);
        }
        #pragma unroll
        for (int r = 0; r < WN; ++r) {
            const int f = tid + 256 * r, j = f % BN, kq = f / BN;
            const long col = n0 + j, kg = k0 + (long)EPV * kq;
            const float* p = a.B + E * (kg + col * a.ldb);
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (col < a.n) {
                if (a.vecB && kg + EPV <= a.k) {
                    const float4 t = *(const float4*)p;
                    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
                } else {
                    #pragma unroll
                    for (int e = 0; e < EPV; ++e)
                        if (kg + e < a.k) {
                            #pragma unroll
                            for (int c = 0; c < E; ++c) v[E * e + c] = p[E * e + c];
                        }
                }
            }
            gb[r] = make_float4(v[0], v[1], v[2], v[3]);
        }
    };
    auto store_tiles = [&](int buf) {
        #pragma unroll
        for (int r = 0; r < 2; ++r) {
            if constexpr (OPC) {
                // the k-contiguous vector of column j goes to rows of the image at dword j: 32 consecutive dwords per lane half
                const int f = tid + 256 * r, j = f % BM, kq = f / BM;
                if constexpr (CPLX) {
                    sA[buf][(2 * kq) * LDA_T + j] = ga[r].x;
                    sA[buf][(BK + 2 * kq) * LDA_T + j] = -ga[r].y;           // conj
                    sA[buf][(2 * kq + 1) * LDA_T + j] = ga[r].z;
                    sA[buf][(BK + 2 * kq + 1) * LDA_T + j] = -ga[r].w;
                } else {
                    sA[buf][(4 * kq) * LDA_T + j] = ga[r].x;
                    sA[buf][(4 * kq + 1) * LDA_T + j] = ga[r].y;
                    sA[buf][(4 * kq + 2) * LDA_T + j] = ga[r].z;
                    sA[buf][(4 * kq + 3) * LDA_T + j] = ga[r].w;
                }
                continue;
            }
            const int f = tid + 256 * r, rg = f % RG, kk = f / RG;
            if constexpr (CPLX) {
                *(float2*)&sA[buf][kk * LDA_T + 2 * rg] = make_float2(ga[r].x, ga[r].z);
                *(float2*)&sA[buf][(BK + kk) * LDA_T + 2 * rg] = make_float2(ga[r].y, ga[r].w);
            } else {
                *(float4*)&sA[buf][kk * LDA_T + 4 * rg] = ga[r];
            }
        }
        #pragma unroll
        for (int r = 0; r < WN; ++r) {
            const int f = tid + 256 * r, j = f % BN, kq = f / BN;
            if constexpr (CPLX) {
                sB[buf][(2 * kq) * LDB_T + j] = gb[r].x;
                sB[buf][(BK + 2 * kq) * LDB_T + j] = gb[r].y;
                sB[buf][(2 * kq + 1) * LDB_T + j] = gb[r].z;
                sB[buf][(BK + 2 * kq + 1) * LDB_T + j] = gb[r].w;
            } else {
                sB[buf][(4 * kq) * LDB_T + j] = gb[r].x;
                sB[buf][(4 * kq + 1) * LDB_T + j] = gb[r].y;
                sB[buf][(4 * kq + 2) * LDB_T + j] = gb[r].z;
                sB[buf][(4 * kq + 3) * LDB_T + j] = gb[r].w;
            }
        }
    };

    auto compute = [&](int buf) {
        const float* As = sA[buf] + wm * 64 + lr;
        const float* Bs = sB[buf] + wn * (32 * WN) + lr;
        #pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
            const int kk = 2 * s + lh;             // lane l holds A[l & 31][k = l >> 5] and B[k = l >> 5][l & 31]
            float fa[2][E], fb[WN][E];
            #pragma unroll
            for (int i = 0; i < 2; ++i)
                #pragma unroll
                for (int p = 0; p < E; ++p) fa[i][p] = As[(p * BK + kk) * LDA_T + 32 * i];
            #pragma unroll
            for (int j = 0; j < WN; ++j)
                #pragma unroll
                for (int p = 0; p < E; ++p) fb[j][p] = Bs[(p * BK + kk) * LDB_T + 32 * j];
            if constexpr (CPLX) {
                #pragma unroll
                for (int i = 0; i < 2; ++i)
                    #pragma unroll
                    for (int j = 0; j < WN; ++j) {
                        acc[i][j][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][0], fb[j][0], acc[i][j][0], 0, 0, 0);
                        acc[i][j][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][0], fb[j][1], acc[i][j][1], 0, 0, 0);
                    }
                #pragma unroll
                for (int i = 0; i < 2; ++i)
                    #pragma unroll
                    for (int j = 0; j < WN; ++j) {
                        acc[i][j][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(-fa[i][1], fb[j][1], acc[i][j][0], 0, 0, 0);
                        acc[i][j][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][1], fb[j][0], acc[i][j][1], 0, 0, 0);
                    }
            } else {
                #pragma unroll
                for (int i = 0; i < 2; ++i)
                    #pragma unroll
                    for (int j = 0; j < WN; ++j)
                        acc[i][j][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][0], fb[j][0], acc[i][j][0], 0, 0, 0);
            }
        }
    };
    k_loop<BK>(a.k, tile_fast, load_fast, load_slow, store_tiles, compute);
#include "gemm_sp_epilogue.h"    // the epilogue, as text: uses a, at, acc (the file says why it is no function)
}

template <bool CPLX, int WN, bool OPC = false, bool WIDE = false>
int launch(hipStream_t st, const Args& a, int tag)
{
    if (tag == 1) hipLaunchKernelGGL((gemm_f32_kernel<CPLX, WN, 1, OPC, WIDE>), dim3(a.total, a.sk), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((gemm_f32_kernel<CPLX, WN, 0, OPC, WIDE>), dim3(a.total, a.sk), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

} // namespace

#ifndef CHASE_HIP_GEMM_F32_KERNEL_ONLY    // gemm_mfma_f32_op.hip takes the kernel above for instantiations of its own

int gemm_f32w(hipStream_t st, bool cplx, char opA, int m, int n, int k, const double* alpha, const float* A, long lda,
              const float* B, long ldb, const double* beta, double* C, long ldc, int num_cu, int tag, double* ws, size_t ws_bytes,
              int min_rounds, int* pieces)
{
    const int bn = wide_tile_cols(KIND_F32, cplx, m, n, num_cu);
    const SplitPlan sp = split_plan(KIND_F32, cplx, m, n, k, bn, num_cu, min_rounds);
    if (pieces) *pieces = sp.sk;
    return wide(st, cplx, opA, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, bn, sp, ws, ws_bytes, [&](const Args& a, bool opc) {
        if (cplx) {
            if (opc) return bn == 64 ? launch<true, 1, true, true>(st, a, tag) : launch<true, 2, true, true>(st, a, tag);
            return bn == 64 ? launch<true, 1, false, true>(st, a, tag) : launch<true, 2, false, true>(st, a, tag);
        }
        if (opc) return bn == 64 ? launch<false, 1, true, true>(st, a, tag) : launch<false, 2, true, true>(st, a, tag);
        return bn == 64 ? launch<false, 1, false, true>(st, a, tag) : launch<false, 2, false, true>(st, a, tag);
    });
}

int gemm_f32(hipStream_t st, bool cplx, char opA, int m, int n, int k, const float* alpha, const float* A, long lda, const float* B,
             long ldb, const float* beta, float* C, long ldc, int num_cu, int tag)
{
    const int bn = tile_cols(m, n, num_cu);
    return narrow(cplx, opA, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, bn, [&](const Args& a) {
        if (cplx) return bn == 64 ? launch<true, 1>(st, a, tag) : launch<true, 2>(st, a, tag);
        return bn == 64 ? launch<false, 1>(st, a, tag) : launch<false, 2>(st, a, tag);
    });
}

#endif // CHASE_HIP_GEMM_F32_KERNEL_ONLY

} // namespace chase_hip
