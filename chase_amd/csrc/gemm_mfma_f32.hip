// gemm_mfma_f32.hip — single-precision GEMM on the gfx950 f32-input matrix cores (v_mfma_f32_32x32x2_f32): the product of the
// mixed-precision Chebyshev filter (ChaseHip::HEMM while the filter call runs in fp32).  Reference: the cublasSgemm / cublasCgemm
// the reference's mixed-precision HEMM issues on its shadow copies (Impl/pchase_gpu/pchase_gpu.hpp:785-901).
//
//   C = alpha * A * B + beta * C           column-major, op(A) = N, real fp32 or interleaved (re, im) complex fp32     (gemm_f32)
//   C64 = alpha * op(A) * B + beta * C64   op(A) = N or C, A and B fp32, C / alpha / beta fp64                        (gemm_f32w)
//
// The second form is the product of the filter on a process grid (pChaseHip): every rank's partial product leaves the kernel in
// fp64 and is summed over the ranks in fp64 by the collectives the fp64 path already has.  OPC reads A as a k x m array
// (contiguous in k: the access pattern of the B tile) and transposes it into the same m-contiguous LDS image the op = N path
// builds: lane l of a 32-lane half stores dword l of an LDS row, one conflict-free ds_write_b32 group, exactly the stores of the
// B tile - the transposition costs no bank conflict that op = N does not have, and the fragment reads are unchanged.  The
// conjugation is the sign of the imaginary plane, applied once at that store, not per MFMA.  WIDE only changes the epilogue.
//
// One 256-thread workgroup owns a 128 x BN output tile (BN = 128 or 64) over the WHOLE K: no split-K, no atomics, one fixed
// summation order per element - results are bitwise reproducible run to run.  Each of the four waves owns 64 x BN/2 of the tile
// as 2 x WN MFMA tiles of 32 x 32.  Operands go HBM -> registers -> LDS (double buffered, one barrier per K step of 16 real /
// 8 complex); complex operands are split into planar (re | im) LDS images on the way in, so that one complex tile step is four
// real MFMAs on planar fragments: Cr += Ar Br - Ai Bi, Ci += Ar Bi + Ai Br.
//
// Any m, n, k >= 0 and any leading dimensions: 16-byte loads / stores are taken where base pointer and leading dimension
// allow and the piece lies inside the matrix, element-wise guarded accesses (zero fill) everywhere else.  beta == 0: C is not read.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kernels.h"

namespace chase_hip {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128;            // tile rows
constexpr int KROWS = 16;          // LDS rows per tile image: 16 k (real) or 2 planes x 8 k (complex)
// (LDS rows are m- / n-contiguous: the 32 lanes of a fragment half read 32 consecutive floats - one conflict-free group of ds_read_b32)

struct Args {
    int m, n, k;
    float ar, ai, br, bi;
    const float* A; long lda;
    const float* B; long ldb;
    float* C; long ldc;
    double war, wai, wbr, wbi;     // WIDE: fp64 scalars and an fp64 C (ldc in its elements)
    double* Cw;
    int gn;                        // tiles along n
    unsigned total;                // tiles
    int vecA, vecB, vecC;          // 16-byte accesses allowed (base pointer and leading dimension)
};

// TAG only gives the launches of the Chebyshev filter (context phase 1) a kernel symbol of their own (profiles list them apart)
// OPC: op(A) = A^H from a k x m array.  WIDE: epilogue in fp64 on an fp64 C.
template <bool CPLX, int WN, int TAG, bool OPC = false, bool WIDE = false>
__global__ __launch_bounds__(256, 2) void gemm_f32_kernel(const Args a)
{
    constexpr int BN = 64 * WN;
    constexpr int LDA_T = BM, LDB_T = BN;      // LDS row strides of the two images
    constexpr int E = CPLX ? 2 : 1;            // floats per element
    constexpr int EPV = 4 / E;                 // elements per 16-byte vector
    constexpr int BK = KROWS / E;              // k per step
    constexpr int RG = BM / EPV;               // 16-byte row groups per column of the A tile
    __shared__ __attribute__((aligned(16))) float sA[2][KROWS * LDA_T];
    __shared__ __attribute__((aligned(16))) float sB[2][KROWS * LDB_T];

    // tile id: eight consecutive workgroups land on eight different XCDs (each with an L2 of its own) - give every XCD a
    // contiguous run of tiles, n fastest, so that the tiles sharing a row block of A meet in one L2
    unsigned id = blockIdx.x;
    if ((a.total & 7u) == 0) id = (id & 7u) * (a.total >> 3) + (id >> 3);
    const int tn = (int)(id % (unsigned)a.gn), tm = (int)(id / (unsigned)a.gn);
    const long m0 = (long)tm * BM, n0 = (long)tn * BN;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w & 1, wn = w >> 1, lr = lane & 31, lh = lane >> 5;

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
    // Whole tile inside the matrix and 16-byte addressable (workgroup-uniform): its full K steps run in a loop of their own whose
    // loads have no branch per lane - all loads of a step are in flight together, behind the MFMAs of the step before, and are
    // waited for only where they are stored to LDS.  Everything else (edge tiles, unaligned operands, the K rest) takes the
    // guarded loads.
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
    // K steps [t0, t1) with one kind of load: step t + 1 is fetched into registers while step t is multiplied from LDS
    auto pipeline = [&](int t0, int t1, auto&& load) {
        if (t0 >= t1) return;
        load((long)t0 * BK);
        store_tiles(0);
        __syncthreads();
        int buf = 0;
        for (int t = t0; t + 1 < t1; ++t) {
            load((long)(t + 1) * BK);
            __builtin_amdgcn_sched_barrier(0);     // the loads are issued here, a whole step of MFMAs ahead of their use -
            compute(buf);                          // left alone, the scheduler sinks them to the end of the step
            __builtin_amdgcn_sched_barrier(0);
            store_tiles(buf ^ 1);
            __syncthreads();
            buf ^= 1;
        }
        compute(buf);
        __syncthreads();                           // (a following pipeline starts over in buffer 0)
    };
    const int T = (a.k + BK - 1) / BK;
    if (tile_fast) {
        const int Tf = a.k / BK;
        pipeline(0, Tf, load_fast);
        pipeline(Tf, T, load_slow);
    } else {
        pipeline(0, T, load_slow);
    }

    // epilogue.  C/D map of the 32 x 32 tile: column = lane & 31, rows 8 g + 4 (lane >> 5) + (0..3) in registers 4 g .. 4 g + 3
    if constexpr (WIDE) {
        const bool useC = (a.wbr != 0.0) || (a.wbi != 0.0);
        #pragma unroll
        for (int i = 0; i < 2; ++i)
            #pragma unroll
            for (int j = 0; j < WN; ++j) {
                const long col = n0 + wn * (32 * WN) + 32 * j + lr;
                if (col >= a.n) continue;
                #pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const long row = m0 + wm * 64 + 32 * i + 8 * g + 4 * lh;
                    if (row >= a.m) continue;
                    double* c = a.Cw + E * (row + col * a.ldc);
                    const bool vec = a.vecC && row + 4 <= a.m;
                    double o[4 * E], c0[4 * E];
                    #pragma unroll
                    for (int q = 0; q < 4 * E; ++q) c0[q] = 0.0;
                    if (useC) {
                        if (vec) {
                            #pragma unroll
                            for (int q = 0; q < 2 * E; ++q) {
                                const double2 t = ((const double2*)c)[q];
                                c0[2 * q] = t.x; c0[2 * q + 1] = t.y;
                            }
                        } else {
                            #pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (row + e < a.m) {
                                    #pragma unroll
                                    for (int p = 0; p < E; ++p) c0[E * e + p] = c[E * e + p];
                                }
                        }
                    }
                    #pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if constexpr (CPLX) {
                            const double xr = (double)acc[i][j][0][4 * g + e], xi = (double)acc[i][j][1][4 * g + e];
                            double yr = a.war * xr - a.wai * xi, yi = a.war * xi + a.wai * xr;
                            if (useC) {
                                yr += a.wbr * c0[2 * e] - a.wbi * c0[2 * e + 1];
                                yi += a.wbr * c0[2 * e + 1] + a.wbi * c0[2 * e];
                            }
                            o[2 * e] = yr; o[2 * e + 1] = yi;
                        } else {
                            double y = a.war * (double)acc[i][j][0][4 * g + e];
                            if (useC) y += a.wbr * c0[e];
                            o[e] = y;
                        }
                    }
                    if (vec) {
                        #pragma unroll
                        for (int q = 0; q < 2 * E; ++q) ((double2*)c)[q] = make_double2(o[2 * q], o[2 * q + 1]);
                    } else {
                        #pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (row + e < a.m) {
                                #pragma unroll
                                for (int p = 0; p < E; ++p) c[E * e + p] = o[E * e + p];
                            }
                    }
                }
            }
        return;
    }
    const bool useC = (a.br != 0.f) || (a.bi != 0.f);
    #pragma unroll
    for (int i = 0; i < 2; ++i)
        #pragma unroll
        for (int j = 0; j < WN; ++j) {
            const long col = n0 + wn * (32 * WN) + 32 * j + lr;
            if (col >= a.n) continue;
            #pragma unroll
            for (int g = 0; g < 4; ++g) {
                const long row = m0 + wm * 64 + 32 * i + 8 * g + 4 * lh;
                if (row >= a.m) continue;
                float* c = a.C + E * (row + col * a.ldc);
                const bool vec = a.vecC && row + 4 <= a.m;
                float o[4 * E], c0[4 * E];
                #pragma unroll
                for (int q = 0; q < 4 * E; ++q) c0[q] = 0.f;
                if (useC) {
                    if (vec) {
                        #pragma unroll
                        for (int q = 0; q < E; ++q) {
                            const float4 t = ((const float4*)c)[q];
                            c0[4 * q] = t.x; c0[4 * q + 1] = t.y; c0[4 * q + 2] = t.z; c0[4 * q + 3] = t.w;
                        }
                    } else {
                        #pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (row + e < a.m) {
                                #pragma unroll
                                for (int p = 0; p < E; ++p) c0[E * e + p] = c[E * e + p];
                            }
                    }
                }
                #pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if constexpr (CPLX) {
                        const float xr = acc[i][j][0][4 * g + e], xi = acc[i][j][1][4 * g + e];
                        float yr = a.ar * xr - a.ai * xi, yi = a.ar * xi + a.ai * xr;
                        if (useC) {
                            yr += a.br * c0[2 * e] - a.bi * c0[2 * e + 1];
                            yi += a.br * c0[2 * e + 1] + a.bi * c0[2 * e];
                        }
                        o[2 * e] = yr; o[2 * e + 1] = yi;
                    } else {
                        float y = a.ar * acc[i][j][0][4 * g + e];
                        if (useC) y += a.br * c0[e];
                        o[e] = y;
                    }
                }
                if (vec) {
                    #pragma unroll
                    for (int q = 0; q < E; ++q) ((float4*)c)[q] = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
                } else {
                    #pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (row + e < a.m) {
                            #pragma unroll
                            for (int p = 0; p < E; ++p) c[E * e + p] = o[E * e + p];
                        }
                }
            }
        }
}

template <bool CPLX, int WN, bool OPC = false, bool WIDE = false>
int launch(hipStream_t st, const Args& a, int tag)
{
    if (tag == 1) hipLaunchKernelGGL((gemm_f32_kernel<CPLX, WN, 1, OPC, WIDE>), dim3(a.total), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((gemm_f32_kernel<CPLX, WN, 0, OPC, WIDE>), dim3(a.total), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// tile width of a product on a device with num_cu compute units: 128 columns unless the 64-column form fills the last round of
// workgroups better (one workgroup's worth of matrix-core work per compute unit and round; N = 16384, n = 640: 640 tiles of
// 128 x 128 leave half of the third round empty, 1280 tiles of 128 x 64 are five full rounds)
int tile_cols(int m, int n, int num_cu)
{
    if (num_cu <= 0) num_cu = 256;
    const long gm = ((long)m + BM - 1) / BM;
    const long t128 = gm * (((long)n + 127) / 128), t64 = gm * (((long)n + 63) / 64);
    // rounds in units of a 128 x 64 tile: a 128-column tile costs two
    const long r128 = 2 * ((t128 + num_cu - 1) / num_cu), r64 = (t64 + num_cu - 1) / num_cu;
    return r64 < r128 ? 64 : 128;
}

// the tile grid and the 16-byte flags of the fp32 operands (A: along m for op = N, along k for op = C - the same test on base
// pointer and leading dimension); false: more tiles than a launch can hold
bool plan(Args& a, bool cplx, int m, int n, int k, const float* A, long lda, const float* B, long ldb, int bn)
{
    a.m = m; a.n = n; a.k = k < 0 ? 0 : k;
    a.A = A; a.lda = lda; a.B = B; a.ldb = ldb;
    const long gm = ((long)m + BM - 1) / BM, gn = ((long)n + bn - 1) / bn;
    if (gm * gn > 0x7fffffffL) return false;
    a.gn = (int)gn;
    a.total = (unsigned)(gm * gn);
    const long ldmask = cplx ? 1 : 3;          // leading dimension in 16-byte units
    a.vecA = (a.k > 0 && al16(A) && (lda & ldmask) == 0) ? 1 : 0;
    a.vecB = (a.k > 0 && al16(B) && (ldb & ldmask) == 0) ? 1 : 0;
    return true;
}

} // namespace

int gemm_f32w(hipStream_t st, bool cplx, char opA, int m, int n, int k, const double* alpha, const float* A, long lda,
              const float* B, long ldb, const double* beta, double* C, long ldc, int num_cu, int tag)
{
    const bool opn = opA == 'N' || opA == 'n';
    const bool opc = opA == 'C' || opA == 'c' || (!cplx && (opA == 'T' || opA == 't'));
    if (!opn && !opc) return GEMM_F32_EOP;
    if (m <= 0 || n <= 0) return 0;
    const int bn = tile_cols(m, n, num_cu);
    Args a;
    if (!plan(a, cplx, m, n, k, A, lda, B, ldb, bn)) return (int)hipErrorInvalidValue;
    a.ar = a.ai = a.br = a.bi = 0.f; a.C = nullptr;
    a.war = alpha[0]; a.wai = cplx ? alpha[1] : 0.0;
    a.wbr = beta[0]; a.wbi = cplx ? beta[1] : 0.0;
    a.Cw = C; a.ldc = ldc;
    a.vecC = (al16(C) && (cplx || (ldc & 1) == 0)) ? 1 : 0;       // 16 bytes: two real / one complex fp64 element
    if (cplx) {
        if (opc) return bn == 64 ? launch<true, 1, true, true>(st, a, tag) : launch<true, 2, true, true>(st, a, tag);
        return bn == 64 ? launch<true, 1, false, true>(st, a, tag) : launch<true, 2, false, true>(st, a, tag);
    }
    if (opc) return bn == 64 ? launch<false, 1, true, true>(st, a, tag) : launch<false, 2, true, true>(st, a, tag);
    return bn == 64 ? launch<false, 1, false, true>(st, a, tag) : launch<false, 2, false, true>(st, a, tag);
}

int gemm_f32(hipStream_t st, bool cplx, char opA, int m, int n, int k, const float* alpha, const float* A, long lda, const float* B,
             long ldb, const float* beta, float* C, long ldc, int num_cu, int tag)
{
    if (opA != 'N' && opA != 'n') return GEMM_F32_EOP;
    if (m <= 0 || n <= 0) return 0;
    const int bn = tile_cols(m, n, num_cu);
    Args a;
    if (!plan(a, cplx, m, n, k, A, lda, B, ldb, bn)) return (int)hipErrorInvalidValue;
    a.ar = alpha[0]; a.ai = cplx ? alpha[1] : 0.f;
    a.br = beta[0]; a.bi = cplx ? beta[1] : 0.f;
    a.C = C; a.ldc = ldc;
    a.war = a.wai = a.wbr = a.wbi = 0.0; a.Cw = nullptr;
    a.vecC = (al16(C) && (ldc & (cplx ? 1 : 3)) == 0) ? 1 : 0;
    if (cplx) return bn == 64 ? launch<true, 1>(st, a, tag) : launch<true, 2>(st, a, tag);
    return bn == 64 ? launch<false, 1>(st, a, tag) : launch<false, 2>(st, a, tag);
}

} // namespace chase_hip
