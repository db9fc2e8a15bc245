// gemm_sp_frame.h — the frame the two single-precision GEMMs share (gemm_mfma_f32.hip: fp32-input MFMA, gemm_mfma_bf16x3.hip:
// split operands on the bf16 MFMA).  Both launch one 256-thread workgroup per 128 x BN output tile (BN = 64 WN) - over the whole K
// unless gemm_min_rounds asks for pieces; bitwise reproducible either way: no atomics, one fixed summation order per element -
// with four waves of 64 x BN/2 = 2 x WN MFMA tiles of 32 x 32 whose fp32 accumulators have the same C/D map.  What differs between
// the two is how operands get from HBM into LDS and how a K step is multiplied: each file keeps its kernel, its LDS images and
// its load_fast / load_slow / store_tiles / compute.  Here, once: the kernel arguments, a thread's place in the grid and the tile,
// the double-buffered K pipeline, and on the host the tile-width rule, the launch plan, the K-split rule of the wide products
// (split_plan: a launch of less than one round of workgroups that shares the chip with a collective is cut into K pieces, each
// an ordinary product into an fp64 slab of its own, summed in piece order by sp_slab_reduce of vec_kernels.hip) and the argument setup of the narrow and the wide
// entry.  The epilogue (fp32 C and fp64 C, one text) is gemm_sp_epilogue.h, which both kernels include after their K loop.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>
#include "kernels.h"

namespace chase_hip {
namespace sp_frame {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128;            // tile rows

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
    int sk, kchunk;                // WIDE: K pieces (gridDim.y) of kchunk k each, the last one takes the rest; 1, k: the whole K
    long slab;                     // WIDE: doubles between the outputs of two pieces (0 with one piece)
};

// ---- device ----------------------------------------------------------------------------------------------------------------------

// a thread's place: first row / column of its workgroup's tile, thread id, its wave's 64 x BN/2 block (wm, wn) and its lane's
// row / column (lr) and k half (lh) in a 32 x 32 MFMA tile
struct Place {
    long m0, n0;
    int tid, wm, wn, lr, lh;
};

template <int BN>
__device__ __forceinline__ Place place(const Args& a)
{
    // tile id: eight consecutive workgroups land on eight different XCDs (each with an L2 of its own) - give every XCD a
    // contiguous run of tiles, n fastest, so that the tiles sharing a row block of A meet in one L2
    unsigned id = blockIdx.x;
    if ((a.total & 7u) == 0) id = (id & 7u) * (a.total >> 3) + (id >> 3);
    const int tn = (int)(id % (unsigned)a.gn), tm = (int)(id / (unsigned)a.gn);
    const long m0 = (long)tm * BM, n0 = (long)tn * BN;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w & 1, wn = w >> 1, lr = lane & 31, lh = lane >> 5;
    return Place{m0, n0, tid, wm, wn, lr, lh};
}

// The product workgroup blockIdx.y of a tile computes: K piece [k0, k0 + k') of the launch's, k0 = blockIdx.y kchunk, as an
// ordinary product on shifted operands into the piece's own output.  One piece (sk = 1, kchunk = k, slab = 0): the launch's
// arguments as they are.  The tile order of place() works on blockIdx.x alone, so all pieces of a tile share an L2.
// The narrow products are never cut.
template <bool CPLX, bool OPC, bool WIDE>
__device__ __forceinline__ Args piece_of(const Args& a)
{
    if constexpr (!WIDE) {
        return a;
    } else {
        constexpr int E = CPLX ? 2 : 1;
        Args p = a;
        const long k0 = (long)blockIdx.y * a.kchunk;
        p.A = a.A + E * (OPC ? k0 : k0 * a.lda);
        p.B = a.B + E * k0;
        p.k = min(a.kchunk, a.k - (int)k0);
        p.Cw = a.Cw + (long)blockIdx.y * a.slab;
        // the shifted pointers as opaque scalar values, which is what the kernel arguments they replace were: seeing the sum,
        // the compiler advanced four per-lane addresses per K step where it used to advance the one scalar base (fp32 kernel,
        // complex, 128 columns, op C: 168 instead of 165 instructions per step, 1.2 % slower over the whole K)
        asm volatile("" : "+s"(p.A), "+s"(p.B));
        return p;
    }
}

// K steps [t0, t1) of BK with one kind of load: step t + 1 is fetched into registers (load(k0)) while step t is multiplied from
// LDS (compute(buf)); store_tiles(buf) moves the fetched step into LDS buffer buf.
// Deliberately NOT __forceinline__: a forced inline happens before any optimisation and gave some kernels another K-loop
// schedule and another guarded-load code than the per-kernel generic lambda this replaces.  Left to the ordinary inliner (static:
// three call sites per kernel), the kernel's lambdas are inlined into it first, as they were into that lambda, and every kernel
// comes out with the same machine code as before.  That rests on the inliner's heuristics: were a compiler to leave pipeline
// a real call, with the lambdas passed by reference, the accumulators would live in scratch - the register-budget and
// no-scratch tests of tests/test_mixed_precision_cpu.py and tests/test_sp_bf16x3_cpu.py are the guard.
template <int BK, class Load, class Store, class Compute>
static __device__ void pipeline(int t0, int t1, Load&& load, Store&& store_tiles, Compute&& compute)
{
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
}

// The whole K.  tile_fast (workgroup-uniform): the tile lies inside the matrix and its operands are addressable the way
// load_fast reads them - its full K steps run in a loop of their own whose loads have no branch per lane: all loads of a step
// are in flight together, behind the MFMAs of the step before, and are waited for only where they are stored to LDS.
// Everything else (edge tiles, unaligned operands, the K rest) takes the guarded loads.
template <int BK, class LoadFast, class LoadSlow, class Store, class Compute>
__device__ __forceinline__ void k_loop(int k, bool tile_fast, LoadFast&& load_fast, LoadSlow&& load_slow, Store&& store_tiles,
                                       Compute&& compute)
{
    const int T = (k + BK - 1) / BK;
    if (tile_fast) {
        const int Tf = k / BK;
        pipeline<BK>(0, Tf, load_fast, store_tiles, compute);
        pipeline<BK>(Tf, T, load_slow, store_tiles, compute);
    } else {
        pipeline<BK>(0, T, load_slow, store_tiles, compute);
    }
}

// 16 bytes of C to / from scalars for the epilogue (gemm_sp_epilogue.h), through HIP's own vector types: with ext_vector_type
// vectors in their place the compiler arranged the code around the K loops differently
__device__ __forceinline__ void get16(const float* p, float* v) { const float4 t = *(const float4*)p; v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
__device__ __forceinline__ void get16(const double* p, double* v) { const double2 t = *(const double2*)p; v[0] = t.x; v[1] = t.y; }
__device__ __forceinline__ void put16(float* p, const float* v) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void put16(double* p, const double* v) { *(double2*)p = make_double2(v[0], v[1]); }

// ---- host ------------------------------------------------------------------------------------------------------------------------

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// tile width of a product on a device with num_cu compute units: 128 columns unless the 64-column form fills the last round of
// workgroups better (one workgroup's worth of matrix-core work per compute unit and round; N = 16384, n = 640: 640 tiles of
// 128 x 128 leave half of the third round empty, 1280 tiles of 128 x 64 are five full rounds)
inline int tile_cols(int m, int n, int num_cu)
{
    if (num_cu <= 0) num_cu = 256;
    const long gm = ((long)m + BM - 1) / BM;
    const long t128 = gm * (((long)n + 127) / 128), t64 = gm * (((long)n + 63) / 64);
    // rounds in units of a 128 x 64 tile: a 128-column tile costs two
    const long r128 = 2 * ((t128 + num_cu - 1) / num_cu), r64 = (t64 + num_cu - 1) / num_cu;
    return r64 < r128 ? 64 : 128;
}

// the grid of 128 x bn tiles and the 16-byte flags of the fp32 operands (A: along m for op = N, along k for op = C - the same
// test on base pointer and leading dimension; the bf16x3 kernel uses vecA only for op = C, whose A it reads along k like B);
// false: more tiles than a launch can hold
inline bool plan(Args& a, bool cplx, int m, int n, int k, const float* A, long lda, const float* B, long ldb, int bn)
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
    a.sk = 1; a.kchunk = a.k; a.slab = 0;
    return true;
}

// ---- the K split of the wide products ----
// A wide product that SHARES the chip with a collective (the context's gemm_min_rounds > 0: the panel products of the pipelined
// distributed HEMM) is cut into sk K pieces per tile by the rule of forced_split (gemm_mfma_f64.hip), so that the CUs an
// all-reduce kernel takes displace a fraction of a tile and a panel with fewer tiles than workgroup slots still fills the chip.
// A function of the shape, the chip and min_rounds ONLY, never of allocation history: the summation order of a shape is fixed.
constexpr int KIND_F32 = 0, KIND_BF16X3 = 1;   // the two kernels
constexpr int MIN_PIECE_STEPS = 64;            // a piece has at least this many K steps of its kernel's BK ...
constexpr int MAX_PIECES = 8;                  // ... and a tile at most this many pieces
constexpr int PIECE_ALIGN = 16;                // pieces start on multiples of this many k: 64 (real) / 128 (complex) bytes of a
                                               // k-contiguous operand and a multiple of either kernel's BK

// k per K step of a kernel (its BK)
inline int step_k(int kind, bool cplx) { return kind == KIND_F32 && cplx ? 8 : 16; }
inline int min_piece_k(int kind, bool cplx) { return MIN_PIECE_STEPS * step_k(kind, cplx); }

// tile width of a wide product: the complex bf16x3 tile is always 128 x 64 (gemm_mfma_bf16x3.hip, LDS)
inline int wide_tile_cols(int kind, bool cplx, int m, int n, int num_cu)
{
    return (kind == KIND_BF16X3 && cplx) ? 64 : tile_cols(m, n, num_cu);
}

// sk pieces of kchunk k each (the last one takes the K rest: (sk - 1) kchunk < k <= sk kchunk, no piece empty), slab_bytes of
// fp64 workspace (0 without a split): every piece writes a dense block of (tile rows) x (tile columns) of its own.
// Only a launch of less than one round is cut: fewer tiles (workgroups) than workgroup slots (two per CU).  Measured
// (profiles/sp_ksplit.txt): such launches gain 1.05 x to 3.7 x, while panels of one round and more, cut by forced_split's
// threshold of min_rounds rounds, lost 1 - 3 % to the slab traffic.  Its work is counted as tile_cols counts it, in 128 x 64 tiles
// (a 128-column tile holds its slot twice as long): as many pieces as bring the launch to min_rounds of them per slot, capped by
// MAX_PIECES, by whole multiples of the minimum piece length in k and by the workspace cap.
struct SplitPlan { int sk, kchunk; size_t slab_bytes; };
inline SplitPlan split_plan(int kind, bool cplx, int m, int n, int k, int bn, int num_cu, int min_rounds)
{
    SplitPlan p{1, k < 0 ? 0 : k, 0};
    if (min_rounds <= 0 || m <= 0 || n <= 0 || k <= 0) return p;
    if (num_cu <= 0) num_cu = 256;
    const long gm = ((long)m + BM - 1) / BM, gn = ((long)n + bn - 1) / bn;
    const long slots = 2L * num_cu, units = gm * gn * (bn / 64), want = (long)min_rounds * slots;
    if (gm * gn >= slots || units >= want) return p;
    const size_t piece_bytes = (size_t)gm * BM * (size_t)gn * bn * sizeof(double) * (cplx ? 2 : 1);
    long sk = (want + units - 1) / units;
    if (sk > MAX_PIECES) sk = MAX_PIECES;
    if (sk > k / min_piece_k(kind, cplx)) sk = k / min_piece_k(kind, cplx);
    if (sk > (long)(GEMM_WS_CAP / piece_bytes)) sk = (long)(GEMM_WS_CAP / piece_bytes);
    if (sk < 2) return p;
    const long per = ((long)k + sk - 1) / sk;
    p.sk = (int)sk;
    p.kchunk = (int)((per + PIECE_ALIGN - 1) / PIECE_ALIGN * PIECE_ALIGN);
    p.slab_bytes = piece_bytes * (size_t)sk;
    return p;
}

// C = alpha A B + beta C in fp32, op(A) = N only, on tiles of bn columns: launch(a) starts the kernel and returns its status
template <class Launch>
int narrow(bool cplx, char opA, int m, int n, int k, const float* alpha, const float* A, long lda, const float* B, long ldb,
           const float* beta, float* C, long ldc, int bn, Launch&& launch)
{
    if (opA != 'N' && opA != 'n') return GEMM_F32_EOP;
    if (m <= 0 || n <= 0) return 0;
    Args a;
    if (!plan(a, cplx, m, n, k, A, lda, B, ldb, bn)) return (int)hipErrorInvalidValue;
    a.ar = alpha[0]; a.ai = cplx ? alpha[1] : 0.f;
    a.br = beta[0]; a.bi = cplx ? beta[1] : 0.f;
    a.C = C; a.ldc = ldc;
    a.war = a.wai = a.wbr = a.wbi = 0.0; a.Cw = nullptr;
    a.vecC = (al16(C) && (ldc & (cplx ? 1 : 3)) == 0) ? 1 : 0;
    return launch(a);
}

// narrow with op(A) = N or C (real: T as well), A for op = C a k x m array: launch(a, opc) starts the kernel.  The generalized
// problem's single-precision drivers (capi_gev.hip); narrow itself keeps refusing anything but N.
template <class Launch>
int narrow_op(bool cplx, char opA, int m, int n, int k, const float* alpha, const float* A, long lda, const float* B, long ldb,
              const float* beta, float* C, long ldc, int bn, Launch&& launch)
{
    const bool opn = opA == 'N' || opA == 'n';
    const bool opc = opA == 'C' || opA == 'c' || (!cplx && (opA == 'T' || opA == 't'));
    if (!opn && !opc) return GEMM_F32_EOP;
    return narrow(cplx, 'N', m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, bn, [&](const Args& a) { return launch(a, opc); });
}

// C64 = alpha op(A) B + beta C64 with fp64 scalars, op(A) = N or C (real: T as well): launch(a, opc) starts the kernel on
// a.total x a.sk workgroups.  sp.sk > 1 (split_plan): the pieces go to the slabs in ws (at least sp.slab_bytes) with
// alpha = 1, beta = 0, and sp_slab_reduce forms C from them on the same stream.
template <class Launch>
int wide(hipStream_t st, bool cplx, char opA, int m, int n, int k, const double* alpha, const float* A, long lda, const float* B,
         long ldb, const double* beta, double* C, long ldc, int bn, const SplitPlan& sp, double* ws, size_t ws_bytes,
         Launch&& launch)
{
    const bool opn = opA == 'N' || opA == 'n';
    const bool opc = opA == 'C' || opA == 'c' || (!cplx && (opA == 'T' || opA == 't'));
    if (!opn && !opc) return GEMM_F32_EOP;
    if (m <= 0 || n <= 0) return 0;
    Args a;
    if (!plan(a, cplx, m, n, k, A, lda, B, ldb, bn)) return (int)hipErrorInvalidValue;
    a.ar = a.ai = a.br = a.bi = 0.f; a.C = nullptr;
    if (sp.sk > 1) {
        if (!ws || ws_bytes < sp.slab_bytes) return GEMM_F64_EWORKSPACE;
        const long lds = (long)(a.total / (unsigned)a.gn) * BM, cols = (long)a.gn * bn;      // a slab: lds x cols elements
        a.war = 1.0; a.wai = a.wbr = a.wbi = 0.0;
        a.Cw = ws; a.ldc = lds; a.vecC = 1;
        a.sk = sp.sk; a.kchunk = sp.kchunk; a.slab = (cplx ? 2 : 1) * lds * cols;
        const int e = launch(a, opc);
        if (e) return e;
        return sp_slab_reduce(st, cplx, m, n, sp.sk, ws, lds, a.slab, alpha, beta, C, ldc);
    }
    a.war = alpha[0]; a.wai = cplx ? alpha[1] : 0.0;
    a.wbr = beta[0]; a.wbi = cplx ? beta[1] : 0.0;
    a.Cw = C; a.ldc = ldc;
    a.vecC = (al16(C) && (cplx || (ldc & 1) == 0)) ? 1 : 0;       // 16 bytes: two real / one complex fp64 element
    return launch(a, opc);
}

} // namespace sp_frame
} // namespace chase_hip
