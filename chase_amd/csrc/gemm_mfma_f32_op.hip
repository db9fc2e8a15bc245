// gemm_mfma_f32_op.hip — C32 = alpha op(A32) B32 + beta C32 with op(A) = N or C: the product of the single-precision generalized
// problem (the _sp entry points of capi_gev.hip, chase_hip_gemm_s_op / _c_op).
//
// The kernel is gemm_f32_kernel of gemm_mfma_f32.hip, taken as text: that file instantiates its OPC operand path - A read
// k-contiguous and transposed into the same m-contiguous LDS image the op N path builds, the conjugate a sign at the LDS store -
// with the fp64 epilogue only (WIDE, the grid filter's product); this translation unit adds the four instantiations with the fp32
// epilogue (real / complex x tile width).  They live here and not there so that the filter's file keeps exactly the kernels the
// filter uses.  op N does not come here at all: it IS gemm_f32, so the bits are gemm_f32's by construction; op C has the LDS image
// and the MFMA order of op N on the explicitly formed A^H, so it is that product bit for bit.  Same tile-width rule, whole K, no
// atomics.
#define CHASE_HIP_GEMM_F32_KERNEL_ONLY
#include "gemm_mfma_f32.hip"

namespace chase_hip {

int gemm_f32_op(hipStream_t st, bool cplx, char opA, int m, int n, int k, const float* alpha, const float* A, long lda, const float* B,
                long ldb, const float* beta, float* C, long ldc, int num_cu, int tag)
{
    if (opA == 'N' || opA == 'n') return gemm_f32(st, cplx, opA, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, num_cu, tag);
    const int bn = tile_cols(m, n, num_cu);
    return narrow_op(cplx, opA, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, bn, [&](const Args& a, bool) {       // op C: op N returned above
        if (cplx) return bn == 64 ? launch<true, 1, true>(st, a, 0) : launch<true, 2, true>(st, a, 0);
        return bn == 64 ? launch<false, 1, true>(st, a, 0) : launch<false, 2, true>(st, a, 0);
    });
}

} // namespace chase_hip
