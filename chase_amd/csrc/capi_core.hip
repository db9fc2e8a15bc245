// capi_core.hip — context, memory plumbing, GEMM and probe entry points of the C ABI (include/chase_hip.h)
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include "../../include/chase_hip.h"
#include "ctx.h"
#include "kernels.h"
#include "gemm_sp_frame.h"

namespace chase_hip {
thread_local std::string g_last_error;
int set_error(int code, const char* what)
{
    g_last_error = what ? what : "";
    return code;
}
int hip_fail(hipError_t e, const char* where)
{
    char buf[512];
    snprintf(buf, sizeof buf, "%s: %s", where, hipGetErrorString(e));
    g_last_error = buf;
    return -(int)e;
}
} // namespace chase_hip

using namespace chase_hip;

#define HIPCHK(x)                                                                                                      \
    do {                                                                                                               \
        hipError_t e_ = (x);                                                                                           \
        if (e_ != hipSuccess) return hip_fail(e_, #x);                                                                 \
    } while (0)

extern "C" {

const char* chase_hip_version(void) { return "chase_hip 0.1 (gfx950)"; }
int chase_hip_device_count(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}
const char* chase_hip_last_error(void) { return g_last_error.c_str(); }

int chase_hip_ctx_create(chase_hip_ctx** out, int device, void* stream)
{
    if (!out) return set_error(CHASE_HIP_EINVAL, "ctx_create: out == NULL");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return set_error(CHASE_HIP_ENODEV, "no HIP device visible");
    if (device < 0 || device >= ndev) return set_error(CHASE_HIP_EINVAL, "ctx_create: bad device ordinal");
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        char buf[256];
        snprintf(buf, sizeof buf, "device %d is %s; this library carries gfx950 (MI355X) code objects only", device,
                 prop.gcnArchName);
        return set_error(CHASE_HIP_ENODEV, buf);
    }
    chase_hip_ctx* c = new chase_hip_ctx();
    c->device = device;
    c->num_cu = prop.multiProcessorCount;
    c->clock_khz = prop.clockRate;
    c->hbm_bytes = prop.totalGlobalMem;
    snprintf(c->name, sizeof c->name, "%s (%s)", prop.name, prop.gcnArchName);
    if (stream) {
        c->stream = (hipStream_t)stream;
        c->own_stream = false;
    } else {
        HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    HIPCHK(hipEventCreate(&c->ev0));
    HIPCHK(hipEventCreate(&c->ev1));
    *out = c;
    return 0;
}

int chase_hip_ctx_destroy(chase_hip_ctx* c)
{
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->ws) (void)hipFree(c->ws);
    for (int i = 0; i < chase_hip_ctx::NBUF; ++i)
        if (c->bufs[i]) (void)hipFree(c->bufs[i]);
    if (c->hstage) (void)hipHostFree(c->hstage);
    (void)hipEventDestroy(c->ev0);
    (void)hipEventDestroy(c->ev1);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return 0;
}

int chase_hip_ctx_sync(chase_hip_ctx* c)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

void* chase_hip_ctx_stream(chase_hip_ctx* c) { return c ? (void*)c->stream : nullptr; }

/* operator log: on != 0 starts a fresh log, 0 stops it; the text ('\n'-separated lines "name a b c d") stays readable until
 * the next call with on != 0 */
int chase_hip_ctx_oplog(chase_hip_ctx* c, int on)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    if (on) { c->oplog.clear(); c->oplog_mute = 0; }
    c->oplog_on = on != 0;
    return 0;
}
/* delta > 0: operators executed from now on are not listed (nestable), delta < 0: listed again */
int chase_hip_ctx_oplog_mute(chase_hip_ctx* c, int delta)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    c->oplog_mute += delta;
    if (c->oplog_mute < 0) c->oplog_mute = 0;
    return 0;
}
const char* chase_hip_ctx_oplog_text(chase_hip_ctx* c)
{
    if (!c) return "";
    c->oplog_text.clear();
    for (const auto& l : c->oplog) { c->oplog_text += l; c->oplog_text += '\n'; }
    return c->oplog_text.c_str();
}

int chase_hip_device_bus_id(chase_hip_ctx* c, char* out, int len)
{
    if (!c || !out || len < 16) return set_error(CHASE_HIP_EINVAL, "device_bus_id: bad argument");
    HIPCHK(hipDeviceGetPCIBusId(out, len, c->device));
    return 0;
}

int chase_hip_device_info(chase_hip_ctx* c, int* num_cu, int* clock_khz, size_t* hbm_bytes, char* name, int name_len)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (num_cu) *num_cu = c->num_cu;
    if (clock_khz) *clock_khz = c->clock_khz;
    if (hbm_bytes) *hbm_bytes = c->hbm_bytes;
    if (name && name_len > 0) {
        strncpy(name, c->name, (size_t)name_len - 1);
        name[name_len - 1] = 0;
    }
    return 0;
}

int chase_hip_malloc(chase_hip_ctx* c, void** dev, size_t bytes)
{
    if (!c || !dev) return set_error(CHASE_HIP_EINVAL, "malloc: NULL argument");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    HIPCHK(hipSetDevice(c->device));
    hipError_t e = hipMalloc(dev, bytes ? bytes : 16);
    if (e == hipErrorOutOfMemory) return set_error(CHASE_HIP_ENOMEM, "hipMalloc: out of memory");
    HIPCHK(e);
    return 0;
}
int chase_hip_free(chase_hip_ctx* c, void* dev)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (dev) {
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipFree(dev));
    }
    return 0;
}
int chase_hip_memcpy_h2d(chase_hip_ctx* c, void* dev, const void* host, size_t bytes)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    HIPCHK(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
int chase_hip_memcpy_d2h(chase_hip_ctx* c, void* host, const void* dev, size_t bytes)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
int chase_hip_memcpy_d2d(chase_hip_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}
int chase_hip_memset(chase_hip_ctx* c, void* dev, int value, size_t bytes)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    HIPCHK(hipMemsetAsync(dev, value, bytes, c->stream));
    return 0;
}
int chase_hip_timer_start(chase_hip_ctx* c)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    return 0;
}
int chase_hip_timer_stop(chase_hip_ctx* c, float* ms)
{
    if (!c || !ms) return set_error(CHASE_HIP_EINVAL, "timer_stop: NULL argument");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    HIPCHK(hipEventSynchronize(c->ev1));
    HIPCHK(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return 0;
}

static int check_gemm(char opA, int m, int n, int k, const void* A, long lda, const void* B, long ldb, const void* C,
                      long ldc)
{
    const bool opn = (opA == 'N' || opA == 'n');
    const bool opc = (opA == 'C' || opA == 'c' || opA == 'T' || opA == 't');
    if (!opn && !opc) return set_error(CHASE_HIP_EINVAL, "gemm: opA must be 'N' or 'C'");
    if (m < 0 || n < 0 || k < 0) return set_error(CHASE_HIP_EINVAL, "gemm: negative dimension");
    if (m == 0 || n == 0) return 0;
    if (!C || (k > 0 && (!A || !B))) return set_error(CHASE_HIP_EINVAL, "gemm: NULL matrix pointer");
    const long arows = opn ? m : k;
    // (an operand without rows - k = 0: a rank that owns no rows of the block - may come with leading dimension 0; the
    // product is then beta C and nothing of A or B is read)
    if (lda < arows || ldb < k || ldc < m || (k > 0 && (lda < 1 || ldb < 1)))
        return set_error(CHASE_HIP_EINVAL, "gemm: leading dimension too small");
    return 0;
}

int chase_hip_gemm_d(chase_hip_ctx* c, char opA, int m, int n, int k, double alpha, const double* A, long lda,
                     const double* B, long ldb, double beta, double* C, long ldc)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    int rc = check_gemm(opA, m, n, k, A, lda, B, ldb, C, ldc);
    if (rc) return rc;
    return c->gemm(false, opA, m, n, k, &alpha, A, lda, B, ldb, &beta, C, ldc);
}

int chase_hip_gemm_z(chase_hip_ctx* c, char opA, int m, int n, int k, const double alpha[2], const void* A, long lda,
                     const void* B, long ldb, const double beta[2], void* C, long ldc)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (!alpha || !beta) return set_error(CHASE_HIP_EINVAL, "gemm_z: NULL alpha/beta");
    int rc = check_gemm(opA, m, n, k, A, lda, B, ldb, C, ldc);
    if (rc) return rc;
    return c->gemm(true, opA, m, n, k, alpha, (const double*)A, lda, (const double*)B, ldb, beta, (double*)C, ldc);
}

// split: the bf16x3 product (gemm_mfma_bf16x3.hip) instead of the fp32 MFMA one
static int gemm32(chase_hip_ctx* c, bool cplx, char opA, int m, int n, int k, const float* alpha, const float* A, long lda,
                  const float* B, long ldb, const float* beta, float* C, long ldc, bool split = false)
{
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (opA != 'N' && opA != 'n')
        return set_error(CHASE_HIP_EINVAL, "gemm_s / gemm_c: opA must be 'N' (the single-precision product is the filter's)");
    int rc = check_gemm(opA, m, n, k, A, lda, B, ldb, C, ldc);
    if (rc || m == 0 || n == 0) return rc;
    if (c->oplog_on) c->oplog_add(split ? (cplx ? "gemm_c3N" : "gemm_s3N") : (cplx ? "gemm_cN" : "gemm_sN"), m, n, k, c->phase * 100);
    int e = (split ? gemm_bf16x3 : gemm_f32)(c->stream, cplx, opA, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, c->num_cu,
                                             c->phase == 1 ? 1 : 0);
    if (e == GEMM_F32_EOP) return set_error(CHASE_HIP_EINVAL, "gemm_s / gemm_c: opA must be 'N'");
    if (e) return hip_fail((hipError_t)e, split ? "gemm_bf16x3 launch" : "gemm_f32 launch");
    return 0;
}

int chase_hip_gemm_s(chase_hip_ctx* c, char opA, int m, int n, int k, float alpha, const float* A, long lda, const float* B,
                     long ldb, float beta, float* C, long ldc)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    return gemm32(c, false, opA, m, n, k, &alpha, A, lda, B, ldb, &beta, C, ldc);
}

int chase_hip_gemm_c(chase_hip_ctx* c, char opA, int m, int n, int k, const float alpha[2], const void* A, long lda,
                     const void* B, long ldb, const float beta[2], void* C, long ldc)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    if (!alpha || !beta) return set_error(CHASE_HIP_EINVAL, "gemm_c: NULL alpha/beta");
    return gemm32(c, true, opA, m, n, k, alpha, (const float*)A, lda, (const float*)B, ldb, beta, (float*)C, ldc);
}

// C32 = alpha op(A32) B32 + beta C32, op(A) = N or C (real: T as well): chase_hip_gemm_s / _c with the k-contiguous operand path
static int gemm32_op(chase_hip_ctx* c, bool cplx, char opA, int m, int n, int k, const float* alpha, const float* A, long lda,
                     const float* B, long ldb, const float* beta, float* C, long ldc)
{
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    const bool opn = opA == 'N' || opA == 'n';
    const bool opc = opA == 'C' || opA == 'c' || (!cplx && (opA == 'T' || opA == 't'));
    if (!opn && !opc)
        return set_error(CHASE_HIP_EINVAL, cplx ? "gemm_c_op: opA must be 'N' or 'C'" : "gemm_s_op: opA must be 'N', 'C' or 'T'");
    int rc = check_gemm(opA, m, n, k, A, lda, B, ldb, C, ldc);
    if (rc || m == 0 || n == 0) return rc;
    if (c->oplog_on) c->oplog_add(cplx ? (opn ? "gemm_c_opN" : "gemm_c_opC") : (opn ? "gemm_s_opN" : "gemm_s_opC"), m, n, k, c->phase * 100);
    int e = gemm_f32_op(c->stream, cplx, opA, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, c->num_cu, c->phase == 1 ? 1 : 0);
    if (e == GEMM_F32_EOP) return set_error(CHASE_HIP_EINVAL, "gemm_s_op / gemm_c_op: bad opA");
    if (e) return hip_fail((hipError_t)e, "gemm_f32_op launch");
    return 0;
}

int chase_hip_gemm_s_op(chase_hip_ctx* c, char opA, int m, int n, int k, float alpha, const float* A, long lda, const float* B,
                        long ldb, float beta, float* C, long ldc)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    return gemm32_op(c, false, opA, m, n, k, &alpha, A, lda, B, ldb, &beta, C, ldc);
}

int chase_hip_gemm_c_op(chase_hip_ctx* c, char opA, int m, int n, int k, const float alpha[2], const void* A, long lda,
                        const void* B, long ldb, const float beta[2], void* C, long ldc)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    if (!alpha || !beta) return set_error(CHASE_HIP_EINVAL, "gemm_c_op: NULL alpha/beta");
    return gemm32_op(c, true, opA, m, n, k, alpha, (const float*)A, lda, (const float*)B, ldb, beta, (float*)C, ldc);
}

int chase_hip_gemm_s_bf16x3(chase_hip_ctx* c, char opA, int m, int n, int k, float alpha, const float* A, long lda, const float* B,
                            long ldb, float beta, float* C, long ldc)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    return gemm32(c, false, opA, m, n, k, &alpha, A, lda, B, ldb, &beta, C, ldc, true);
}

int chase_hip_gemm_c_bf16x3(chase_hip_ctx* c, char opA, int m, int n, int k, const float alpha[2], const void* A, long lda,
                            const void* B, long ldb, const float beta[2], void* C, long ldc)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    if (!alpha || !beta) return set_error(CHASE_HIP_EINVAL, "gemm_c: NULL alpha/beta");
    return gemm32(c, true, opA, m, n, k, alpha, (const float*)A, lda, (const float*)B, ldb, beta, (float*)C, ldc, true);
}

// ---- the bf16x3 product on a packed A (gemm_mfma_bf16x3p.hip) ----
int chase_hip_bf16x3_pack_bytes(int cplx, int m, int k, size_t* bytes)
{
    if (!bytes) return set_error(CHASE_HIP_EINVAL, "bf16x3_pack_bytes: bytes == NULL");
    if (m < 0 || k < 0) return set_error(CHASE_HIP_EINVAL, "bf16x3_pack_bytes: negative dimension");
    *bytes = bf16x3_pack_bytes(cplx != 0, m, k);
    return 0;
}

int chase_hip_bf16x3_pack(chase_hip_ctx* c, int cplx, int src_f64, int m, int k, const void* A, long lda, void* packed)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "bf16x3_pack: NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add("bf16x3_pack", m, k, 0, 0);
    if (m < 0 || k < 0 || lda < m) return set_error(CHASE_HIP_EINVAL, "bf16x3_pack: bad shape");
    if (m == 0 || k == 0) return 0;
    if (!A || !packed) return set_error(CHASE_HIP_EINVAL, "bf16x3_pack: NULL matrix");
    if (((uintptr_t)packed & 15) != 0) return set_error(CHASE_HIP_EINVAL, "bf16x3_pack: packed must be 16-byte aligned");
    int e = bf16x3_pack(c->stream, cplx != 0, src_f64 != 0, m, k, A, lda, packed);
    if (e) return hip_fail((hipError_t)e, "bf16x3_pack launch");
    return 0;
}

int chase_hip_bf16x3_pack_diag(chase_hip_ctx* c, int cplx, int n, const void* H64, long ldh, void* packed)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "bf16x3_pack_diag: NULL ctx");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    if (c->oplog_on) c->oplog_add("bf16x3_pack_diag", n, 0, 0, 0);
    if (n < 0 || ldh < n) return set_error(CHASE_HIP_EINVAL, "bf16x3_pack_diag: bad shape");
    if (n == 0) return 0;
    if (!H64 || !packed) return set_error(CHASE_HIP_EINVAL, "bf16x3_pack_diag: NULL argument");
    int e = bf16x3_pack_diag(c->stream, cplx != 0, n, (const double*)H64, ldh, packed);
    if (e) return hip_fail((hipError_t)e, "bf16x3_pack_diag launch");
    return 0;
}

static int gemm32p(chase_hip_ctx* c, bool cplx, int m, int n, int k, const float* alpha, const void* packedA, const float* B, long ldb,
                   const float* beta, float* C, long ldc)
{
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    int rc = check_gemm('N', m, n, k, packedA, m, B, ldb, C, ldc);
    if (rc || m == 0 || n == 0) return rc;
    if (k > 0 && ((uintptr_t)packedA & 15) != 0) return set_error(CHASE_HIP_EINVAL, "gemm_bf16x3p: packedA must be 16-byte aligned");
    if (c->oplog_on) c->oplog_add(cplx ? "gemm_c3pN" : "gemm_s3pN", m, n, k, c->phase * 100);
    int e = gemm_bf16x3p(c->stream, cplx, m, n, k, alpha, packedA, B, ldb, beta, C, ldc, c->num_cu, c->phase == 1 ? 1 : 0);
    if (e) return hip_fail((hipError_t)e, "gemm_bf16x3p launch");
    return 0;
}

int chase_hip_gemm_s_bf16x3p(chase_hip_ctx* c, int m, int n, int k, float alpha, const void* packedA, const float* B, long ldb,
                             float beta, float* C, long ldc)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    return gemm32p(c, false, m, n, k, &alpha, packedA, B, ldb, &beta, C, ldc);
}

int chase_hip_gemm_c_bf16x3p(chase_hip_ctx* c, int m, int n, int k, const float alpha[2], const void* packedA, const void* B, long ldb,
                             const float beta[2], void* C, long ldc)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    if (!alpha || !beta) return set_error(CHASE_HIP_EINVAL, "gemm_c_bf16x3p: NULL alpha/beta");
    return gemm32p(c, true, m, n, k, alpha, packedA, (const float*)B, ldb, beta, (float*)C, ldc);
}

// fp32 operands, fp64 result and scalars, op(A) = N or C: the filter product of the grid solver
static int gemm32w(chase_hip_ctx* c, bool cplx, char opA, int m, int n, int k, const double* alpha, const float* A, long lda,
                   const float* B, long ldb, const double* beta, double* C, long ldc, bool split = false)
{
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    const bool opn = opA == 'N' || opA == 'n';
    const bool opc = opA == 'C' || opA == 'c' || (!cplx && (opA == 'T' || opA == 't'));
    if (!opn && !opc)
        return set_error(CHASE_HIP_EINVAL, cplx ? "gemm_cz: opA must be 'N' or 'C'" : "gemm_sd: opA must be 'N', 'C' or 'T'");
    int rc = check_gemm(opA, m, n, k, A, lda, B, ldb, C, ldc);
    if (rc || m == 0 || n == 0) return rc;
    if (c->oplog_on) {
        const char* name = split ? (cplx ? (opn ? "gemm_cz3N" : "gemm_cz3C") : (opn ? "gemm_sd3N" : "gemm_sd3C"))
                                 : (cplx ? (opn ? "gemm_czN" : "gemm_czC") : (opn ? "gemm_sdN" : "gemm_sdC"));
        c->oplog_add(name, m, n, k, c->phase * 100);
    }
    // gemm_min_rounds > 0: the product may be cut into K pieces (sp_frame::split_plan) - the slabs live in the context's
    // split-K workspace, sized for the shape as chase_hip_ctx::gemm sizes it; 0: not one launch or allocation more than before
    if (c->gemm_min_rounds > 0) {
        const size_t need = chase_hip_gemm_sp_workspace_bytes(split, cplx, opA, m, n, k, c->num_cu, c->gemm_min_rounds);
        if (need && (rc = c->ensure_ws((need + ((size_t)32 << 20) - 1) & ~(((size_t)32 << 20) - 1)))) return rc;
    }
    int pieces = 1;
    int e = (split ? gemm_bf16x3w : gemm_f32w)(c->stream, cplx, opA, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, c->num_cu,
                                               c->phase == 1 ? 1 : 0, (double*)c->ws, c->ws_bytes, c->gemm_min_rounds, &pieces);
    if (e == GEMM_F32_EOP) return set_error(CHASE_HIP_EINVAL, "gemm_sd / gemm_cz: bad opA");
    if (e == GEMM_F64_EWORKSPACE)
        return set_error(CHASE_HIP_EINVAL, "gemm_sd / gemm_cz: split-K workspace smaller than gemm_sp_workspace_bytes for this shape");
    if (e) return hip_fail((hipError_t)e, split ? "gemm_bf16x3w launch" : "gemm_f32w launch");
    ++c->sp_wide_calls;
    if (pieces > 1) { ++c->sp_split_calls; c->sp_pieces += (unsigned long long)pieces; }
    return 0;
}

int chase_hip_gemm_sd(chase_hip_ctx* c, char opA, int m, int n, int k, double alpha, const float* A, long lda, const float* B,
                      long ldb, double beta, double* C, long ldc)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    return gemm32w(c, false, opA, m, n, k, &alpha, A, lda, B, ldb, &beta, C, ldc);
}

int chase_hip_gemm_cz(chase_hip_ctx* c, char opA, int m, int n, int k, const double alpha[2], const void* A, long lda,
                      const void* B, long ldb, const double beta[2], void* C, long ldc)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    if (!alpha || !beta) return set_error(CHASE_HIP_EINVAL, "gemm_cz: NULL alpha/beta");
    return gemm32w(c, true, opA, m, n, k, alpha, (const float*)A, lda, (const float*)B, ldb, beta, (double*)C, ldc);
}

int chase_hip_gemm_sd_bf16x3(chase_hip_ctx* c, char opA, int m, int n, int k, double alpha, const float* A, long lda, const float* B,
                             long ldb, double beta, double* C, long ldc)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    return gemm32w(c, false, opA, m, n, k, &alpha, A, lda, B, ldb, &beta, C, ldc, true);
}

int chase_hip_gemm_cz_bf16x3(chase_hip_ctx* c, char opA, int m, int n, int k, const double alpha[2], const void* A, long lda,
                             const void* B, long ldb, const double beta[2], void* C, long ldc)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "ctx == NULL");
    if (!alpha || !beta) return set_error(CHASE_HIP_EINVAL, "gemm_cz: NULL alpha/beta");
    return gemm32w(c, true, opA, m, n, k, alpha, (const float*)A, lda, (const float*)B, ldb, beta, (double*)C, ldc, true);
}

/* the launch of a wide single-precision product (chase_hip_gemm_sd / _cz, bf16x3 != 0: their _bf16x3 twins) on a device with
 * num_cu compute units while the context's gemm_min_rounds is min_rounds: host only, a pure function of its arguments */
int chase_hip_gemm_sp_plan(int bf16x3, int cplx, char opA, int m, int n, int k, int num_cu, int min_rounds,
                           chase_hip_gemm_sp_launch* out)
{
    const bool opn = (opA == 'N' || opA == 'n'), opc = (opA == 'C' || opA == 'c' || (!cplx && (opA == 'T' || opA == 't')));
    if (!opn && !opc) return set_error(CHASE_HIP_EINVAL, "gemm_sp_plan: opA must be 'N' or 'C'");
    if (m < 0 || n < 0 || k < 0 || !out) return set_error(CHASE_HIP_EINVAL, "gemm_sp_plan: bad argument");
    const int kind = bf16x3 ? sp_frame::KIND_BF16X3 : sp_frame::KIND_F32;
    const int bn = sp_frame::wide_tile_cols(kind, cplx != 0, m, n, num_cu);
    const sp_frame::SplitPlan sp = sp_frame::split_plan(kind, cplx != 0, m, n, k, bn, num_cu, min_rounds);
    out->bn = bn;
    out->gm = (int)(((long)m + sp_frame::BM - 1) / sp_frame::BM);
    out->gn = (int)(((long)n + bn - 1) / bn);
    out->sk = sp.sk;
    out->kchunk = sp.kchunk;
    out->min_piece_k = sp_frame::min_piece_k(kind, cplx != 0);
    out->slab_bytes = sp.slab_bytes;
    return 0;
}
/* bytes of split-K workspace that launch uses (0: whole K) */
size_t chase_hip_gemm_sp_workspace_bytes(int bf16x3, int cplx, char opA, int m, int n, int k, int num_cu, int min_rounds)
{
    chase_hip_gemm_sp_launch l;
    return chase_hip_gemm_sp_plan(bf16x3, cplx, opA, m, n, k, num_cu, min_rounds, &l) == 0 ? l.slab_bytes : 0;
}
int chase_hip_ctx_gemm_sp_counters(chase_hip_ctx* c, unsigned long long* wide_calls, unsigned long long* split_calls,
                                   unsigned long long* pieces, int reset)
{
    if (!c) return set_error(CHASE_HIP_EINVAL, "gemm_sp_counters: NULL context");
    if (wide_calls) *wide_calls = c->sp_wide_calls;
    if (split_calls) *split_calls = c->sp_split_calls;
    if (pieces) *pieces = c->sp_pieces;
    if (reset) c->sp_wide_calls = c->sp_split_calls = c->sp_pieces = 0;
    return 0;
}

/* bytes of split-K workspace chase_hip_gemm_{d,z} uses for this shape on a device with num_cu compute units (a pure function
 * of the shape: the launcher never picks another split to fit what happens to be allocated) */
size_t chase_hip_gemm_workspace_bytes(int cplx, char opA, int m, int n, int k, int num_cu, int min_rounds)
{
    return gemm_f64_ws_need(cplx != 0, opA, m, n, k, num_cu, min_rounds);
}
int chase_hip_gemm_plan(int cplx, char opA, int m, int n, int k, long lda, long ldb, int aligned16, int phase, int num_cu,
                        int min_rounds, chase_hip_gemm_launch* out, int max_out)
{
    const bool opn = (opA == 'N' || opA == 'n'), opc = (opA == 'C' || opA == 'c' || opA == 'T' || opA == 't');
    if (!opn && !opc) return set_error(CHASE_HIP_EINVAL, "gemm_plan: opA must be 'N' or 'C'");
    if (m < 0 || n < 0 || k < 0 || num_cu <= 0 || max_out < 0) return set_error(CHASE_HIP_EINVAL, "gemm_plan: bad argument");
    return gemm_f64_plan(cplx != 0, opA, m, n, k, lda, ldb, aligned16 != 0, phase, num_cu, min_rounds < 0 ? 0 : min_rounds, out,
                         max_out);
}
int chase_hip_gemm3m_enabled(void) { return gemm3m_enabled(); }
int chase_hip_set_gemm3m(int on)
{
    gemm3m_set(on);
    return 0;
}

int chase_hip_ctx_gemm_counters(chase_hip_ctx* c, int phase, double* flops_model, double* flops_executed,
                                unsigned long long* calls, int reset)
{
    if (!c || phase < 0 || phase > 3) return set_error(CHASE_HIP_EINVAL, "gemm_counters: bad argument");
    if (flops_model) *flops_model = c->flops_model[phase];
    if (flops_executed) *flops_executed = c->flops_exec[phase];
    if (calls) *calls = c->gemm_calls[phase];
    if (reset) { c->flops_model[phase] = c->flops_exec[phase] = 0; c->gemm_calls[phase] = 0; }
    return 0;
}

int chase_hip_mfma_f64_peak(chase_hip_ctx* c, double* tflops)
{
    if (!c || !tflops) return set_error(CHASE_HIP_EINVAL, "mfma_peak: NULL argument");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    const int blocks = c->num_cu * 2, iters = 16384;           // ~7 ms at peak: long enough for the clock to settle
    double* out = nullptr;
    HIPCHK(hipMalloc((void**)&out, (size_t)blocks * 256 * sizeof(double)));
    mfma_f64_peak(c->stream, out, blocks, 64); // warm-up
    float best = 1e30f;
    for (int rep = 0; rep < 5; ++rep) {
        HIPCHK(hipEventRecord(c->ev0, c->stream));
        int e = mfma_f64_peak(c->stream, out, blocks, iters);
        if (e) { hipFree(out); return hip_fail((hipError_t)e, "mfma_peak launch"); }
        HIPCHK(hipEventRecord(c->ev1, c->stream));
        HIPCHK(hipEventSynchronize(c->ev1));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        if (ms < best) best = ms;
    }
    HIPCHK(hipFree(out));
    // per wave per iteration: 16 MFMAs x (16*16*4*2) flops
    const double flops = (double)blocks * 4 /*waves*/ * iters * 16.0 * 2048.0;
    *tflops = flops / (best * 1e-3) / 1e12;
    return 0;
}

int chase_hip_hbm_copy_peak(chase_hip_ctx* c, size_t bytes, double* gbps)
{
    if (!c || !gbps) return set_error(CHASE_HIP_EINVAL, "hbm_copy_peak: NULL argument");
    (void)hipSetDevice(c->device);      // entry points may be called with another device current
    bytes &= ~(size_t)4095;
    if (bytes < 4096) return set_error(CHASE_HIP_EINVAL, "hbm_copy_peak: size too small");
    char *a = nullptr, *b = nullptr;
    HIPCHK(hipMalloc((void**)&a, bytes));
    hipError_t e = hipMalloc((void**)&b, bytes);
    if (e != hipSuccess) { hipFree(a); return hip_fail(e, "hipMalloc"); }
    hipMemsetAsync(a, 1, bytes, c->stream);
    stream_copy(c->stream, b, a, bytes);
    float best = 1e30f;
    for (int rep = 0; rep < 5; ++rep) {
        hipEventRecord(c->ev0, c->stream);
        stream_copy(c->stream, b, a, bytes);
        hipEventRecord(c->ev1, c->stream);
        hipEventSynchronize(c->ev1);
        float ms = 0;
        hipEventElapsedTime(&ms, c->ev0, c->ev1);
        if (ms < best) best = ms;
    }
    hipFree(a);
    hipFree(b);
    *gbps = 2.0 * (double)bytes / (best * 1e-3) / 1e9;
    return 0;
}

} // extern "C"
