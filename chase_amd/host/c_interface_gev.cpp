// c_interface_gev.cpp — the generalized problem H x = lambda S x for callers of the C interface (include/chase_c_interface.h):
// ?chase_gev_reduce_ and ?chase_gev_backtransform_ are the ppotrf + phegst and the ptrtrs that the reference's
// docs/example/gev.rst puts around chase::Solve.  Host pointers in, results in place; the matrices are moved to the device,
// worked on by capi_gev.hip (fp64, or fp32 through its _sp entry points) and moved back.  The intended sequence: reduce -> ?chase_init_ / ?chase_ / ?chase_finalize_ on the
// reduced H -> backtransform of the eigenvectors with the U that reduce left in S.  The _itype forms and ?chase_gev_starttransform_
// add LAPACK's problem types 2 and 3 and the warm step of a sequence (mode 'A'): reduce_itype -> starttransform of the previous
// block -> ?chase_ -> backtransform_itype.
#include <cstdlib>
#include "../../include/chase_c_interface.h"
#include "../../include/chase_hip.h"

namespace {
chase_hip_ctx* g_gev_ctx = nullptr;

bool ensure_ctx()
{
    if (g_gev_ctx) return true;
    int dev = 0;
    if (const char* e = std::getenv("CHASE_HIP_DEVICE")) dev = std::atoi(e);
    return chase_hip_ctx_create(&g_gev_ctx, dev, nullptr) == 0;
}

struct DevMat {                                   // an m x n device copy of a host matrix, ld = m; sp: 4-byte scalars
    chase_hip_ctx* c;
    bool sp;
    void* p = nullptr;
    DevMat(chase_hip_ctx* c_, bool sp_) : c(c_), sp(sp_) {}
    ~DevMat() { if (p) chase_hip_free(c, p); }
    int up(int cplx, int m, int n, const void* host, int ldh)
    {
        int rc = chase_hip_malloc(c, &p, (size_t)m * n * (cplx ? 2 : 1) * (sp ? 4 : 8));
        return rc ? rc : (sp ? chase_hip_upload_matrix_sp : chase_hip_upload_matrix)(c, cplx, m, n, host, ldh, p, m);
    }
    int down(int cplx, int m, int n, void* host, int ldh)
    {
        return (sp ? chase_hip_download_matrix_sp : chase_hip_download_matrix)(c, cplx, m, n, p, m, host, ldh);
    }
};

// itype 0: the plain entry point (chase_hip_gev_reduce).  sp: float / float _Complex host matrices (the _sp entry points of
// capi_gev.hip), itype 1 only
void reduce(bool sp, int cplx, int itype, int factor, int N, void* H, int ldh, void* S, int lds, int* info)
{
    if (!info) return;
    *info = CHASE_HIP_EINVAL;
    if (itype < 0 || itype > 3 || (sp && itype != 1) || (factor != 0 && factor != 1)) return;       // itype 2 / 3: fp64 only
    if (N < 0 || ldh < N || lds < N || (N > 0 && (!H || !S))) return;
    *info = 0;
    if (N == 0) return;
    if (!ensure_ctx()) { *info = CHASE_HIP_ENODEV; return; }
    DevMat dH(g_gev_ctx, sp), dS(g_gev_ctx, sp);
    int rc = dH.up(cplx, N, N, H, ldh);
    if (!rc) rc = dS.up(cplx, N, N, S, lds);
    if (!rc) rc = sp           ? chase_hip_gev_reduce_sp(g_gev_ctx, cplx, factor, N, dH.p, N, dS.p, N)
                  : itype == 0 ? chase_hip_gev_reduce(g_gev_ctx, cplx, N, dH.p, N, dS.p, N)
                               : chase_hip_gev_reduce_itype(g_gev_ctx, cplx, itype, factor, N, dH.p, N, dS.p, N);
    if (rc) { *info = rc; return; }               // S not positive definite (rc > 0) or a runtime error: H and S as they were
    rc = dH.down(cplx, N, N, H, ldh);
    if (!rc && factor) rc = dS.down(cplx, N, N, S, lds);    // the strictly lower triangle comes back as it went
    *info = rc;
}

// itype 0: the plain entry point (chase_hip_gev_backtransform); start: chase_hip_gev_starttransform; sp: as in reduce
void backtransform(bool sp, int cplx, int itype, bool start, int N, int ncols, void* U, int ldu, void* V, int ldv, int* info)
{
    if (!info) return;
    *info = CHASE_HIP_EINVAL;
    if (itype < 0 || itype > 3 || (sp && itype != 1)) return;
    if (N < 0 || ncols < 0 || ldu < N || ldv < N || (N > 0 && (!U || (ncols > 0 && !V)))) return;
    *info = 0;
    if (N == 0 || ncols == 0) return;
    if (!ensure_ctx()) { *info = CHASE_HIP_ENODEV; return; }
    DevMat dU(g_gev_ctx, sp), dV(g_gev_ctx, sp);
    int rc = dU.up(cplx, N, N, U, ldu);
    if (!rc) rc = dV.up(cplx, N, ncols, V, ldv);
    if (!rc && sp)
        rc = start ? chase_hip_gev_starttransform_sp(g_gev_ctx, cplx, N, ncols, dU.p, N, dV.p, N)
                   : chase_hip_gev_backtransform_sp(g_gev_ctx, cplx, N, ncols, dU.p, N, dV.p, N);
    else if (!rc)
        rc = start        ? chase_hip_gev_starttransform(g_gev_ctx, cplx, itype, N, ncols, dU.p, N, dV.p, N)
             : itype == 0 ? chase_hip_gev_backtransform(g_gev_ctx, cplx, N, ncols, dU.p, N, dV.p, N)
                          : chase_hip_gev_backtransform_itype(g_gev_ctx, cplx, itype, N, ncols, dU.p, N, dV.p, N);
    if (!rc) rc = dV.down(cplx, N, ncols, V, ldv);
    *info = rc;
}

// the _itype entry points take itype 1 .. 3 only
bool itype_ok(int itype, int* info)
{
    if (itype >= 1 && itype <= 3) return true;
    if (info) *info = CHASE_HIP_EINVAL;
    return false;
}
} // namespace

extern "C" {
void dchase_gev_reduce_(int* N, double* H, int* ldh, double* S, int* lds, int* info) { reduce(false, 0, 0, 1, *N, H, *ldh, S, *lds, info); }
void zchase_gev_reduce_(int* N, void* H, int* ldh, void* S, int* lds, int* info) { reduce(false, 1, 0, 1, *N, H, *ldh, S, *lds, info); }
void dchase_gev_backtransform_(int* N, int* ncols, double* U, int* ldu, double* V, int* ldv, int* info)
{
    backtransform(false, 0, 0, false, *N, *ncols, U, *ldu, V, *ldv, info);
}
void zchase_gev_backtransform_(int* N, int* ncols, void* U, int* ldu, void* V, int* ldv, int* info)
{
    backtransform(false, 1, 0, false, *N, *ncols, U, *ldu, V, *ldv, info);
}
void dchase_gev_reduce_itype_(int* itype, int* factor, int* N, double* H, int* ldh, double* S, int* lds, int* info)
{
    if (itype_ok(*itype, info)) reduce(false, 0, *itype, *factor, *N, H, *ldh, S, *lds, info);
}
void zchase_gev_reduce_itype_(int* itype, int* factor, int* N, void* H, int* ldh, void* S, int* lds, int* info)
{
    if (itype_ok(*itype, info)) reduce(false, 1, *itype, *factor, *N, H, *ldh, S, *lds, info);
}
void dchase_gev_backtransform_itype_(int* itype, int* N, int* ncols, double* U, int* ldu, double* V, int* ldv, int* info)
{
    if (itype_ok(*itype, info)) backtransform(false, 0, *itype, false, *N, *ncols, U, *ldu, V, *ldv, info);
}
void zchase_gev_backtransform_itype_(int* itype, int* N, int* ncols, void* U, int* ldu, void* V, int* ldv, int* info)
{
    if (itype_ok(*itype, info)) backtransform(false, 1, *itype, false, *N, *ncols, U, *ldu, V, *ldv, info);
}
void dchase_gev_starttransform_(int* itype, int* N, int* ncols, double* U, int* ldu, double* V, int* ldv, int* info)
{
    if (itype_ok(*itype, info)) backtransform(false, 0, *itype, true, *N, *ncols, U, *ldu, V, *ldv, info);
}
void zchase_gev_starttransform_(int* itype, int* N, int* ncols, void* U, int* ldu, void* V, int* ldv, int* info)
{
    if (itype_ok(*itype, info)) backtransform(false, 1, *itype, true, *N, *ncols, U, *ldu, V, *ldv, info);
}

// single precision: the d / z signatures with float data; itype 2 / 3: *info = CHASE_HIP_EINVAL
void schase_gev_reduce_(int* N, float* H, int* ldh, float* S, int* lds, int* info) { reduce(true, 0, 1, 1, *N, H, *ldh, S, *lds, info); }
void cchase_gev_reduce_(int* N, void* H, int* ldh, void* S, int* lds, int* info) { reduce(true, 1, 1, 1, *N, H, *ldh, S, *lds, info); }
void schase_gev_backtransform_(int* N, int* ncols, float* U, int* ldu, float* V, int* ldv, int* info)
{
    backtransform(true, 0, 1, false, *N, *ncols, U, *ldu, V, *ldv, info);
}
void cchase_gev_backtransform_(int* N, int* ncols, void* U, int* ldu, void* V, int* ldv, int* info)
{
    backtransform(true, 1, 1, false, *N, *ncols, U, *ldu, V, *ldv, info);
}
void schase_gev_reduce_itype_(int* itype, int* factor, int* N, float* H, int* ldh, float* S, int* lds, int* info)
{
    reduce(true, 0, *itype, *factor, *N, H, *ldh, S, *lds, info);
}
void cchase_gev_reduce_itype_(int* itype, int* factor, int* N, void* H, int* ldh, void* S, int* lds, int* info)
{
    reduce(true, 1, *itype, *factor, *N, H, *ldh, S, *lds, info);
}
void schase_gev_backtransform_itype_(int* itype, int* N, int* ncols, float* U, int* ldu, float* V, int* ldv, int* info)
{
    backtransform(true, 0, *itype, false, *N, *ncols, U, *ldu, V, *ldv, info);
}
void cchase_gev_backtransform_itype_(int* itype, int* N, int* ncols, void* U, int* ldu, void* V, int* ldv, int* info)
{
    backtransform(true, 1, *itype, false, *N, *ncols, U, *ldu, V, *ldv, info);
}
void schase_gev_starttransform_(int* itype, int* N, int* ncols, float* U, int* ldu, float* V, int* ldv, int* info)
{
    backtransform(true, 0, *itype, true, *N, *ncols, U, *ldu, V, *ldv, info);
}
void cchase_gev_starttransform_(int* itype, int* N, int* ncols, void* U, int* ldu, void* V, int* ldv, int* info)
{
    backtransform(true, 1, *itype, true, *N, *ncols, U, *ldu, V, *ldv, info);
}
}
