"""The launch sequence and the output bits of every entry point of chase_amd/csrc/capi_gev.hip, fp64 and fp32: the case list and
the function that runs it on a context.  tests/test_gpu_gev_launches.py holds a build against tests/golden/gev_launches.json.

The golden file pins the drivers as they were BEFORE they were written once for both precisions: it was recorded with run_cases on
a build of commit 1360b4a (two recordings, which agreed), and a later build must reproduce it - the file is not regenerated from
a build under test.  A refactoring of the drivers may change neither the launches (their order, their shapes, the nested lines an
entry point logs below itself) nor a bit of what they compute; the bounds of test_gpu_gev*.py would notice neither a reordered
product nor a dropped log line.

Shapes: n = 321 and 33 columns, real and complex - the smallest that cross every loop boundary once: two 256-row blocks, the second
ragged, and a ragged last 64-row step; outer_nb / nb = 128 gives three outer blocks.  Inputs: the seeded generators of
gev_refs.py as gev_sp_refs.py rounds them to fp32 (widened again for the fp64 cases), in leading dimension n + 3 with the canary
in the extra rows and NaN in every triangle the contracts call "never read".

Per case the record holds
* lines: the context's operator log of the call(s) - names and shapes only, the same on every device;
* sha256: of the bytes of every downloaded device array, whole and padded (untouched rows and triangles included), followed by
  the returned values.  The fp64 GEMM plan depends on the number of compute units, so these compare on a device with the
  recording's num_cu only;
* inputs: sha256 of the host arrays that went in.  The generators go through the host's LAPACK, whose last bits differ between
  hosts; the inputs are rounded to fp32 to absorb that, and should a host still produce other input bits for a case, that
  case's output hash says nothing about the device code and is not compared."""
import hashlib

import numpy as np

import gev_sp_refs as R

N, NCOLS, PAD, BLOCK = 321, 33, 3, 128
KAPPA = 10.0


def _sha(arrays, extra=()):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.asfortranarray(a).tobytes(order="F"))
    h.update(repr(tuple(int(x) for x in extra)).encode())
    return h.hexdigest()


def _inputs(cplx, sp):
    """name -> padded host array.  Both precisions start from the fp32-rounded inputs of gev_sp_refs.py, fp64 from their exact
    widening: the generators go through the host's QR, products and Cholesky, whose last bits differ from host to host, and the
    rounding to fp32 absorbs that"""
    pad = lambda a: R.padded(R.nan_lower(a if sp else R.wide(a)), N + PAD)
    U, X = R.trsm_inputs(N, NCOLS, cplx)
    A, _ = R.hegst_inputs(N, cplx, KAPPA)
    S = R.potrf_input(N, cplx, KAPPA)
    return {"U": pad(U), "X": R.padded(X if sp else R.wide(X), N + PAD), "A": pad(A), "S": pad(S)}


def _cases(ctx, cplx, sp):
    """(name, names of the inputs, fn(device arrays) -> tuple of returned values); a device array's row count is its ld"""
    n, k, c = N, NCOLS, ctx
    a = lambda d: (d.ptr, d.ld)
    out = []
    if sp:
        for op in "NC":
            out.append((f"trsm_left_upper_sp op={op}", "UX", lambda U, X, op=op: c.trsm_left_upper_sp(op, n, k, *a(U), *a(X), cplx)))
            out.append((f"trmm_left_upper_sp op={op}", "UX", lambda U, X, op=op: c.trmm_left_upper_sp(op, n, k, *a(U), *a(X), cplx)))
        for ob in (0, BLOCK):
            out.append((f"potrf_upper_blocked_sp outer_nb={ob}", "S", lambda S, ob=ob: c.potrf_upper_blocked_sp(n, *a(S), cplx, ob)))
        out.append(("hegst_upper_sp", "AU", lambda A, U: c.hegst_upper_sp(n, *a(A), *a(U), cplx)))
        out.append(("gev_reduce_sp factor=1,0", "AS", lambda A, S: (c.gev_reduce_sp(1, n, *a(A), *a(S), cplx),
                                                                    c.gev_reduce_sp(0, n, *a(A), *a(S), cplx))))
        out.append(("gev_backtransform_sp", "UX", lambda U, X: c.gev_backtransform_sp(n, k, *a(U), *a(X), cplx)))
        out.append(("gev_starttransform_sp", "UX", lambda U, X: c.gev_starttransform_sp(n, k, *a(U), *a(X), cplx)))
        return out
    for op in "NC":
        out.append((f"trsm_left_upper op={op}", "UX", lambda U, X, op=op: c.trsm_left_upper(op, n, k, *a(U), *a(X), cplx)))
        out.append((f"trmm_left_upper op={op}", "UX", lambda U, X, op=op: c.trmm_left_upper(op, n, k, *a(U), *a(X), cplx)))
    for ob in (0, BLOCK):
        out.append((f"potrf_upper_blocked outer_nb={ob}", "S", lambda S, ob=ob: c.potrf_upper_blocked(n, *a(S), cplx, ob)))
        out.append((f"hegst_upper nb={ob}", "AU", lambda A, U, ob=ob: c.hegst_upper(n, *a(A), *a(U), cplx, ob)))
    out.append(("hegst_product_upper", "AU", lambda A, U: c.hegst_product_upper(n, *a(A), *a(U), cplx)))
    out.append(("gev_reduce", "AS", lambda A, S: c.gev_reduce(n, *a(A), *a(S), cplx)))
    out.append(("gev_backtransform", "UX", lambda U, X: c.gev_backtransform(n, k, *a(U), *a(X), cplx)))
    for it in (1, 2, 3):
        out.append((f"gev_reduce_itype itype={it} factor=1,0", "AS", lambda A, S, it=it: (c.gev_reduce_itype(it, 1, n, *a(A), *a(S), cplx),
                                                                                        c.gev_reduce_itype(it, 0, n, *a(A), *a(S), cplx))))
        out.append((f"gev_backtransform_itype itype={it}", "UX", lambda U, X, it=it: c.gev_backtransform_itype(it, n, k, *a(U), *a(X), cplx)))
        out.append((f"gev_starttransform itype={it}", "UX", lambda U, X, it=it: c.gev_starttransform(it, n, k, *a(U), *a(X), cplx)))
    return out


def run_cases(ctx):
    """runs every case on ctx (phase 0, no gemm_min_rounds); case id -> dict(lines, sha256, inputs), in a fixed order"""
    from chase_amd.capi import check, lib
    check(lib.chase_hip_ctx_set_phase(ctx.h, 0), "set_phase")
    ctx.set_gemm_min_rounds(0)
    rows = {}
    for sp in (False, True):
        for cplx in (False, True):
            host = _inputs(cplx, sp)
            for name, args, fn in _cases(ctx, cplx, sp):
                bufs = [host[x] for x in args]
                dev = [ctx.empty(b.shape, b.dtype).upload(b) for b in bufs]
                try:
                    ctx.oplog(True)
                    ret = fn(*dev)
                    lines = ctx.oplog_lines()
                finally:
                    ctx.oplog(False)
                ret = ret if isinstance(ret, tuple) else (0 if ret is None else ret,)
                rows[f"{name} {'complex' if cplx else 'real'}"] = dict(lines=lines, sha256=_sha([d.download() for d in dev], ret),
                                                                    inputs=_sha(bufs))
                for d in dev:
                    d.free()
    return rows
