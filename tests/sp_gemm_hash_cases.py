"""Content hashes of the single-precision products (chase_amd/csrc/gemm_mfma_f32.hip, gemm_mfma_bf16x3.hip and their shared frame
gemm_sp_frame.h): the case list, the function that runs it on a context, and - run as a script - the generator of
tests/golden/sp_gemm_hashes.json.

Families: {fp32 MFMA, bf16x3} x {real, complex} x {narrow op N, wide op N, wide op C}.  Every family runs the four SHAPES in
context phase 0, the first shape again in phase 1 (the filter's kernel symbols) and once more with beta = 0 (C is not read).
All inputs are made on the device: A, B, C from chase_hip_fill_normal with seeds 1, 2, 3, rounded to fp32 by Context.to_single;
alpha = 0.5 - 0.25j, beta = 0.25 + 0.5j (their real parts for real types).  A narrow result is widened by Context.to_double
(exact) before Context.hash64.  Leading dimensions are unpadded.

The kernels have no split-K and one fixed summation order per element; the tile widths named below are those the tile-width
rule picks on a device with num_cu = 256 compute units.

The golden file pins the bits of the kernels as they were BEFORE the shared frame: it was written by this script under
CHASE_HIP_LIB=<a build of commit 4f62c9a>, and a later build must reproduce it.  A mismatch means the arithmetic changed (look
for an epilogue expression that contracts differently) - the file is not regenerated from a build under test.

    CHASE_HIP_LIB=<build of the commit to pin> python tests/sp_gemm_hash_cases.py [--out FILE]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sp_gemm_hashes.json")

# (k = 72 leaves a K rest after the full steps of 16 of real fp32 and of bf16x3; complex fp32 steps by 8, so there 72 is nine full
# steps: its guarded K rest runs only at k = 37, after guarded steps, and no complex fp32 row restarts the pipeline after fast ones)
SHAPES = [(8320, 256, 72),       # 128-column tiles (65 x 2 against 65 x 4: two rounds either way); 16-byte fast path plus K rest
          (8200, 250, 37),        # 128-column tiles, ragged in m, n and k: guarded path only
          (256, 128, 72),         # 64-column tiles, fast path plus K rest
          (130, 70, 37)]          # one ragged row of 64-column tiles
FORMS = [("narrow", "N"), ("wide", "N"), ("wide", "C")]
ALPHA, BETA = 0.5 - 0.25j, 0.25 + 0.5j
# (shape, phase, beta = 0) of every family
RUNS = [(sh, 0, False) for sh in SHAPES] + [(SHAPES[0], 1, False), (SHAPES[0], 0, True)]
COUNT = 2 * 2 * len(FORMS) * len(RUNS)


def _normal(ctx, cplx, r, c, seed):
    from chase_amd.capi import check, lib
    d = ctx.empty((r, c), np.complex128 if cplx else np.float64)
    check(lib.chase_hip_fill_normal(ctx.h, int(cplx), r, c, d.ptr, r, 0, 0, r, seed), "fill_normal")
    return d


def run_cases(ctx):
    """runs every case on ctx; rows of dict(kind, cplx, form, op, m, n, k, phase, beta0, hash) in a fixed order"""
    from chase_amd.capi import check, lib
    rows = []
    try:
        for cplx in (False, True):
            alpha = ALPHA if cplx else ALPHA.real
            for (m, n, k) in SHAPES:
                runs = [(ph, b0) for (sh, ph, b0) in RUNS if sh == (m, n, k)]
                A64 = {"N": _normal(ctx, cplx, m, k, 1), "C": _normal(ctx, cplx, k, m, 1)}
                B64 = _normal(ctx, cplx, k, n, 2)
                A = {op: ctx.to_single(d) for op, d in A64.items()}
                B = ctx.to_single(B64)
                for split in (False, True):
                    for (form, op) in FORMS:
                        for (phase, beta0) in runs:
                            beta = 0.0 if beta0 else (BETA if cplx else BETA.real)
                            check(lib.chase_hip_ctx_set_phase(ctx.h, phase), "set_phase")
                            Cw = _normal(ctx, cplx, m, n, 3)
                            if form == "narrow":
                                Cs = ctx.to_single(Cw)
                                ctx.gemm32(op, m, n, k, alpha, A[op].ptr, A[op].ld, B.ptr, k, beta, Cs.ptr, m, cplx, split=split)
                                Cw.free()
                                Cw = ctx.to_double(Cs)
                                Cs.free()
                            else:
                                ctx.gemm32w(op, m, n, k, alpha, A[op].ptr, A[op].ld, B.ptr, k, beta, Cw.ptr, m, cplx, split=split)
                            rows.append(dict(kind="bf16x3" if split else "fp32", cplx=cplx, form=form, op=op, m=m, n=n, k=k,
                                             phase=phase, beta0=beta0, hash="%016x" % ctx.hash64(Cw.ptr, m, n, m, cplx)))
                            Cw.free()
                for d in list(A64.values()) + list(A.values()) + [B64, B]:
                    d.free()
    finally:
        lib.chase_hip_ctx_set_phase(ctx.h, 0)
    assert len(rows) == COUNT
    return rows


def main():
    sys.path.insert(0, ROOT)
    from chase_amd.capi import Context
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    with Context(0) as ctx:
        info = ctx.info()
        rows = run_cases(ctx)
    for r in rows:
        print(r, flush=True)
    with open(out, "w") as f:
        json.dump(dict(source="tests/sp_gemm_hash_cases.py on a build of commit 4f62c9a (before gemm_sp_frame.h)",
                       num_cu=info["num_cu"], rows=rows), f, indent=0)
        f.write("\n")
    print(f"{len(rows)} rows -> {out}")


if __name__ == "__main__":
    main()
