"""Mixed-precision Chebyshev filter: what the fp32 product and the switch buy.  Writes profiles/mixed_precision.txt.

(a) the fp32 filter product (chase_hip_gemm_s / _c) against the fp64 one (chase_hip_gemm_d / _z) at the same full-width shape, both
    launched in phase 1 like the filter does: N = 16384, n = 640 and N = 32768, n = 2560, real and complex.  The two are timed
    alternately in one process: HIP events around a window of back-to-back products, median over the windows.
(b) whole solves of bench.py's cfg2 (N = 16384 complex, nev 512, nex 128) and cfg3 (N = 32768 real, nev 1024, nex 256) on the
    bench's matrix with mixed_precision off and on: seconds, iterations, filtered vectors, columns filtered in fp32.

    python scripts/dev_mixed_precision.py [--out FILE] [--skip-solves] [--small]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MATRIX_SCALE, MATRIX_PERTURB = 100.0, 1e-6          # bench.py's matrix
PEAK_F64, PEAK_F32 = 78.6, 157.3                     # TF/s, matrix cores (spec)


def column(ctx, dA, j):
    from chase_amd.capi import lib, check
    out = np.empty(dA.shape[0], dtype=dA.dtype)
    check(lib.chase_hip_memcpy_d2h(ctx.h, out.ctypes.data, dA.offset(j), out.nbytes), "memcpy_d2h")
    return out


def product_case(ctx, N, n, cplx, windows, reps, say):
    from chase_amd.capi import lib, check
    dt = np.complex128 if cplx else np.float64
    H = ctx.gen_clement(N, cplx, scale=MATRIX_SCALE / N, perturb=MATRIX_PERTURB, seed=42)
    V = ctx.empty((N, n), dt)
    check(lib.chase_hip_fill_normal(ctx.h, int(cplx), N, n, V.ptr, N, 0, 0, N, 1337), "fill_normal")
    W = ctx.empty((N, n), dt)
    Hs, Vs = ctx.to_single(H), ctx.to_single(V)
    Ws = ctx.empty((N, n), Hs.dtype)
    alpha, beta = 0.01, 0.0

    def f64():
        ctx.gemm("N", N, n, N, alpha, H.ptr, N, V.ptr, N, beta, W.ptr, N, cplx)

    def f32():
        ctx.gemm32("N", N, n, N, alpha, Hs.ptr, N, Vs.ptr, N, beta, Ws.ptr, N, cplx)

    check(lib.chase_hip_ctx_set_phase(ctx.h, 1), "set_phase")
    for _ in range(2):                                  # warm-up: code objects, workspace, clocks
        f64(); f32()
    ctx.sync()
    # same inputs, same sizes as timed: the fp32 result against the fp64 one on two columns
    worst = 0.0
    for j in (0, n - 1):
        a, b = column(ctx, W, j), column(ctx, Ws, j)
        worst = max(worst, float(np.max(np.abs(a - b)) / np.max(np.abs(a))))
    t64, t32 = [], []
    for _ in range(windows):                            # alternating windows
        for fn, acc in ((f64, t64), (f32, t32)):
            ctx.timer_start()
            for _ in range(reps):
                fn()
            acc.append(ctx.timer_stop() / reps)
    check(lib.chase_hip_ctx_set_phase(ctx.h, 0), "set_phase")
    flops = 2.0 * (4 if cplx else 1) * N * N * n
    m64, m32 = statistics.median(t64), statistics.median(t32)
    say(f"  N={N:6d} n={n:5d} {'complex' if cplx else 'real   '}  fp64 {m64:9.3f} ms ({flops / m64 * 1e-9:6.1f} TF/s model, "
        f"min {min(t64):.3f} max {max(t64):.3f})   fp32 {m32:9.3f} ms ({flops / m32 * 1e-9:6.1f} TF/s = "
        f"{flops / m32 * 1e-9 / PEAK_F32:.2f} of the fp32 peak, min {min(t32):.3f} max {max(t32):.3f})   "
        f"ratio fp64/fp32 = {m64 / m32:.2f}   max |fp32 - fp64| / max |fp64| on two columns = {worst:.1e}")
    for a in (H, V, W, Hs, Vs, Ws):
        a.free()
    return m64 / m32


def solve_case(ctx, name, N, cplx, nev, nex, say):
    from chase_amd.capi import Solver
    dH = ctx.gen_clement(N, cplx, scale=MATRIX_SCALE / N, perturb=MATRIX_PERTURB, seed=42)
    ctx.sync()
    s = Solver(ctx, None, nev, nex, h_on_device_ptr=dH.ptr, N=N, cplx=cplx)
    s.set(device_rng=1)
    res = {}
    for label, on, runs in (("warm-up (off)", 0, 1), ("off", 0, 2), ("on", 1, 2), ("off", 0, 1), ("on", 1, 1)):
        s.set(mixed_precision=on)
        for _ in range(runs):
            s.set(reset_counters=1)
            ctx.sync()
            t0 = time.perf_counter()
            st = s.solve()
            ctx.sync()
            dt = time.perf_counter() - t0
            r = s.recompute_residuals(nev)
            rec = (dt, st["iterations"], st["filtered_vecs"], int(s.get("hemm_sp_vecs")), int(s.get("sp_filters")),
                   st["locked"], float(np.max(r)), s.get("filter_ms") * 1e-3)
            if not label.startswith("warm"):
                res.setdefault(label, []).append(rec)
            say(f"  {name} {label:13s} {dt:8.3f} s  filter {rec[7]:7.3f} s  iterations {rec[1]:2d}  filtered vectors {rec[2]:7d}  "
                f"in fp32 {rec[3]:7d} ({rec[4]} filter calls)  locked {rec[5]}  max fresh fp64 residual {rec[6]:.2e}")
    off = statistics.median(r[0] for r in res["off"])
    on = statistics.median(r[0] for r in res["on"])
    say(f"  {name}: median of 3 solves each, alternated: off {off:.3f} s, on {on:.3f} s -> the whole solve is "
        f"{'FASTER' if on < off else 'NOT faster'} with mixed precision ({off / on:.3f}x)")
    s.close()
    dH.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_precision.txt"))
    ap.add_argument("--skip-solves", action="store_true")
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    from chase_amd.capi import Context
    ctx = Context(0)
    info = ctx.info()
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)

    say("Mixed-precision Chebyshev filter (scripts/dev_mixed_precision.py)")
    say(f"device: {info['name']}, {info['num_cu']} CUs, {info['clock_khz'] / 1000:.0f} MHz max engine clock; "
        f"peaks used: fp64 MFMA {PEAK_F64} TF/s, fp32 MFMA {PEAK_F32} TF/s")
    say("(a) full-width filter product, phase 1, alpha = 0.01, beta = 0; H = the bench's Clement matrix, V ~ N(0,1); 2 warm-up "
        "products each, then alternating windows of back-to-back products between HIP events; ms per product = median of the windows")
    shapes = [(1024, 96, 3, 4), (2048, 160, 3, 4)] if args.small else [(16384, 640, 7, 20), (32768, 2560, 5, 3)]
    ratios = {}
    for (N, n, windows, reps) in shapes:
        for cplx in (False, True):
            ratios[(N, n, cplx)] = product_case(ctx, N, n, cplx, windows, reps, say)
    slow = [k for k, v in ratios.items() if v <= 1.0]
    say("  fp32 product faster than the fp64 product at every shape and type: " + ("yes" if not slow else f"NO - not at {slow}"))
    if not args.skip_solves:
        say("(b) whole solves (defaults: tol 1e-10, deg 20, opt; device start vectors), host clock around solve + synchronise; "
            "one warm-up solve, then off, off, on, on, off, on")
        cases = [("toy", 2048, True, 64, 32)] if args.small else [("cfg2", 16384, True, 512, 128), ("cfg3", 32768, False, 1024, 256)]
        for case in cases:
            solve_case(ctx, *case, say)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
