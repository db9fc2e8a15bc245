"""The single-precision Hermitian solver (capi.SpSolver) against the fp64 one (capi.Solver) under identical settings.  Writes
profiles/sp_solver.txt; method of scripts/dev_h2_mixed.py: one process, five alternating windows, the window spread as the margin.

For config 2's and config 3's shapes (bench.py: N = 16384 complex, 512 + 128 columns; N = 32768 real, 1024 + 256 columns) on a
unit-norm matrix (chase_hip_gen_clement scaled by 1 / N, perturbation 1e-6; the fp32 matrix is its rounding, both used in place in
HBM):
(a) whole solves with the reference's float defaults on both solvers (tol 1e-5, deg 10, maxDeg 18, lanczosIter 12, optimised degrees,
    host start vectors - the single-precision solver has no device generator): host clock around solve + synchronise, one warm-up
    solve of each, then fp64 / fp32 alternated; iterations, filtered vectors, phase times, residuals, and device_bytes of both
    (the Impl's own allocations) next to the bytes of the matrix each one works on;
(b) one full-width filter product V2 = alpha H V1 of each (chase_hip_gemm_d / _z against chase_hip_gemm_s / _c), alternated windows.

    python scripts/dev_sp_solver.py [--out FILE] [--cases cfg2,cfg3] [--append] [--small]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FLOAT_DEFAULTS = dict(tol=1e-5, deg=10, maxdeg=18, lanczositer=12)


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def verdict(r, margin):
    return "faster" if r > 1 + margin else ("slower" if r < 1 - margin else "within the spread")


def solve_case(ctx, name, N, cplx, nev, nex, dH64, dH32, windows, say):
    from chase_amd.capi import Solver, SpSolver
    es = 2 if cplx else 1
    solvers = {"fp64": Solver(ctx, None, nev, nex, h_on_device_ptr=dH64.ptr, N=N, cplx=cplx),
               "fp32": SpSolver(ctx, None, nev, nex, h_on_device_ptr=dH32.ptr, N=N, cplx=cplx, ldh=N)}
    solvers["fp64"].set(**FLOAT_DEFAULTS)
    for k, s in solvers.items():
        assert all(s.get(key) == v for key, v in FLOAT_DEFAULTS.items()), k
    t = {k: [] for k in solvers}
    last = {}
    for w in range(windows + 1):                                # window 0: warm-up (code objects, workspaces, host LAPACK)
        for k, s in solvers.items():
            s.set(reset_counters=1)
            ctx.sync()
            t0 = time.perf_counter()
            st = s.solve()
            ctx.sync()
            dt = time.perf_counter() - t0
            if w:
                t[k].append((dt, dt - st["t_init"], s.get("filter_ms") * 1e-3))
            last[k] = st
            say(f"  {name} {'warm-up' if not w else 'window %d' % w} {k} {dt:8.3f} s (init {st['t_init']:.3f} lanczos {st['t_lanczos']:.3f} "
                f"filter {st['t_filter']:.3f} [device {s.get('filter_ms') * 1e-3:.3f}] qr {st['t_qr']:.3f} rr {st['t_rr']:.3f} resid "
                f"{st['t_resid']:.3f})  iterations {st['iterations']:2d}  filtered vectors {st['filtered_vecs']:7d}  locked {st['locked']}  "
                f"max solver residual {float(np.max(s.resid()[:nev])):.2e}")
    for col, what in ((0, "whole solve"), (1, "solve without initVecs (host random numbers, the same for both)"), (2, "filter, device time")):
        med = {k: statistics.median(x[col] for x in v) for k, v in t.items()}
        margin = max(spread([x[col] for x in v]) for v in t.values())
        r = med["fp64"] / med["fp32"]
        say(f"  {name} {what}: median of {windows} alternated windows: fp64 {med['fp64']:.3f} s, fp32 {med['fp32']:.3f} s: fp64 / fp32 = "
            f"{r:.3f} (fp32 {verdict(r, margin)}; largest window spread {100 * margin:.2f} %)")
    lam = {k: s.ritzv[:nev].copy() for k, s in solvers.items()}
    fresh = solvers["fp32"].recompute_residuals(nev)
    say(f"  {name}: iterations / filtered vectors fp64 {last['fp64']['iterations']} / {last['fp64']['filtered_vecs']}, fp32 "
        f"{last['fp32']['iterations']} / {last['fp32']['filtered_vecs']}; max |Ritz value fp32 - fp64| = "
        f"{float(np.max(np.abs(np.sort(lam['fp32']) - np.sort(lam['fp64'])))):.2e}; fp32 solver: max fresh residual (fp32 product, fp64 norm) "
        f"{float(np.max(fresh)):.2e}; fp32 products {int(solvers['fp32'].get('hemm_sp_calls'))}, fp64 products {int(solvers['fp32'].get('hemm_calls'))}")
    say(f"  {name}: device_bytes (the Impl's own allocations; both matrices are the caller's, used in place): fp64 "
        f"{int(solvers['fp64'].get('device_bytes'))} + matrix {N * N * 8 * es}, fp32 {int(solvers['fp32'].get('device_bytes'))} + matrix "
        f"{N * N * 4 * es}")
    for s in solvers.values():
        s.close()


def product_case(ctx, name, N, cplx, ne, dH64, dH32, min_ms, windows, say):
    rng = np.random.default_rng(7)
    V = rng.standard_normal((N, ne)) + (1j * rng.standard_normal((N, ne)) if cplx else 0)
    d64 = ctx.array(np.asfortranarray(V))
    d32 = ctx.to_single(d64)
    o64, o32 = ctx.empty(d64.shape, d64.dtype), ctx.empty(d32.shape, d32.dtype)
    run = {"fp64": lambda: ctx.gemm("N", N, ne, N, 0.5, dH64.ptr, N, d64.ptr, N, 0.0, o64.ptr, N, cplx),
           "fp32": lambda: ctx.gemm32("N", N, ne, N, 0.5, dH32.ptr, N, d32.ptr, N, 0.0, o32.ptr, N, cplx)}

    def window(k, reps):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            run[k]()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / reps

    reps = {}
    for k in run:
        window(k, 2)
        reps[k] = max(1, int(np.ceil(min_ms / windows / window(k, 1))))
    t = {k: [] for k in run}
    for _ in range(windows):
        for k in run:
            t[k].append(window(k, reps[k]))
    med = {k: statistics.median(v) for k, v in t.items()}
    flops = 2.0 * (4 if cplx else 1) * N * N * ne
    margin = max(spread(v) for v in t.values())
    r = med["fp64"] / med["fp32"]
    say(f"  {name} N={N} ncols={ne} {'complex' if cplx else 'real'}  " + "   ".join(
        f"{k} {med[k]:9.3f} ms ({flops / med[k] * 1e-9:6.1f} TF/s, min {min(t[k]):.3f} max {max(t[k]):.3f}, {len(t[k])} x {reps[k]})"
        for k in t) + f"   fp64 / fp32 = {r:.3f} (fp32 {verdict(r, margin)}; window spread {100 * margin:.2f} %)")
    for a in (d64, d32, o64, o32):
        a.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sp_solver.txt"))
    ap.add_argument("--cases", default="cfg2,cfg3", help="which of the shapes to run")
    ap.add_argument("--append", action="store_true", help="add to FILE (a second call for the other shape) instead of replacing it")
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    from chase_amd.capi import Context
    ctx = Context(0)
    info = ctx.info()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    cases = [("toy-c", 2048, True, 64, 16), ("toy-r", 3000, False, 96, 32)] if args.small else \
        [c for c in [("cfg2", 16384, True, 512, 128), ("cfg3", 32768, False, 1024, 256)] if c[0] in args.cases.split(",")]
    min_ms, windows = (100.0, 2) if args.small else (1500.0, 5)
    say("single-precision Hermitian solver (SpSolver: H and vectors fp32 from start to end) against the fp64 solver under the same settings "
        "(scripts/dev_sp_solver.py)")
    say(f"device: {info['name']}, {info['num_cu']} CUs, {info['clock_khz'] / 1000:.0f} MHz max engine clock")
    say(f"settings of both: {FLOAT_DEFAULTS}, optimised degrees, CholQR, host start vectors; matrices: chase_hip_gen_clement scaled by 1 / N "
        "(unit norm), perturbation 1e-6, the fp32 one its rounding")
    for name, N, cplx, nev, nex in cases:
        dH64 = ctx.gen_clement(N, cplx, scale=1.0 / N, perturb=1e-6)
        dH32 = ctx.to_single(dH64)
        ctx.sync()
        say(f"{name}: N = {N} {'complex' if cplx else 'real'}, nev {nev}, nex {nex}")
        say(f" (a) whole solves, {windows} alternated windows after one warm-up of each")
        solve_case(ctx, name, N, cplx, nev, nex, dH64, dH32, windows, say)
        say(f" (b) one full-width filter product (alpha H V, beta = 0), {windows} alternated windows, at least {min_ms / 1000:.1f} s per kind")
        product_case(ctx, name, N, cplx, nev + nex, dH64, dH32, min_ms, windows, say)
        dH64.free(); dH32.free()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
