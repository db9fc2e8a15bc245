"""The single-precision pseudo-Hermitian solver (capi.SpPseudoSolver) against the fp64 one (capi.PseudoSolver).  Writes
profiles/sp_pseudo.txt; method of scripts/dev_sp_solver.py: one process, five alternating windows, the window spread as the margin.

At config 5's shape (bench.py: N = 32768 complex, nev 256 + nex 64 = 320 first-half columns) on the bench's synthetic Bethe-Salpeter
matrix (chase_hip_gen_bse) scaled on the device by 1/16 (exact: spectrum within +-0.69); the fp32 matrix is its rounding
(chase_hip_convert_d2s); both are used in place in HBM:
(a) one H^2 filter step V2 = alpha H (H V1) + beta V2 + gamma V1 over all 320 columns through each solver's own HEMM_H2 inside a
    bracketed filter call: fp64 (two chase_hip_gemm_z, the scalar upload, chase_hip_col_axpy) against fp32 (two chase_hip_gemm_c,
    chase_hip_axpy_sp); back-to-back steps between two stream synchronisations on the host clock; the scalars keep the iterates
    bounded;
(b) whole solves of both under the reference's float defaults (tol 1e-5, deg 10, maxDeg 18, lanczosIter 12, optimised degrees,
    host start vectors - the single-precision solver has no device generator): iterations, filtered vectors, phase times,
    residuals, and device_bytes of both next to the bytes of the matrix each one works on.

    python scripts/dev_sp_pseudo.py [--out FILE] [--skip-solves] [--small]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BSE_MATRIX = {"dmin": 1.0, "dmax": 11.0, "offdiag": 1e-3}          # bench.py's BSE_MATRIX
SCALE = 1.0 / 16.0
STEP = (256.0 / 242.0, -1.0, -0.25)              # alpha, beta, gamma: |alpha lambda^2 + gamma| <= 1/4 on [1/16, 11/16]
FLOAT_DEFAULTS = dict(tol=1e-5, deg=10, maxdeg=18, lanczositer=12)


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def verdict(r, margin):
    return "faster" if r > 1 + margin else ("slower" if r < 1 - margin else "within the spread")


def make_solvers(ctx, N, nev, nex, dH64, dH32):
    from chase_amd.capi import PseudoSolver, SpPseudoSolver
    s = {"fp64": PseudoSolver(ctx, None, nev, nex, h_on_device_ptr=dH64.ptr, N=N, cplx=True),
         "fp32": SpPseudoSolver(ctx, None, nev, nex, h_on_device_ptr=dH32.ptr, N=N, cplx=True, ldh=N)}
    s["fp64"].set(**FLOAT_DEFAULTS)
    for k, v in s.items():
        assert all(v.get(key) == val for key, val in FLOAT_DEFAULTS.items()), k
        assert v.get("h2_mixed_precision") == 0
    return s


def step_case(ctx, N, nev, nex, dH64, dH32, min_ms, windows, say):
    ne = nev + nex
    solvers = make_solvers(ctx, N, nev, nex, dH64, dH32)
    a, b, g = STEP
    for s in solvers.values():
        s.Start(); s.initVecs(True); s.QR(0, 1.0)

    def window(k, reps):
        s = solvers[k]
        s.FilterPhaseStart()
        s.HEMM_H2(ne, a, b, g, 0)                       # untimed: the same bracket as scripts/dev_h2_mixed.py
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            s.HEMM_H2(ne, a, b, g, 0)
        ctx.sync()
        dt = (time.perf_counter() - t0) * 1e3 / reps
        if reps % 2 == 0:
            s.HEMM_H2(0, 0, 0, 0, 0)                    # an even number of swaps per call
        s.FilterPhaseEnd()
        return dt

    reps = {}
    for k in solvers:
        window(k, 2)                                    # warm-up: code objects, workspace, clocks
        reps[k] = max(1, int(np.ceil(min_ms / windows / window(k, 1))))
    for s in solvers.values():
        s.set(reset_counters=1)
    t = {k: [] for k in solvers}
    for _ in range(windows):
        for k in solvers:
            t[k].append(window(k, reps[k]))
    med = {k: statistics.median(v) for k, v in t.items()}
    flops = 2 * 2.0 * 4 * N * N * ne                    # two complex N x N x ne products
    say(f"  N={N} ncols={ne} complex  " + "   ".join(
        f"{k} {med[k]:9.3f} ms per step ({flops / med[k] * 1e-9:6.1f} TF/s, min {min(t[k]):.3f} max {max(t[k]):.3f}, spread "
        f"{100 * spread(t[k]):.2f} %, {len(t[k])} x {reps[k]})" for k in t))
    margin = max(spread(v) for v in t.values())
    r = med["fp64"] / med["fp32"]
    say(f"  fp64 / fp32 = {r:.3f} (fp32 {verdict(r, margin)}; window spread {100 * margin:.2f} %); counters of the timed windows: fp64 solver "
        f"{int(solvers['fp64'].get('hemm_calls'))} fp64 and {int(solvers['fp64'].get('hemm_sp_calls'))} fp32 products, fp32 solver "
        f"{int(solvers['fp32'].get('hemm_calls'))} fp64 and {int(solvers['fp32'].get('hemm_sp_calls'))} fp32 products")
    for k, s in solvers.items():
        say(f"  {k}: max |V| after all windows: {float(np.max(np.abs(s.peek_v()[:, :ne]))):.3e} (bounded iterates)")
        s.close()


def solve_case(ctx, name, N, nev, nex, dH64, dH32, windows, say):
    solvers = make_solvers(ctx, N, nev, nex, dH64, dH32)
    t = {k: [] for k in solvers}
    last = {}
    for w in range(windows + 1):                        # window 0: warm-up (code objects, workspaces, host LAPACK)
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
        f"{last['fp32']['iterations']} / {last['fp32']['filtered_vecs']}; locked fp64 {last['fp64']['locked']}, fp32 {last['fp32']['locked']}; "
        f"max |Ritz value fp32 - fp64| = {float(np.max(np.abs(np.sort(lam['fp32']) - np.sort(lam['fp64'])))):.2e}; fp32 solver: max fresh "
        f"residual (fp32 product, fp64 norm) {float(np.max(fresh)):.2e}; fp32 products {int(solvers['fp32'].get('hemm_sp_calls'))}, fp64 "
        f"products {int(solvers['fp32'].get('hemm_calls'))}")
    say(f"  {name}: device_bytes (the Impl's own allocations; both matrices are the caller's, used in place): fp64 "
        f"{int(solvers['fp64'].get('device_bytes'))} + matrix {N * N * 16}, fp32 {int(solvers['fp32'].get('device_bytes'))} + matrix "
        f"{N * N * 8}")
    for s in solvers.values():
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sp_pseudo.txt"))
    ap.add_argument("--skip-solves", action="store_true")
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    from chase_amd.capi import Context, check, lib
    ctx = Context(0)
    info = ctx.info()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    name, N, nev, nex = ("toy", 2048, 64, 16) if args.small else ("cfg5", 32768, 256, 64)
    min_ms, windows = (100.0, 2) if args.small else (2000.0, 5)
    say("single-precision pseudo-Hermitian solver (SpPseudoSolver: H and vectors fp32 from start to end) against the fp64 PseudoSolver "
        "(scripts/dev_sp_pseudo.py)")
    say(f"device: {info['name']}, {info['num_cu']} CUs, {info['clock_khz'] / 1000:.0f} MHz max engine clock")
    say(f"matrix: chase_hip_gen_bse N = {N} complex, dmin 1, dmax 11, off-diagonal 1e-3 (the bench's {name}), scaled on the device by 1/16 "
        f"(exact); the fp32 one its rounding; nev {nev}, nex {nex}")
    dH64 = ctx.gen_bse(N, True, **BSE_MATRIX)
    check(lib.chase_hip_scale_rows(ctx.h, 1, N, N, dH64.ptr, N, 0, SCALE), "scale_rows")
    dH32 = ctx.to_single(dH64)
    ctx.sync()
    say(f"(a) one H^2 step over all {nev + nex} first-half columns through HEMM_H2 inside a bracketed filter call; alpha, beta, gamma = "
        f"{STEP[0]:.6f}, {STEP[1]}, {STEP[2]}; {windows} alternating windows, at least {min_ms / 1000:.1f} s of steps per kind; host clock "
        "between two stream synchronisations, launch overhead and (fp64) the scalar upload per step included")
    step_case(ctx, N, nev, nex, dH64, dH32, min_ms, windows, say)
    if not args.skip_solves:
        say(f"(b) whole solves under the float defaults {FLOAT_DEFAULTS}, optimised degrees, CholQR, host start vectors; "
            f"host clock around solve + synchronise; {windows} alternated windows after one warm-up of each")
        solve_case(ctx, name, N, nev, nex, dH64, dH32, windows, say)
    dH64.free(); dH32.free()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
