"""The pseudo-Hermitian solver's fp32 H^2 filter (h2_mixed_precision = 1) against its fp64 one.  Writes profiles/h2_mixed.txt;
method of scripts/dev_sp_prepack.py: one process, alternating windows, median and spread of the windows.

(a) one H^2 filter step V2 = alpha H (H V1) + beta V2 + gamma V1 at config 5's shape (N = 32768 complex, nev + nex = 320 columns; the
    bench's synthetic Bethe-Salpeter matrix, chase_hip_gen_bse) through the solver's own HEMM_H2: in fp64 (two chase_hip_gemm_z,
    the scalar upload and chase_hip_col_axpy) and in fp32 (two chase_hip_gemm_c and chase_hip_axpy_sp on the shadows).  A window is
    one bracketed filter call: FilterPhaseStart with the residual buffer at 1e-4 (fp64) or 1.0 (fp32), one untimed step (it
    converts the vectors), then back-to-back steps between two stream synchronisations on the host clock.  The scalars keep the
    iterates bounded (a two-term recurrence with its roots on the unit circle), so every window multiplies numbers of the same size.
(b) whole config-5 solves on the single-GPU solver with the key off and on, alternated: time, device filter time, iterations,
    filtered vectors, Ritz values, fresh fp64 residuals.

    python scripts/dev_h2_mixed.py [--out FILE] [--skip-solves] [--small]
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
STEP = (1.0 / 242.0, -1.0, -0.25)                                    # alpha, beta, gamma: |alpha lambda^2 + gamma| <= 1/4 on [1, 11]


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def set_resid(s, value):
    from chase_amd.capi import lib
    np.ctypeslib.as_array(lib.chase_hip_solver_resid(s.h), shape=(s.ncol,))[:] = value


def step_case(ctx, dH, N, nev, nex, min_ms, windows, say):
    from chase_amd.capi import PseudoSolver
    ne = nev + nex
    s = PseudoSolver(ctx, None, nev, nex, h_on_device_ptr=dH.ptr, N=N, cplx=True)
    s.set(device_rng=1, h2_mixed_precision=1)
    s.Start(); s.initVecs(True); s.QR(0, 1.0)
    a, b, g = STEP

    def window(resid, reps):
        set_resid(s, resid)
        s.FilterPhaseStart()
        s.HEMM_H2(ne, a, b, g, 0)                       # untimed: the first step of a call converts the vectors
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

    kinds = {"fp64": 1e-4, "fp32": 1.0}
    reps = {}
    for k, r in kinds.items():
        window(r, 2)                                    # warm-up: code objects, workspace, the shadows, clocks
        reps[k] = max(1, int(np.ceil(min_ms / windows / window(r, 1))))
    s.set(reset_counters=1)
    t = {k: [] for k in kinds}
    for _ in range(windows):
        for k, r in kinds.items():
            t[k].append(window(r, reps[k]))
    med = {k: statistics.median(v) for k, v in t.items()}
    flops = 2 * 2.0 * 4 * N * N * ne                    # two complex N x N x ne products
    say(f"  N={N} ncols={ne} complex  " + "   ".join(
        f"{k} {med[k]:9.3f} ms per step ({flops / med[k] * 1e-9:6.1f} TF/s, min {min(t[k]):.3f} max {max(t[k]):.3f}, spread "
        f"{100 * spread(t[k]):.2f} %, {len(t[k])} x {reps[k]})" for k in t))
    margin = max(spread(t["fp64"]), spread(t["fp32"]))
    r = med["fp64"] / med["fp32"]
    verdict = "faster" if r > 1 + margin else ("slower" if r < 1 - margin else "within the spread")
    say(f"  fp64 / fp32 = {r:.3f} (fp32 {verdict}; window spread {100 * margin:.2f} %); counters of the timed windows: "
        f"{int(s.get('hemm_calls'))} fp64 and {int(s.get('hemm_sp_calls'))} fp32 products, {int(s.get('sp_filters'))} calls in fp32, "
        f"{int(s.get('sp_h_converts'))} conversions of H (it was converted once, in the warm-up)")
    V = s.peek_v()
    say(f"  max |V| after all windows: {float(np.max(np.abs(V[:, :ne]))):.3e} (bounded iterates)")
    s.close()
    return r, margin


def solve_case(ctx, dH, name, N, nev, nex, rounds, say):
    from chase_amd.capi import PseudoSolver
    s = PseudoSolver(ctx, None, nev, nex, h_on_device_ptr=dH.ptr, N=N, cplx=True)
    s.set(device_rng=1, numlanczos=10, lanczositer=50)      # the bench's settings for config 5
    res, ritz, its = {}, {}, {}
    for label in ["warm-up"] + ["off", "on"] * rounds:
        s.set(h2_mixed_precision=0 if label == "off" else 1, reset_counters=1)    # (the warm-up also allocates the shadows)
        ctx.sync()
        t0 = time.perf_counter()
        st = s.solve()
        ctx.sync()
        dt = time.perf_counter() - t0
        r = s.recompute_residuals(nev)
        if label != "warm-up":
            res.setdefault(label, []).append((dt, s.get("filter_ms") * 1e-3))
            ritz[label] = s.ritzv[:nev].copy()
            its[label] = (st["iterations"], st["filtered_vecs"])
        say(f"  {name} {label:8s} {dt:8.3f} s  filter {s.get('filter_ms') * 1e-3:7.3f} s  iterations {st['iterations']:2d}  filtered vectors "
            f"{st['filtered_vecs']:7d}  fp64 products {int(s.get('hemm_calls')):4d}  fp32 products {int(s.get('hemm_sp_calls')):4d} "
            f"({int(s.get('sp_filters'))} filter calls, {int(s.get('sp_h_converts'))} conversion of H)  locked {st['locked']}  "
            f"max solver residual {float(np.max(s.resid()[:nev])):.2e}  max fresh fp64 residual {float(np.max(r)):.2e}")
    med = {k: statistics.median(x[0] for x in v) for k, v in res.items()}
    medf = {k: statistics.median(x[1] for x in v) for k, v in res.items()}
    sp = max(spread([x[0] for x in v]) for v in res.values())
    r = med["off"] / med["on"]
    verdict = "faster" if r > 1 + sp else ("slower" if r < 1 - sp else "within the spread")
    say(f"  {name}: median of {rounds} solves each, alternated: key off {med['off']:.3f} s (filter {medf['off']:.3f} s), key on {med['on']:.3f} s "
        f"(filter {medf['on']:.3f} s): off / on = {r:.3f} ({verdict}; largest spread of a setting {100 * sp:.2f} %); iterations / filtered "
        f"vectors off {its['off'][0]} / {its['off'][1]}, on {its['on'][0]} / {its['on'][1]}; max |Ritz value on - off| = "
        f"{float(np.max(np.abs(np.sort(ritz['on']) - np.sort(ritz['off'])))):.2e}")
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "h2_mixed.txt"))
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

    name, N, nev, nex = ("toy", 2048, 64, 16) if args.small else ("cfg5", 32768, 256, 64)
    min_ms, windows, rounds = (100.0, 3, 1) if args.small else (2000.0, 5, 2)
    say("fp32 H^2 filter of the single-GPU pseudo-Hermitian solver (h2_mixed_precision = 1) against the fp64 one (scripts/dev_h2_mixed.py)")
    say(f"device: {info['name']}, {info['num_cu']} CUs, {info['clock_khz'] / 1000:.0f} MHz max engine clock")
    say(f"matrix: chase_hip_gen_bse N = {N} complex, dmin 1, dmax 11, off-diagonal 1e-3 (the bench's {name}), nev {nev}, nex {nex}")
    dH = ctx.gen_bse(N, True, **BSE_MATRIX)
    ctx.sync()
    say(f"(a) one H^2 step over all {nev + nex} first-half columns through HEMM_H2 inside a bracketed filter call; alpha, beta, gamma = "
        f"{STEP[0]:.6f}, {STEP[1]}, {STEP[2]}; {windows} alternating windows, at least {min_ms / 1000:.1f} s of steps per kind; host clock "
        "between two stream synchronisations, launch overhead and (fp64) the scalar upload per step included; conversions excluded")
    step_case(ctx, dH, N, nev, nex, min_ms, windows, say)
    if not args.skip_solves:
        say("(b) whole solves (tol 1e-10, deg 20, opt, numLanczos 10, lanczosIter 50; device start vectors), host clock around solve + "
            f"synchronise; one warm-up solve, then key off / key on, {rounds} rounds")
        solve_case(ctx, dH, name, N, nev, nex, rounds, say)
    dH.free()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
