"""The single-precision product of the mixed-precision filter: fp32 MFMA against the bf16x3 split product (sp_product = 1).
Writes profiles/sp_bf16x3.txt.

(a) the filter product at full width, phase 1 like the filter launches it: fp64 (chase_hip_gemm_d / _z), fp32 MFMA
    (chase_hip_gemm_s / _c) and bf16x3 (chase_hip_gemm_s_bf16x3 / _c_bf16x3) at N = 16384, n = 640 and N = 32768, n = 2560, real and
    complex (the shapes of profiles/mixed_precision.txt).  The three are timed alternately in one process: HIP events around a
    window of back-to-back products, at least a second of work per product kind, median over the windows.
(b) the panel product of one rank of the 4 x 2 grid (the shapes of profiles/mixed_precision_grid.txt), op N and op C: fp64 with
    gemm_min_rounds = 4, convert + chase_hip_gemm_sd / _cz, convert + chase_hip_gemm_sd_bf16x3 / _cz_bf16x3.
(c) whole solves of bench.py's cfg2 (N = 16384 complex, nev 512, nex 128) and cfg3 (N = 32768 real, nev 1024, nex 256) with the
    switch off, with the fp32 MFMA product and with bf16x3, alternated.

    python scripts/dev_sp_product.py [--out FILE] [--skip-solves] [--small] [--one real|complex]

--one launches a single full-width bf16x3 product (N = 16384, n = 640) and nothing else: the launch a counter pass profiles.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MATRIX_SCALE, MATRIX_PERTURB = 100.0, 1e-6          # bench.py's matrix
PEAK_F32 = 157.3                                     # TF/s, f32-input matrix cores (spec)
CEILING = 16.0 / 6.0                                 # six 32-cycle bf16 MFMAs for eight 64-cycle f32 ones per 16 k


def timed(ctx, kinds, min_ms, windows):
    """kinds: {name: fn}; alternating windows of back-to-back calls between device events; ms per call, per window"""
    reps = {}
    for name, fn in kinds.items():
        for _ in range(2):                              # warm-up: code objects, workspace, clocks
            fn()
        ctx.timer_start(); fn(); one = max(ctx.timer_stop(), 1e-3)
        reps[name] = max(1, int(np.ceil(min_ms / windows / one)))
    t = {name: [] for name in kinds}
    for _ in range(windows):
        for name, fn in kinds.items():
            ctx.timer_start()
            for _ in range(reps[name]):
                fn()
            t[name].append(ctx.timer_stop() / reps[name])
    return t, reps


def report(say, head, flops, t, reps, worst):
    med = {k: statistics.median(v) for k, v in t.items()}
    parts = [f"{k} {med[k]:9.3f} ms ({flops / med[k] * 1e-9:6.1f} TF/s, min {min(t[k]):.3f} max {max(t[k]):.3f}, {len(t[k])} x {reps[k]})"
             for k in t]
    r = med["fp32"] / med["bf16x3"]
    say(f"  {head}  " + "   ".join(parts) + f"   fp32 / bf16x3 = {r:.2f} (ceiling {CEILING:.2f}), fp64 / bf16x3 = {med['fp64'] / med['bf16x3']:.2f}, "
        f"bf16x3 at {flops / med['bf16x3'] * 1e-9 / (PEAK_F32 * CEILING):.2f} of its {PEAK_F32 * CEILING:.0f} TF/s ceiling   "
        f"max |x - fp64| / max |fp64| on a column: fp32 {worst['fp32']:.1e}, bf16x3 {worst['bf16x3']:.1e}")
    return r


def product_case(ctx, N, n, cplx, min_ms, windows, say):
    from chase_amd.capi import lib, check
    dt = np.complex128 if cplx else np.float64
    H = ctx.gen_clement(N, cplx, scale=MATRIX_SCALE / N, perturb=MATRIX_PERTURB, seed=42)
    V = ctx.empty((N, n), dt)
    check(lib.chase_hip_fill_normal(ctx.h, int(cplx), N, n, V.ptr, N, 0, 0, N, 1337), "fill_normal")
    W = ctx.empty((N, n), dt)
    Hs, Vs = ctx.to_single(H), ctx.to_single(V)
    Ws, W3 = ctx.empty((N, n), Hs.dtype), ctx.empty((N, n), Hs.dtype)
    alpha, beta = 0.01, 0.0
    kinds = {"fp64": lambda: ctx.gemm("N", N, n, N, alpha, H.ptr, N, V.ptr, N, beta, W.ptr, N, cplx),
             "fp32": lambda: ctx.gemm32("N", N, n, N, alpha, Hs.ptr, N, Vs.ptr, N, beta, Ws.ptr, N, cplx),
             "bf16x3": lambda: ctx.gemm32("N", N, n, N, alpha, Hs.ptr, N, Vs.ptr, N, beta, W3.ptr, N, cplx, split=True)}
    check(lib.chase_hip_ctx_set_phase(ctx.h, 1), "set_phase")
    t, reps = timed(ctx, kinds, min_ms, windows)
    check(lib.chase_hip_ctx_set_phase(ctx.h, 0), "set_phase")
    a = W.download()[:, n - 1]
    worst = {k: float(np.max(np.abs(a - X.download()[:, n - 1])) / np.max(np.abs(a))) for k, X in (("fp32", Ws), ("bf16x3", W3))}
    r = report(say, f"N={N:6d} n={n:5d} {'complex' if cplx else 'real   '}", 2.0 * (4 if cplx else 1) * N * N * n, t, reps, worst)
    for d in (H, V, W, Hs, Vs, Ws, W3):
        d.free()
    return r


def panel_case(ctx, m_loc, n_loc, w, cplx, min_ms, windows, say):
    from chase_amd.capi import lib, check
    dt = np.complex128 if cplx else np.float64
    H = ctx.empty((m_loc, n_loc), dt)
    check(lib.chase_hip_fill_normal(ctx.h, int(cplx), m_loc, n_loc, H.ptr, m_loc, 0, 0, m_loc, 42), "fill_normal")
    Hs = ctx.to_single(H)
    out = {}
    check(lib.chase_hip_ctx_set_phase(ctx.h, 1), "set_phase")
    for op in ("N", "C"):
        rows_out, rows_in = (m_loc, n_loc) if op == "N" else (n_loc, m_loc)
        X = ctx.empty((rows_in, w), dt)
        check(lib.chase_hip_fill_normal(ctx.h, int(cplx), rows_in, w, X.ptr, rows_in, 0, 0, rows_in, 1337), "fill_normal")
        Xs = ctx.empty((rows_in, w), Hs.dtype)
        Y, Ym, Y3 = (ctx.empty((rows_out, w), dt) for _ in range(3))
        alpha, beta = 0.01, 0.0

        def f64():
            check(lib.chase_hip_ctx_set_gemm_min_rounds(ctx.h, 4), "min_rounds")
            ctx.gemm(op, rows_out, w, rows_in, alpha, H.ptr, m_loc, X.ptr, rows_in, beta, Y.ptr, rows_out, cplx)
            check(lib.chase_hip_ctx_set_gemm_min_rounds(ctx.h, 0), "min_rounds")

        def mixed(out, split):
            ctx.convert_d2s(rows_in, w, X.ptr, rows_in, Xs.ptr, rows_in, cplx)
            ctx.gemm32w(op, rows_out, w, rows_in, alpha, Hs.ptr, m_loc, Xs.ptr, rows_in, beta, out.ptr, rows_out, cplx, split=split)

        t, reps = timed(ctx, {"fp64": f64, "fp32": lambda: mixed(Ym, False), "bf16x3": lambda: mixed(Y3, True)}, min_ms, windows)
        a = Y.download()[:, 0]
        worst = {k: float(np.max(np.abs(a - Z.download()[:, 0])) / np.max(np.abs(a))) for k, Z in (("fp32", Ym), ("bf16x3", Y3))}
        out[op] = report(say, f"H_loc {m_loc} x {n_loc} {'complex' if cplx else 'real   '} op {op} {w} columns (convert + product)",
                         2.0 * (4 if cplx else 1) * m_loc * n_loc * w, t, reps, worst)
        for d in (X, Xs, Y, Ym, Y3):
            d.free()
    check(lib.chase_hip_ctx_set_phase(ctx.h, 0), "set_phase")
    H.free(); Hs.free()
    return out


def solve_case(ctx, name, N, cplx, nev, nex, say):
    from chase_amd.capi import Solver
    dH = ctx.gen_clement(N, cplx, scale=MATRIX_SCALE / N, perturb=MATRIX_PERTURB, seed=42)
    ctx.sync()
    s = Solver(ctx, None, nev, nex, h_on_device_ptr=dH.ptr, N=N, cplx=cplx)
    s.set(device_rng=1)
    modes = {"off": (0, 0), "fp32": (1, 0), "bf16x3": (1, 1)}
    res = {}
    for label in ("warm-up", "off", "fp32", "bf16x3", "off", "fp32", "bf16x3", "off", "fp32", "bf16x3"):
        mp, sp = modes.get(label, (0, 0))
        s.set(mixed_precision=mp, sp_product=sp, reset_counters=1)
        ctx.sync()
        t0 = time.perf_counter()
        st = s.solve()
        ctx.sync()
        dt = time.perf_counter() - t0
        r = s.recompute_residuals(nev)
        if label != "warm-up":
            res.setdefault(label, []).append(dt)
        say(f"  {name} {label:8s} {dt:8.3f} s  filter {s.get('filter_ms') * 1e-3:7.3f} s  iterations {st['iterations']:2d}  filtered vectors "
            f"{st['filtered_vecs']:7d}  in fp32 {int(s.get('hemm_sp_vecs')):7d} ({int(s.get('sp_filters'))} filter calls, "
            f"{int(s.get('hemm_sp_split_calls'))} of {int(s.get('hemm_sp_calls'))} products split)  locked {st['locked']}  "
            f"max fresh fp64 residual {float(np.max(r)):.2e}")
    med = {k: statistics.median(v) for k, v in res.items()}
    say(f"  {name}: median of 3 solves each, alternated: off {med['off']:.3f} s, fp32 {med['fp32']:.3f} s ({med['off'] / med['fp32']:.3f}x), "
        f"bf16x3 {med['bf16x3']:.3f} s ({med['off'] / med['bf16x3']:.3f}x of off, {med['fp32'] / med['bf16x3']:.3f}x of fp32)")
    s.close()
    dH.free()


def one_launch(ctx, cplx):
    from chase_amd.capi import lib, check
    N, n = 16384, 640
    dt = np.complex64 if cplx else np.float32
    Hs, Vs, Ws = ctx.empty((N, N), dt), ctx.empty((N, n), dt), ctx.empty((N, n), dt)
    check(lib.chase_hip_memset(ctx.h, Hs.ptr, 0x3c, Hs.nbytes), "memset")      # finite values, no denormals: 0x3c3c3c3c = 0.0115
    check(lib.chase_hip_memset(ctx.h, Vs.ptr, 0x3c, Vs.nbytes), "memset")
    check(lib.chase_hip_ctx_set_phase(ctx.h, 1), "set_phase")
    ctx.gemm32("N", N, n, N, 0.01, Hs.ptr, N, Vs.ptr, N, 0.0, Ws.ptr, N, cplx, split=True)
    ctx.sync()
    check(lib.chase_hip_ctx_set_phase(ctx.h, 0), "set_phase")
    for d in (Hs, Vs, Ws):
        d.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sp_bf16x3.txt"))
    ap.add_argument("--skip-solves", action="store_true")
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    ap.add_argument("--one", choices=["real", "complex"])
    args = ap.parse_args()
    from chase_amd.capi import Context
    ctx = Context(0)
    if args.one:
        one_launch(ctx, args.one == "complex")
        ctx.close()
        return
    info = ctx.info()
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)

    min_ms, windows = (50.0, 3) if args.small else (1000.0, 5)
    say("Single-precision product of the mixed-precision filter: fp32 MFMA and bf16x3 (scripts/dev_sp_product.py)")
    say(f"device: {info['name']}, {info['num_cu']} CUs, {info['clock_khz'] / 1000:.0f} MHz max engine clock; fp32 MFMA peak {PEAK_F32} TF/s, "
        f"bf16x3 compute ceiling 16/6 of it = {PEAK_F32 * CEILING:.0f} TF/s fp32-equivalent")
    say("(a) full-width filter product, phase 1, alpha = 0.01, beta = 0; H = the bench's Clement matrix, V ~ N(0,1); 2 warm-up "
        f"products each, then {windows} alternating windows of back-to-back products between HIP events, at least {min_ms / 1000:.2f} s of "
        "work per kind; ms per product = median of the windows (windows x products per window in brackets)")
    shapes = [(1024, 96), (2048, 160)] if args.small else [(16384, 640), (32768, 2560)]
    ratios = {}
    for (N, n) in shapes:
        for cplx in (False, True):
            ratios[("full", N, n, cplx)] = product_case(ctx, N, n, cplx, min_ms, windows, say)
    say("(b) panel product of one rank of the 4 x 2 grid, phase 1, operands ~ N(0,1); fp64 with gemm_min_rounds = 4 as the pipeline "
        "issues it; fp32 and bf16x3 include convert_d2s of the input panel")
    panels = [(512, 768, 64, False), (512, 1024, 64, True)] if args.small else [(16384, 16384, 256, False), (16384, 32768, 256, True)]
    for (m_loc, n_loc, w, cplx) in panels:
        for op, r in panel_case(ctx, m_loc, n_loc, w, cplx, min_ms, windows, say).items():
            ratios[("panel", m_loc, n_loc, cplx, op)] = r
    lose = [k for k, v in ratios.items() if v <= 1.0]
    say("  bf16x3 faster than the fp32 MFMA product at every shape, type and op: " + ("yes" if not lose else f"NO - not at {lose}"))
    if not args.skip_solves:
        say("(c) whole solves (defaults: tol 1e-10, deg 20, opt; device start vectors), host clock around solve + synchronise; one "
            "warm-up solve, then off, fp32 (mixed_precision = 1), bf16x3 (mixed_precision = 1, sp_product = 1), three rounds")
        cases = [("toy", 2048, True, 64, 32)] if args.small else [("cfg2", 16384, True, 512, 128), ("cfg3", 32768, False, 1024, 256)]
        for case in cases:
            solve_case(ctx, *case, say)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
