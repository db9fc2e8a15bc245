"""The single-precision generalized problem (chase_hip_gemm_s_op / _c_op, chase_hip_potrf_upper_blocked_sp, chase_hip_gev_reduce_sp,
chase_hip_gev_backtransform_sp / _starttransform_sp, SpGevSolver) measured against the fp64 routines of the same commit.  Writes
profiles/gev_sp.txt; method of scripts/dev_gev.py / dev_gev_seq.py: one process, fp32 and fp64 alternated in five windows after one
warm-up of each, the window spread next to every ratio, host clock around a synchronised call.

At N = 16384, real and complex:
(a) the full-width product N x 640 x N: chase_hip_gemm_s / _c (op N) against chase_hip_gemm_s_op / _c_op with op C, and the fp64
    product; the fp32 op N rate is the yardstick that turns a routine's NOMINAL flops (n^3 / 3 for the Cholesky, 2 n^3 for the two
    full solves of the reduction, n^2 m for a transform of m columns; complex: x 4) into "time at the full-width rate";
(b) the Cholesky; (c) the reduction with factor = 1 and (d) with factor = 0; (e) back- and start-transform of 640 columns.
At config 2's shape (N = 16384 complex, 512 + 128 columns, tol 1e-5, float defaults - what scripts/dev_sp_solver.py uses):
(f) reduce + solve + back-transformation, fp32 (the steps of SpGevSolver) against fp64 (those of GevSolver) on the same pencil.

S = 2 I + Clement-type matrix of norm 1/2, H = Clement-type matrix of norm 1, generated on the device in fp64 and rounded there.

    python scripts/dev_gev_sp.py [--out FILE] [--cases real,complex,solve] [--small] [--windows W]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from dev_gev import spread  # noqa: E402


class Pair:
    """the same pencil in fp64 and fp32 on the device, with work copies of each"""

    def __init__(self, ctx, N, cplx):
        from chase_amd import capi
        self.capi, self.lib, self.ctx, self.N, self.cplx = capi, capi.lib, ctx, N, cplx
        self.dt = {64: np.complex128 if cplx else np.float64, 32: np.complex64 if cplx else np.float32}
        H0 = ctx.gen_clement(N, cplx, scale=1.0 / N, perturb=1e-6)
        S0 = ctx.gen_clement(N, cplx, scale=0.5 / N, perturb=1e-6, seed=7)
        capi.check(self.lib.chase_hip_shift_diag(ctx.h, int(cplx), N, S0.ptr, N, 2.0), "shift_diag")
        self.H0 = {64: H0, 32: ctx.to_single(H0)}
        self.S0 = {64: S0, 32: ctx.to_single(S0)}
        self.A = {p: ctx.empty((N, N), self.dt[p]) for p in (64, 32)}
        self.S = {p: ctx.empty((N, N), self.dt[p]) for p in (64, 32)}

    def copy(self, p, src, dst, ncols=None):
        f = self.lib.chase_hip_lacpy if p == 64 else self.lib.chase_hip_lacpy_sp
        self.capi.check(f(self.ctx.h, int(self.cplx), self.N, ncols or self.N, src.ptr, self.N, dst.ptr, self.N), "lacpy")

    def free(self):
        for d in (self.H0, self.S0, self.A, self.S):
            for a in d.values():
                a.free()


def timed(ctx, prepare, run):
    prepare()
    ctx.sync()
    t0 = time.perf_counter()
    run()
    ctx.sync()
    return time.perf_counter() - t0


def compare(ctx, say, title, kinds, windows, flops=None, rate=None, base=None):
    """kinds: name -> (prepare, run); one warm-up of each, then alternated windows.  base: the kind every other one is divided by,
    window by window (the ratio's own spread is printed)."""
    t = {k: [] for k in kinds}
    for w in range(windows + 1):
        for k, (prep, run) in kinds.items():
            dt = timed(ctx, prep, run)
            if w:
                t[k].append(dt)
    med = {k: statistics.median(v) for k, v in t.items()}
    for k in kinds:
        line = (f"  {title} {k:40s} {med[k] * 1e3:10.1f} ms (min {min(t[k]) * 1e3:.1f} max {max(t[k]) * 1e3:.1f}, {windows} windows, spread "
                f"{100 * spread(t[k]):.1f} %)")
        if flops and rate and k.startswith("fp32"):
            line += f"  nominal {flops * 1e-12:.3f} Tflop = {flops / rate * 1e3:.1f} ms at the fp32 full-width rate: {med[k] * rate / flops:.2f} x"
        if base and k != base:
            r = [a / b for a, b in zip(t[k], t[base])]
            line += f"  / {base} = {statistics.median(r):.2f} (min {min(r):.2f} max {max(r):.2f})"
        say(line)
    return med


def routine_case(ctx, N, cplx, ncols, windows, say):
    from chase_amd.capi import lib, check
    b = Pair(ctx, N, cplx)
    c, F = int(cplx), (4.0 if cplx else 1.0)
    say(f"{'complex' if cplx else 'real'}, N = {N}")
    # (a) the products
    V = {p: ctx.empty((N, ncols), b.dt[p]) for p in (64, 32)}
    W = {p: ctx.empty((N, ncols), b.dt[p]) for p in (64, 32)}
    check(lib.chase_hip_fill_normal(ctx.h, c, N, ncols, V[64].ptr, N, 0, 0, N, 11), "fill_normal")
    ctx.convert_d2s(N, ncols, V[64].ptr, N, V[32].ptr, N, cplx)
    nop, reps = (lambda: None), 8
    kinds = {
        "fp32 gemm32 op N": (nop, lambda: [ctx.gemm32("N", N, ncols, N, 0.5, b.H0[32].ptr, N, V[32].ptr, N, 0.0, W[32].ptr, N, cplx) for _ in range(reps)]),
        "fp32 gemm32op op C": (nop, lambda: [ctx.gemm32op("C", N, ncols, N, 0.5, b.H0[32].ptr, N, V[32].ptr, N, 0.0, W[32].ptr, N, cplx) for _ in range(reps)]),
        "fp64 gemm op N": (nop, lambda: [ctx.gemm("N", N, ncols, N, 0.5, b.H0[64].ptr, N, V[64].ptr, N, 0.0, W[64].ptr, N, cplx) for _ in range(reps)]),
        "fp64 gemm op C": (nop, lambda: [ctx.gemm("C", N, ncols, N, 0.5, b.H0[64].ptr, N, V[64].ptr, N, 0.0, W[64].ptr, N, cplx) for _ in range(reps)]),
    }
    med = compare(ctx, say, f"(a) {reps} products N x {ncols} x N:", kinds, windows, base="fp32 gemm32 op N")
    rate = reps * 2.0 * F * N * N * ncols / med["fp32 gemm32 op N"]
    say(f"      fp32 op N: {rate * 1e-12:.1f} Tflop/s (the yardstick below); op C {reps * 2.0 * F * N * N * ncols / med['fp32 gemm32op op C'] * 1e-12:.1f}, "
        f"fp64 op N {reps * 2.0 * F * N * N * ncols / med['fp64 gemm op N'] * 1e-12:.1f} Tflop/s")
    # (b) Cholesky
    prepS = {p: (lambda p=p: b.copy(p, b.S0[p], b.S[p])) for p in (64, 32)}
    compare(ctx, say, "(b)", {
        "fp32 potrf_upper_blocked_sp": (prepS[32], lambda: check(ctx.potrf_upper_blocked_sp(N, b.S[32].ptr, N, cplx, 0), "potrf_sp")),
        "fp64 potrf_upper_blocked": (prepS[64], lambda: check(ctx.potrf_upper_blocked(N, b.S[64].ptr, N, cplx, 0), "potrf")),
    }, windows, flops=F * N ** 3 / 3.0, rate=rate, base="fp64 potrf_upper_blocked")
    # (c) reduction, factor = 1
    def prepAS(p):
        b.copy(p, b.H0[p], b.A[p]); b.copy(p, b.S0[p], b.S[p])
    compare(ctx, say, "(c)", {
        "fp32 gev_reduce_sp factor=1": (lambda: prepAS(32), lambda: check(ctx.gev_reduce_sp(1, N, b.A[32].ptr, N, b.S[32].ptr, N, cplx), "reduce_sp")),
        "fp64 gev_reduce_itype factor=1": (lambda: prepAS(64), lambda: check(ctx.gev_reduce_itype(1, 1, N, b.A[64].ptr, N, b.S[64].ptr, N, cplx), "reduce")),
    }, windows, flops=F * N ** 3 * (2.0 + 1.0 / 3.0), rate=rate, base="fp64 gev_reduce_itype factor=1")
    # (d) factor = 0: S holds U from the last run of (c)
    compare(ctx, say, "(d)", {
        "fp32 gev_reduce_sp factor=0": (lambda: b.copy(32, b.H0[32], b.A[32]), lambda: check(ctx.gev_reduce_sp(0, N, b.A[32].ptr, N, b.S[32].ptr, N, cplx), "reduce_sp")),
        "fp64 gev_reduce_itype factor=0": (lambda: b.copy(64, b.H0[64], b.A[64]), lambda: check(ctx.gev_reduce_itype(1, 0, N, b.A[64].ptr, N, b.S[64].ptr, N, cplx), "reduce")),
    }, windows, flops=F * N ** 3 * 2.0, rate=rate, base="fp64 gev_reduce_itype factor=0")
    # (e) transforms of ncols columns
    prepX = {p: (lambda p=p: b.copy(p, V[p], W[p], ncols)) for p in (64, 32)}
    compare(ctx, say, f"(e) {ncols} columns:", {
        "fp32 gev_backtransform_sp": (prepX[32], lambda: ctx.gev_backtransform_sp(N, ncols, b.S[32].ptr, N, W[32].ptr, N, cplx)),
        "fp64 gev_backtransform": (prepX[64], lambda: ctx.gev_backtransform(N, ncols, b.S[64].ptr, N, W[64].ptr, N, cplx)),
    }, windows, flops=F * float(N) * N * ncols, rate=rate, base="fp64 gev_backtransform")
    compare(ctx, say, f"(e) {ncols} columns:", {
        "fp32 gev_starttransform_sp": (prepX[32], lambda: ctx.gev_starttransform_sp(N, ncols, b.S[32].ptr, N, W[32].ptr, N, cplx)),
        "fp64 gev_starttransform": (prepX[64], lambda: ctx.gev_starttransform(1, N, ncols, b.S[64].ptr, N, W[64].ptr, N, cplx)),
    }, windows, flops=F * float(N) * N * ncols, rate=rate, base="fp64 gev_starttransform")
    for d in (V, W):
        for a in d.values():
            a.free()
    b.free()


def solve_case(ctx, N, cplx, nev, nex, windows, say):
    from chase_amd.capi import Solver, SpSolver
    b = Pair(ctx, N, cplx)
    say(f"(f) config 2's shape: N = {N} {'complex' if cplx else 'real'}, nev {nev}, nex {nex}, tol 1e-5 and the float defaults (deg 10, maxdeg 18, "
        "lanczositer 12) for both")
    s = {64: Solver(ctx, None, nev, nex, h_on_device_ptr=b.A[64].ptr, N=N, cplx=cplx),
         32: SpSolver(ctx, None, nev, nex, h_on_device_ptr=b.A[32].ptr, N=N, cplx=cplx, ldh=N)}
    s[64].set(tol=1e-5, deg=10, maxdeg=18, lanczositer=12)
    X = {p: ctx.empty((N, nev), b.dt[p]) for p in (64, 32)}
    t = {p: {"reduce": [], "solve": [], "backtransform": []} for p in (64, 32)}
    last = {}
    for w in range(windows + 1):
        for p in (32, 64):
            b.copy(p, b.H0[p], b.A[p]); b.copy(p, b.S0[p], b.S[p])
            ctx.sync()
            t0 = time.perf_counter()
            if p == 32:
                assert ctx.gev_reduce_sp(1, N, b.A[32].ptr, N, b.S[32].ptr, N, cplx) == 0
            else:
                assert ctx.gev_reduce(N, b.A[64].ptr, N, b.S[64].ptr, N, cplx) == 0
            ctx.sync()
            t1 = time.perf_counter()
            st = s[p].solve()
            ctx.sync()
            t2 = time.perf_counter()
            X[p].upload(s[p].V[:, :nev])
            (ctx.gev_backtransform_sp if p == 32 else ctx.gev_backtransform)(N, nev, b.S[p].ptr, N, X[p].ptr, N, cplx)
            ctx.sync()
            t3 = time.perf_counter()
            assert st["locked"] >= nev, st
            last[p] = st
            if w:
                t[p]["reduce"].append(t1 - t0); t[p]["solve"].append(t2 - t1); t[p]["backtransform"].append(t3 - t2)
    whole = {}
    for p in (32, 64):
        med = {k: statistics.median(v) for k, v in t[p].items()}
        whole[p] = [sum(x) for x in zip(*t[p].values())]
        say(f"  fp{p}: reduce {med['reduce']:.3f} s (spread {100 * spread(t[p]['reduce']):.1f} %) + solve {med['solve']:.3f} s (spread "
            f"{100 * spread(t[p]['solve']):.1f} %; {last[p]['iterations']} iterations, {last[p]['filtered_vecs']} filtered vectors) + upload and "
            f"back-transformation of {nev} columns {med['backtransform']:.3f} s = {statistics.median(whole[p]):.3f} s (spread {100 * spread(whole[p]):.1f} %)")
        es = 8 if p == 64 else 4
        say(f"        device memory: solver's own allocations {int(s[p].get('device_bytes'))} bytes + C and U in place 2 x {N * N * es * (2 if cplx else 1)} bytes")
    r = [a / c for a, c in zip(whole[32], whole[64])]
    say(f"  fp32 / fp64, whole: {statistics.median(r):.2f} (min {min(r):.2f} max {max(r):.2f}, {windows} windows)")
    for p in (32, 64):
        s[p].close()
        X[p].free()
    b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gev_sp.txt"))
    ap.add_argument("--cases", default="real,complex,solve")
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    from chase_amd.capi import Context
    ctx = Context(0)
    info = ctx.info()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def say(text):
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    N = 1536 if args.small else 16384
    cases = args.cases.split(",")
    say("the generalized problem in single precision against the fp64 routines of the same commit (scripts/dev_gev_sp.py)")
    say(f"device: {info['name']}, {info['num_cu']} CUs, {info['clock_khz'] / 1000:.0f} MHz max engine clock; fp32 and fp64 alternated, {args.windows} "
        "windows after one warm-up of each; 'x' = time over the time of the nominal flops at the fp32 full-width rate of (a)")
    for name, cplx in (("real", False), ("complex", True)):
        if name in cases:
            routine_case(ctx, N, cplx, 64 if args.small else 640, args.windows, say)
    if "solve" in cases:
        solve_case(ctx, N, True, *((64, 16) if args.small else (512, 128)), args.windows, say)
    ctx.close()
    out.close()


if __name__ == "__main__":
    main()
