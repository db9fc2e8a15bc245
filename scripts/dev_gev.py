"""The reduction of the generalized problem H x = lambda S x (chase_hip_potrf_upper_blocked, chase_hip_hegst_upper,
chase_hip_gev_backtransform) measured at N = 16384, real and complex.  Writes profiles/gev.txt; method of
scripts/dev_sp_solver.py: one process, alternated windows, the window spread as the margin, host clock around a synchronised call
(every operator here runs for tens of milliseconds to seconds).

(a) the full-width product chase_hip_gemm_d / _z (N x 640 x N, op N) as the yardstick: its rate turns the flops an operator
    EXECUTES (the context's phase-0 counter, read around the call) into the time they would take at that rate;
(b) chase_hip_potrf_upper_blocked for outer_nb in 256 ... 2048 against chase_hip_potrf_upper on the same S;
(c) chase_hip_hegst_upper: the blocked recurrence for nb in 128 ... 2048 against the two-full-solve formulation (nb = 0: complete
    A, A U^{-1} by chase_hip_trsm_right_upper, U^{-H} (.) by the left solve, one triangle mirrored);
(d) chase_hip_gev_backtransform at 640 columns;
(e) config 2's shape (N = 16384 complex, 512 + 128 columns, tol 1e-10): reduce + solve + back-transformation, what GevSolver does
    after its uploads, next to the plain Solver on the reduced matrix.

S = 2 I + Clement-type matrix of norm 1/2 (positive definite, condition below 2), H = Clement-type matrix of norm 1, both generated
on the device.

    python scripts/dev_gev.py [--out FILE] [--cases real,complex,solve] [--append] [--small]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return (max(v) - min(v)) / statistics.median(v) if len(v) > 1 else 0.0


class Bench:
    def __init__(self, ctx, N, cplx, say):
        from chase_amd import capi
        self.capi, self.lib, self.ctx, self.N, self.cplx, self.say = capi, capi.lib, ctx, N, cplx, say
        self.dt = np.complex128 if cplx else np.float64
        self.H0 = ctx.gen_clement(N, cplx, scale=1.0 / N, perturb=1e-6)
        self.S0 = ctx.gen_clement(N, cplx, scale=0.5 / N, perturb=1e-6, seed=7)
        capi.check(self.lib.chase_hip_shift_diag(ctx.h, int(cplx), N, self.S0.ptr, N, 2.0), "shift_diag")
        self.A, self.S = ctx.empty((N, N), self.dt), ctx.empty((N, N), self.dt)
        self.rate = None

    def copy(self, src, dst):
        self.capi.check(self.lib.chase_hip_lacpy(self.ctx.h, int(self.cplx), self.N, self.N, src.ptr, self.N, dst.ptr, self.N), "lacpy")

    def timed(self, prepare, run):
        """(seconds, executed flops) of one run() after an untimed prepare()"""
        prepare()
        self.capi.gemm_counters(self.ctx, 0, reset=True)
        self.ctx.sync()
        t0 = time.perf_counter()
        run()
        self.ctx.sync()
        dt = time.perf_counter() - t0
        return dt, self.capi.gemm_counters(self.ctx, 0)[1]

    def compare(self, title, kinds, windows):
        """kinds: name -> (prepare, run); one warm-up of each, then alternated windows"""
        t, fl = {k: [] for k in kinds}, {}
        for w in range(windows + 1):
            for k, (prep, run) in kinds.items():
                dt, f = self.timed(prep, run)
                fl[k] = f
                if w:
                    t[k].append(dt)
        for k in kinds:
            med = statistics.median(t[k])
            at_rate = fl[k] / self.rate if self.rate else float("nan")
            self.say(f"  {title} {k:34s} {med * 1e3:10.1f} ms (min {min(t[k]) * 1e3:.1f} max {max(t[k]) * 1e3:.1f}, {windows} windows, spread "
                     f"{100 * spread(t[k]):.1f} %)  executed {fl[k] * 1e-12:7.3f} Tflop = {at_rate * 1e3:8.1f} ms at the full-width rate: "
                     f"{med / at_rate if at_rate else float('nan'):5.2f} x")
        return {k: statistics.median(v) for k, v in t.items()}

    def gemm_rate(self, ncols, windows):
        N, ctx, cplx = self.N, self.ctx, self.cplx
        V, W = ctx.empty((N, ncols), self.dt), ctx.empty((N, ncols), self.dt)
        self.capi.check(self.lib.chase_hip_fill_normal(ctx.h, int(cplx), N, ncols, V.ptr, N, 0, 0, N, 11), "fill_normal")
        run = lambda: [ctx.gemm("N", N, ncols, N, 0.5, self.H0.ptr, N, V.ptr, N, 0.0, W.ptr, N, cplx) for _ in range(8)]
        ts = [self.timed(lambda: None, run) for _ in range(windows + 1)][1:]
        med = statistics.median(x[0] for x in ts)
        self.rate = ts[0][1] / med
        self.say(f"  (a) chase_hip_gemm_{'z' if cplx else 'd'} N x {ncols} x N, op N, phase 0: {med / 8 * 1e3:.2f} ms per product, "
                 f"{self.rate * 1e-12:.1f} Tflop/s executed (spread {100 * spread([x[0] for x in ts]):.1f} %)")
        V.free(); W.free()


def reduction_case(ctx, N, cplx, windows, say, small):
    from chase_amd.capi import lib, check
    b = Bench(ctx, N, cplx, say)
    c = int(cplx)
    say(f"{'complex' if cplx else 'real'} fp64, N = {N}")
    b.gemm_rate(640 if not small else 64, windows)
    # (b) Cholesky
    prepS = lambda: b.copy(b.S0, b.S)
    kinds = {"potrf_upper (parent's routine)": (prepS, lambda: check(lib.chase_hip_potrf_upper(ctx.h, c, N, b.S.ptr, N), "potrf"))}
    for ob in (256, 512, 1024, 2048):
        kinds[f"potrf_upper_blocked outer_nb={ob}"] = (prepS, lambda ob=ob: check(ctx.potrf_upper_blocked(N, b.S.ptr, N, cplx, ob), "potrf_b"))
    b.compare("(b)", kinds, windows)
    # U for the rest
    b.copy(b.S0, b.S)
    assert ctx.potrf_upper_blocked(N, b.S.ptr, N, cplx, 0) == 0
    # (c) two-sided reduction
    prepA = lambda: b.copy(b.H0, b.A)
    kinds = {}
    for nb in (128, 256, 512, 1024, 2048):
        kinds[f"hegst_upper nb={nb} (recurrence)"] = (prepA, lambda nb=nb: ctx.hegst_upper(N, b.A.ptr, N, b.S.ptr, N, cplx, nb))
    kinds["hegst_upper nb=0 (two full solves)"] = (prepA, lambda: ctx.hegst_upper(N, b.A.ptr, N, b.S.ptr, N, cplx, 0))
    b.compare("(c)", kinds, windows)
    # (d) back-transformation
    ncols = 640 if not small else 64
    X = ctx.empty((N, ncols), b.dt)
    prepX = lambda: check(lib.chase_hip_fill_normal(ctx.h, c, N, ncols, X.ptr, N, 0, 0, N, 13), "fill_normal")
    b.compare("(d)", {f"gev_backtransform {ncols} columns": (prepX, lambda: ctx.gev_backtransform(N, ncols, b.S.ptr, N, X.ptr, N, cplx))}, windows)
    for a in (X, b.A, b.S, b.H0, b.S0):
        a.free()


def solve_case(ctx, N, cplx, nev, nex, windows, say):
    from chase_amd.capi import Solver
    b = Bench(ctx, N, cplx, say)
    say(f"(e) config 2's shape: N = {N} {'complex' if cplx else 'real'}, nev {nev}, nex {nex}, tol 1e-10, otherwise the solver's defaults")
    s = Solver(ctx, None, nev, nex, h_on_device_ptr=b.A.ptr, N=N, cplx=cplx)
    s.set(tol=1e-10)
    X = ctx.empty((N, nev), b.dt)
    t = {"reduce": [], "solve": [], "backtransform": []}
    for w in range(windows + 1):
        b.copy(b.H0, b.A); b.copy(b.S0, b.S)
        ctx.sync()
        t0 = time.perf_counter()
        assert ctx.gev_reduce(N, b.A.ptr, N, b.S.ptr, N, cplx) == 0
        ctx.sync()
        t1 = time.perf_counter()
        st = s.solve()
        ctx.sync()
        t2 = time.perf_counter()
        X.upload(s.V[:, :nev])                                          # (the host copy of the vectors is the solver's result)
        ctx.sync()
        t3 = time.perf_counter()
        ctx.gev_backtransform(N, nev, b.S.ptr, N, X.ptr, N, cplx)
        ctx.sync()
        t4 = time.perf_counter()
        say(f"  {'warm-up' if not w else 'window %d' % w}: reduce {t1 - t0:.3f} s, plain Solver on the reduced matrix {t2 - t1:.3f} s "
            f"({st['iterations']} iterations, {st['filtered_vecs']} filtered vectors, locked {st['locked']}), back-transformation of {nev} "
            f"columns {t4 - t3:.3f} s (+ {t3 - t2:.3f} s upload of the vectors)")
        if w:
            t["reduce"].append(t1 - t0); t["solve"].append(t2 - t1); t["backtransform"].append(t4 - t2)
    med = {k: statistics.median(v) for k, v in t.items()}
    whole = sum(med.values())
    say(f"  medians: reduce {med['reduce']:.3f} s + solve {med['solve']:.3f} s + back-transformation {med['backtransform']:.3f} s = "
        f"{whole:.3f} s for the generalized problem against {med['solve']:.3f} s for the plain Solver on the reduced matrix: "
        f"{whole / med['solve']:.2f} x")
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gev.txt"))
    ap.add_argument("--cases", default="real,complex,solve")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    ap.add_argument("--windows", type=int, default=3)
    args = ap.parse_args()
    from chase_amd.capi import Context
    ctx = Context(0)
    info = ctx.info()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    N = 1536 if args.small else 16384
    cases = args.cases.split(",")
    say("reduction of the generalized Hermitian-definite problem to standard form (scripts/dev_gev.py)")
    say(f"device: {info['name']}, {info['num_cu']} CUs, {info['clock_khz'] / 1000:.0f} MHz max engine clock; {args.windows} alternated windows "
        "after one warm-up of each kind; 'x' = time over the time of the executed flops at the rate of (a)")
    for name, cplx in (("real", False), ("complex", True)):
        if name in cases:
            reduction_case(ctx, N, cplx, args.windows, say, args.small)
    if "solve" in cases:
        solve_case(ctx, N, True, *((64, 16) if args.small else (512, 128)), args.windows, say)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
