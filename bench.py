#!/usr/bin/env python3
"""bench.py — headline benchmark of the MI355X-native ChASE hot path (contract: see the task prompt / DESIGN.md §6).

Workload (every GPU count): BASELINE.json's metric configuration, configs[3] = "cfg4": N = 65536 complex Hermitian fp64,
nev = 2048, nex = 512 (it fits one MI355X: H = 68.7 GB), so the 1 / 2 / 4 / 8 GPU values form a STRONG-scaling series.
The matrix is generated in HBM before the timed region.

A "step" is ONE OUTER ITERATION of the ChASE solve (Chebyshev filter + QR + Rayleigh-Ritz + residuals + locking,
algorithm/algorithm.inc:1491-1720); whole solves run back to back and an iteration observer in the C++ driver
(chase_hip_solver_set_iteration_hook) marks the iteration boundaries: W warm-up iterations are skipped, then EXACTLY K
iterations are timed between two (device sync + barrier) brackets.  Everything a solve does before its first filter
(start vectors, first QR, Lanczos bounds) belongs to that solve's first iteration.  A complete solve takes 9 iterations.
On one GPU the solve in flight ends with the last warm-up step, the timed steps start with a fresh solve, and the solve
in flight ends with the last timed step.
  metric  = Chebyshev-filter HEMM GFLOP/s = flops of the reference's model (2*F*N^2 per filtered vector, F = 4 complex:
            algorithm/performance.hpp:248-260) of the filter HEMMs of the timed iterations / HIP-event time between
            FilterPhaseStart/End (max over ranks, all-reduces included), whole job
  extra   = roofline of the timed filter HEMMs (EXECUTED MFMA flops: the complex filter kernel forms a complex product
            from 3 real MFMA products); with --full also eigenpairs_per_sec (nev / wall of the complete solves), per-phase
            seconds, the parity guard on a complete solve, the four-product kernel timed on full-width HEMMs, the CPU
            oracle on the host cores.
`--dump-outputs DIR` (one GPU) writes the Ritz values, residuals and a seeded row sample of the Ritz vectors as they
stand after the last timed step to DIR/*.npy: the inputs are seeded, so two builds can be compared output for output.
`python bench.py --gpus N` with N > 1 starts its N ranks itself (one process per GPU, RCCL row/column all-reduces over
xGMI on the reference's 2D grid, grid/mpiGrid2D.hpp); under torch.distributed.run (RANK set) it is one of the ranks.
`--ranks threads` runs the N ranks as threads of ONE process (one thread per GPU).  A multi-GPU run proves its transport
before it solves (bus bandwidth of a 256 MB all-reduce per communicator, `transport_proof` in the JSON line) and exits
non-zero instead of printing a scaling number when RCCL is not on xGMI; with `--ranks auto` (default) the way the ranks
hold their devices is settled by short-lived probe children BEFORE this process touches the GPU.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP64_MFMA_PEAK_TFLOPS = 78.6      # MI355X fp64 matrix == vector peak (vendor figure)

# Workload matrix: the Clement-type matrix of the reference's solve tests with its dense Hermitian
# N(0,1)*1e-6 perturbation, scaled by 100/N so that the spectrum spans [-100, 100] like the reference driver's
# --isMatGen matrix (dmax = 100).  Unscaled, ||H|| = N puts the reference's ABSOLUTE tol = 1e-10 below the fp64 residual
# floor at N = 16384 and both the oracle and this backend run into maxIter (measured).
MATRIX_SCALE = 100.0
MATRIX_PERTURB = 1e-6

DEFAULT_WORKLOAD = "cfg4"                    # BASELINE.json "metric": N=64k nev=2048 — on every GPU count (strong scaling)
DEFAULT_BLOCK_CYCLIC = {"cfg4": 64}          # BASELINE configs[3]: block-cyclic distribution (nb = 64, examples/1_hello_world)

WORKLOADS = {
    # name: (N, complex, nev, nex)
    "cfg1": (4096, False, 100, 40),
    "cfg2": (16384, True, 512, 128),
    "cfg3": (32768, False, 1024, 256),
    "cfg3c": (32768, True, 1024, 256),
    "cfg4": (65536, True, 2048, 512),
    # BASELINE configs[4]: pseudo-Hermitian Bethe-Salpeter, chase::Solve_pseudo, nex = nev/4 like the other configurations;
    # synthetic matrix chase_hip_gen_bse (dmin 1, dmax 11, off-diagonal 1e-3 N(0,1)); always runs the grid Impl
    "cfg5": (32768, True, 256, 64),
}
PSEUDO_WORKLOADS = {"cfg5"}
BSE_MATRIX = {"dmin": 1.0, "dmax": 11.0, "offdiag": 1e-3}
PHASES = ("t_all", "t_init", "t_lanczos", "t_filter", "t_qr", "t_rr", "t_resid")


def spectrum_check(lam, N, nev):
    """Full-size parity property: the unperturbed Clement-type matrix has the exact spectrum {-N, -N+2, ..., N}
    (SURVEY.md §8c), the 1e-6 dense Hermitian perturbation moves an eigenvalue by O(1e-6) (first order: eps * v^H G v), and
    the bench matrix is that matrix times MATRIX_SCALE / N.  Returns the largest deviation of the nev computed
    eigenvalues from the analytic ones and the bound it must meet."""
    scale = MATRIX_SCALE / N
    exact = scale * (-N + 2.0 * np.arange(nev))
    dev = float(np.max(np.abs(np.sort(np.asarray(lam)[:nev]) - exact)))
    tol = 50.0 * MATRIX_PERTURB * scale
    return {"max_abs_dev_from_analytic": dev, "bound": tol, "ok": bool(dev <= tol)}


def usable_cores():
    """Host cores this process may really use: the affinity mask, cut by a cgroup CPU quota if there is one (a GPU box
    hands a job a share of its cores; os.cpu_count() reports the machine)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max",):
        try:
            quota, period = open(path).read().split()[:2]
            if quota != "max":
                n = min(n, max(1, int(float(quota) / float(period) + 0.5)))
        except (OSError, ValueError):
            pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        if q > 0 and per > 0:
            n = min(n, max(1, int(q / per + 0.5)))
    except (OSError, ValueError):
        pass
    return max(1, n)


def cpu_baseline(N, cplx, ncols, budget_s=25.0):
    """The CPU path beside the GPU number: the oracle's operators (oracle/chase_oracle.py - numpy on the
    host BLAS / LAPACK, the restatement of Impl/chase_cpu's HEMM = one t_gemm per call, chase_cpu.hpp:449-508) on a BOUNDED
    sample of the workload: a 16384 x 16384 slice of the operator times 1024 columns (2.2e12 flops per complex HEMM call),
    a few full HEMM steps and ONE QR / Rayleigh-Ritz / residual pass at that slice.  `value` is the HEMM rate of the sample;
    the full-size figure is an extrapolation from it and is labelled so."""
    from oracle import chase_oracle as O
    cores = usable_cores()
    blas = "numpy BLAS"
    limiter = None
    try:
        from threadpoolctl import threadpool_info, threadpool_limits
        limiter = threadpool_limits(limits=cores)           # as many BLAS threads as cores we may use, not as the box has
        info = [i for i in threadpool_info() if i.get("user_api") == "blas"]
        if info:
            blas = "%s %s (%s threads)" % (info[0].get("internal_api"), info[0].get("version"), info[0].get("num_threads"))
    except Exception:
        pass
    F = 4 if cplx else 1
    n_s = N
    while n_s * n_s * (16 if cplx else 8) > 6e9:             # the oracle needs its operator on the host: bound the slice
        n_s //= 2
    cols = min(ncols, 1024)
    H = O.clement(n_s, cplx, perturb=0)
    k = O.OracleCPU(H, cols // 2, cols - cols // 2)
    del H
    rng = np.random.default_rng(0)
    k.V1[:] = rng.standard_normal(k.V1.shape)
    if cplx:
        k.V1.imag[:] = rng.standard_normal(k.V1.shape)
    k.V2[:] = k.V1
    t0 = time.perf_counter()
    k.HEMM(cols, 0.01, 0.0, 0)                       # warm-up / thread pool start
    t_first = time.perf_counter() - t0
    hemm_budget = 0.5 * budget_s
    reps = int(max(1, min(10, (hemm_budget - t_first) / max(t_first, 1e-3))))
    t0 = time.perf_counter()
    for _ in range(reps):
        k.HEMM(cols, 0.01, -0.5, 0)
    dt = (time.perf_counter() - t0) / reps
    gflops = 2.0 * F * n_s * n_s * cols / dt / 1e9
    out = {"value": gflops, "unit": "GFLOP/s", "cores": cores, "kind": "port",
           "blas": blas,
           "sample": ("oracle filter HEMM (%s, %s, %d threads on the %d host cores this job may use; the machine reports "
                      "%d) on a %d x %d slice of the workload's operator times %d of its %d columns, %d full steps; the "
                      "rate for the full N = %d workload is extrapolated from this sample, not measured at full size")
                     % ("zgemm" if cplx else "dgemm", blas, cores, cores, os.cpu_count() or 0, n_s, n_s, cols, ncols, reps, N),
           "sample_shape": {"N": n_s, "ncols": cols, "reps": reps, "seconds_per_call": dt,
                            "flop_per_call": 2.0 * F * n_s * n_s * cols}}
    # one QR / Rayleigh-Ritz / residual pass of the oracle at the same slice
    try:
        k.V1[:] = rng.standard_normal(k.V1.shape)
        k.V2[:] = k.V1
        k.Start()
        ops = {}
        t0 = time.perf_counter(); k.QR(0, 1.0); ops["qr_seconds"] = time.perf_counter() - t0
        t0 = time.perf_counter(); k.RR(k.ritzv, cols); ops["rr_seconds"] = time.perf_counter() - t0
        t0 = time.perf_counter(); k.Resd(k.ritzv, k.resid, 0); ops["resd_seconds"] = time.perf_counter() - t0
        ops["qr_variant"] = k.qr_variant
        out["operator_pass"] = ops
    except Exception as e:
        out["operator_pass"] = {"error": str(e)}
    del k
    # second bounded sample: one complete oracle solve of the reference's CPU-runnable configuration (BASELINE configs[0]:
    # N = 4096 real, nev = 100, nex = 40; the reference itself measured 5.44 s on 8 vCPU)
    try:
        t0 = time.perf_counter()
        Hs = O.clement(4096, False, perturb=0)
        ks = O.OracleCPU(Hs, 100, 40)
        so = O.solve(ks)
        ts = time.perf_counter() - t0
        out["solve_sample"] = {"workload": "cfg1 (N=4096 real, nev=100, nex=40), oracle solve", "seconds": ts,
                               "eigenpairs_per_sec": 100.0 / ts, "iterations": so["iterations"],
                               "filtered_vecs": so["filtered_vecs"]}
    except Exception as e:  # the HEMM sample above is the contract; this one is informative
        out["solve_sample"] = {"error": str(e)}
    if limiter is not None:
        limiter.restore_original_limits()
    return out


class CpuBaselineJob:
    """The CPU baseline as a CPU-only CHILD process started at the beginning of the run (it imports numpy / scipy and the
    oracle, never HIP or torch) and joined before the timed region starts: its ~35 s run beside the untimed warm-up
    iterations instead of serially after the GPU work (round-3 verdict: the bench's wall budget), and never beside a timed
    one.  The child gets a clean environment (no profiler preload), so `rocprofv3 -- python bench.py` profiles one GPU
    process."""

    def __init__(self, N, cplx, ncols, budget_s):
        env = {k: v for k, v in os.environ.items()
               if k != "LD_PRELOAD" and not k.startswith(("ROCP", "ROCPROF", "HSA_TOOLS", "ROCTRACER"))}
        self.args = (N, cplx, ncols, budget_s)
        self.out = tempfile.TemporaryFile(mode="w+")
        self.err = tempfile.TemporaryFile(mode="w+")
        self.t0 = time.perf_counter()
        self.proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-baseline-child",
                                      f"{N},{int(bool(cplx))},{ncols},{budget_s}"], env=env, stdout=self.out, stderr=self.err)
        self.waited_s = None

    def join(self):
        """blocks until the child is done; returns the seconds this call had to wait (0 when it finished during warm-up)"""
        if self.waited_s is None:
            t = time.perf_counter()
            self.proc.wait()
            self.waited_s = time.perf_counter() - t
            self.total_s = time.perf_counter() - self.t0
        return self.waited_s

    def result(self):
        self.join()
        self.out.seek(0)
        lines = [l for l in self.out.read().splitlines() if l.startswith("{") and l.endswith("}")]
        if self.proc.returncode == 0 and lines:
            rec = json.loads(lines[-1])
            rec["ran"] = ("CPU-only child process started with the run, beside the untimed warm-up iterations of the GPU "
                          "process (one busy host thread); joined before the timed region (waited %.1f s there)" % self.waited_s)
            return rec
        self.err.seek(0)
        print("bench: cpu-baseline child failed (rc %s): %s - running it in this process" %
              (self.proc.returncode, self.err.read()[-400:]), file=sys.stderr, flush=True)
        return cpu_baseline(*self.args)


def converged_ok(lam, resid, resid_re, tol, spec):
    """The parity guard of a bench line: finite eigenvalues, the reference tests' residual bar (1e-8,
    tests/chase_serial_solve.cpp:144-148) on the solver's and on the independently recomputed residuals, the analytic
    spectrum, and the solver's OWN tolerance on what the reference would see: no pair the solver took as converged
    (residual <= tol; stagnating pairs are locked above it on purpose, algorithm.inc:519-578) may be above tol when its
    residual is recomputed from a fresh four-product H v (two correct evaluations of one residual differ by ~1e-14 ||H||,
    i.e. ~1e-4 tol: the bar is tol (1 + 1e-3))."""
    lam, resid, resid_re = np.asarray(lam), np.asarray(resid), np.asarray(resid_re)
    above = int(np.sum((resid <= tol) & (resid_re > tol * (1 + 1e-3))))
    return bool(np.all(np.isfinite(lam)) and np.max(resid) < 1e-8 and np.max(resid_re) < 1e-8 and above == 0
                and (spec is None or spec["ok"]))


class StepTimer:
    """Times exactly `steps` outer iterations after `warmup` untimed ones, across back-to-back solves.

    sync(): device synchronisation of this rank; barrier(): all ranks; snapshot(): dict of cumulative counters.  The
    boundaries are bracketed sync -> barrier -> clock on both sides, like the contract asks for whole steps."""

    def __init__(self, steps, warmup, sync, barrier, snapshot, progress=None, before_timed=None, cut=False):
        self.steps, self.warmup = steps, warmup
        # cut: the solve in flight at the end of the warm-up is ended there and the timed steps start with a fresh solve,
        # and the solve in flight at the end of the timed steps is ended there too (nothing runs after the last timed step)
        self.cut = cut
        self.sync, self.barrier, self.snapshot = sync, barrier, snapshot
        self.before_timed = before_timed      # called once, right before the opening bracket of the timed region
        self.boundary = 0                     # outer iterations completed so far (all solves)
        self.t0 = self.t1 = None
        self.c0 = self.c1 = None
        self.filtered_timed = 0
        self.per_iter = []                    # (solve index, iteration, filtered vectors, seconds since previous boundary)
        self.solve_index = 0
        self.complete_solves = 0
        self.outside = {}                     # solve index -> seconds its hooks spent outside the solve (joins, brackets)
        self.in_solve = False                 # set by run_timed_solves around each solve: waits before the first solve are nobody's
        self._last = None
        if progress is None:
            progress = os.environ.get("RANK", "0") == "0"
        self.progress = progress and os.environ.get("CHASE_BENCH_QUIET") != "1"

    @property
    def running(self):
        return self.t0 is not None and self.t1 is None

    @property
    def done(self):
        return self.t1 is not None

    def _bracket(self):
        self.sync()
        self.barrier()
        return time.perf_counter(), self.snapshot()

    def start_if_due(self):
        if self.t0 is None and self.boundary == self.warmup:
            # device work the solve has queued up to this boundary (deferred swaps, asynchronous launches) is the SOLVE's time:
            # drain it first, and count as a bench wait only what comes after (round-5 advisor)
            self.sync()
            t = time.perf_counter()
            if self.before_timed is not None:
                self.before_timed()             # (joins the CPU-baseline child: seconds that are not the solve's)
            self.t0, self.c0 = self._bracket()
            self._last = self.t0
            if self.in_solve:
                self.outside[self.solve_index] = self.outside.get(self.solve_index, 0.0) + (self.t0 - t)

    def hook(self, it, filtered, locked, unconverged):
        self.boundary += 1
        if self.progress:                      # one line per outer iteration on stderr: a long run is visibly alive
            print(f"bench: solve {self.solve_index} iteration {it}: {filtered} vectors filtered, {locked} locked, "
                  f"{unconverged} unconverged" + (" [timed]" if self.running else ""), file=sys.stderr, flush=True)
        if self.running:
            self.filtered_timed += filtered
            now = time.perf_counter()          # host clock only: informative per-iteration split, not the timed bracket
            self.per_iter.append((self.solve_index, it, filtered, now - self._last))
            self._last = now
            if self.boundary == self.warmup + self.steps:
                self.sync()                    # (the solve's own queued work, see start_if_due)
                drained = time.perf_counter()
                self.t1, self.c1 = self._bracket()
                if self.in_solve:
                    self.outside[self.solve_index] = self.outside.get(self.solve_index, 0.0) + (self.t1 - drained)
                if self.cut:
                    return True                # end the solve at the last timed step
        if self.cut:
            # the warm-up's solve ends at the last warm-up step; run_timed_solves opens the timed region before the next
            # solve, so the timed steps are the first iterations of fresh solves (the costliest ones of a solve: W warm-up
            # steps then cost about what W timed steps do)
            return self.t0 is None and self.boundary == self.warmup
        self.start_if_due()
        # never cut a solve short: the solve in flight when the timed region ends runs to completion (its remaining
        # iterations are the cheap ones), so that the LAST solve is always a complete one and the independent residual
        # check after the timed region sees that solve's eigenvectors on the device
        return False

    def diff(self, key):
        return self.c1[key] - self.c0[key]


def run_timed_solves(s, timer, nev, capture, after_timed=None, need_complete=True):
    """Back-to-back solves until the timer has its iterations.  capture() returns (eigenvalues, residuals) of the solver's
    last solve; the last COMPLETE solve (all nev pairs locked) is what the parity guard checks.  after_timed() is called
    once, right after the solve that holds the last timed step has returned.  With a cutting timer (StepTimer(cut=True))
    and need_complete, a timed region that ends inside a solve is followed by one complete, untimed solve, so that the
    last solve is a complete one; without need_complete nothing runs after the timed region."""
    complete, last_complete = [], None
    s.set_iteration_hook(timer.hook)
    timer.start_if_due()
    while True:
        timer.in_solve = True
        try:
            st = s.solve()
        finally:
            timer.in_solve = False
        # the solve's own seconds: what its iteration hooks spent waiting (the join of the CPU-baseline child, the barriers of the
        # timed region's brackets) is not the solver's time (round 5: a short default run reported 18.7 s for a 1.7 s solve)
        spent_outside = timer.outside.get(timer.solve_index, 0.0)
        if 0.0 < spent_outside < st["t_all"]:
            st["t_all_with_bench_waits"] = st["t_all"]
            st["t_all"] = st["t_all"] - spent_outside
        if st["locked"] >= nev:
            timer.complete_solves += 1
            complete.append(st)
            last_complete = capture()
        timer.solve_index += 1
        if timer.done and after_timed is not None:
            after_timed()
            after_timed = None
        if timer.cut:
            if timer.done and (not need_complete or st["locked"] >= nev):
                break
            timer.start_if_due()               # (the timed region opens between two solves)
        elif timer.done and timer.complete_solves >= 1:
            break
        if timer.solve_index > timer.warmup + timer.steps + 2:
            raise RuntimeError("bench: solves do not converge (no complete solve within the iteration budget)")
    s.set_iteration_hook(None)
    return complete, last_complete


def fullwidth_probe(s, ctx, N, cplx, nevex, three_m, reps=4):
    """A few full-width filter HEMMs (phase-1 kernel symbol) timed with HIP events on the launch stream, with the
    three-multiplication scheme on or off: the four-product run is the reference's zgemm arithmetic."""
    from chase_amd.capi import lib, check, gemm_counters
    lib.chase_hip_set_gemm3m(1 if three_m else 0)
    try:
        s.Start()
        s.initVecs(True)
        check(lib.chase_hip_ctx_set_phase(ctx.h, 1), "set_phase")
        s.HEMM(nevex, 0.01, -0.5, 0)                     # untimed: first launch of this instantiation
        ctx.sync()
        m0, e0, n0 = gemm_counters(ctx, 1)
        ctx.timer_start()
        for _ in range(reps):
            s.HEMM(nevex, 0.01, -0.5, 0)
        ms = ctx.timer_stop()
        m1, e1, n1 = gemm_counters(ctx, 1)
    finally:
        check(lib.chase_hip_ctx_set_phase(ctx.h, 0), "set_phase")
        lib.chase_hip_set_gemm3m(1)
    model, execd = (m1 - m0) / (ms * 1e-3) / 1e12, (e1 - e0) / (ms * 1e-3) / 1e12
    return {"bound": "mfma",
            "kernel": "gemm_f64_kernel<cplx,op=N,TAG=1,%s> full-width filter HEMM (ncols = %d)" % ("3M" if three_m else "4M", nevex),
            "achieved": execd, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": execd / FP64_MFMA_PEAK_TFLOPS,
            "algorithmic": model, "launches": int(n1 - n0), "avg_launch_ms": ms / max(int(n1 - n0), 1), "traffic": None}


def whole_run_object(tot, world):
    """The same per-call figures over EVERY filter HEMM call of the process so far (warm-up, timed and trailing iterations
    of all solves, before the full-width probes): the set of launches a `rocprofv3 --kernel-trace --stats` summary of this
    command averages over (sum of the TAG=1 kernels' time / calls)."""
    calls = max(int(tot["hemm_calls"]), 1)
    fs = tot["filter_ms"] * 1e-3
    return {"launches": calls, "avg_launch_ms": tot["filter_ms"] / calls, "filter_seconds_device": fs,
            "achieved": tot["exec"] / fs / 1e12 / world if fs > 0 else None,
            "algorithmic": tot["model"] / fs / 1e12 / world if fs > 0 else None}


def roofline_object(model_flops, exec_flops, filt_s, calls, world, note_extra=""):
    """roofline of the dominant kernel: EXECUTED MFMA flops / HIP-event filter time / peak, per GPU (<= 1); the rate in the
    reference's flop model (which `value` is quoted in) is `algorithmic`."""
    execd = exec_flops / filt_s / 1e12 / world
    model = model_flops / filt_s / 1e12 / world
    return {"bound": "mfma", "kernel": "gemm_f64_kernel<cplx,op,TAG=1> (Chebyshev-filter HEMM), per GPU",
            "achieved": execd, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": execd / FP64_MFMA_PEAK_TFLOPS,
            "traffic": None, "algorithmic": model, "algorithmic_frac_of_peak": model / FP64_MFMA_PEAK_TFLOPS,
            "executed_over_model": exec_flops / model_flops if model_flops else None,
            "launches": calls, "avg_launch_ms": filt_s * 1e3 / max(calls, 1),
            "flop_per_launch_avg": model_flops / max(calls, 1) / world,
            "launch_unit": "one HEMM call per GPU = whole-tile kernel (+ ragged-column kernel when the width is not a "
                           "multiple of the tile width) + tail reduce; rocprofv3: sum over the TAG=1 kernels",
            "note": "achieved/frac = flops the matrix cores EXECUTE (the complex filter kernel forms each complex product "
                    "from 3 real MFMA products, 3/4 of the reference model's 4) / HIP-event time between "
                    "FilterPhaseStart/End on the launch stream; algorithmic = the reference's model "
                    "2*F*N^2*ncols, F = 4 (the unit of `value`)" + note_extra}


def attach_traffic(out, workload):
    pmc = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if os.path.exists(pmc):
        try:
            rec = json.load(open(pmc))
            if rec.get("workload") == workload:
                out["roofline"]["traffic"] = rec.get("hbm_bytes_per_launch")
                out["roofline"]["traffic_source"] = ("profiles/pmc_traffic.json (%s): a separate rocprofv3 --pmc pass over "
                                                     "one full-width launch of this kernel, NOT measured in this run"
                                                     % rec.get("source", "see the file"))
                out["roofline"]["traffic_note"] = rec.get("note")
        except Exception:
            pass


def attach_replay(out, workload):
    """The compute side of the multi-GPU solve as measured by the single-rank replay (bench.py --replay-rank, a SEPARATE run on
    one GPU, recorded in profiles/): T_rank per grid and the speed-up bound it implies.  Context for the scaling series this
    line starts; not measured in this run and labelled so."""
    path = os.path.join(ROOT, "profiles", "r06_replay_cfg4.json")
    if workload != "cfg4" or not os.path.exists(path):
        return
    try:
        rec = json.load(open(path))
        out["multi_gpu_compute_side"] = {
            "source": "profiles/r06_replay_cfg4.json: `bench.py --replay-rank 4x2,2x2,2x1` - ONE rank of each grid replaying the "
                      "taped call sequence of a real single-GPU solve on a loopback grid (no communication), NOT measured in this run",
            "single_gpu_solve_seconds": rec["single_gpu"]["solve_seconds"],
            "T_rank_seconds": {r["grid"]: r["T_rank_seconds"] for r in rec["replays"]},
            "speedup_bound": {r["grid"]: r["compute_side_speedup_bound"] for r in rec["replays"]}}
    except Exception:
        pass


DUMP_ROWS = 1024                 # --dump-outputs: rows of the eigenvector block written (a fixed, seeded sample)


def dump_outputs(path, N, nev, ritzv, resid, V):
    """--dump-outputs: what a caller of the solve receives after the last timed step - the Ritz values and residuals of all
    nev + nex columns and the first nev Ritz vectors on a fixed, seeded sample of DUMP_ROWS rows (real and imaginary part
    in the last axis for a complex workload), all float64 (< 64 MB for every workload)."""
    os.makedirs(path, exist_ok=True)
    rows = np.sort(np.random.default_rng(20240).choice(N, size=min(N, DUMP_ROWS), replace=False))
    vs = np.asarray(V)[rows, :nev]
    if np.iscomplexobj(vs):
        vs = np.stack([vs.real, vs.imag], axis=-1)
    arrays = {"ritz_values": ritzv, "residuals": resid, "ritz_vectors_sample": vs, "ritz_vectors_sample_rows": rows}
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def run_single(args):
    """One GPU, the single-GPU Impl.  A plain run sets up, runs W warm-up and K timed outer iterations (StepTimer(cut=True):
    the timed steps start with a fresh solve and nothing runs after the last of them) and reports the filter rate of the
    timed steps.  --full adds what takes runs or checks of its own: the CPU baseline child, one complete solve behind the
    timed steps for the parity guard (analytic spectrum, residuals recomputed from H), the full-width 4M / 3M kernel probes,
    the bare MFMA loop and the figures recorded in profiles/."""
    from chase_amd.capi import Context, Solver, gemm_counters
    N, cplx, nev, nex = WORKLOADS[args.workload]
    if args.n:
        N = args.n
    nevex = nev + nex
    cpu_job = None if (args.no_cpu_baseline or not args.full) else CpuBaselineJob(N, cplx, nevex, args.cpu_budget)
    ctx = Context(0)
    info = ctx.info()
    dH = ctx.gen_clement(N, cplx, scale=MATRIX_SCALE / N, perturb=MATRIX_PERTURB, seed=42)
    ctx.sync()
    s = Solver(ctx, None, nev, nex, h_on_device_ptr=dH.ptr, N=N, cplx=cplx)
    s.set(device_rng=1)
    F = 4 if cplx else 1

    def snapshot():
        model, execd, calls = gemm_counters(ctx, 1)
        return {"filter_ms": s.get("filter_ms"), "hemm_calls": s.get("hemm_calls"),
                "reused": s.get("hemm_reused_vecs"), "model": model, "exec": execd, "gemms": calls}

    def after_timed():
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, N, nev, s.ritzv, s.resid(), s.V)

    timer = StepTimer(args.steps, args.warmup, ctx.sync, lambda: None, snapshot,
                      before_timed=(cpu_job.join if cpu_job is not None else None), cut=True)
    complete, last = run_timed_solves(s, timer, nev, lambda: (s.ritzv[:nev].copy(), s.resid()[:nev].copy()),
                                      after_timed=after_timed, need_complete=args.full)
    wall = timer.t1 - timer.t0
    filt_s = timer.diff("filter_ms") * 1e-3
    calls = int(timer.diff("hemm_calls"))
    reused = int(timer.diff("reused"))
    model_flops, exec_flops = timer.diff("model"), timer.diff("exec")
    hemm_vecs = timer.filtered_timed - reused
    # the kernel-side books must agree with the reference's count: 2*F*N^2 per vector that went through a HEMM
    formula = 2.0 * F * N * N * hemm_vecs
    assert abs(model_flops - formula) <= 1e-9 * formula, (model_flops, formula)
    gflops = model_flops / filt_s / 1e9
    out = {
        "metric": "chebyshev_filter_hemm_gflops", "value": gflops, "unit": "GFLOP/s",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": wall / args.steps * 1e3,
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "complex f64" if cplx else "f64", "data": "synthetic",
        "config": {"workload": f"{args.workload}: ChASE solve, perturbed Clement-type Hermitian (x100/N) N={N} "
                               f"{'complex' if cplx else 'real'} fp64, nev={nev} nex={nex}, tol 1e-10, deg 20 opt, 1x1 grid; "
                               "step = one outer iteration (filter+QR+RR+residuals+locking), solves back to back, "
                               "the timed steps from a fresh solve",
                   "N": N, "nev": nev, "nex": nex, "grid": "1x1", "step": "outer iteration"},
        "full": bool(args.full), "complete_solves": len(complete),
        "pct_fp64_mfma_peak": 100.0 * exec_flops / filt_s / 1e12 / FP64_MFMA_PEAK_TFLOPS,
        "timed": {"filtered_vecs": timer.filtered_timed, "hemm_vecs": hemm_vecs, "first_step_vecs_from_rr": reused,
                  "filter_seconds_device": filt_s, "wall_seconds": wall,
                  "iterations": [{"solve": a, "iteration": b, "filtered_vecs": c, "seconds": d} for a, b, c, d in timer.per_iter]},
        "device": info["name"],
        "roofline": roofline_object(model_flops, exec_flops, filt_s, calls, 1),
    }
    if complete:
        st = complete[-1]
        solve_s = float(np.mean([c["t_all"] for c in complete]))
        out.update({"eigenpairs_per_sec": nev / solve_s, "solve_seconds": solve_s,
                    "iterations_per_solve": st["iterations"], "filtered_vecs_per_solve": st["filtered_vecs"],
                    "phase_seconds_last_complete_solve": {k: st[k] for k in PHASES}})
    out["roofline"]["whole_run"] = whole_run_object(snapshot(), 1)
    if args.full:
        lam, resid = last
        spec = spectrum_check(lam, N, nev)
        # independent check outside the timed region (the reference's solve tests: tests/chase_serial_solve.cpp:144-148,
        # 195-199): one fresh four-product H V over the nev eigenvectors of the last solve (a complete one) + the
        # residual-norm kernel.  The solver's own residuals come from (H Q) A left behind by Rayleigh-Ritz,
        # these from H itself.
        resid_re = s.recompute_residuals(nev, lam)
        out.update({"converged": converged_ok(lam, resid, resid_re, s.get("tol"), spec), "max_resid": float(np.max(resid)),
                    "max_resid_recomputed": float(np.max(resid_re)),
                    "residuals_rechecked_on_the_tolerance": int(s.get("resd_rechecked")), "spectrum_check": spec})
        attach_traffic(out, args.workload)
        attach_replay(out, args.workload)
        if not args.no_probe and cplx:
            # reference arithmetic (four real products per complex product, the reference's zgemm) on the same launch shape
            out["roofline_4m"] = fullwidth_probe(s, ctx, N, cplx, nevex, three_m=False)
            out["roofline_3m_fullwidth"] = fullwidth_probe(s, ctx, N, cplx, nevex, three_m=True)
        # what THIS device's matrix pipe sustains in a bare register-resident MFMA loop right after the sustained load
        # above (context for `frac`: the boxes of the pool differ by a few per cent on the 3M kernel; never its denominator)
        try:
            out["roofline"]["bare_mfma_loop_tflops_this_device"] = ctx.mfma_f64_peak()
        except Exception:  # informative only
            out["roofline"]["bare_mfma_loop_tflops_this_device"] = None
    s.close()
    del dH
    ctx.close()
    if cpu_job is not None:
        out["cpu_baseline"] = cpu_job.result()
    return out


def kfd_gpu_count():
    """GPUs of this node from the driver's topology files - without initialising any GPU runtime in this process."""
    n = 0
    base = "/sys/class/kfd/kfd/topology/nodes"
    try:
        for d in os.listdir(base):
            try:
                props = dict(l.split()[:2] for l in open(os.path.join(base, d, "properties")) if len(l.split()) >= 2)
                if int(props.get("simd_count", "0")) > 0:
                    n += 1
            except (OSError, ValueError):
                pass
    except OSError:
        return 0
    return n


def bind_one_device(env, local_rank):
    """One process per GPU means one GPU per process: restrict the ROCm runtime of a rank to its own device BEFORE the rank
    touches HIP, so that no rank holds the other ranks' devices open (the reference picks device = node-local rank,
    grid/mpiGrid2D.hpp:225-233; the pool's boxes allow only a few processes per card).  ROCR_VISIBLE_DEVICES is what keeps
    the runtime from opening a device at all (HIP_VISIBLE_DEVICES only hides it from the HIP API); RCCL finds its xGMI peers
    through the driver topology, not through visibility.  An existing visibility list is honoured: the rank takes ITS entry.
    CHASE_HIP_BIND=0 restores full visibility (every rank then selects device local_rank itself).  Edits `env` in place and
    returns the physical index (or None when binding is off)."""
    if env.get("CHASE_HIP_BIND", "1") == "0" or env.get("CHASE_HIP_TRANSPORT") == "host":
        return None                                       # (the host test transport lets ranks SHARE a device)
    def ids(name):
        v = env.get(name, "").strip()
        return [x.strip() for x in v.split(",") if x.strip()] if v else None
    rocr = ids("ROCR_VISIBLE_DEVICES")
    hipv = ids("HIP_VISIBLE_DEVICES") or ids("CUDA_VISIBLE_DEVICES")
    pick = str(local_rank)
    if hipv is not None:                                  # HIP's list indexes into the runtime's list
        pick = hipv[local_rank % len(hipv)]
    if rocr is not None:
        pick = rocr[int(pick) % len(rocr)] if pick.isdigit() else pick
    elif pick.isdigit():
        ngpu = kfd_gpu_count()
        if ngpu and int(pick) >= ngpu:                    # more ranks than devices: wrap like device = local_rank % ndev
            pick = str(int(pick) % ngpu)
    env["ROCR_VISIBLE_DEVICES"] = pick
    env.pop("HIP_VISIBLE_DEVICES", None)
    env.pop("CUDA_VISIBLE_DEVICES", None)
    env["CHASE_HIP_BOUND_DEVICE"] = pick                  # for the rank's report line; device ordinal inside the rank is 0
    return pick


# ---- how the ranks of a multi-GPU run hold their devices -------------------------------------------------------------------
# "bound":   one process per GPU, each process's ROCm runtime sees ONLY its device (ROCR_VISIBLE_DEVICES): one process per
#            card (the pool's boxes allow few), RCCL must reach the invisible peers through IPC handles
# "unbound": one process per GPU, all devices visible, device = local rank - what the reference does
#            (grid/mpiGrid2D.hpp:225-233) and what RCCL is tested with most; every process opens every card
# "threads": ONE process, one thread per GPU - no IPC, no visibility question, one process per card; under
#            torch.distributed.run rank 0 hosts the threads and the other ranks leave without touching the GPU
# `--ranks auto` tries them in this order with short-lived PROBE children (bench.py --transport-probe: context, RCCL
# communicators, the 256 MB all-reduce proof) started before this process has touched the GPU; the first mode whose probe
# exits 0 runs the bench.  A mode is never switched inside a process that has initialised HIP.
MODES = ("bound", "unbound", "threads")
PROBE_TIMEOUT_S = float(os.environ.get("CHASE_BENCH_PROBE_TIMEOUT", "150"))


def fake_hosts(env):
    """CHASE_BENCH_FAKE_HOSTS=1: a functional rehearsal of the multi-GPU run with REAL RCCL collectives on a box with ONE GPU.
    RCCL refuses two ranks of a communicator on one device of one host, but tells hosts apart by NCCL_HOSTID: every rank process
    gets its own "host" and the ranks talk through RCCL's socket transport over loopback, all on the box's one device (the
    binding wraps local ranks onto the devices there are).  Tests only: the numbers say nothing about xGMI, and the transport
    proof's bar is lowered to 0.  The mode selection runs as in a real job - probe children, real communicators."""
    return env.get("CHASE_BENCH_FAKE_HOSTS") == "1"


def mode_env(env, mode, local_rank):
    """environment of a rank process in `mode` (edits a copy)"""
    env = dict(env)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.pop("CHASE_HIP_BOUND_DEVICE", None)
    if fake_hosts(env):
        env["NCCL_HOSTID"] = "chase-bench-host-%d" % local_rank
        for k, v in (("NCCL_SOCKET_IFNAME", "lo"), ("NCCL_IB_DISABLE", "1"), ("NCCL_NET", "Socket"), ("NCCL_SHM_DISABLE", "1"),
                     ("NCCL_P2P_DISABLE", "1"), ("CHASE_HIP_MIN_BUSBW_GBPS", "0")):
            env.setdefault(k, v)
    if mode == "bound":
        env["CHASE_HIP_BIND"] = "1"
        bind_one_device(env, local_rank)
    else:
        env["CHASE_HIP_BIND"] = "0"
    return env


def free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def run_children(cmds_envs, timeout_s):
    """Starts the given (argv, env, stdout) children, waits for all of them; the first failure stops the others (exactly the
    processes started here).  Returns the first non-zero exit status (124 for a timeout), else 0."""
    procs = [subprocess.Popen(argv, env=env, stdout=out if out is not None else sys.stderr, stderr=sys.stderr)
             for argv, env, out in cmds_envs]
    rc, t0, term_at = 0, time.perf_counter(), None
    try:
        alive = set(range(len(procs)))
        while alive:
            for r in sorted(alive):
                code = procs[r].poll()
                if code is None:
                    continue
                alive.discard(r)
                if code != 0 and rc == 0:
                    rc = code if code > 0 else 1
                    print(f"bench: rank {r} exited with status {code}; stopping the other ranks", file=sys.stderr)
                    for q in alive:
                        procs[q].terminate()
                    term_at = term_at or time.perf_counter()
            if alive and timeout_s and time.perf_counter() - t0 > timeout_s:
                print(f"bench: ranks still running after {timeout_s:.0f} s; stopping them", file=sys.stderr)
                rc = rc or 124
                for q in alive:
                    procs[q].terminate()
                term_at = term_at or time.perf_counter()
                timeout_s = None
            if alive and term_at and time.perf_counter() - term_at > 15.0:
                for q in alive:                         # a rank that ignores SIGTERM (stuck in a collective): exactly these pids
                    procs[q].kill()
                term_at = time.perf_counter()
            time.sleep(0.2)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return rc


def fake_probe_rc(mode):
    """test hook (tests/test_bench_contract.py): CHASE_BENCH_FAKE_PROBE='{"bound": 5, "unbound": 0}' answers the probe of a
    mode without touching a GPU"""
    spec = os.environ.get("CHASE_BENCH_FAKE_PROBE")
    if not spec:
        return None
    return int(json.loads(spec).get(mode, 1))


def choose_mode_as_parent(args, argv):
    """`python bench.py --gpus N` without a launcher: try the process modes with N probe children each"""
    n = args.gpus
    for mode in MODES[:2]:
        rc = fake_probe_rc(mode)
        if rc is None:
            port = free_port()
            kids = []
            for r in range(n):
                env = mode_env(os.environ, mode, r)
                env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                           MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
                kids.append(([sys.executable, os.path.abspath(__file__)] + argv + ["--transport-probe"], env, None))
            rc = run_children(kids, PROBE_TIMEOUT_S)
        print(f"bench: probe of mode '{mode}': exit status {rc}", file=sys.stderr, flush=True)
        if rc == 0:
            return mode
    return "threads"


def choose_mode_as_rank(args, argv):
    """Under torch.distributed.run: this process is one of N rank processes and has NOT touched the GPU.  Every rank starts
    its own probe child per candidate mode; the children of all ranks meet on a port derived from MASTER_PORT, agree on the
    outcome among themselves and exit with the same status, so every rank reaches the same decision without talking."""
    rank = int(os.environ["RANK"])
    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    base = int(os.environ.get("MASTER_PORT", "29500"))
    for i, mode in enumerate(MODES[:2]):
        rc = fake_probe_rc(mode)
        if rc is None:
            env = mode_env(os.environ, mode, local_rank)
            env["MASTER_PORT"] = str(base + 101 + i if base + 101 + i < 65536 else base - 101 - i)
            # the children rendezvous among themselves: rank 0's child hosts the store on that port (the launcher's agent store
            # on MASTER_PORT belongs to the rank processes)
            for k in [k for k in env if k.startswith("TORCHELASTIC_")]:
                env.pop(k)
            env["CHASE_BENCH_QUIET"] = "1"
            rc = run_children([([sys.executable, os.path.abspath(__file__)] + argv + ["--transport-probe"], env, None)],
                              PROBE_TIMEOUT_S)
        if rank == 0:
            print(f"bench: probe of mode '{mode}': exit status {rc}", file=sys.stderr, flush=True)
        if rc == 0:
            return mode
    return "threads"


def spawn_ranks(args, argv, mode):
    """`python bench.py --gpus N` (N > 1) without a launcher: start N ranks of this script as child processes — one per
    GPU, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set like torch.distributed.run does (the reference bootstraps its own
    communicators too, grid/mpiGrid2D.hpp:448-484).  Nothing in this parent has touched HIP or torch.  Rank 0's JSON line
    is relayed as the last line of stdout; the exit status is non-zero if any rank failed."""
    port = free_port()
    n = args.gpus
    out0 = tempfile.TemporaryFile(mode="w+")
    kids = []
    for r in range(n):
        env = mode_env(os.environ, mode, r)
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), CHASE_BENCH_MODE=mode)
        kids.append(([sys.executable, os.path.abspath(__file__)] + argv, env, out0 if r == 0 else None))
    rc = run_children(kids, None)
    out0.seek(0)
    lines = [l.rstrip("\n") for l in out0.read().splitlines() if l.strip()]
    js = [l for l in lines if l.startswith("{") and l.endswith("}")]
    for l in lines:
        if not js or l is not js[-1]:
            print(l, file=sys.stderr)
    if rc == 0 and not js:
        print("bench: rank 0 produced no result line", file=sys.stderr)
        rc = 1
    if js and rc == 0:
        print(js[-1], flush=True)
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: 3 warm-up + 6 timed iterations = the 9 iterations of one complete cfg4 solve (minutes on one GPU)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default=None, choices=sorted(WORKLOADS))
    ap.add_argument("--n", "--size", dest="n", type=int, default=0, help="override N (development only)")
    ap.add_argument("--full", action="store_true",
                    help="besides the timed steps: the CPU baseline, the parity guard on a complete solve, the full-width "
                         "kernel probes and the recorded profile figures (a plain run measures the headline figure only)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the solve hands its caller after the last timed step to DIR/<name>.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-probe", action="store_true", help="--full: skip the full-width 4M / 3M kernel probes")
    ap.add_argument("--cpu-budget", type=float, default=25.0)
    ap.add_argument("--dist", action="store_true",
                    help="run the grid Impl (pChaseHip) even on one GPU (1x1 grid; development: panel-pipeline overheads)")
    ap.add_argument("--block-cyclic", type=int, default=-1,
                    help="block size of a block-cyclic H distribution (0 = block layout, -1 = the workload's default)")
    ap.add_argument("--ranks", default="auto", choices=("auto", "processes", "threads") + MODES,
                    help="how the ranks of a multi-GPU run hold their devices: processes (= bound: one process per GPU, one "
                         "visible device each), unbound (all devices visible), threads (one process, one thread per GPU), "
                         "auto (default): the first of bound / unbound / threads whose transport probe passes")
    ap.add_argument("--no-autotune", action="store_true",
                    help="multi-GPU runs: keep the default panel width / K-piece granularity / communication streams instead "
                         "of measuring them before the first solve (chase_amd/autotune.py)")
    ap.add_argument("--replay-rank", default=None, metavar="GRIDS",
                    help="single-rank replay (chase_amd/replay.py): e.g. 4x2 or 4x2,2x2,2x1 - ONE rank of each grid is driven "
                         "through the taped call sequence of a real single-GPU solve of the workload on a loopback grid (no "
                         "communication): the compute side of the multi-GPU solve, measured on one GPU")
    ap.add_argument("--loopback-busbw", default=None, metavar="GBPS[,GBPS...]",
                    help="replay: MODEL the absent collectives - each all-reduce / broadcast holds its communication stream and "
                         "32 workgroups for latency + wire bytes / this bus bandwidth (0 = nothing enqueued); one replay per value")
    ap.add_argument("--loopback-latency-us", type=float, default=20.0)
    ap.add_argument("--loopback-wgs", default="32", help="replay: workgroups a modelled collective holds (comma list)")
    ap.add_argument("--replay-panel", type=int, default=0, help="replay: panel width of the pipelined HEMM (columns)")
    ap.add_argument("--replay-panel-rounds", type=int, default=-1, help="replay: K-piece granularity of the panel products (0 = off)")
    ap.add_argument("--replay-comm-streams", type=int, default=0, help="replay: 1 or 2 communication streams")
    ap.add_argument("--replay-autotune", type=int, default=0, metavar="TRIALS",
                    help="replay: run the first-contact self-tuning (chase_amd/autotune.py) on the replayed rank first, with this "
                         "trial budget, against the modelled collectives")
    ap.add_argument("--replay-no-pipeline", action="store_true", help="replay: every collective waited for where it is issued")
    ap.add_argument("--tape", default=None, help="scalar tape file (.npz): loaded if it exists, else recorded and saved there")
    ap.add_argument("--replay-rank-index", type=int, default=0, help="which rank of the grid is replayed (default 0 = (0,0))")
    ap.add_argument("--oplog-out", default=None, help="write the replayed rank's operator log there (%%g = grid)")
    ap.add_argument("--transport-probe", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--cpu-baseline-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.cpu_baseline_child:
        # CPU-only child of CpuBaselineJob: numpy / scipy / the oracle, nothing that touches a GPU
        N, cplx, ncols, budget = args.cpu_baseline_child.split(",")
        print(json.dumps(cpu_baseline(int(N), bool(int(cplx)), int(ncols), float(budget))), flush=True)
        return
    if args.steps < 1 or args.warmup < 0:
        ap.error("need --steps >= 1 and --warmup >= 0")
    if args.workload is None:
        args.workload = DEFAULT_WORKLOAD
    if args.dump_outputs and (args.gpus > 1 or args.dist or args.replay_rank or args.workload in PSEUDO_WORKLOADS
                              or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        ap.error("--dump-outputs: only the single-GPU solve (--gpus 1, a Hermitian workload) writes its outputs")
    if args.dump_outputs:
        args.dump_outputs = os.path.abspath(args.dump_outputs)
    if args.ranks == "processes":
        args.ranks = "bound"
    argv = [a for a in sys.argv[1:] if a != "--transport-probe"]
    launched = "RANK" in os.environ and "WORLD_SIZE" in os.environ
    world = int(os.environ.get("WORLD_SIZE", "1")) if launched else 1
    host_transport = os.environ.get("CHASE_HIP_TRANSPORT") == "host"

    # ---- settle the mode of a multi-GPU run BEFORE anything initialises HIP / torch in this process ---------------------
    mode = os.environ.get("CHASE_BENCH_MODE") or (args.ranks if args.ranks != "auto" else None)
    if mode is None and os.environ.get("CHASE_HIP_BIND") == "0":
        mode = "unbound"                                 # (round 3's switch, kept)
    if args.gpus > 1 and not launched:
        if mode is None:
            mode = "bound" if host_transport else choose_mode_as_parent(args, argv)
        if mode != "threads":
            sys.exit(spawn_ranks(args, argv, mode))
    elif launched and world > 1 and not args.transport_probe:
        if mode is None:
            mode = "bound" if host_transport else choose_mode_as_rank(args, argv)
        if mode == "threads" and int(os.environ["RANK"]) != 0:
            return                                       # rank 0 hosts the threads; this rank never touches the GPU
        if mode in ("bound", "unbound"):
            os.environ.update(mode_env(os.environ, mode, int(os.environ.get("LOCAL_RANK", os.environ["RANK"]))))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # stdout carries the ONE JSON line and nothing else: whatever libraries write to file descriptor 1 on the way (gloo's
    # connection notes, RCCL's banner) is sent to stderr, the line goes to the real stdout at the end
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    def emit(out):
        if out is not None:
            os.write(real_stdout, (json.dumps(out) + "\n").encode())

    if args.replay_rank:
        from chase_amd.replay import run as run_replay
        emit(run_replay(args))
        return
    if mode == "threads" and (args.gpus > 1 or world > 1):
        from chase_amd.dist_bench import run_threads
        emit(run_threads(args, max(args.gpus, world)))
        return
    if world > 1 or args.dist or args.workload in PSEUDO_WORKLOADS:
        if not launched:
            # grid Impl on a 1x1 grid (communicator-free) when started directly on one GPU
            os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()))
        from chase_amd.dist_bench import run_distributed
        emit(run_distributed(args, probe_only=args.transport_probe))
        return
    emit(run_single(args))


if __name__ == "__main__":
    main()
