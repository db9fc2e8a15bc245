"""Mixed-precision filter on the process grid: what the fp32-input / fp64-output product and the switch buy a rank.  Writes
profiles/mixed_precision_grid.txt.

(a) the panel product of one rank as the pipelined HEMM issues it: local block 16384 x 32768 complex (one rank of N = 65536 on
    4 x 2) and 16384 x 16384 real (one rank of config 3, N = 32768 on 2 x 2), 256 columns, op N (row -> column product) and op C
    (column -> row).  fp64: chase_hip_gemm_d / _z in phase 1 with gemm_min_rounds = 4 (the K-split the panels get beside a
    collective).  Mixed: chase_hip_convert_d2s of the 256-column input panel + chase_hip_gemm_sd / _cz on the fp32 shadow of the
    block.  Timed alternately in one process: HIP events around windows of back-to-back products, median and spread of the windows.
(b) whole solves on a 2 x 2 grid of rank threads on the shared-device transport (one GPU: the four ranks share its CUs) with
    mixed_precision off and on, alternated: seconds, iterations, filtered vectors, columns filtered in fp32.
(c) `bench.py --replay-rank 4x2 --tape profiles/r05_cfg4_tape.npz`, unchanged, in a child process with
    CHASE_HIP_MIXED_PRECISION unset and = 1: T_rank and the filter phase of one rank of the 4 x 2 grid.

    python scripts/dev_mixed_precision_grid.py [--out FILE] [--skip-solves] [--skip-replay] [--small]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MATRIX_SCALE, MATRIX_PERTURB = 100.0, 1e-6          # bench.py's matrix


def panel_case(ctx, m_loc, n_loc, w, cplx, windows, reps, say):
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
        Y, Ym = ctx.empty((rows_out, w), dt), ctx.empty((rows_out, w), dt)
        alpha, beta = 0.01, 0.0

        def f64():
            check(lib.chase_hip_ctx_set_gemm_min_rounds(ctx.h, 4), "min_rounds")
            ctx.gemm(op, rows_out, w, rows_in, alpha, H.ptr, m_loc, X.ptr, rows_in, beta, Y.ptr, rows_out, cplx)
            check(lib.chase_hip_ctx_set_gemm_min_rounds(ctx.h, 0), "min_rounds")

        def mixed():
            ctx.convert_d2s(rows_in, w, X.ptr, rows_in, Xs.ptr, rows_in, cplx)
            ctx.gemm32w(op, rows_out, w, rows_in, alpha, Hs.ptr, m_loc, Xs.ptr, rows_in, beta, Ym.ptr, rows_out, cplx)

        for _ in range(2):                              # warm-up: code objects, workspace, clocks
            f64(); mixed()
        ctx.sync()
        a, b = Y.download()[:, 0], Ym.download()[:, 0]
        worst = float(np.max(np.abs(a - b)) / np.max(np.abs(a)))
        t64, tmx = [], []
        for _ in range(windows):                        # alternating windows
            for fn, acc in ((f64, t64), (mixed, tmx)):
                ctx.timer_start()
                for _ in range(reps):
                    fn()
                acc.append(ctx.timer_stop() / reps)
        flops = 2.0 * (4 if cplx else 1) * m_loc * n_loc * w
        m64, mmx = statistics.median(t64), statistics.median(tmx)
        say(f"  H_loc {m_loc} x {n_loc} {'complex' if cplx else 'real   '} op {op} {w} columns: fp64 {m64:8.3f} ms "
            f"({flops / m64 * 1e-9:6.1f} TF/s model, min {min(t64):.3f} max {max(t64):.3f})   convert + fp32 product {mmx:8.3f} ms "
            f"({flops / mmx * 1e-9:6.1f} TF/s, min {min(tmx):.3f} max {max(tmx):.3f})   ratio fp64 / mixed = {m64 / mmx:.2f}   "
            f"max |mixed - fp64| / max |fp64| on a column = {worst:.1e}")
        out[op] = m64 / mmx
        for d in (X, Xs, Y, Ym):
            d.free()
    check(lib.chase_hip_ctx_set_phase(ctx.h, 0), "set_phase")
    H.free(); Hs.free()
    return out


def scenario_solves(ctx, grid, comm, N, cplx, nev, nex, lines):
    from chase_amd import dist as cd
    rl, cl = cd.Layout(N, 0, grid.nprow), cd.Layout(N, 0, grid.npcol)
    dH = cd.gen_clement_local(ctx, N, cplx, rl, cl, grid.myrow, grid.mycol, scale=MATRIX_SCALE / N, perturb=MATRIX_PERTURB)
    s = cd.DistSolver(ctx, grid, dH, N, nev, nex, cplx, 0, 0)
    s.set(device_rng=1)
    res = {}
    for label, on in (("warm-up (off)", 0), ("off", 0), ("on", 1), ("off", 0), ("on", 1), ("off", 0), ("on", 1)):
        s.set(mixed_precision=on, reset_counters=1)
        ctx.sync(); comm.barrier()
        t0 = time.perf_counter()
        st = s.solve()
        ctx.sync(); comm.barrier()
        dt = time.perf_counter() - t0
        r = s.recompute_residuals(nev)
        if comm.rank == 0:
            lines.append(f"  2x2 N={N} {'complex' if cplx else 'real'} {nev}/{nex} {label:13s} {dt:8.3f} s  filter {s.get('filter_ms') * 1e-3:7.3f} s  "
                         f"iterations {st['iterations']:2d}  filtered vectors {st['filtered_vecs']:7d}  in fp32 "
                         f"{int(s.get('hemm_sp_vecs')):7d} ({int(s.get('sp_filters'))} filter calls)  locked {st['locked']}  "
                         f"max fresh fp64 residual {float(np.max(r)):.2e}")
            if not label.startswith("warm"):
                res.setdefault(label, []).append(dt)
    if comm.rank == 0:
        off, on = statistics.median(res["off"]), statistics.median(res["on"])
        lines.append(f"  median of 3 solves each, alternated: off {off:.3f} s (min {min(res['off']):.3f} max {max(res['off']):.3f}), on "
                     f"{on:.3f} s (min {min(res['on']):.3f} max {max(res['on']):.3f}) -> the whole solve is "
                     f"{'FASTER' if on < off else 'NOT faster'} with mixed precision ({off / on:.3f}x)")
    s.close()
    dH.free()


def replay(tape, say):
    """bench.py --replay-rank 4x2 as it stands, in child processes (before this process opens the GPU)"""
    from chase_amd.replay import load_tape
    if not os.path.exists(tape):
        say(f"  tape {os.path.relpath(tape, ROOT)} not found: not run")
        return
    _, meta = load_tape(tape)
    got = {}
    for label, val in (("off", None), ("on", "1")):
        env = dict(os.environ)
        env.pop("CHASE_HIP_MIXED_PRECISION", None)
        if val:
            env["CHASE_HIP_MIXED_PRECISION"] = val
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--replay-rank", "4x2", "--tape", tape, "--workload",
                            meta["workload"]], env=env, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            say(f"  replay with the switch {label} FAILED (exit {p.returncode}): {p.stderr.strip().splitlines()[-1:]}")
            return
        rec = json.loads(p.stdout.strip().splitlines()[-1])["replays"][0]
        got[label] = rec
        say(f"  switch {label:3s}: T_rank {rec['T_rank_seconds']:.2f} s, filter (device) {rec['filter_seconds_device']:.2f} s, local block "
            f"{rec['local_shape_H']}, {rec['filtered_vecs']} vectors filtered, of these in fp32 {rec.get('filtered_vecs_in_fp32')}, call "
            f"sequence equals the recording: {rec['call_sequence_equals_recording']}, phases {rec['phases']}")
    if len(got) == 2:
        say(f"  the tape drives the switch from the environment: {'yes' if got['on'].get('filtered_vecs_in_fp32') else 'NO'}; T_rank off / on = "
            f"{got['off']['T_rank_seconds'] / got['on']['T_rank_seconds']:.3f}, filter off / on = "
            f"{got['off']['filter_seconds_device'] / got['on']['filter_seconds_device']:.3f} (one run each: no spread)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_precision_grid.txt"))
    ap.add_argument("--tape", default=os.path.join(ROOT, "profiles", "r05_cfg4_tape.npz"))
    ap.add_argument("--skip-solves", action="store_true")
    ap.add_argument("--skip-replay", action="store_true")
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    say("Mixed-precision Chebyshev filter on the process grid (scripts/dev_mixed_precision_grid.py)")
    if not args.skip_replay and not args.small:
        say("(c) single-rank replay, `bench.py --replay-rank 4x2` unchanged, CHASE_HIP_MIXED_PRECISION unset / = 1 (the replayed Resd "
            "puts the RECORDED residuals into the buffer Shift decides from, so the decision is the recorded solve's):")
        replay(args.tape, say)
        flush()
    from chase_amd.capi import Context
    ctx = Context(0)
    info = ctx.info()
    say(f"device: {info['name']}, {info['num_cu']} CUs, {info['clock_khz'] / 1000:.0f} MHz max engine clock")
    say("(a) panel product of one rank, phase 1, alpha = 0.01, beta = 0, operands ~ N(0,1); fp64 with gemm_min_rounds = 4 as the "
        "pipeline issues it; mixed = convert_d2s of the input panel + gemm_sd / gemm_cz; 2 warm-up products each, then alternating "
        "windows of back-to-back products between HIP events; ms per product = median of the windows")
    shapes = [(1024, 2048, 128, True, 3, 4), (1024, 1024, 128, False, 3, 4)] if args.small else \
        [(16384, 32768, 256, True, 7, 10), (16384, 16384, 256, False, 7, 20)]
    ratios = {}
    for (m_loc, n_loc, w, cplx, windows, reps) in shapes:
        for op, r in panel_case(ctx, m_loc, n_loc, w, cplx, windows, reps, say).items():
            ratios[(m_loc, n_loc, cplx, op)] = r
    slow = [k for k, v in ratios.items() if v <= 1.0]
    say("  mixed panel product faster than the fp64 one at every shape, type and op: " + ("yes" if not slow else f"NO - not at {slow}"))
    ctx.close()
    flush()
    if not args.skip_solves:
        from chase_amd.rank_threads import run_ranks
        say("(b) whole solves on 2 x 2 rank threads, shared-device transport, ONE GPU shared by the four ranks (defaults: tol 1e-10, "
            "deg 20, opt; device start vectors), host clock between barriers around solve + synchronise")
        N, cplx, nev, nex = (1024, True, 48, 16) if args.small else (8192, True, 256, 64)
        out = []
        run_ranks(2, 2, scenario_solves, N, cplx, nev, nex, out, transport="shared")
        for t in out:
            say(t)
    flush()


if __name__ == "__main__":
    main()
