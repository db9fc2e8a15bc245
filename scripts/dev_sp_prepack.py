"""The bf16x3 filter product on a packed H (sp_prepack = 1) against the unpacked bf16x3 product and the fp32 MFMA.
Writes profiles/sp_prepack.txt; method and shapes of scripts/dev_sp_product.py (profiles/sp_bf16x3.txt).

(a) the narrow filter product, phase 1 like the filter launches it: fp32 MFMA (chase_hip_gemm_s / _c), bf16x3 (chase_hip_gemm_s_bf16x3
    / _c_bf16x3: the kernel of the parent commit, same build, same process) and bf16x3 on the packed H (chase_hip_gemm_s_bf16x3p /
    _c_bf16x3p) at N = 16384, n = 640 and N = 32768, n = 2560, real and complex, and at N = 16384, n = 256 real (one tile per CU, the
    panel shape at which bf16x3 loses to fp32).  The three are timed alternately in one process: HIP events around a window of
    back-to-back products, at least a second of work per kind, five windows, median and spread reported.  The packed result is
    compared with the unpacked one bit for bit.
(b) the one-off pack of H from fp64 (chase_hip_bf16x3_pack), its diagonal refresh (chase_hip_bf16x3_pack_diag), and what they
    replace: chase_hip_convert_d2s of H and chase_hip_diag_d2s.
(c) whole solves of bench.py's cfg2 (N = 16384 complex, nev 512, nex 128) and cfg3 (N = 32768 real, nev 1024, nex 256) with
    mixed_precision = 1 and the three settings fp32 MFMA, bf16x3, bf16x3 + sp_prepack, alternated.

    python scripts/dev_sp_prepack.py [--out FILE] [--skip-solves] [--small] [--one real|complex]

--one launches a single full-width packed product (N = 16384, n = 640) and nothing else: the launch a counter pass profiles
(scripts/dev_sp_prepack_pmc.sh).
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
from dev_sp_product import CEILING, MATRIX_PERTURB, MATRIX_SCALE, PEAK_F32, timed  # noqa: E402


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def product_case(ctx, N, n, cplx, min_ms, windows, say):
    from chase_amd.capi import lib, check
    dt = np.complex128 if cplx else np.float64
    H = ctx.gen_clement(N, cplx, scale=MATRIX_SCALE / N, perturb=MATRIX_PERTURB, seed=42)
    V = ctx.empty((N, n), dt)
    check(lib.chase_hip_fill_normal(ctx.h, int(cplx), N, n, V.ptr, N, 0, 0, N, 1337), "fill_normal")
    Hs, Vs = ctx.to_single(H), ctx.to_single(V)
    V.free()
    Hp = ctx.empty((ctx.bf16x3_pack_bytes(N, N, cplx),), np.uint8)
    Ws, W3, Wp = (ctx.empty((N, n), Hs.dtype) for _ in range(3))
    alpha, beta = 0.01, 0.0
    # (b) the pack and its refresh against the conversions of the fp32 shadow
    prep = {"pack": lambda: ctx.bf16x3_pack(N, N, H.ptr, N, Hp.ptr, cplx, src_f64=True),
            "pack_diag": lambda: ctx.bf16x3_pack_diag(N, H.ptr, N, Hp.ptr, cplx),
            "convert_d2s": lambda: ctx.convert_d2s(N, N, H.ptr, N, Hs.ptr, N, cplx),
            "diag_d2s": lambda: ctx.diag_d2s(N, H.ptr, N, Hs.ptr, N, cplx)}
    tp, rp = timed(ctx, prep, min_ms / 5, windows)
    H.free()
    kinds = {"fp32": lambda: ctx.gemm32("N", N, n, N, alpha, Hs.ptr, N, Vs.ptr, N, beta, Ws.ptr, N, cplx),
             "bf16x3": lambda: ctx.gemm32("N", N, n, N, alpha, Hs.ptr, N, Vs.ptr, N, beta, W3.ptr, N, cplx, split=True),
             "packed": lambda: ctx.gemm32p(N, n, N, alpha, Hp.ptr, Vs.ptr, N, beta, Wp.ptr, N, cplx)}
    check(lib.chase_hip_ctx_set_phase(ctx.h, 1), "set_phase")
    t, reps = timed(ctx, kinds, min_ms, windows)
    check(lib.chase_hip_ctx_set_phase(ctx.h, 0), "set_phase")
    same = W3.download().tobytes() == Wp.download().tobytes()
    flops = 2.0 * (4 if cplx else 1) * N * N * n
    med = {k: statistics.median(v) for k, v in t.items()}
    head = f"N={N:6d} n={n:5d} {'complex' if cplx else 'real   '}"
    say(f"  {head}  " + "   ".join(f"{k} {med[k]:9.3f} ms ({flops / med[k] * 1e-9:6.1f} TF/s, min {min(t[k]):.3f} max {max(t[k]):.3f}, "
                                  f"spread {100 * spread(t[k]):.2f} %, {len(t[k])} x {reps[k]})" for k in t))
    margin = max(spread(t["bf16x3"]), spread(t["packed"]))
    r = med["bf16x3"] / med["packed"]
    verdict = "faster" if r > 1 + margin else ("slower" if r < 1 - margin else "within the spread")
    say(f"  {' ' * len(head)}  bf16x3 / packed = {r:.3f} ({verdict}; window spread {100 * margin:.2f} %), fp32 / bf16x3 = {med['fp32'] / med['bf16x3']:.3f}, "
        f"fp32 / packed = {med['fp32'] / med['packed']:.3f} (ceiling {CEILING:.2f}), packed at {flops / med['packed'] * 1e-9 / (PEAK_F32 * CEILING):.2f} of "
        f"{PEAK_F32 * CEILING:.0f} TF/s; packed == bf16x3 bit for bit: {'yes' if same else 'NO'}")
    mp = {k: statistics.median(v) for k, v in tp.items()}
    say(f"  {' ' * len(head)}  H from fp64: pack {mp['pack']:.3f} ms ({Hp.nbytes / 2 ** 30:.2f} GiB written; = {mp['pack'] / med['packed']:.2f} packed products), "
        f"pack_diag {mp['pack_diag'] * 1e3:.1f} us; convert_d2s {mp['convert_d2s']:.3f} ms ({Hs.nbytes / 2 ** 30:.2f} GiB), diag_d2s "
        f"{mp['diag_d2s'] * 1e3:.1f} us")
    for d in (Hs, Vs, Hp, Ws, W3, Wp):
        d.free()
    return r, margin, same


def solve_case(ctx, name, N, cplx, nev, nex, say):
    from chase_amd.capi import Solver
    dH = ctx.gen_clement(N, cplx, scale=MATRIX_SCALE / N, perturb=MATRIX_PERTURB, seed=42)
    ctx.sync()
    s = Solver(ctx, None, nev, nex, h_on_device_ptr=dH.ptr, N=N, cplx=cplx)
    s.set(device_rng=1, mixed_precision=1)
    modes = {"fp32": (0, 0), "bf16x3": (1, 0), "packed": (1, 1)}
    res, ritz = {}, {}
    for label in ("warm-up", "fp32", "bf16x3", "packed", "fp32", "bf16x3", "packed", "fp32", "bf16x3", "packed"):
        sp, pp = modes.get(label, (1, 1))                      # (the warm-up also makes every allocation of the packed path)
        s.set(sp_product=sp, sp_prepack=pp, reset_counters=1)
        ctx.sync()
        t0 = time.perf_counter()
        st = s.solve()
        ctx.sync()
        dt = time.perf_counter() - t0
        r = s.recompute_residuals(nev)
        if label != "warm-up":
            res.setdefault(label, []).append(dt)
            ritz[label] = s.ritzv.tobytes()
        say(f"  {name} {label:8s} {dt:8.3f} s  filter {s.get('filter_ms') * 1e-3:7.3f} s  iterations {st['iterations']:2d}  filtered vectors "
            f"{st['filtered_vecs']:7d}  in fp32 {int(s.get('hemm_sp_vecs')):7d} ({int(s.get('sp_filters'))} filter calls, "
            f"{int(s.get('hemm_sp_split_calls'))} of {int(s.get('hemm_sp_calls'))} products split, {int(s.get('hemm_sp_packed_calls'))} packed; "
            f"{int(s.get('sp_pack_full'))} packs, {int(s.get('sp_pack_diag'))} diagonal refreshes)  locked {st['locked']}  "
            f"max fresh fp64 residual {float(np.max(r)):.2e}")
    med = {k: statistics.median(v) for k, v in res.items()}
    sp = max(spread(v) for v in res.values())
    say(f"  {name}: median of 3 solves each, alternated: fp32 {med['fp32']:.3f} s, bf16x3 {med['bf16x3']:.3f} s ({med['fp32'] / med['bf16x3']:.3f}x of "
        f"fp32), bf16x3 + prepack {med['packed']:.3f} s ({med['fp32'] / med['packed']:.3f}x of fp32, {med['bf16x3'] / med['packed']:.3f}x of bf16x3); "
        f"largest spread of a setting {100 * sp:.2f} %; Ritz values of bf16x3 and bf16x3 + prepack identical: "
        f"{'yes' if ritz['bf16x3'] == ritz['packed'] else 'NO'}")
    s.close()
    dH.free()


def one_launch(ctx, cplx):
    from chase_amd.capi import lib, check
    N, n = 16384, 640
    dt = np.complex64 if cplx else np.float32
    Hs, Vs, Ws = ctx.empty((N, N), dt), ctx.empty((N, n), dt), ctx.empty((N, n), dt)
    Hp = ctx.empty((ctx.bf16x3_pack_bytes(N, N, cplx),), np.uint8)
    check(lib.chase_hip_memset(ctx.h, Hs.ptr, 0x3c, Hs.nbytes), "memset")      # finite values, no denormals: 0x3c3c3c3c = 0.0115
    check(lib.chase_hip_memset(ctx.h, Vs.ptr, 0x3c, Vs.nbytes), "memset")
    ctx.bf16x3_pack(N, N, Hs.ptr, N, Hp.ptr, cplx)
    check(lib.chase_hip_ctx_set_phase(ctx.h, 1), "set_phase")
    ctx.gemm32p(N, n, N, 0.01, Hp.ptr, Vs.ptr, N, 0.0, Ws.ptr, N, cplx)
    ctx.sync()
    check(lib.chase_hip_ctx_set_phase(ctx.h, 0), "set_phase")
    for d in (Hs, Vs, Ws, Hp):
        d.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sp_prepack.txt"))
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
    say("bf16x3 filter product on a packed H (sp_prepack = 1) against the unpacked bf16x3 product and the fp32 MFMA (scripts/dev_sp_prepack.py)")
    say(f"device: {info['name']}, {info['num_cu']} CUs, {info['clock_khz'] / 1000:.0f} MHz max engine clock; fp32 MFMA peak {PEAK_F32} TF/s, "
        f"bf16x3 compute ceiling 16/6 of it = {PEAK_F32 * CEILING:.0f} TF/s fp32-equivalent")
    say("(a) narrow filter product C = alpha H V, phase 1, alpha = 0.01, beta = 0; H = the bench's Clement matrix, V ~ N(0,1); 2 warm-up "
        f"products each, then {windows} alternating windows of back-to-back products between HIP events, at least {min_ms / 1000:.2f} s of "
        "work per kind; ms per product = median of the windows; spread = (max - min) / median of a kind's windows; bf16x3 is the kernel of "
        "the parent commit in the same process.  (b) on the line below each shape: the one-off pack of H and its diagonal refresh "
        "against the conversions of the fp32 shadow they replace (a fifth of the work per kind)")
    shapes = [(1024, 96), (2048, 160), (1024, 64)] if args.small else [(16384, 640), (32768, 2560), (16384, 256)]
    out = {}
    for (N, n) in shapes:
        for cplx in ((False,) if (N, n) == shapes[2] else (False, True)):
            out[(N, n, cplx)] = product_case(ctx, N, n, cplx, min_ms, windows, say)
    say("  packed faster than unpacked bf16x3 by more than the window spread: " +
        ", ".join(f"{N} x {n} {'complex' if c else 'real'}: {'yes' if r > 1 + m else 'no'} ({r:.3f})" for (N, n, c), (r, m, _) in out.items()))
    say("  packed == bf16x3 bit for bit at every shape: " + ("yes" if all(s for (_, _, s) in out.values()) else "NO"))
    if not args.skip_solves:
        say("(c) whole solves (defaults: tol 1e-10, deg 20, opt; device start vectors; mixed_precision = 1), host clock around solve + "
            "synchronise; one warm-up solve, then fp32 (sp_product = 0), bf16x3 (sp_product = 1), packed (sp_product = 1, sp_prepack = 1), "
            "three rounds")
        cases = [("toy", 2048, True, 64, 32)] if args.small else [("cfg2", 16384, True, 512, 128), ("cfg3", 32768, False, 1024, 256)]
        for case in cases:
            solve_case(ctx, *case, say)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
