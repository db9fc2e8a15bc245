"""K split of the wide single-precision products under gemm_min_rounds: what it buys the panel product of a grid rank.  Writes
profiles/sp_ksplit.txt.

(a)-(c) the panel product of one rank as the pipelined HEMM issues it while a filter call runs in single precision: phase 1,
    gemm_min_rounds = 4, chase_hip_convert_d2s of the input panel + chase_hip_gemm_sd / _cz (fp32 MFMA) or their _bf16x3 twins, op N
    and op C.  TWO builds of the library in ONE process: the parent commit's (its path in CHASE_HIP_LIB; it ignores
    gemm_min_rounds in these products) and this tree's, on the same device buffers, in alternating windows of back-to-back
    products of about a second between HIP events; ms per product = median of the windows, and the spread of the windows.
      (a) 4096 x 4096 complex, 128 columns   - a rank of N = 8192 on 2 x 2: 64 tiles for 512 workgroup slots
      (b) 16384 x 16384 real, 256 columns    - a rank of config 3 on 2 x 2: one tile per CU
      (c) 16384 x 32768 complex, 256 columns - a rank of N = 65536 on 4 x 2
    The two builds' results are compared on the same inputs (they differ by the order of summation only).
(d) whole solves on 2 x 2 rank threads sharing ONE GPU, N = 8192 complex, nev 256, this tree's library, mixed_precision off and
    on, three solves each, alternated.

    CHASE_HIP_LIB=<parent build>/libchase_hip.so python scripts/dev_sp_ksplit.py [--out FILE] [--skip-solves] [--small]
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# The parent's library is loaded FIRST, privately and bound to itself (RTLD_DEEPBIND): both builds export the same names, and
# neither may resolve its internal calls into the other.  chase_amd.capi then loads this tree's library as usual.
PARENT_PATH = os.environ.pop("CHASE_HIP_LIB", None)
try:                                    # (as chase_amd.capi does: one HIP runtime in the process, the one torch brings)
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is plumbing only
    pass
PARENT = ctypes.CDLL(PARENT_PATH, mode=os.RTLD_LOCAL | os.RTLD_NOW | os.RTLD_DEEPBIND) if PARENT_PATH else None

from chase_amd import capi  # noqa: E402
from chase_amd.capi import check, lib  # noqa: E402

USED = ("chase_hip_ctx_create", "chase_hip_ctx_destroy", "chase_hip_ctx_sync", "chase_hip_ctx_set_phase",
        "chase_hip_ctx_set_gemm_min_rounds", "chase_hip_convert_d2s", "chase_hip_timer_start", "chase_hip_timer_stop",
        "chase_hip_gemm_sd", "chase_hip_gemm_cz", "chase_hip_gemm_sd_bf16x3", "chase_hip_gemm_cz_bf16x3", "chase_hip_last_error")


class Side:
    """one build of the library with a context of its own on device 0"""

    def __init__(self, name, dll):
        self.name, self.lib = name, dll
        if dll is not lib:
            for n in USED:
                f, g = getattr(dll, n), getattr(lib, n)
                f.argtypes, f.restype = g.argtypes, g.restype
        self.h = ctypes.c_void_p()
        self.ok(dll.chase_hip_ctx_create(ctypes.byref(self.h), 0, None), "ctx_create")
        self.ok(dll.chase_hip_ctx_set_phase(self.h, 1), "set_phase")

    def ok(self, rc, where):
        if rc != 0:
            raise RuntimeError(f"{self.name}: {where} failed with status {rc}: {self.lib.chase_hip_last_error().decode()}")

    def product(self, split, cplx, op, m, n, k, alpha, Hs, ldh, X, ldx, Xs, Y, ldy):
        """what Ops::product of the grid filter issues for one panel: convert the input panel, multiply"""
        L = self.lib
        self.ok(L.chase_hip_ctx_set_gemm_min_rounds(self.h, 4), "min_rounds")
        self.ok(L.chase_hip_convert_d2s(self.h, int(cplx), k, n, X, ldx, Xs, ldx), "convert_d2s")
        if cplx:
            f = L.chase_hip_gemm_cz_bf16x3 if split else L.chase_hip_gemm_cz
            self.ok(f(self.h, op.encode(), m, n, k, capi._z2(alpha), Hs, ldh, Xs, ldx, capi._z2(0.0), Y, ldy), "gemm_cz")
        else:
            f = L.chase_hip_gemm_sd_bf16x3 if split else L.chase_hip_gemm_sd
            self.ok(f(self.h, op.encode(), m, n, k, float(alpha), Hs, ldh, Xs, ldx, 0.0, Y, ldy), "gemm_sd")
        self.ok(L.chase_hip_ctx_set_gemm_min_rounds(self.h, 0), "min_rounds")

    def time(self, fn, reps):
        self.ok(self.lib.chase_hip_timer_start(self.h), "timer_start")
        for _ in range(reps):
            fn()
        ms = ctypes.c_float()
        self.ok(self.lib.chase_hip_timer_stop(self.h, ctypes.byref(ms)), "timer_stop")
        return ms.value / reps

    def sync(self):
        self.ok(self.lib.chase_hip_ctx_sync(self.h), "ctx_sync")

    def close(self):
        self.lib.chase_hip_ctx_destroy(self.h)


def panel_case(label, ctx, sides, m_loc, n_loc, w, cplx, windows, window_ms, say):
    """-> {(kind, op): (parent ms, new ms, spread)}"""
    dt = np.complex128 if cplx else np.float64
    H = ctx.empty((m_loc, n_loc), dt)
    check(lib.chase_hip_fill_normal(ctx.h, int(cplx), m_loc, n_loc, H.ptr, m_loc, 0, 0, m_loc, 42), "fill_normal")
    Hs = ctx.to_single(H)
    H.free()
    ctx.sync()
    num_cu = ctx.info()["num_cu"]
    out = {}
    for op in ("N", "C"):
        rows_out, rows_in = (m_loc, n_loc) if op == "N" else (n_loc, m_loc)
        X = ctx.empty((rows_in, w), dt)
        check(lib.chase_hip_fill_normal(ctx.h, int(cplx), rows_in, w, X.ptr, rows_in, 0, 0, rows_in, 1337), "fill_normal")
        Xs = ctx.empty((rows_in, w), Hs.dtype)
        Ys = {s.name: ctx.empty((rows_out, w), dt) for s in sides}
        ctx.sync()
        for split in (False, True):
            kind = "bf16x3" if split else "fp32"
            p = capi.gemm_sp_plan(cplx, op, rows_out, w, rows_in, split=split, num_cu=num_cu, min_rounds=4)
            fns = {s.name: (lambda s=s: s.product(split, cplx, op, rows_out, w, rows_in, 0.01, Hs.ptr, m_loc, X.ptr, rows_in, Xs.ptr,
                                                  Ys[s.name].ptr, rows_out)) for s in sides}
            est = {}
            for s in sides:                              # warm-up: code objects, workspace, clocks - and the size of a window
                fns[s.name](); s.sync()
                est[s.name] = s.time(fns[s.name], 3)
            cols = {s.name: Ys[s.name].download()[:, :2] for s in sides}
            ref = cols[sides[0].name]
            worst = max(float(np.max(np.abs(c - ref)) / np.max(np.abs(ref))) for c in cols.values())
            t = {s.name: [] for s in sides}
            for _ in range(windows):                     # alternating windows
                for s in sides:
                    t[s.name].append(s.time(fns[s.name], max(3, int(window_ms / est[s.name]))))
            flops = 2.0 * (4 if cplx else 1) * m_loc * n_loc * w
            med = {k: statistics.median(v) for k, v in t.items()}
            spread = max(max(v) - min(v) for v in t.values())
            txt = "   ".join(f"{k} {med[k]:8.4f} ms ({flops / med[k] * 1e-9:6.1f} TF/s, min {min(t[k]):.4f} max {max(t[k]):.4f})" for k in t)
            line = (f"  ({label}) H_loc {m_loc} x {n_loc} {'complex' if cplx else 'real   '} {w} columns op {op} {kind:6s} "
                    f"{p['gm'] * p['gn']} tiles of 128 x {p['bn']} in {p['sk']} K pieces of {p['kchunk']}, slabs "
                    f"{p['slab_bytes'] / 2 ** 20:.0f} MB: {txt}")
            if len(sides) == 2:
                a, b = med[sides[0].name], med[sides[1].name]
                verdict = "FASTER" if a - b > spread else ("SLOWER" if b - a > spread else "within the spread")
                line += (f"   parent / new = {a / b:.3f}, largest window spread {spread:.4f} ms: {verdict}   "
                         f"max |new - parent| / max |parent| on two columns = {worst:.1e}")
                out[(kind, op)] = (a, b, spread)
            say(line)
        for d in [X, Xs] + list(Ys.values()):
            d.free()
    Hs.free()
    return out


def scenario_solves(ctx, grid, comm, N, cplx, nev, nex, lines):
    import time
    from chase_amd import dist as cd
    rl, cl = cd.Layout(N, 0, grid.nprow), cd.Layout(N, 0, grid.npcol)
    dH = cd.gen_clement_local(ctx, N, cplx, rl, cl, grid.myrow, grid.mycol, scale=100.0 / N, perturb=1e-6)       # bench.py's matrix
    s = cd.DistSolver(ctx, grid, dH, N, nev, nex, cplx, 0, 0)
    s.set(device_rng=1)
    res = {}
    for label, on in (("warm-up (off)", 0), ("warm-up (on)", 1), ("off", 0), ("on", 1), ("off", 0), ("on", 1), ("off", 0), ("on", 1)):
        s.set(mixed_precision=on, reset_counters=1)
        ctx.gemm_sp_counters(reset=True)
        ctx.sync(); comm.barrier()
        t0 = time.perf_counter()
        st = s.solve()
        ctx.sync(); comm.barrier()
        dt = time.perf_counter() - t0
        r = s.recompute_residuals(nev)
        wide, cut, pieces = ctx.gemm_sp_counters()
        if comm.rank == 0:
            lines.append(f"  2x2 N={N} {'complex' if cplx else 'real'} {nev}/{nex} {label:13s} {dt:8.3f} s  filter {s.get('filter_ms') * 1e-3:7.3f} s  "
                         f"iterations {st['iterations']:2d}  filtered vectors {st['filtered_vecs']:7d}  in fp32 "
                         f"{int(s.get('hemm_sp_vecs')):7d}  wide single-precision products {wide}, cut {cut} into {pieces} pieces  "
                         f"locked {st['locked']}  max fresh fp64 residual {float(np.max(r)):.2e}")
            if not label.startswith("warm"):
                res.setdefault(label, []).append(dt)
    if comm.rank == 0:
        off, on = statistics.median(res["off"]), statistics.median(res["on"])
        lines.append(f"  median of 3 solves each, alternated: off {off:.3f} s (min {min(res['off']):.3f} max {max(res['off']):.3f}), on "
                     f"{on:.3f} s (min {min(res['on']):.3f} max {max(res['on']):.3f}): off / on = {off / on:.3f}")
    s.close()
    dH.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sp_ksplit.txt"))
    ap.add_argument("--skip-solves", action="store_true")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=1000.0)
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

    say("K split of the wide single-precision products under gemm_min_rounds (scripts/dev_sp_ksplit.py)")
    ctx = capi.Context(0)
    info = ctx.info()
    say(f"device: {info['name']}, {info['num_cu']} CUs, {info['clock_khz'] / 1000:.0f} MHz max engine clock")
    sides = ([Side("parent", PARENT)] if PARENT is not None else []) + [Side("new", lib)]
    say("(a)-(c) panel product of one rank, phase 1, gemm_min_rounds = 4, alpha = 0.01, beta = 0, operands ~ N(0,1): convert_d2s of the "
        "input panel + the wide product; " + ("the parent commit's library and this one" if PARENT is not None else
                                              "this library ONLY (CHASE_HIP_LIB not set: no comparison)") +
        f" in one process on the same buffers, {args.windows} alternating windows of about {args.window_ms / 1000:.1f} s between HIP events; "
        "ms per product = median of the windows")
    shapes = [("a", 1024, 1024, 64, True), ("b", 2048, 2048, 128, False)] if args.small else \
        [("a", 4096, 4096, 128, True), ("b", 16384, 16384, 256, False), ("c", 16384, 32768, 256, True)]
    res = {}
    for (label, m_loc, n_loc, w, cplx) in shapes:
        for k, v in panel_case(label, ctx, sides, m_loc, n_loc, w, cplx, args.windows, args.window_ms, say).items():
            res[(label,) + k] = v
        flush()
    if PARENT is not None:
        a_ok = all(p - n > s for k, (p, n, s) in res.items() if k[0] == "a")
        bc_bad = [k for k, (p, n, s) in res.items() if k[0] != "a" and n - p > s]
        say(f"  (a) faster than the parent by more than the spread at every op and product: {'yes' if a_ok else 'NO'};  (b), (c) slower "
            f"than the parent by more than the spread: {bc_bad if bc_bad else 'nowhere'}")
    for s in sides:
        s.close()
    ctx.close()
    flush()
    if not args.skip_solves:
        from chase_amd.rank_threads import run_ranks
        say("(d) whole solves on 2 x 2 rank threads, shared-device transport, ONE GPU shared by the four ranks (defaults: tol 1e-10, "
            "deg 20, opt, panel_rounds 4; device start vectors), this library, host clock between barriers around solve + synchronise; "
            "counters of rank 0")
        N, cplx, nev, nex = (2048, True, 48, 16) if args.small else (8192, True, 256, 64)
        out = []
        run_ranks(2, 2, scenario_solves, N, cplx, nev, nex, out, transport="shared")
        for t in out:
            say(t)
    flush()


if __name__ == "__main__":
    main()
