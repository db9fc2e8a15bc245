"""Sequences of generalized problems and itype 2 / 3 (chase_hip_trmm_left_upper, chase_hip_hegst_product_upper,
chase_hip_gev_reduce_itype / _starttransform / _backtransform_itype) measured at N = 16384.  Writes profiles/gev_seq.txt; method
of scripts/dev_gev.py, whose Bench is used: one process, five alternated windows after one warm-up of each kind, the window
spread as the margin, host clock around a synchronised call.

(a) the full-width product chase_hip_gemm_d / _z (N x 640 x N, op N) as the yardstick, as in profiles/gev.txt;
(b) chase_hip_trmm_left_upper at 640 columns, op N and C, against the only way to form op(U) X without it: chase_hip_gemm on a
    zero-completed copy of U (twice the flops, out of place);
(c) chase_hip_hegst_product_upper against two full products with the zero-completed U and its explicit conjugate transpose,
    W = A U^H, C = U W (no mirroring, no exactly Hermitian result: only the flops);
(d) a three-step sequence at config 2's shape (N = 16384 complex, 512 + 128 columns, tol 1e-10), every pencil a perturbation
    of the one before by 1e-3 (H: of ||H||_2, S: of a lower bound of lambda_min(S); norms by power iteration), warm (mode 'A'
    through the start transform) against cold, S changed in every step against S unchanged (factor = 0: no Cholesky).

H_k = (Clement + p G_k) / N, S_k = 2 I + (Clement + q G'_k) / (2 N) with G Hermitian N(0,1) matrices, generated on the device;
p and q are calibrated so that the measured ||H_k - H_{k-1}||_2 and ||S_k - S_{k-1}||_2 are what (d) says.

    python scripts/dev_gev_seq.py [--out FILE] [--cases real,complex,sequence] [--small] [--windows W]
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
from dev_gev import Bench, spread  # noqa: E402


def product_case(ctx, N, cplx, ncols, windows, say):
    from chase_amd.capi import lib, check
    b = Bench(ctx, N, cplx, say)
    c = int(cplx)
    say(f"{'complex' if cplx else 'real'} fp64, N = {N}")
    b.gemm_rate(ncols, windows)
    b.copy(b.S0, b.S)
    assert ctx.potrf_upper_blocked(N, b.S.ptr, N, cplx, 0) == 0                      # U, S's lower triangle below it
    # the zero-completed U and its conjugate transpose, made by the product itself from the identity (exact)
    Uz, Lz = ctx.empty((N, N), b.dt), ctx.empty((N, N), b.dt)
    for M, op in ((Uz, "N"), (Lz, "C")):
        check(lib.chase_hip_memset(ctx.h, M.ptr, 0, M.nbytes), "memset")
        check(lib.chase_hip_shift_diag(ctx.h, c, N, M.ptr, N, 1.0), "shift_diag")
        ctx.trmm_left_upper(op, N, N, b.S.ptr, N, M.ptr, N, cplx)
    X, X0, W = ctx.empty((N, ncols), b.dt), ctx.empty((N, ncols), b.dt), ctx.empty((N, ncols), b.dt)
    check(lib.chase_hip_fill_normal(ctx.h, c, N, ncols, X0.ptr, N, 0, 0, N, 13), "fill_normal")
    prepX = lambda: check(lib.chase_hip_lacpy(ctx.h, c, N, ncols, X0.ptr, N, X.ptr, N), "lacpy")
    for op in "NC":
        med = b.compare(f"(b) op {op}", {
            f"trmm_left_upper {ncols} columns": (prepX, lambda op=op: ctx.trmm_left_upper(op, N, ncols, b.S.ptr, N, X.ptr, N, cplx)),
            "gemm on the zero-completed U": (prepX, lambda op=op: ctx.gemm(op, N, ncols, N, 1.0, Uz.ptr, N, X.ptr, N, 0.0, W.ptr, N, cplx)),
        }, windows)
        k = list(med)
        say(f"      op {op}: full product / triangular product = {med[k[1]] / med[k[0]]:.2f}")
        # where the time goes: the same routine on the leading 64 x 64 (one trmm_diag launch) and 256 x 256 (one block without its
        # long product: 4 trmm_diag + 3 rectangles) corners, 64 calls per window; the long products are the rest
        part = {}
        for nn in (64, 256):
            run = lambda nn=nn, op=op: [ctx.trmm_left_upper(op, nn, ncols, b.S.ptr, N, X.ptr, N, cplx) for _ in range(64)]
            ts = [b.timed(prepX, run)[0] for _ in range(windows + 1)][1:]
            part[nn] = statistics.median(ts) / 64
        nblk, ndiag = (N + 255) // 256, (N + 63) // 64
        say(f"      op {op}: one trmm_diag launch {part[64] * 1e6:.1f} us, one 256-row block without its long product {part[256] * 1e6:.1f} us "
            f"(back to back, no long product between them): {ndiag} launches = {ndiag * part[64] * 1e3:.1f} ms, {nblk} blocks = "
            f"{nblk * part[256] * 1e3:.1f} ms of the {med[k[0]] * 1e3:.1f} ms; the {nblk - 1} long products (256 rows x {ncols} columns each) take the rest")
    for a in (X, X0, W):
        a.free()
    # (c) A <- U A U^H
    W = ctx.empty((N, N), b.dt)
    prepA = lambda: b.copy(b.H0, b.A)

    def two_gemms():
        ctx.gemm("N", N, N, N, 1.0, b.A.ptr, N, Lz.ptr, N, 0.0, W.ptr, N, cplx)
        ctx.gemm("N", N, N, N, 1.0, Uz.ptr, N, W.ptr, N, 0.0, b.A.ptr, N, cplx)
    med = b.compare("(c)", {"hegst_product_upper": (prepA, lambda: ctx.hegst_product_upper(N, b.A.ptr, N, b.S.ptr, N, cplx)),
                            "two gemms on zero-completed U": (prepA, two_gemms)}, windows)
    k = list(med)
    say(f"      two full products / hegst_product_upper = {med[k[1]] / med[k[0]]:.2f}")
    for a in (W, Uz, Lz, b.A, b.S, b.H0, b.S0):
        a.free()


def norm2(ctx, N, cplx, apply, iters=12):
    """|| M ||_2 of a Hermitian M given as apply(v_dev, out_dev), by power iteration from a fixed start (a lower estimate, within
    a few per cent after 12 steps for the matrices here)"""
    dt = np.complex128 if cplx else np.float64
    v = np.random.default_rng(5).standard_normal(N).astype(dt)
    dv, dw = ctx.empty((N, 1), dt), ctx.empty((N, 1), dt)
    nrm = 0.0
    for _ in range(iters):
        dv.upload((v / np.linalg.norm(v)).reshape(N, 1))
        apply(dv, dw)
        v = dw.download()[:, 0]
        nrm = float(np.linalg.norm(v))
    dv.free(); dw.free()
    return nrm


def sequence_case(ctx, N, cplx, nev, nex, windows, say, steps=3):
    from chase_amd.capi import lib, check, Solver
    c, dt, nc = int(cplx), (np.complex128 if cplx else np.float64), nev + nex
    say(f"(d) a sequence of {steps} pencils at config 2's shape: N = {N} {'complex' if cplx else 'real'}, nev {nev}, nex {nex}, tol 1e-10, "
        "otherwise the solver's defaults")

    def gen_h(p, seed):
        return ctx.gen_clement(N, cplx, scale=1.0 / N, perturb=p, seed=seed)

    def gen_s(q, seed):
        S = ctx.gen_clement(N, cplx, scale=0.5 / N, perturb=q, seed=seed)
        check(lib.chase_hip_shift_diag(ctx.h, c, N, S.ptr, N, 2.0), "shift_diag")
        return S

    def diff(A, B, shift=0.0):
        def apply(dv, dw):
            ctx.gemm("N", N, 1, N, 1.0, A.ptr, N, dv.ptr, N, 0.0, dw.ptr, N, cplx)
            if B is not None:
                ctx.gemm("N", N, 1, N, -1.0, B.ptr, N, dv.ptr, N, 1.0, dw.ptr, N, cplx)
            if shift:
                dw.upload(dw.download() - shift * dv.download())
        return apply

    # calibration: the difference of two pencils is linear in p (q)
    p = q = 0.05
    a, b2 = gen_h(p, 100), gen_h(p, 101)
    nH = norm2(ctx, N, cplx, diff(a, None))
    p *= 1e-3 * nH / norm2(ctx, N, cplx, diff(a, b2))
    a.free(); b2.free()
    a, b2 = gen_s(q, 200), gen_s(q, 201)
    lmin_bound = 2.0 - norm2(ctx, N, cplx, diff(a, None, shift=2.0))
    q *= 1e-3 * lmin_bound / norm2(ctx, N, cplx, diff(a, b2))
    a.free(); b2.free()
    Hs, Ss = [gen_h(p, 100 + k) for k in range(steps)], [gen_s(q, 200 + k) for k in range(steps)]
    say(f"  p = {p:.4g}, q = {q:.4g}; measured ||H_1 - H_0|| / ||H_0|| = {norm2(ctx, N, cplx, diff(Hs[1], Hs[0])) / nH:.3g}, "
        f"||S_1 - S_0|| = {norm2(ctx, N, cplx, diff(Ss[1], Ss[0])):.3g} = 1e-3 x {lmin_bound:.3f} (2 - ||S_0 - 2 I||, a lower bound of lambda_min(S_0))")

    A, S = ctx.empty((N, N), dt), ctx.empty((N, N), dt)
    X = ctx.empty((N, nc), dt)
    s = Solver(ctx, None, nev, nex, h_on_device_ptr=A.ptr, N=N, cplx=cplx)
    s.set(tol=1e-10)
    cp = lambda src, dst: check(lib.chase_hip_lacpy(ctx.h, c, N, N, src.ptr, N, dst.ptr, N), "lacpy")

    def run(warm, s_changes):
        """one sequence; per step (reduce, start transform incl. the block's way to the host, solve, back-transformation of all
        columns incl. the block's way to the device, filtered vectors)"""
        out = []
        for k in range(steps):
            cp(Hs[k], A)
            if k == 0 or s_changes:
                cp(Ss[k if s_changes else 0], S)
            ctx.sync()
            t0 = time.perf_counter()
            assert ctx.gev_reduce_itype(1, 1 if (k == 0 or s_changes) else 0, N, A.ptr, N, S.ptr, N, cplx) == 0
            ctx.sync()
            t1 = time.perf_counter()
            if warm and k > 0 and s_changes:                 # X holds the previous step's back-transformed block
                ctx.gev_starttransform(1, N, nc, S.ptr, N, X.ptr, N, cplx)
                s.V[...] = X.download()
            s.set(approx=1 if (warm and k > 0) else 0)
            ctx.sync()
            t2 = time.perf_counter()
            st = s.solve()
            ctx.sync()
            t3 = time.perf_counter()
            X.upload(s.V)
            ctx.gev_backtransform_itype(1, N, nc, S.ptr, N, X.ptr, N, cplx)
            ctx.sync()
            t4 = time.perf_counter()
            assert st["locked"] >= nev
            out.append((t1 - t0, t2 - t1, t3 - t2, t4 - t3, st["filtered_vecs"]))
        return out

    kinds = {"S changes, warm": (True, True), "S changes, cold": (False, True), "S unchanged, warm": (True, False),
             "S unchanged, cold": (False, False)}
    res = {k: [] for k in kinds}
    for w in range(windows + 1):
        for k, (warm, sc) in kinds.items():
            r = run(warm, sc)
            if w:
                res[k].append(r)
    tot = {}
    for k in kinds:
        for j in range(steps):
            col = lambda i: [r[j][i] for r in res[k]]
            m = [statistics.median(col(i)) for i in range(4)]
            say(f"  {k:18s} step {j}: reduce {m[0]:.3f} s, start transform {m[1]:.3f} s, solve {m[2]:.3f} s (spread {100 * spread(col(2)):.1f} %), "
                f"back-transformation of {nc} columns {m[3]:.3f} s, {res[k][0][j][4]} filtered vectors")
        whole = [sum(sum(r[j][:4]) for j in range(1, steps)) for r in res[k]]
        tot[k] = statistics.median(whole)
        say(f"  {k:18s} steps 1 .. {steps - 1} together: {tot[k]:.3f} s (min {min(whole):.3f} max {max(whole):.3f}, {windows} windows, spread "
            f"{100 * spread(whole):.1f} %)")
    say(f"  cold / warm over steps 1 .. {steps - 1}: S changes {tot['S changes, cold'] / tot['S changes, warm']:.2f}, "
        f"S unchanged {tot['S unchanged, cold'] / tot['S unchanged, warm']:.2f}; "
        f"S changes / S unchanged, warm: {tot['S changes, warm'] / tot['S unchanged, warm']:.2f}")
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gev_seq.txt"))
    ap.add_argument("--cases", default="real,complex,sequence")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    ap.add_argument("--windows", type=int, default=5)
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
    say("sequences of generalized problems and itype 2 / 3: the triangular product and what is built on it (scripts/dev_gev_seq.py)")
    say(f"device: {info['name']}, {info['num_cu']} CUs, {info['clock_khz'] / 1000:.0f} MHz max engine clock; {args.windows} alternated windows "
        "after one warm-up of each kind; 'x' = time over the time of the executed flops at the rate of (a)")
    for name, cplx in (("real", False), ("complex", True)):
        if name in cases:
            product_case(ctx, N, cplx, 64 if args.small else 640, args.windows, say)
    if "sequence" in cases:
        sequence_case(ctx, N, True, *((64, 16) if args.small else (512, 128)), args.windows, say)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
