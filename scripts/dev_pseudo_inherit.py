"""ChaseHipPseudo as a class derived from ChaseHip: this tree's library against a build of the parent commit.
Writes profiles/pseudo_inherit.txt.

The same solves run in fresh child processes, one child with CHASE_HIP_LIB pointing at the parent commit's library, the next
with this tree's, each under its own `timeout`; the first child that fails ends the script.

(a) chase::Solve_pseudo of the reference's real BSE fixture (200 x 200, nev = nex = 20), as tests/test_gpu_pseudo.py solves it
(b) chase::Solve_pseudo of the generated complex BSE matrix, N = 400, nev 16, nex 10, as tests/test_gpu_pseudo.py solves it
(c) chase::Solve of a complex Clement matrix, N = 512, nev 24, nex 8, mixed_precision off
(d) the same with mixed_precision on

Every child records the operator log of its solve, the SHA-256 of ritzv, resid() and V after the solve and stats().  Bitwise:
per scenario the logs are equal line for line, the hashes are equal, iterations and filtered vectors are equal.
Host time (all a refactor of host headers could move): (b) and (c) run in five alternating children per side; each child times
one further solve after the recorded one (its warm-up).  Bar: this tree's median is not above the parent's median by more than
the parent's own min-max spread.  Then `python bench.py` once per build, both headline lines recorded.

    python scripts/dev_pseudo_inherit.py [--parent-lib SO | --parent-rev REV] [--out FILE] [--skip-bench] [--diff-stat FILE]

Without --parent-lib the parent (REV, default HEAD~1) is exported with `git archive` into a scratch directory and built there
with `make`.  --diff-stat: a file holding `git diff --stat REV -- chase_amd/csrc include`, for a machine without the history.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCENARIOS = {"a": "Solve_pseudo, real BSE fixture 200 x 200, nev 20, nex 20",
             "b": "Solve_pseudo, generated complex BSE N = 400, nev 16, nex 10",
             "c": "Solve, complex Clement N = 512, nev 24, nex 8, mixed_precision off",
             "d": "Solve, complex Clement N = 512, nev 24, nex 8, mixed_precision on"}
TIMED = ("b", "c")
CHILD_LIMIT, BENCH_LIMIT = 180, 900          # seconds


def make_solver(ctx, which):
    import numpy as np
    from chase_amd.capi import PseudoSolver, Solver
    from oracle import chase_oracle as O
    if which == "a":
        from conftest import read_ref_matrix
        s = PseudoSolver(ctx, read_ref_matrix("double_random_BSE.bin", 200, 200, False), 20, 20)
        s.set(tol=1e-10, numlanczos=10, lanczositer=50)
    elif which == "b":
        H = np.asfortranarray(ctx.gen_bse(400, True, dmin=1.0, dmax=11.0, offdiag=1e-3, seed=7).download())
        s = PseudoSolver(ctx, H, 16, 10)
        s.set(tol=1e-10, numlanczos=10, lanczositer=50)
    else:
        s = Solver(ctx, O.clement(512, True), 24, 8)
        s.set(mixed_precision=1 if which == "d" else 0)
    return s


def child(which, out, timed):
    from chase_amd.capi import Context, LIB_PATH
    sha = lambda a: hashlib.sha256(a.tobytes(order="F")).hexdigest()
    with Context(0) as ctx:
        s = make_solver(ctx, which)
        ctx.oplog(True)
        st = s.solve()                                    # ends with End(): V is the caller's block again
        log = ctx.oplog_lines()
        ctx.oplog(False)
        rec = {"lib": LIB_PATH, "oplog": log, "ritzv": sha(s.ritzv), "resid": sha(s.resid()), "V": sha(s.V), "stats": st}
        s.close()
        if timed:
            s = make_solver(ctx, which)
            t0 = time.perf_counter()
            s.solve()
            rec["solve_s"] = time.perf_counter() - t0
            s.close()
    with open(out, "w") as f:
        json.dump(rec, f)


def run_child(which, lib, work, tag, timed):
    out = os.path.join(work, f"{which}_{tag}.json")
    env = dict(os.environ)
    env.pop("CHASE_HIP_LIB", None)
    if lib:
        env["CHASE_HIP_LIB"] = lib
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child", which, "--record", out]
    rc = subprocess.call(cmd + (["--timed"] if timed else []), env=env, cwd=ROOT)
    if rc != 0:
        sys.exit(f"child {which}/{tag} ended with status {rc}: stopping here")
    return json.load(open(out))


def run_bench(lib):
    env = dict(os.environ)
    env.pop("CHASE_HIP_LIB", None)
    if lib:
        env["CHASE_HIP_LIB"] = lib
    p = subprocess.run(["timeout", "-k", "10", str(BENCH_LIMIT), sys.executable, os.path.join(ROOT, "bench.py")], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit(f"bench.py ({'parent' if lib else 'this tree'}) ended with status {p.returncode}: stopping here")
    return [l for l in p.stdout.splitlines() if l.startswith("{")][-1]


def build_parent(rev):
    d = tempfile.mkdtemp(prefix="chase_parent_")
    subprocess.check_call(f"git -C {ROOT} archive {rev} | tar -x -C {d}", shell=True)
    subprocess.check_call(["make", "-C", d, "-j8", "chase_amd/lib/libchase_hip.so"], stdout=subprocess.DEVNULL)
    return os.path.join(d, "chase_amd", "lib", "libchase_hip.so")


def compare(which, p, n, say):
    """-> number of differences between a parent record and a record of this tree"""
    bad = 0
    a, b = p["oplog"], n["oplog"]
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)
    if first is None and len(a) != len(b):
        first = min(len(a), len(b))
    if first is not None:
        bad += 1
        say(f"  ({which}) operator logs DIFFER at line {first + 1}: parent {a[first] if first < len(a) else '<end>'!r}, "
            f"this tree {b[first] if first < len(b) else '<end>'!r}")
    for k in ("ritzv", "resid", "V"):
        if p[k] != n[k]:
            bad += 1
            say(f"  ({which}) sha256 of {k} DIFFERS: parent {p[k]}, this tree {n[k]}")
    for k in ("iterations", "filtered_vecs"):
        if p["stats"][k] != n["stats"][k]:
            bad += 1
            say(f"  ({which}) {k} DIFFERS: parent {p['stats'][k]}, this tree {n['stats'][k]}")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-rev", default="HEAD~1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pseudo_inherit.txt"))
    ap.add_argument("--skip-bench", action="store_true")
    ap.add_argument("--diff-stat", default=None)
    ap.add_argument("--child", default=None, choices=sorted(SCENARIOS))
    ap.add_argument("--record", default=None)
    ap.add_argument("--timed", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.record, args.timed)

    parent = os.path.abspath(args.parent_lib) if args.parent_lib else build_parent(args.parent_rev)
    work = tempfile.mkdtemp(prefix="pseudo_inherit_")
    lines = []
    def say(x=""):
        print(x, flush=True)
        lines.append(x)
    say("ChaseHipPseudo derived from ChaseHip: the parent commit's library and this tree's in alternating fresh processes")
    say("(scripts/dev_pseudo_inherit.py).  Per scenario: operator log of the whole solve, sha256 of ritzv / resid() / V, stats().")
    if args.diff_stat:
        stat = open(args.diff_stat).read().strip()
    else:
        stat = subprocess.run(["git", "-C", ROOT, "diff", "--stat", args.parent_rev, "--", "chase_amd/csrc", "include"],
                              stdout=subprocess.PIPE, text=True).stdout.strip()
    say("git diff --stat <parent> -- chase_amd/csrc include: " + (stat if stat else "empty - no kernel and no C ABI file changed, the "
        "code objects of all kernels (the filter's among them) are built from the parent's sources"))
    say()
    bad, times = 0, {}
    for which in sorted(SCENARIOS):
        reps = 5 if which in TIMED else 1
        recs = {"parent": [], "new": []}
        for i in range(reps):                                 # parent, new, parent, new, ...
            recs["parent"].append(run_child(which, parent, work, f"parent{i}", which in TIMED))
            recs["new"].append(run_child(which, None, work, f"new{i}", which in TIMED))
        diffs = sum(compare(which, p, n, say) for p, n in zip(recs["parent"], recs["new"]))
        bad += diffs
        p0 = recs["parent"][0]
        say(f"({which}) {SCENARIOS[which]}: {len(p0['oplog'])} log lines, {p0['stats']['iterations']} iterations, "
            f"{p0['stats']['filtered_vecs']} filtered vectors, V sha256 {p0['V'][:16]}...; {reps} pair(s) of children: "
            + ("logs, hashes, iterations and filtered vectors IDENTICAL" if diffs == 0 else f"{diffs} DIFFERENCES"))
        if which in TIMED:
            times[which] = {k: [r["solve_s"] * 1e3 for r in v] for k, v in recs.items()}
    say()
    say("Host wall time of one solve (ms; second solve of each child, five alternating children per side):")
    for which, t in times.items():
        pm, nm = statistics.median(t["parent"]), statistics.median(t["new"])
        spread = max(t["parent"]) - min(t["parent"])
        ok = nm <= pm + spread
        bad += not ok
        say(f"  ({which}) parent median {pm:8.2f} (min {min(t['parent']):.2f}, max {max(t['parent']):.2f}, spread {spread:.2f})   "
            f"this tree median {nm:8.2f} (min {min(t['new']):.2f}, max {max(t['new']):.2f})   "
            f"allowed {pm + spread:.2f}: {'within the bar' if ok else 'SLOWER than the bar'}")
    if not args.skip_bench:
        say()
        say("python bench.py (default workload), once per build:")
        say("  parent:    " + run_bench(parent))
        say("  this tree: " + run_bench(None))
    say()
    say("verdict: " + ("all criteria met" if bad == 0 else f"{bad} criteria MISSED"))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
