"""Two builds of the library on the single-precision products: writes profiles/sp_gemm_frame.txt from four outputs of

    [CHASE_HIP_LIB=<parent build>] python scripts/dev_sp_product.py --skip-solves --out FILE

run in one job in the order parent, new, parent, new.  Per shape and product kind (fp32 MFMA, bf16x3) the medians of the four
runs side by side and a verdict: each of the two new medians may exceed the slower parent median by at most the gap between the
two parent medians - the noise the job itself measured at that line.

    python scripts/dev_sp_frame_compare.py PARENT1 NEW1 PARENT2 NEW2 [--out FILE]"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def medians(path):
    """{(line head, kind): ms} of the product lines of one output, and its device line"""
    out, device = {}, ""
    for line in open(path):
        if line.startswith("device:"):
            device = line.strip()
        m = re.match(r"\s+((?:N=|H_loc).*?)\s+fp64\s", line)
        if m:
            for kind in ("fp32", "bf16x3"):
                out[(m.group(1), kind)] = float(re.search(r"\s%s\s+([\d.]+) ms" % kind, line).group(1))
    return out, device


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "sp_gemm_frame.txt")
    if "--out" in sys.argv:
        args.remove(out)
    (p1, dev), (n1, _), (p2, _), (n2, _) = [medians(a) for a in args]
    assert p1 and p1.keys() == n1.keys() == p2.keys() == n2.keys()
    lines = ["Single-precision products before and after the shared frame (gemm_sp_frame.h): scripts/dev_sp_product.py --skip-solves run four",
             "times in one job - parent commit's library, this one, parent, this one - and compared by scripts/dev_sp_frame_compare.py.",
             dev,
             "ms per product (median of five alternating windows, see profiles/sp_bf16x3.txt for the method).  Allowed for each new run: the",
             "slower parent run plus the gap between the two parent runs at that line (the noise this job measured itself).", "",
             f"{'shape':78s} {'kind':7s} {'parent 1':>9s} {'new 1':>9s} {'parent 2':>9s} {'new 2':>9s} {'allowed':>9s}  verdict"]
    bad = 0
    for key in p1:
        a, b = p1[key], p2[key]
        allowed = max(a, b) + abs(a - b)
        ok = n1[key] <= allowed and n2[key] <= allowed
        bad += not ok
        lines.append(f"{key[0]:78s} {key[1]:7s} {a:9.3f} {n1[key]:9.3f} {b:9.3f} {n2[key]:9.3f} {allowed:9.3f}  "
                     f"{'within the parent gap' if ok else 'SLOWER'}")
    lines += ["", f"{len(p1)} lines, {bad} slower than the parent beyond its own gap"]
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
