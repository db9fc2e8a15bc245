#!/bin/bash
# Counter passes over ONE full-width packed bf16x3 filter product (N = 16384, n = 640; scripts/dev_sp_prepack.py --one real|complex):
# one counter group per rocprofv3 run, counters only (no trace domain), every run under a time limit of its own, and the first
# run that fails ends the script.  usage: scripts/dev_sp_prepack_pmc.sh <out.txt>   (appends to out.txt)
set -u
OUT=$(realpath -m "$1")
REPO=$(cd "$(dirname "$0")/.." && pwd)
TMP=$(mktemp -d)
GROUPS_=(
 "SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_LDS_BANK_CONFLICT SQ_INSTS_MFMA"
 "SQ_WAIT_INST_LDS SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VALU"
)
echo "(d) rocprofv3 --pmc <group>, one group per run, no tracing, over one full-width packed product (N = 16384, n = 640, phase 1)" >> "$OUT"
for kind in real complex; do
  i=0
  for g in "${GROUPS_[@]}"; do
    d=$TMP/${kind}_$i
    timeout -k 10 240 rocprofv3 --pmc $g -f csv -d "$d" -- python3 "$REPO/scripts/dev_sp_prepack.py" --one $kind \
      > "$TMP/${kind}_$i.log" 2>&1 || { echo "rocprofv3 failed on '$g' ($kind)"; tail -20 "$TMP/${kind}_$i.log"; exit 1; }
    f=$(find "$d" -name "*counter_collection.csv" | head -1)
    python3 - "$f" "$kind" >> "$OUT" <<'PY' || exit 1
import csv, sys, collections
acc = collections.defaultdict(list)
for r in csv.DictReader(open(sys.argv[1])):
    if "gemm_bf16x3p_kernel" in r["Kernel_Name"]:
        acc[(r["Kernel_Name"][:70], r["Counter_Name"])].append(float(r["Counter_Value"]))
for (k, c), v in sorted(acc.items()):
    print(f"  {sys.argv[2]:7s} {c:28s} launches={len(v):2d} mean={sum(v) / len(v):.6g}  kernel={k}")
PY
    i=$((i+1))
  done
done
rm -rf "$TMP"
