"""Launch-plan cases of the GEMM tests: which products reach which launcher decisions (gemm_mfma_f64.hip launch_gemm ->
for_each_piece -> decide_part), read from chase_hip_gemm_plan.  tests/test_gemm_plan_cpu.py checks on the host that the
cases cover every class below; tests/test_gpu_gemm_plans.py runs each case on the device against exact and long-double
references.  Shapes whose class depends on the chip are derived from num_cu (the figures in the comments are those of
256 CUs)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def cases(num_cu):
    """dicts: cplx, op, m, n, k, phase, min_rounds, pad (extra rows of A, B, C: leading dimensions), coff (first column of
    the product in B and C), cls (the class the case is there for: one of plan_classes' labels)."""
    def c(name, cplx, op, m, n, k, phase, cls, min_rounds=0, pad=None, coff=1):
        pad = pad or ((2, 1, 3) if cplx else (2, 2, 3))           # real: even leading dimensions keep the LDS-DMA path
        return dict(name=name, cplx=cplx, op=op, m=m, n=n, k=k, phase=phase, min_rounds=min_rounds, pad=pad, coff=coff, cls=cls)
    s = 2 * num_cu                                # workgroup slots: two per CU
    return [
        # group_rows = 4: at least 16 column tiles and 16 rounds of the chip
        c("cfg4_full_width", True, "N", 128 * s, 1024, 64, 1, "zN 3M whole gr4"),                  # 65536 x 1024: 8192 whole tiles
        c("gr4_mixed_partial", True, "N", 128 * (num_cu + 2), 2048, 512, 1, "zN 3M mixed gr4-partial"),   # 33024: 8192 + 64 x 8
        c("gr4_mixed_partial_hq", True, "C", 128 * (num_cu + 2), 2048, 512, 2, "zC 3M mixed gr4-partial"),
        c("gr4_mixed_partial_verify", True, "C", 128 * (num_cu + 2), 2048, 512, 3, "zC 4M mixed gr4-partial"),
        c("rank2x2_odd_width", True, "N", 128 * num_cu, 39 * 64, 256, 1, "zN 3M mixed gr4"),        # 32768 x 2496: 9728 + 256 x 2
        c("real_gr4_partial_n", False, "N", 128 * (s + 2), 2048, 512, 0, "dN 4M mixed gr4-partial"),  # 65792: 8192 + 32 x 4
        c("real_gr4_partial_c", False, "C", 128 * (s + 2), 2048, 512, 0, "dC 4M mixed gr4-partial"),
        # group_rows = 2, whole tiles plus a K-split tail in one grid
        c("cfg2_filter", True, "N", 64 * num_cu, 640, 256, 1, "zN 3M mixed gr2"),                  # 16384 x 640: 1024 + 256 x 2
        c("cfg3_rank_real", False, "N", 64 * num_cu, 1200, 256, 0, "dN 4M mixed gr2 ragged"),      # 16384 x 1200: 1024 + 256 x 2
        c("two_piece_mixed_first", True, "N", 64 * num_cu, 656, 256, 1, "two-piece mixed-first", pad=(0, 2, 3)),
        # what the older parity tests reach, one or two each
        c("all_tail", True, "C", 512, 256, 2048, 1, "zC 3M all-tail gr2"),
        c("forced_split", True, "N", 128 * (s // 4), 256, 2048, 1, "work:forced", min_rounds=4),   # one round: cut by min_rounds
        c("forced_split_real", False, "N", 128 * (s // 4), 512, 2048, 0, "work:forced", min_rounds=4),
        c("uniform_ragged", True, "N", 4096, 133, 4096, 1, "cols:uniform"),
        c("real_narrow_rest", False, "N", 4096, 300, 4096, 0, "cols:whole+narrow"),
        c("real_narrow_block", False, "C", 256, 40, 512, 1, "cols:narrow"),
        c("bulk_and_rims_n", True, "N", 1153, 96, 1001, 1, "3M-bulk+4M-rims"),
        c("bulk_and_rims_c", True, "C", 1280, 133, 1003, 1, "3M-bulk+4M-rims"),
        c("register_path_real", False, "N", 4096, 200, 4100, 0, "register-path", pad=(1, 1, 3)),   # odd lda / ldb
    ]


def k0_cases():
    """k = 0 (a rank that owns no rows of the block): C = beta C, for both types in every phase; m a multiple of 128 so that a
    complex product in phases 1 and 2 would qualify for the three-multiplication kernel by its shape."""
    return [dict(name=f"k0_{'z' if cplx else 'd'}_ph{ph}", cplx=cplx, op=op, m=256, n=70, k=0, phase=ph, min_rounds=0,
                 pad=(0, 0, 3), coff=1, cls="k0")
            for cplx in (True, False) for ph in (0, 1, 2, 3) for op in ("N", "C")]


# Every value of every launcher decision, and the production launches of the filter and the grid's panels.  A launcher branch
# that adds a value needs a case here (test_gemm_plan_cpu.py checks that the cases reach each of these at 256 CUs).
DECLARED = [
    "cols:whole", "cols:ragged", "cols:uniform", "cols:narrow", "cols:whole+ragged", "cols:whole+narrow",
    "work:whole", "work:all-tail", "work:mixed", "work:forced", "k0",
    "gr:2", "gr:4", "gr:4-partial",
    "mult:3M", "mult:4M", "3M-bulk+4M-rims", "beta-one",
    "lds-dma", "register-path",
    "zN 3M whole gr4", "zN 3M mixed gr4-partial", "zC 3M mixed gr4-partial", "zC 4M mixed gr4-partial", "zN 3M mixed gr4",
    "dN 4M mixed gr4-partial", "dC 4M mixed gr4-partial", "zN 3M mixed gr2", "dN 4M mixed gr2 ragged", "two-piece mixed-first",
]


def tile_width(cplx, narrow):
    return 64 if (cplx or narrow) else 128


def work_class(r):
    if r["k"] == 0:
        return "k0"
    if r["forced_split"]:
        return "forced"
    if r["tail_tiles"] == 0:
        return "whole"
    return "all-tail" if r["full_tiles"] == 0 else "mixed"


def plan_classes(plan, cplx, op):
    """The class labels a plan (chase_hip_gemm_plan records) reaches."""
    out = set()
    t = ("z" if cplx else "d") + op
    groups = {}
    for r in plan:
        groups.setdefault((r["row0"], r["k0"]), []).append(r)
    if len(groups) > 1:
        out.add("3M-bulk+4M-rims")
    for g in groups.values():
        if len(g) == 2:
            out.add("cols:whole+narrow" if g[1]["narrow"] else "cols:whole+ragged")
            if work_class(g[0]) == "mixed":
                out.add("two-piece mixed-first")
        else:
            r = g[0]
            if r["narrow"]:
                out.add("cols:narrow")
            elif r["bn_cols"] < tile_width(cplx, False):
                out.add("cols:uniform")
            else:
                out.add("cols:ragged" if r["ragged"] else "cols:whole")
    for r in plan:
        w = work_class(r)
        out.add("k0" if w == "k0" else "work:" + w)
        gr = r["group_rows"]
        partial = gr > 1 and r["gm"] % gr != 0
        out.add(f"gr:{gr}")
        if partial:
            out.add(f"gr:{gr}-partial")
        mult = "3M" if r["m3"] else "4M"
        out.add("mult:" + mult)
        out.add("lds-dma" if r["glds_ok"] else "register-path")
        if r["beta_one"]:
            out.add("beta-one")
        out.add(f"{t} {mult} {w} gr{gr}" + ("-partial" if partial else "") + (" ragged" if r["ragged"] else ""))
    return out
