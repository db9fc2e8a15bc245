"""The GEMM launch plan (chase_hip_gemm_plan, host-only): the case table of the GPU plan tests reaches every launcher decision,
and over a seeded sweep of shapes every plan is a valid decomposition of its product.  No GPU needed."""
import numpy as np
import pytest

import gemm_plan_cases as G
from chase_amd.capi import gemm_plan, lib


def _plan(c, num_cu):
    ra = c["m"] if c["op"] == "N" else c["k"]
    return gemm_plan(c["cplx"], c["op"], c["m"], c["n"], c["k"], lda=ra + c["pad"][0], ldb=c["k"] + c["pad"][1],
                     phase=c["phase"], num_cu=num_cu, min_rounds=c["min_rounds"])


def test_case_table_covers_every_launcher_decision():
    """At 256 CUs (the MI355X) each case reaches the class it is listed for, and together they reach every declared class."""
    reached = set()
    for c in G.cases(256) + G.k0_cases():
        cls = G.plan_classes(_plan(c, 256), c["cplx"], c["op"])
        assert c["cls"] in cls, (c["name"], sorted(cls))
        reached |= cls
    missing = [d for d in G.DECLARED if d not in reached]
    assert not missing, missing


def test_num_cu_derived_cases_keep_their_class_on_other_chips():
    for num_cu in (80, 304):
        for c in G.cases(num_cu):
            if c["name"] in ("all_tail", "uniform_ragged", "real_narrow_rest", "real_narrow_block", "bulk_and_rims_n",
                             "bulk_and_rims_c", "register_path_real"):
                continue                                     # fixed shapes: their class is the 256-CU one
            assert c["cls"] in G.plan_classes(_plan(c, num_cu), c["cplx"], c["op"]), (num_cu, c["name"])


def _check_plan(plan, cplx, op, m, n, k, lda, ldb, aligned, phase, num_cu, min_rounds):
    ctx = (cplx, op, m, n, k, lda, ldb, aligned, phase, num_cu, min_rounds)
    if m == 0 or n == 0:
        assert plan == [], ctx
        return
    assert plan, ctx
    ws = lib.chase_hip_gemm_workspace_bytes(int(cplx), op.encode(), m, n, k, num_cu, min_rounds)
    rows = sorted({0, m} | {r["row0"] for r in plan} | {r["row0"] + r["m"] for r in plan})
    cols = sorted({0, n} | {r["col0"] for r in plan} | {r["col0"] + r["n"] for r in plan})
    # partition: every cell of the grid the pieces' edges make is covered by pieces whose K ranges tile [0, k) exactly, the
    # first of them (in launch order) applies beta and every later one adds into it
    for i0, i1 in zip(rows[:-1], rows[1:]):
        for j0, j1 in zip(cols[:-1], cols[1:]):
            cover = [r for r in plan if r["row0"] <= i0 and i1 <= r["row0"] + r["m"] and r["col0"] <= j0 and j1 <= r["col0"] + r["n"]]
            assert cover, (ctx, i0, j0)
            assert [r["beta_one"] for r in cover] == [0] + [1] * (len(cover) - 1), (ctx, i0, j0)
            kr = sorted((r["k0"], r["k0"] + r["k"]) for r in cover)
            assert kr[0][0] == 0 and kr[-1][1] == k and all(a[1] == b[0] for a, b in zip(kr[:-1], kr[1:])), (ctx, kr)
    for r in plan:
        assert 0 <= r["row0"] and r["row0"] + r["m"] <= m and 0 <= r["col0"] and r["col0"] + r["n"] <= n, (ctx, r)
        bm, bn = 128, (64 if (cplx or r["narrow"]) else 128)
        assert r["gm"] == -(-r["m"] // bm) and r["gn"] == -(-r["n"] // r["bn_cols"]) and 16 <= r["bn_cols"] <= bn, (ctx, r)
        assert r["bn_cols"] % 16 == 0 or r["bn_cols"] == bn, (ctx, r)
        assert r["full_tiles"] + r["tail_tiles"] == r["gm"] * r["gn"], (ctx, r)
        # the launcher refuses (GEMM_F64_EWORKSPACE) a piece whose slabs + plane do not fit what the context allocates
        assert ((r["slab_bytes"] + 255) & ~255) + r["plane_bytes"] <= ws or (r["plane_bytes"] == 0 and r["slab_bytes"] <= ws), (ctx, r, ws)
        assert r["slab_bytes"] == (r["tail_tiles"] * r["tail_sk"] * bm * bn * 8 * (2 if cplx else 1) if r["tail_tiles"] else 0), (ctx, r)
        if r["k"] > 0:
            assert r["tail_sk"] * r["tail_kchunk"] >= r["k"], (ctx, r)
            assert r["tail_kchunk"] % (8 if cplx else 16) == 0, (ctx, r)
        if r["tail_tiles"] == 0:
            assert r["tail_sk"] == 1, (ctx, r)
        else:
            assert r["tail_sk"] >= 2, (ctx, r)
        if r["forced_split"]:
            assert min_rounds > 0 and r["full_tiles"] == 0, (ctx, r)
        else:
            assert r["tail_tiles"] < 2 * num_cu, (ctx, r)
        if r["m3"]:
            assert cplx and phase in (1, 2) and r["glds_ok"] and r["k"] > 0, (ctx, r)
            assert r["m"] % 128 == 0 and r["k"] % 8 == 0 and r["tail_kchunk"] % 8 == 0 and aligned, (ctx, r)
            assert r["plane_bytes"] == -(-r["n"] // r["bn_cols"]) * (r["k"] // 8) * 4096, (ctx, r)
        else:
            assert r["plane_bytes"] == 0, (ctx, r)
        if not aligned or (not cplx and (lda % 2 or ldb % 2)):
            assert not r["glds_ok"], (ctx, r)
        assert r["group_rows"] in (2, 4), (ctx, r)
        assert (r["group_rows"] == 4) == (r["gn"] >= 16 and r["gm"] * r["gn"] >= 32 * num_cu), (ctx, r)
    if cplx and phase in (1, 2) and aligned and m % 128 == 0 and k % 8 == 0 and k > 0:
        assert any(r["m3"] for r in plan), ctx          # a qualifying filter product does run on three multiplications


def test_plans_partition_the_product_and_fit_the_workspace():
    """A seeded sweep of shapes (m, k up to 70 000, n up to 3 000), both types and ops, every phase, min_rounds 0 / 4 and
    three chip sizes: the decomposition invariants of every plan."""
    rng = np.random.default_rng(2026)
    count = 0
    for t in range(3000):
        cplx = bool(t % 2)
        op = "N" if (t // 2) % 2 == 0 else "C"
        num_cu = (256, 304, 80)[t % 3]
        min_rounds = 4 if t % 7 < 2 else 0
        phase = int(rng.integers(0, 4))
        kind = t % 5
        if kind == 0:      # whole tiles along M and K: the 3M kernels' shapes
            m, k = 128 * int(rng.integers(1, 547)), 8 * int(rng.integers(1, 8750))
        elif kind == 1:    # small
            m, k = int(rng.integers(0, 700)), int(rng.integers(0, 700))
        else:
            m, k = int(rng.integers(1, 70001)), int(rng.integers(0, 70001))
        n = int(rng.integers(1, 3001)) if t % 4 else int(rng.choice([1, 16, 40, 64, 65, 128, 133, 256, 640, 1024, 2560]))
        ra = m if op == "N" else k
        lda, ldb = ra + int(rng.integers(0, 3)), k + int(rng.integers(0, 3))
        aligned = bool(t % 11)
        plan = gemm_plan(cplx, op, m, n, k, lda=lda, ldb=ldb, aligned=aligned, phase=phase, num_cu=num_cu, min_rounds=min_rounds)
        _check_plan(plan, cplx, op, m, n, k, lda, ldb, aligned, phase, num_cu, min_rounds)
        count += len(plan)
    assert count > 3000


def test_plan_follows_the_three_multiplication_switch():
    from chase_amd.capi import ChaseHipError
    assert lib.chase_hip_gemm3m_enabled() == 1
    on = gemm_plan(True, "N", 4096, 640, 4096, phase=1)
    try:
        lib.chase_hip_set_gemm3m(0)
        off = gemm_plan(True, "N", 4096, 640, 4096, phase=1)
    finally:
        lib.chase_hip_set_gemm3m(1)
    assert all(r["m3"] for r in on) and not any(r["m3"] for r in off)
    for ph in (0, 3):
        assert not any(r["m3"] for r in gemm_plan(True, "N", 4096, 640, 4096, phase=ph))
    assert gemm_plan(True, "N", 0, 5, 5) == [] and gemm_plan(False, "C", 5, 0, 5) == []
    with pytest.raises(ChaseHipError):
        gemm_plan(True, "X", 4, 4, 4)
    with pytest.raises(ChaseHipError):
        gemm_plan(False, "N", 4, 4, -1)


@pytest.mark.parametrize("cplx", [True, False])
def test_k0_products_take_four_multiplications(cplx):
    """k = 0 (C = beta C) has nothing to multiply: no three-multiplication launch, whose operand-sum plane would be a launch of
    zero workgroups."""
    for ph in range(4):
        plan = gemm_plan(cplx, "N", 256, 70, 0, lda=256, ldb=1, phase=ph)
        assert len(plan) == 1 and plan[0]["k"] == 0 and not plan[0]["m3"] and plan[0]["tail_tiles"] == 0
