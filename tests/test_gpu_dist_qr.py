"""chase_hip_houseqr_dist (chase_amd/csrc/hhqr.hip: dhh_partial_kernel, dhh_update_kernel, set_identity_stacked_kernel, larft_kernel
from an all-reduced Gram matrix) called directly on grids whose ranks are threads of this process, and held against the checkers
its single-GPU twin is held to (tests/dense_chain_refs.py: 8 x LAPACK's own measured error, componentwise orthogonality, the
nested column spaces against LAPACK's Q).  What the solver's own calls never produce is produced here: ranks with more than 256
rows (the 256-stride loops take up to five passes), a leading dimension of mloc + 3 with a canary below every block, a rank
without rows inside the stacked order, a rank with one row, ranks shorter than a panel, m == n, three panels with a ragged last
one, the H = I branch and the complex pivot over a zero tail.  The cases and why each exists: tests/dist_qr_refs.py; that the
bounds see a kernel that drops rows from 256 on or stores with the wrong leading dimension: tests/test_dist_qr_refs_cpu.py.

Largest ratios measured on an MI355X (measured error / bound; a test fails above 1), real | complex, over all inputs of a case:
    case                      orth             span             tril             g_off              g_diag
    five_passes               0.0094 | 0.0047  0.0043 | 0.0036  0.015 | 0.014    0.0018  | 0.00091  0.0078 | 0.0067
    two_ranks                 0.0036 | 0.0036  0.0031 | 0.0026  0.014 | 0.013    0.0012  | 0.00061  0.0036 | 0.0027
    replicas (host, shared)   0.0045 | 0.0027  0.0030 | 0.0025  0.014 | 0.012    0.00077 | 0.00068  0.0036 | 0.0027
    empty_and_one             0.0045 | 0.0036  0.0030 | 0.0026  0.014 | 0.013    0.0011  | 0.00065  0.0032 | 0.0027
    square                    0.0024 | 0.0019  0.0023 | 0.0027  0.017 | 0.023    (not compared: m == n)
    tiny, tiny_empty_last     0.047  | 0.018   0.027  | 0.030   0.18  | 0.30     0.013   | 0.016    0.0051 | 0.012
    two_ranks, nb = 2         0.0036 | 0.0027  0.0030 | 0.0025  0.012 | 0.011    0.00085 | 0.00067  0.0036 | 0.0018
    two_ranks, nb = 17        0.0045 | 0.0027  0.0029 | 0.0024  0.013 | 0.012    0.00082 | 0.00061  0.0045 | 0.0027
    two_ranks, nb = 48, 200   0.0036 | 0.0027  0.0031 | 0.0026  0.015 | 0.014    0.0012  | 0.00058  0.0036 | 0.0027
    solver, 2 x 2 block       0.0036 | 0.0036  0.0031 | 0.0026  0.014 | 0.013    0.0012  | 0.00061  0.0036 | 0.0027
    solver, 3 x 2 cyclic 16   0.0045 | 0.0031  0.0032 | 0.0026  0.015 | 0.012    0.00069 | 0.00067  0.0036 | 0.0027
The older normwise orthogonality (||Q^H Q - I||_F / sqrt(n) against 25 eps) peaks at 0.21 (square, complex).  The numpy model of
the same algorithm sits at the same figures (tests/test_dist_qr_refs_cpu.py prints them): no ratio comes near 1, no defect found."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dense_chain_refs as D  # noqa: E402
import dist_qr_refs as Q  # noqa: E402
from rank_threads import run_ranks  # noqa: E402

pytestmark = pytest.mark.gpu
CPLX = pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
EINVAL = -1001


def _run_case(name, cplx, transport="host"):
    import dist_qr_scenarios as S
    _, nprow, npcol, counts, n = Q.CASE[name]
    out = {}
    run_ranks(nprow, npcol, S.scenario_houseqr_dist, name, cplx, out, transport=transport)
    assert list(out) == list(Q.inputs(name, cplx)), list(out)
    return out


def _check_case(name, cplx, out, tag=""):
    """the assertions of every direct test: ratios <= 1, canary intact, finite, replicas and the second call equal bit for bit"""
    _, nprow, npcol, counts, n = Q.CASE[name]
    peak, bad = {}, []
    for kind, res in out.items():
        V, bufs = res["V"], res["bufs"]
        Qs = Q.gather(bufs[0], counts)
        r = Q.ratios(V, Qs, kind)
        assert ("g_off" in r) == (kind == "random" and name != "square") or "finite" in r, (kind, r)
        for k, v in r.items():
            peak[k] = max(peak.get(k, 0.0), float(v))
            if not v <= 1:
                bad.append((kind, k, float(v)))
        if not np.all(np.isfinite(Qs)):
            bad.append((kind, "finite"))
        for j in range(npcol):
            if not Q.padding_intact(bufs[j], counts):
                bad.append((kind, "canary overwritten in grid column %d" % j))
            if not all(D.same_bits(a, b) for a, b in zip(bufs[0], bufs[j])):
                bad.append((kind, "replica in grid column %d differs" % j))
            if not all(D.same_bits(a, b) for a, b in zip(bufs[j], res["again"][j])):
                bad.append((kind, "second call differs in grid column %d" % j))
    print("houseqr_dist", name, "complex" if cplx else "real", tag, "largest ratios:", {k: float("%.3g" % v) for k, v in peak.items()})
    assert not bad, bad[:8]
    return peak


@CPLX
@pytest.mark.parametrize("name", [c[0] for c in Q.CASES])
def test_houseqr_dist_against_the_checkers_of_the_single_gpu_qr(name, cplx):
    _check_case(name, cplx, _run_case(name, cplx))


@CPLX
@pytest.mark.parametrize("nb", Q.PANEL_WIDTHS)
def test_houseqr_dist_panel_widths(monkeypatch, nb, cplx):
    """CHASE_HOUSEHOLDER_NB = 2 (35 panels), 17 (ragged: 17, 17, 17, 17, 2), 48 (the kernels' capacity) and 200, which is clamped
    to 48: the same bits as 48.  Set before the ranks start, so no rank changes the environment while others run."""
    monkeypatch.delenv("CHASE_QR_OUTER_BLOCK_NB", raising=False)
    monkeypatch.setenv("CHASE_HOUSEHOLDER_NB", str(nb))
    out = _run_case("two_ranks", cplx)
    _check_case("two_ranks", cplx, out, "nb=%d" % nb)
    if nb > Q.HMAX:
        monkeypatch.setenv("CHASE_HOUSEHOLDER_NB", str(Q.HMAX))
        ref = _run_case("two_ranks", cplx)
        for kind in out:
            assert all(D.same_bits(a, b) for a, b in zip(out[kind]["bufs"][0], ref[kind]["bufs"][0])), kind


@CPLX
def test_houseqr_dist_on_the_shared_device_transport(cplx):
    """the replica case with device-side collectives between the ranks' streams instead of the host callbacks"""
    _check_case("replicas", cplx, _run_case("replicas", cplx, transport="shared"), "shared")


def _refused(ctx, grid, comm, cplx, out):
    from chase_amd import dist as cd
    from chase_amd.capi import lib
    mloc, n = 40, 8
    V = D.rnd(np.random.default_rng(5), (mloc, n), cplx)
    buf = D.padded(V, mloc + Q.PAD)
    dV = ctx.array(buf)
    call = lambda mloc_, n_, ptr, ldv, off: lib.chase_hip_houseqr_dist(ctx.h, grid.h, cd.COL, int(cplx), mloc_, n_, ptr, ldv, off)
    out["rc"] = {"ldv < mloc": call(mloc, n, dV.ptr, mloc - 1, 0), "n < 0": call(mloc, -1, dV.ptr, mloc + Q.PAD, 0),
                 "row_offset < 0": call(mloc, n, dV.ptr, mloc + Q.PAD, -1), "mloc < 0": call(-1, n, dV.ptr, mloc + Q.PAD, 0),
                 "NULL block": call(mloc, n, None, mloc + Q.PAD, 0)}
    out["message"] = lib.chase_hip_last_error().decode()
    out["n == 0"] = call(mloc, 0, dV.ptr, mloc + Q.PAD, 0)
    out["untouched"] = D.same_bits(dV.download(), buf)
    dV.free()


@CPLX
def test_houseqr_dist_refuses_bad_shapes_before_any_launch(cplx):
    out = {}
    run_ranks(1, 1, _refused, cplx, out)
    assert out["rc"] == {k: EINVAL for k in out["rc"]}, out["rc"]
    assert "houseqr_dist" in out["message"]
    assert out["n == 0"] == 0 and out["untouched"]              # nothing written by the refused calls or the empty one


@CPLX
@pytest.mark.parametrize("nprow,npcol,mb", [(2, 2, 0), (3, 2, 16)], ids=["2x2-block", "3x2-blockcyclic16"])
def test_the_solvers_householder_at_600_rows(nprow, npcol, mb, cplx):
    """pChaseHip::householder() through DistSolver.QR with 300 / 200 rows on a rank (block) and rows dealt in blocks of 16
    (block-cyclic): the offset it derives from the layout, Householder requested and as the fall-through of a failed potrf"""
    import dist_qr_scenarios as S
    out = {}
    run_ranks(nprow, npcol, S.scenario_householder_caller, cplx, mb, out)
    assert list(out) == [("random", 0), ("duplicate_column", 0), ("cholqr_breaks", 1)]
    peak, bad = {}, []
    for (kind, cholqr), res in out.items():
        r = Q.ratios(res["V"], res["Q"], kind)
        for k, v in r.items():
            peak[k] = max(peak.get(k, 0.0), float(v))
            if not v <= 1:
                bad.append((kind, k, float(v)))
        if res["variant"] != [0]:
            bad.append((kind, "qr_variant", res["variant"]))
        if not res["replicas_equal"]:
            bad.append((kind, "replicas differ between the grid columns"))
    print("householder()", (nprow, npcol, mb), "complex" if cplx else "real", "largest ratios:",
          {k: float("%.3g" % v) for k, v in peak.items()})
    assert not bad, bad
