"""The reference side of the distributed Householder QR tests (tests/dist_qr_refs.py) is checked itself, without a GPU:
* the plain numpy model of chase_hip_houseqr_dist stays inside every bound of the checkers on every case and input the GPU tests
  run - so the algorithm, done in double precision in any summation order, has room under the bounds;
* the model with ONE seeded defect - rows from 256 on left out of the column sums, or the reflectors stored with the wrong
  leading dimension - misses a bound by more than 10x at the shapes with more than 256 rows on a rank: the shapes and bounds chosen
  can see a subtly wrong kernel;
* LAPACK stays inside the recorded LAPACK_QR_* constants on the new shapes (tests/test_dense_chain_refs_cpu.py: the older ones)."""
import numpy as np
import pytest
import scipy.linalg as sla
import dense_chain_refs as D
import dist_qr_refs as Q

CPLX = pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
NAMES = [c[0] for c in Q.CASES]
LONG = [c[0] for c in Q.CASES if max(c[3]) > 256]                  # a 256-stride loop takes a second pass on some rank
TAILS = ("random", "zero_column", "duplicate_column")              # inputs with something below their pivots


def test_stacked_split_deals_the_rows_in_rank_order():
    off, sl = Q.stacked_split(600, (300, 0, 299, 1))
    assert off == [0, 300, 300, 599]
    assert [(s.start, s.stop) for s in sl] == [(0, 300), (300, 300), (300, 599), (599, 600)]
    assert Q.stacked_split(9, (3, 3, 3, 0))[0] == [0, 3, 6, 9]
    with pytest.raises(AssertionError):
        Q.stacked_split(10, (3, 3, 3))


def test_the_cases_are_what_they_are_for():
    assert NAMES == ["five_passes", "two_ranks", "replicas", "empty_and_one", "square", "tiny", "tiny_empty_last"]
    assert LONG == ["five_passes", "two_ranks", "replicas", "empty_and_one"]
    for name, nprow, npcol, counts, n in Q.CASES:
        assert len(counts) == nprow and sum(counts) >= n and nprow >= npcol
    assert -(-1100 // 256) == 5 and Q.CASE["five_passes"][4] == 32 + 8
    assert Q.CASE["two_ranks"][4] == 32 + 32 + 6 and Q.CASE["two_ranks"][3][0] >= 70           # every pivot on rank 0
    assert Q.CASE["replicas"][2] == 2 and Q.CASE["replicas"][3] == (257, 343)                   # one row into the second pass
    assert 0 in Q.CASE["empty_and_one"][3][1:-1] and 1 in Q.CASE["empty_and_one"][3]
    _, _, _, counts, n = Q.CASE["square"]
    assert sum(counts) == n == 130 and max(counts[:3]) <= 48 and sum(counts[:3]) < n            # pivots on all four ranks
    assert Q.SHAPES == [(9, 4), (130, 130), (600, 70), (1100, 40)]
    assert [Q.panel_width(w) for w in [None] + Q.PANEL_WIDTHS] == [32, 2, 17, 48, 48]
    assert list(Q.inputs("tiny", True)) == ["random", "zero_column", "duplicate_column", "upper_triangular",
                                            "upper_triangular_complex_diagonal"]
    assert list(Q.inputs("tiny", False)) == ["random", "zero_column", "duplicate_column", "upper_triangular"]


@CPLX
@pytest.mark.parametrize("name", NAMES)
def test_the_clean_model_passes_every_checker(name, cplx):
    _, _, _, counts, n = Q.CASE[name]
    peak = {}
    for kind, V in Q.inputs(name, cplx).items():
        for nb in ([None] + Q.PANEL_WIDTHS if name == "two_ranks" else [None]):
            bufs = Q.model_houseqr_dist(V, counts, nb=nb)
            assert Q.padding_intact(bufs, counts), (kind, nb)
            r = Q.ratios(V, Q.gather(bufs, counts), kind)
            assert ("g_off" in r) == (kind == "random" and name != "square"), (kind, r)
            for k, v in r.items():
                peak[k] = max(peak.get(k, 0.0), float(v))
            assert D.worst(r)[0] <= 1, (kind, nb, r)
    print(name, "complex" if cplx else "real", "largest ratios:", {k: float("%.3g" % v) for k, v in peak.items()})


@CPLX
def test_the_model_does_not_depend_on_where_the_empty_ranks_are(cplx):
    """an empty rank contributes zeros to every sum: the same bits with and without it"""
    for kind, V in Q.inputs("tiny", cplx).items():
        a = Q.gather(Q.model_houseqr_dist(V, (3, 3, 3)), (3, 3, 3))
        for counts in ((3, 3, 3, 0), (0, 3, 3, 3), (3, 0, 3, 0, 3)):
            assert D.same_bits(a, Q.gather(Q.model_houseqr_dist(V, counts), counts)), (kind, counts)


@CPLX
@pytest.mark.parametrize("name", LONG)
def test_each_seeded_defect_misses_a_bound_by_more_than_ten_times(name, cplx):
    _, _, _, counts, n = Q.CASE[name]
    for kind, V in Q.inputs(name, cplx).items():
        clean = Q.gather(Q.model_houseqr_dist(V, counts), counts)
        for defect in ({"drop_rows_from": 256}, {"wrong_ld": True}):
            bufs = Q.model_houseqr_dist(V, counts, **defect)
            r = Q.ratios(V, Q.gather(bufs, counts), kind)
            if kind in TAILS:
                assert D.worst(r)[0] > 10, (kind, defect, r)
            elif "drop_rows_from" in defect:
                # triangular inputs: nothing below any pivot, so no sum has a row to lose - the reason the GPU tests do not
                # rest on them alone
                assert D.same_bits(Q.gather(bufs, counts), clean), kind
            if "wrong_ld" in defect:
                assert not Q.padding_intact(bufs, counts), kind               # ... while the canary sees a wrong store on every input


@CPLX
def test_the_defects_are_invisible_below_257_rows_and_with_ld_equal_to_the_extent(cplx):
    """why the GPU tests need a rank with more than 256 rows and the three pad rows"""
    for name in ("square", "tiny"):
        counts = Q.CASE[name][3]
        for kind, V in Q.inputs(name, cplx).items():
            a = Q.model_houseqr_dist(V, counts)
            b = Q.model_houseqr_dist(V, counts, drop_rows_from=256)
            assert all(D.same_bits(x, y) for x, y in zip(a, b)), (name, kind)
    counts = Q.CASE["two_ranks"][3]
    V = Q.inputs("two_ranks", cplx)["random"]
    a = Q.model_houseqr_dist(V, counts, pad=0)
    b = Q.model_houseqr_dist(V, counts, pad=0, wrong_ld=True)
    assert all(D.same_bits(x, y) for x, y in zip(a, b))


def test_lapack_stays_inside_the_recorded_constants_on_the_new_shapes():
    mx = np.zeros(4)
    for m, n in Q.SHAPES:
        for cplx in (False, True):
            for kind, V in D.qr_cases(np.random.default_rng(D.seed_of(3, m, n, cplx)), m, n, cplx).items():
                Ql = sla.qr(V, mode="economic")[0]
                g = (0.0, 0.0)
                if kind == "random" and m > n:
                    g = D.qr_g_raw(V, np.linalg.qr(V)[0], Ql)                   # (kappa_2 <= 1e3 is asserted inside)
                mx = np.maximum(mx, list(D.qr_raw(V, Ql)) + [max(g)])
                assert D.worst(D.qr_ratios(V, Ql))[0] <= 1, (m, n, cplx, kind, D.qr_ratios(V, Ql))
    print("LAPACK on", Q.SHAPES, "orth span tril g:", mx)
    assert np.all(mx <= [D.LAPACK_QR_ORTH, D.LAPACK_QR_SPAN, D.LAPACK_QR_TRIL, D.LAPACK_QR_G]), mx
    assert mx[2] > 0.045                      # the (9, 4) block is what LAPACK_QR_TRIL was raised for
