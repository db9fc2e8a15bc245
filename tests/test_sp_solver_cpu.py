"""The emulation of the single-precision Hermitian solver (tests/sp_solver_ref.py) on the issue's four cases - no GPU.

Clement matrices clement(N, cplx, 1e-6) / N rounded to fp32, the reference's float defaults (tol 1e-5, deg 10, maxDeg 18,
lanczosIter 12).  The emulation must take the iteration and filtered-vector counts of the fp64 oracle on the same matrix, lock
at least nev pairs, and leave every wanted residual - its own, and the fp64 one against the fp32 matrix - at or below tol."""
import numpy as np
import pytest

import sp_solver_ref as R

TOL = R.FLOAT_DEFAULTS["tol"]
# iterations and filtered vectors read when the emulation was designed (the largest fp64 residuals against the fp32 matrix were
# about 8.0e-6, 4.6e-6, 9.5e-6 and 9.99e-6 then; they depend on the host BLAS in the last digits - 9.993e-6 for the last case
# with this one - so the assertion on them is the issue's: at or below tol)
DESIGN = {(256, 24, 16, False): (3, 1148), (256, 24, 16, True): (3, 1264),
          (301, 30, 20, True): (3, 1432), (1001, 100, 60, False): (4, 5334)}


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "N%d-%d-%d-%s" % (c[0], c[1], c[2], "c" if c[3] else "r"))
def test_emulation_takes_the_fp64_counts_and_reaches_tol(case):
    N, nev, nex, cplx = case
    e = R.emulated(*case)
    print(case, e["fp64"], {k: v for k, v in e["sp"].items() if k not in ("own_resid", "ritzv")}, float(np.max(e["sp"]["own_resid"])))
    assert e["sp"]["iterations"] == e["fp64"]["iterations"]
    assert e["sp"]["filtered_vecs"] == e["fp64"]["filtered_vecs"]
    assert e["sp"]["hemm_sp_vecs"] == e["sp"]["filtered_vecs"]
    assert e["sp"]["locked"] >= nev
    assert np.max(e["sp"]["own_resid"]) <= TOL
    assert e["sp"]["max_resid"] <= TOL
    assert e["sp"]["h_restored"]                        # every unshift gave the saved diagonal back bit for bit
    assert (e["sp"]["iterations"], e["sp"]["filtered_vecs"]) == DESIGN[case]
    # and the eigenvalues are those of the fp32 matrix to within the residual
    ev = np.linalg.eigvalsh(R.widen(R.case_matrix(N, cplx)))[:nev]
    assert np.max(np.abs(np.sort(e["sp"]["ritzv"]) - ev)) <= e["sp"]["max_resid"]


def test_shift_from_the_saved_diagonal_does_not_drift():
    """fp32 (h + c) - c does not give h back; the saved-diagonal form does, after any number of brackets"""
    H = R.case_matrix(64, True)
    H[np.arange(64), np.arange(64)] = np.random.default_rng(3).standard_normal(64).astype(np.float32)
    k = R.OracleSp(H, 4, 4)
    drift = H.copy()
    idx = np.arange(64)
    for c in (0.37, 1.113, 0.0501):
        k.Shift(-c)
        assert np.array_equal(k.H[idx, idx].real, (H[idx, idx].real.astype(np.float64) - c).astype(np.float32))
        assert np.array_equal(k.H[idx, idx].imag, H[idx, idx].imag)
        k.Shift(+c, True)
        assert np.array_equal(k.H, H)
        drift[idx, idx] = (drift[idx, idx] + np.float32(-c)) + np.float32(c)
    assert not np.array_equal(drift, H)


def test_resid_norms_bound_is_tight_enough_to_see_a_wrong_entry():
    rng = np.random.default_rng(5)
    W = rng.standard_normal((133, 5)).astype(np.float32)
    V = rng.standard_normal((133, 5)).astype(np.float32)
    lam = rng.standard_normal(5)
    exact = R.resid_norms_exact(W, V, lam)
    b = R.resid_norms_bound(W, V, lam)
    fp64 = np.linalg.norm(W.astype(np.float64) - V.astype(np.float64) * lam[None, :], axis=0)
    assert np.all(np.abs(fp64 - exact) <= b)
    W2 = W.copy(); W2[7, 2] = np.nextafter(W2[7, 2], np.float32(np.inf))          # one ulp of one fp32 entry
    moved = np.abs(R.resid_norms_exact(W2, V, lam) - exact)
    assert moved[2] > 100 * b[2]
