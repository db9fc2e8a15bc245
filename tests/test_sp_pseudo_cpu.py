"""The numerics of the single-precision pseudo-Hermitian solver (ChaseHipSpPseudo) on the CPU: the emulation of
tests/sp_pseudo_ref.py over the oracle on the reference's float BSE fixtures divided by 64, and the numpy references of the two new
fp32 kernels against hand-written answers.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sp_pseudo_ref as R  # noqa: E402
from chase_amd import capi  # noqa: E402

# what the emulation stands for: the entry points and the binding of the solver (host-only lookups)
ENTRY_POINTS = ("chase_hip_solver_create_pseudo_sp", "chase_hip_scale_rows_sp", "chase_hip_kconj_sp", "cchase_init_pseudo_",
                "cchase_init_pseudo_internal_", "cchase_pseudo_")
for _n in ENTRY_POINTS:
    getattr(capi.lib, _n)
assert issubclass(capi.SpPseudoSolver, capi.PseudoSolver)


def test_fixtures_are_pseudo_hermitian_and_their_shipped_spectrum_is_the_dense_one():
    for kind in ("complex", "real"):
        for tiny in (False, True):
            H = R.fixture(kind, tiny)
            N = H.shape[0]
            h = N // 2
            A, B = H[:h, :h], H[:h, h:]
            assert np.array_equal(H[h:, :h], -np.conj(B)) and np.array_equal(H[h:, h:], -np.conj(A))
            name, dt = (R.TINY if tiny else R.FIXTURES)[kind]
            shipped = np.fromfile(os.path.join(R._DIR, "eigs_" + name), dtype=dt)
            assert shipped.size == N
            dense = np.sort(np.linalg.eigvals(R.widen(H)).real) * R.SCALE
            # the shipped values come from an fp32 eigensolver: backward error of order N 2^-24 ||H||, ||H||_2 <= 40
            assert np.max(np.abs(np.sort(shipped.real.astype(np.float64)) - dense)) <= N * R.U * 40.0
    nrm = np.linalg.norm(R.widen(R.fixture("complex")), 2)
    assert np.sqrt(R.N_FIXTURE) * R.U * nrm < 1e-6 < R.FLOAT_DEFAULTS["tol"]         # the residual floor is below tol


@pytest.mark.parametrize("kind,nev,nex", R.CASES, ids=["%s-%d-%d" % c for c in R.CASES])
def test_emulated_single_precision_solve(kind, nev, nex):
    r = R.emulated(kind, nev, nex)
    d, s = r["fp64"], r["sp"]
    print(f"{kind} {nev}/{nex}: fp64 oracle {d['iterations']} iterations / {d['filtered_vecs']} filtered vectors, emulation "
          f"{s['iterations']} / {s['filtered_vecs']}, largest own residual {np.max(s['own_resid']):.2e}, largest fp64 residual "
          f"{s['max_resid']:.2e}, eigenvalue error {s['eig_err']:.2e}")
    assert d["locked"] >= nev and s["locked"] >= nev
    assert np.all(s["own_resid"] <= 1e-5)
    assert s["max_resid"] <= 1e-5
    assert abs(s["iterations"] - d["iterations"]) <= 1
    assert abs(s["filtered_vecs"] - d["filtered_vecs"]) <= 0.05 * d["filtered_vecs"]
    assert s["hemm_sp_vecs"] == s["filtered_vecs"]
    assert s["eig_err"] <= 1e-5


def test_scale_rows_sp_reference_on_hand_written_answers():
    f, c = np.float32, np.complex64
    X = np.array([[1.5], [-2.0]], dtype=f)                                              # N = 2, real
    assert R.scale_rows_sp_ref(X, 1, -1.0).tolist() == [[1.5], [2.0]]
    assert R.scale_rows_sp_ref(X, 0, 2.0).tolist() == [[3.0], [-4.0]]
    assert R.scale_rows_sp_ref(X, 2, -1.0).tobytes() == X.tobytes()                     # row0 == m: nothing
    Z = np.array([[1 + 2j], [-3 + 0.5j]], dtype=c)                                      # N = 2, complex
    assert R.scale_rows_sp_ref(Z, 1, -1.0).tolist() == [[1 + 2j], [3 - 0.5j]]
    X = np.arange(1, 21, dtype=f).reshape((10, 2), order="F")                           # N = 10
    got = R.scale_rows_sp_ref(X, 5, f(0.001))
    want = X.copy()
    for j in range(2):
        for i in range(5, 10):
            want[i, j] = f(X[i, j]) * f(0.001)
    assert got.tobytes() == want.tobytes() and got.dtype == f
    Z = (X + 1j * (X + 100)).astype(c)
    got = R.scale_rows_sp_ref(Z, 5, f(0.001))
    for j in range(2):
        for i in range(10):
            re, im = f(Z[i, j].real), f(Z[i, j].imag)
            if i >= 5:
                re, im = re * f(0.001), im * f(0.001)
            assert got[i, j].real == re and got[i, j].imag == im
    assert float(f(0.001)) != 0.001                                                          # the factor is the rounded one


def test_kconj_sp_reference_on_hand_written_answers():
    f, c = np.float32, np.complex64
    assert R.kconj_sp_ref(np.array([[1.0], [2.0]], dtype=f)).tolist() == [[2.0], [1.0]]                     # N = 2, real
    assert R.kconj_sp_ref(np.array([[1 + 2j], [3 - 4j]], dtype=c)).tolist() == [[3 + 4j], [1 - 2j]]         # N = 2, complex
    X = np.arange(20, dtype=f).reshape((10, 2), order="F")                                                  # N = 10, h = 5
    assert R.kconj_sp_ref(X)[:, 0].tolist() == [5, 6, 7, 8, 9, 0, 1, 2, 3, 4]
    assert R.kconj_sp_ref(X)[:, 1].tolist() == [15, 16, 17, 18, 19, 10, 11, 12, 13, 14]
    Z = (X + 1j * (X + 0.5)).astype(c)
    got = R.kconj_sp_ref(Z)
    for j in range(2):
        for i in range(5):
            assert got[i + 5, j] == Z[i, j].real - 1j * Z[i, j].imag and got[i, j] == Z[i + 5, j].real - 1j * Z[i + 5, j].imag
    assert R.kconj_sp_ref(R.kconj_sp_ref(Z)).tobytes() == Z.tobytes()                                      # an involution


def test_emulation_locked_columns_keep_their_bits_through_qr():
    H = R.fixture("complex")
    k = R.OracleSpPseudo(H, 6, 4)
    k.initVecs(True)
    k.QR(0, 1.0)
    k.Lock(3)
    k.ApplyKconjugate(3)                           # (fills some second-half columns: any data will do)
    before = k.V1.copy()
    k.QR(3, 50.0)
    nc = k.ncol
    assert k.V1[:, :3].tobytes() == before[:, :3].tobytes() and k.V1[:, nc - 3:].tobytes() == before[:, nc - 3:].tobytes()
    assert k.V2[:, :3].tobytes() == before[:, :3].tobytes() and k.V2[:, nc - 3:].tobytes() == before[:, nc - 3:].tobytes()
    Q = R.widen(k.V1[:, 3:nc - 3])
    assert np.linalg.norm(Q.conj().T @ Q - np.eye(nc - 6)) / np.sqrt(nc - 6) <= (np.sqrt(H.shape[0]) + 2) * R.U
