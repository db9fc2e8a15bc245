"""The numerics of the pseudo-Hermitian solver's opt-in fp32 H^2 filter (h2_mixed_precision) on the CPU: the emulation of
tests/h2_mixed_ref.py over the oracle on both reference BSE fixtures, and the numpy reference of axpy_sp against its own bound.
No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import h2_mixed_ref as R  # noqa: E402


@pytest.mark.parametrize("kind,nev,nex", R.CASES, ids=["%s-%d-%d" % c for c in R.CASES])
def test_emulated_mixed_solve(kind, nev, nex):
    r = R.emulated(kind, nev, nex)
    d, m = r["fp64"], r["mixed"]
    print(f"{kind} {nev}/{nex}: fp64 {d['iterations']} iterations / {d['filtered_vecs']} filtered vectors, mixed "
          f"{m['iterations']} / {m['filtered_vecs']}, {m['hemm_sp_calls']} of {m['hemm_sp_calls'] + m['hemm_calls']} products in "
          f"fp32, max residual {m['max_resid']:.2e}, eigenvalue error {m['eig_err']:.2e}")
    assert d["hemm_sp_calls"] == 0 and d["sp_filters"] == 0 and d["sp_h_converts"] == 0
    assert m["locked"] >= nev
    assert m["max_resid"] <= 1e-10
    assert m["eig_err"] <= 1e-9
    assert m["hemm_sp_calls"] > 0 and m["sp_filters"] >= 1          # at least one call in fp32 ...
    assert m["hemm_calls"] > 0                                        # ... and at least one in fp64
    assert m["sp_h_converts"] == 1                                    # H is rounded once per matrix
    assert m["iterations"] <= d["iterations"] + 1


def test_emulation_with_the_switch_off_is_the_oracle():
    from oracle import chase_oracle as O
    H, _ = R.fixture("complex")
    a = R.OraclePseudoMixed(H, 12, 8, mixed=False)
    b = O.OraclePseudoCPU(H, 12, 8)
    for k in (a, b):
        k.config.num_lanczos, k.config.lanczos_iter = 10, 50
    sa, sb = R.solve_pseudo(a), O.solve_pseudo(b)
    assert sa == sb and a.ritzv.tobytes() == b.ritzv.tobytes() and a.V1.tobytes() == b.V1.tobytes()
    assert O.filter_H2.__name__ == "filter_H2"                        # the bracket is gone after the solve


@pytest.mark.parametrize("cplx", [False, True])
def test_axpy_sp_reference_within_its_bound(cplx):
    rng = np.random.default_rng(5)
    m, n = 133, 5
    scale = 10.0 ** rng.integers(-6, 6, (m, n))
    X = rng.standard_normal((m, n)) * scale
    Y = rng.standard_normal((m, n)) * scale
    if cplx:
        X = X + 1j * rng.standard_normal((m, n)) * scale
        Y = Y + 1j * rng.standard_normal((m, n))
    st = np.complex64 if cplx else np.float32
    X, Y = X.astype(st), Y.astype(st)
    for gamma in ([-0.2, 1.75, 0.0] if not cplx else [-0.2, 0.3 - 0.7j, 1.1j]):
        got = R.axpy_sp_ref(gamma, X, Y)
        assert got.dtype == st
        worst = R.axpy_sp_within_bound(gamma, X, Y, got)
        print(f"axpy_sp reference {'c' if cplx else 's'} gamma={gamma}: max err / bound = {worst:.3f}")
        assert worst <= 1.0
    # the bound is not slack by orders of magnitude: an update whose gamma is off by 2^-20 (16 ulp) exceeds it
    g = 0.3 - 0.7j if cplx else 1.75
    off = R.axpy_sp_ref(st(g) * st(1 + 2.0 ** -20), X, Y)
    assert R.axpy_sp_within_bound(g, X, Y, off) > 1.0
    # gamma = 0 leaves Y as it is, bit for bit
    assert R.axpy_sp_ref(0.0, X, Y).tobytes() == Y.tobytes()
