"""The folded trace-secant formula on the oracle's matrices, on the CPU: the even and the odd block
of order N / 2 plus the rank-2 correction of the SingularityHandler's last-column rule give tr(M^-1 M') to rounding, and
without the correction they do not -- so the first check exercises that term and not a sum that is right by accident.

Measured (tokamak example, omega = -0.8 + 0.25i, d omega = 0.01 omega): N = 24: 2.1e-14 with, 2.9e-4 without the
rank-2 term; N = 64: 9.4e-15 and 1.6e-5."""
import numpy as np
import pytest

from fold_reference import folded_trace, structured_pair
from oracle.binding import example_tokamak

W = -0.8 + 0.25j


@pytest.mark.parametrize("n", [24, 64])
def test_folded_formula_on_oracle_matrices(oracle, n):
    po = oracle.params(example_tokamak(npoints=n))
    dw = 0.01 * W
    M_old, _ = oracle.assemble(po, W)
    M, _ = oracle.assemble(po, W + dw)
    want = np.trace(np.linalg.solve(M, (M - M_old) / dw))
    got = folded_trace(M, M_old, dw)
    bare = folded_trace(M, M_old, dw, rank2=False)
    err, err_bare = abs(got - want) / abs(want), abs(bare - want) / abs(want)
    print(f"folded formula N={n}: rel err {err:.3g}, without the rank-2 term {err_bare:.3g}")
    assert err <= 1e-12, (n, err)
    assert err_bare > 1e-6, (n, err_bare)


@pytest.mark.parametrize("n", [2, 4, 30])
def test_folded_formula_on_structured_matrices(n):
    """The generator test_gpu_fold.py uses gives what the formula is for."""
    rng = np.random.default_rng(7 + n)
    M, M_old = structured_pair(rng, n)
    dw = 0.3 - 0.2j
    want = np.trace(np.linalg.solve(M, (M - M_old) / dw))
    got = folded_trace(M, M_old, dw)
    assert abs(got - want) <= 1e-12 * abs(want), (n, got, want)
