"""The premises of test_gpu_range_edge.py, recomputed from the oracle alone for every (shape, N, set, omega) of
tests/range_edge_cases.py.  These are conditions, not measurements: a GPU assertion never rests on a premise that nobody
checked.

  in range   the oracle's matrix is finite, every integral's |Re| and |Im| is <= 1e148 (two decades inside
             EMME_MAX_ENTRY) and the interval total is the same at omega (1 +- 1e-13)
  sharp      and the oracle's matrix moves by <= 1e-9 max|M| under omega (1 + 1e-13)
  beyond     the oracle's matrix is finite and at least one integral's |Re| or |Im| is >= 1e152
  lost       the oracle's matrix holds a non-finite entry
"""
import numpy as np
import pytest

import range_edge_cases as rc


def _id(case):
    shape, n, second, role, w = case
    return f"{shape}-N{n}-set{int(second)}-{role}"


@pytest.mark.parametrize("case", rc.cases(), ids=_id)
def test_premises_hold_in_the_oracle(case):
    shape, n, second, role, w = case
    M, tot = rc.oracle_fill(shape, n, second, w)
    if role == "lost":
        assert not np.isfinite(M.view(np.float64)).all(), (shape, n, w)
        return
    assert np.isfinite(M.view(np.float64)).all(), (shape, n, w)
    comp = rc.oracle_comp(shape, n, second, w)
    print(f"{shape} N={n} {role} {w}: max|M| {np.abs(M).max():.3g}, comp max {comp.max():.3g}, intervals {tot}")
    if role == "beyond":
        assert comp.max() >= rc.BEYOND_COMP, (shape, n, w, comp.max())
        return
    assert role in rc.IN_RANGE
    assert comp.max() <= rc.IN_RANGE_COMP, (shape, n, w, comp.max())
    spread, same_tree = rc.oracle_spread(shape, n, second, w)
    print(f"    spread {spread:.3g}")
    assert same_tree, (shape, n, w)
    if role in rc.SHARP:
        assert spread <= rc.SHARP_SPREAD, (shape, n, w, spread)


@pytest.mark.parametrize("shape", sorted(rc.SHAPES))
def test_derivative_reference_walks_one_tree(shape):
    """The Richardson reference of M' (section B of the GPU test): every oracle fill at omega +- h, omega +- h/2 along
    both axes has the interval total of omega itself, M' is about 300 M -- so the sharp_large omega, not the edge, is
    where M' stays in range -- and the two extrapolations agree to a few 1e-11 (measured: 1.8e-11 .. 6.5e-11)."""
    for n in rc.grids(shape):
        Mp, disagreement, same_tree = rc.oracle_derivative(shape, n)
        M, _ = rc.oracle_fill(shape, n, False, complex(rc.OMEGAS[shape]["sharp_large"]))
        print(f"{shape} N={n}: max|M'| {np.abs(Mp).max():.3g} = {np.abs(Mp).max() / np.abs(M).max():.3g} max|M|, "
              f"Re/Im extrapolations disagree by {disagreement:.3g}")
        assert same_tree, (shape, n)
        assert np.isfinite(Mp.view(np.float64)).all() and np.abs(Mp).max() < rc.IN_RANGE_COMP
        assert disagreement <= 1e-9, (shape, n, disagreement)  # (the GPU bar is 10 x this: it stays a tight one)


@pytest.mark.parametrize("key", sorted(rc.RECORDED), ids=lambda k: "-".join(k))
def test_recorded_figures_are_the_oracles(key):
    """The table the cases were chosen from (smallest grid, set 0): interval totals exactly, max|M| to its two digits."""
    shape, role = key
    maxabs, intervals = rc.RECORDED[key]
    M, tot = rc.oracle_fill(shape, rc.grids(shape)[0], False, complex(rc.OMEGAS[shape][role]))
    assert tot == intervals, (key, tot)
    if maxabs is None:
        assert not np.isfinite(M.view(np.float64)).all()
    else:
        assert abs(np.abs(M).max() / maxabs - 1.0) <= 0.05, (key, np.abs(M).max())
