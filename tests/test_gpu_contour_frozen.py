"""The contour entry points against what they returned before search_contours became the one driver of both region
searches and k_contour_moments_groups the one moments kernel.

tests/golden/contour_parent.npz was written by tools/record_contour_golden.py at the parent of that change, from the
old single search, k_contour_solve<G, false> and k_contour_moments; this file replays every recorded case the way the
recorder ran it -- a fresh context per case, the case its first contour call -- and compares.  Integers are equal.  A
float array is equal bit for bit unless the recorder's two runs, in two processes, differed in it (`not_reproduced` in
the file: empty, all 96 arrays reproduced); such an array would be held to the bounds of the existing tests instead:
1e-13 relative in the Frobenius norm for A0 / A1, 1e-10 for log-dets, 10 tol |omega| for roots.  Nothing the code under
test computes is an expected value here."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_contour_golden", os.path.join(ROOT, "tools", "record_contour_golden.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "contour_parent.npz")) as f:
        data = {k: f[k] for k in f.files}
    for v in data.values():
        v.setflags(write=False)
    return data


def _compare(golden, got, tol=None):
    loose = set(golden["not_reproduced"].tolist())
    for key, have in got.items():
        want = golden[key]
        have = np.asarray(have)
        print(f"{key}: bit-equal {have.shape == want.shape and have.tobytes() == want.tobytes()}")
        assert have.shape == want.shape and have.dtype == want.dtype, key
        if key not in loose or not np.issubdtype(want.dtype, np.inexact):
            assert have.tobytes() == want.tobytes(), key
        elif key.endswith(("_A0", "_A1")):
            assert np.linalg.norm(have - want) <= 1e-13 * np.linalg.norm(want), key
        elif key.endswith("_logdet"):
            ok = np.isfinite(want.real)
            assert np.array_equal(ok, np.isfinite(have.real)), key
            assert np.all(np.abs(have[ok].real - want[ok].real) <= 1e-10 * np.maximum(1.0, np.abs(want[ok].real))), key
            assert np.all(np.abs(np.angle(np.exp(1j * (have[ok].imag - want[ok].imag)))) <= 1e-10), key
        else:
            assert key.endswith("_roots"), key
            assert np.all(np.abs(have - want) <= 10 * tol * np.abs(want)), key


@pytest.mark.parametrize("call", ["batch", "groups"])
@pytest.mark.parametrize("L", rec.MOMENT_L)
@pytest.mark.parametrize("n", rec.MOMENT_N)
def test_moments_return_what_the_parent_returned(emme, golden, n, L, call):
    got = rec.run_moments(emme, n, L, call)
    assert set(got) == {k for k in golden if k.startswith(f"moments_n{n}_L{L}_{call}_")}
    assert got[f"moments_n{n}_L{L}_{call}_info"][5] > 0  # the singular matrix is left out, as recorded
    _compare(golden, got)


@pytest.mark.parametrize("name", sorted(rec.SEARCH_CASES))
def test_search_returns_what_the_parent_returned(emme, golden, name):
    circle = rec.SEARCH_CASES[name][1]
    got = rec.run_search(emme, name, golden[f"circle_{circle}_center"], golden[f"circle_{circle}_radius"])
    assert set(got) == {k for k in golden if k.startswith(f"search_{name}_") and k not in ("search_b_points", "search_b_probes")}
    _compare(golden, got, tol=emme.params_from_dict(rec.model_dict(rec.SEARCH_CASES[name][0])).iteration_precision)


def test_the_recorded_cases_take_every_path(golden):
    """what keeps the comparison from passing on nothing: midpoint rounds and L doublings in b (one probe, four roots:
    L went 1, 2, 4, 8 at the parent), an unresolved count at the cap in c, roots everywhere"""
    b = rec.SEARCH_CASES["b"][3]
    assert (golden["search_b_points"], golden["search_b_probes"]) == (b["points"], b["probes"]) == (4, 1)
    assert golden["search_b_points_used"] > 4 and golden["search_b_n_roots"] > 1
    assert golden["search_c_winding"] == -1 and golden["search_c_points_used"] == 8 and not golden["search_c_complete"]
    for name in rec.SEARCH_CASES:
        assert golden[f"search_{name}_n_roots"] >= 1
        if name != "c":
            assert golden[f"search_{name}_complete"] and golden[f"search_{name}_winding"] == golden[f"search_{name}_n_roots"]
    assert golden["search_d_points_used"] > 32  # the electromagnetic case doubles its nodes too
    # the tile fill's matrices are not the node cache's: f is a case of its own
    assert golden["search_f_roots"].tobytes() != golden["search_a_roots"].tobytes()
