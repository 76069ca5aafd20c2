"""The kernels that solve on the factors of an in-place LU against what they returned before they shared one workgroup
frame (tri_solve.hpp: one LDS layout, one block_sum, one start vector) and the folded steps one host driver (DESIGN.md
§5.4c, §14, §14.2).

tests/golden/solver_parent.json was written by tools/record_solver_golden.py on a library built at the parent of that
change: per case the SHA-256 digest of the bytes of every array the call returns, and the info codes, iteration counts
and folded-step counters themselves.  The recorder ran every case in two processes and every value reproduced
(`not_reproduced` in the file is empty), so this file replays each case the way the recorder ran it and compares value
for value.  Nothing the code under test computes is an expected value here."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_solver_golden", os.path.join(ROOT, "tools", "record_solver_golden.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

IDS = [rec.case_id(c) for c in rec.CASES]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "solver_parent.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ctx(emme):
    from oracle.binding import example_tokamak
    with emme.Context(emme.params_from_dict(example_tokamak(npoints=16)), device=0, **rec.OPTIONS) as c:
        yield c


@pytest.mark.parametrize("case", rec.CASES, ids=IDS)
def test_solver_returns_what_the_parent_returned(emme, ctx, golden, case):
    assert golden["not_reproduced"] == []
    want = golden[rec.case_id(case)]
    got = rec.run_case(emme, ctx, case)
    for k in want:
        print(f"{rec.case_id(case)} {k}: equal {got[k] == want[k]}")
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])


def test_the_recorded_cases_take_every_path(golden):
    """what keeps the comparison from passing on nothing: the file holds the recorder's cases and no others; the items
    made singular came back with a code and every other item with none; both searches counted folded steps"""
    assert sorted(k for k in golden if k != "not_reproduced") == sorted(IDS)
    n_singular = 0
    for case in rec.CASES:
        g = golden[rec.case_id(case)]
        call, n, _ = case
        n_singular += g["singular"] is not None
        if call in ("solve_roots", "solve_eigenpairs_secant"):  # (a chain of a search may fail: its code is compared too)
            assert len(g["info"]) == 6 and g["info"].count(0) >= 5
            continue
        for b, code in enumerate(g["info"]):
            assert (code != 0) == (b == g["singular"]), (rec.case_id(case), g["info"])
        if n == 1026:
            assert len(g["info"]) == 1
        else:
            assert len(g["info"]) == 3 and (g["singular"] == 1 or (n == 2 and call.endswith(("folded", "folded_step"))))
    assert n_singular == len(rec.CASES) - 5  # (the two searches, n = 1026 and the two folded cases of order 2)
    assert golden["solve_roots-n24-fold"]["folded_steps"][0] >= 1
    assert golden["solve_eigenpairs_secant-n24-fold"]["folded_steps"][1] >= 1
