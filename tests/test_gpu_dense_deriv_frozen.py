"""The cached derivative fills against what they returned before k_assemble_dense_deriv and
k_assemble_dense_shape_deriv<PTS, NM> became two readings of one text (assemble_dense_deriv_text.hpp).

The device code of that change is its parent's, instruction for instruction; what can differ is what the merged
launchers hand the kernels -- arguments and grids.  tests/golden/dense_deriv_parent.json was written by
tools/record_dense_deriv_golden.py on a library built at the parent: per case SHA-256 digests of the bytes of M and of
M', the interval counts, the tile tasks and the number of integrals handed to the list kernel.  The recorder ran every
case in two processes and every value reproduced (`not_reproduced` in the file is empty), so this file replays each case
the way the recorder ran it -- a fresh context per case -- and compares value for value.  Nothing the code under test
computes is an expected value here."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_dense_deriv_golden",
                                               os.path.join(ROOT, "tools", "record_dense_deriv_golden.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "dense_deriv_parent.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("shape,opts", rec.CASES, ids=[f"{s}-{o}" for s, o in rec.CASES])
def test_fill_returns_what_the_parent_returned(emme, golden, shape, opts):
    assert golden["not_reproduced"] == []
    want = golden[f"{shape}-{opts}"]
    got = rec.run_case(emme, shape, opts)
    for k in rec.KEYS:
        print(f"{shape}-{opts} {k}: equal {got[k] == want[k]}")
    assert got["tile_tasks"] > 0, "the derivative fill did not go through the cached kernel"
    for k in rec.KEYS:
        assert got[k] == want[k], (k, got[k], want[k])


def test_the_recorded_cases_take_every_path(golden):
    """what keeps the comparison from passing on nothing: every case ran tile tasks, at least a chunk per tile; the
    shallow cases handed integrals to the list kernels; es15 has a partial second chunk (10 omegas: 8 + 2)"""
    assert sorted(k for k in golden if k != "not_reproduced") == sorted(f"{s}-{o}" for s, o in rec.CASES)
    ntiles = {"es15": 24, "em31": 6, "em15": 6, "es31": 24}
    for shape, opts in rec.CASES:
        g = golden[f"{shape}-{opts}"]
        assert len(g["intervals"]) == 10 and min(g["intervals"]) > 0
        assert g["tile_tasks"] >= 2 * ntiles[shape] and g["tile_tasks"] % ntiles[shape] == 0
        if opts == "shallow":
            assert g["handed_over"] > 0
        assert g["M_sha256"] != g["Mp_sha256"]
