#!/usr/bin/env python3
"""Record what the cached derivative fills return into tests/golden/dense_deriv_parent.json, the file
tests/test_gpu_dense_deriv_frozen.py replays.  Run it at the commit whose results are to be frozen (the parent of a
change to emme_amd/csrc/assemble_dense_deriv_text.hpp or its two units), never at the commit under test; EMME_LIB may
name a library built elsewhere.

A case is one assemble_derivative(WS10, want_intervals=True) on a context of its own, with derivative cache shapes ALL:
SHA-256 digests of the bytes of M and of M', the interval counts, the tile tasks and the number of integrals handed to
the list kernel.  Digests, not arrays: the file stays a few KB.  Four shapes -- es15 is example_tokamak(npoints=28): 378
pairs, 24 tiles with the last one partial, a chunk of 8 omegas beside a chunk of 2; em31, em15 (14 points: 91 pairs, 6
tiles, the second workgroup with two waves) and es31 are SHAPES of tests/test_gpu_dense_shape_deriv.py -- times two
option sets: "default" (node_cache_gb = 8, deriv_cached = 1, the cache settled on the omegas first) and "shallow" (the
options of test_leaving_the_cache_shallow_cache: a budget that holds the shallowest cache shape only, so that integrals
leave the cache and the list launchers run; the fill is the context's first call and builds the cache itself).

Without --child the tool starts itself twice as a child process (two processes: two independent runs), compares the two
and writes the first together with `not_reproduced`, the "case.key" names whose two runs differ.

FROZEN WITH THE FILE: the test loads this module by path and replays the cases through CASES, WS10 and run_case.
Whoever edits one of them changes what that test replays: record the file again, or leave them alone."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "dense_deriv_parent.json")

# the ten omegas of tests/test_gpu_dense_shape_deriv.py: both contour classes, a damped one
WS10 = np.array([-0.8 + 0.25j, -0.6 - 0.21j, 0.5 + 0.1j, -1.656 + 2.49j, 0.153 - 0.316j, -0.7 + 0.3j, -0.9 + 0.1j,
                 -0.5 + 0.2j, -0.65 + 0.27j, -1.0 + 0.05j])
# shape: (model, its arguments, GiB of the shallow budget: 24 tiles x 8 KB, 6 x 16 KB, 6 x 8 KB, 24 x 16 KB per interval)
SHAPES = {
    "es15": ("tokamak", dict(npoints=28), 0.03),
    "em31": ("stellarator", dict(npoints=14), 0.015),
    "em15": ("stellarator", dict(npoints=14, integration_start_points=15), 0.008),
    "es31": ("tokamak", dict(npoints=28, integration_start_points=31), 0.06),
}
# the suite's contexts (tests/conftest.py): the node cache serves calls of any size
OPTIONS = dict(cache_min_batch=1)
CASES = [(shape, opts) for shape in SHAPES for opts in ("default", "shallow")]
KEYS = ("M_sha256", "Mp_sha256", "intervals", "tile_tasks", "handed_over")


def model_dict(shape):
    from oracle.binding import example_stellarator, example_tokamak
    model, kw, _ = SHAPES[shape]
    return (example_tokamak if model == "tokamak" else example_stellarator)(**kw)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(emme, shape, opts):
    """{key: value} of one case, on a fresh context"""
    if opts == "default":
        options = dict(node_cache_gb=8.0, deriv_cached=1)
    else:
        options = dict(node_cache_gb=SHAPES[shape][2], cache_min_depth=1, wl_min=1, deriv_cached=1)
    with emme.Context(emme.params_from_dict(model_dict(shape)), device=0, **OPTIONS, **options) as ctx:
        ctx.set_deriv_cache_shapes(emme.DERIV_CACHE_SHAPES_ALL)
        if opts == "default":
            ctx.cache_settle(WS10)
        ctx.profile(True)
        ctx.profile_read(reset=True)
        M, Mp, iv = ctx.assemble_derivative(WS10, want_intervals=True)
        pr = ctx.profile_read(reset=True)
        handed = int(ctx.last_deferred())
    return {"M_sha256": _sha(M), "Mp_sha256": _sha(Mp), "intervals": [int(x) for x in iv],
            "tile_tasks": int(pr.tile_tasks), "handed_over": handed}


def record(emme, out):
    data = {}
    for shape, opts in CASES:
        got = run_case(emme, shape, opts)
        print(shape, opts, got, flush=True)
        data[f"{shape}-{opts}"] = got
    with open(out, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--child", action="store_true", help="one run, written to --out as it is")
    a = ap.parse_args()
    if a.child:
        import emme_amd
        emme_amd.load()
        record(emme_amd, a.out)
        return
    with tempfile.TemporaryDirectory() as tmp:
        runs = []
        for k in range(2):
            path = os.path.join(tmp, f"run{k}.json")
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", "--out", path])
            with open(path) as f:
                runs.append(json.load(f))
    first, second = runs
    assert first.keys() == second.keys()
    differ = [f"{case}.{k}" for case in first for k in KEYS if first[case][k] != second[case][k]]
    for k in differ:
        print("the two runs differ in", k, flush=True)
    print(f"{len(first) * len(KEYS) - len(differ)} of {len(first) * len(KEYS)} values agree between the two runs")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(first, not_reproduced=differ), f, indent=1)
        f.write("\n")
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
