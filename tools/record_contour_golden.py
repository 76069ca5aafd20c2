#!/usr/bin/env python3
"""Record what the contour entry points return into tests/golden/contour_parent.npz, the file
tests/test_gpu_contour_frozen.py replays.  Run it at the commit whose results are to be frozen (the parent of a refactor
of emme_amd/csrc/contour.hip), never at the commit under test.

Every case runs on a fresh context and is the first contour call on that context (the node cache makes later calls
differ).  Moments cases: the inputs of test_moments_groups_match_numpy_and_the_ungrouped_call (tests/
test_gpu_contour_sets.py) for n = 5 and 64, internal probes, L = 1, 8, 64, through contour_moments on all 16 matrices
and through contour_moments_groups with GROUP.  Search cases, all through find_roots_in_contour: see SEARCH_CASES.

Without --child the tool starts itself twice as a child process (two processes: two independent runs), compares the
two runs array by array and writes the first run together with `not_reproduced`, the names of the arrays whose two runs
differ in any bit.  The circles of the search cases come from the lattice helpers of tests/test_gpu_contour.py, on a
context of their own, and are stored so that the test does not recompute them.

FROZEN WITH THE FILE: tests/test_gpu_contour_frozen.py loads this module by path and replays the cases through
GROUP, MOMENT_N, MOMENT_L, OPTIONS, SEARCH_CASES, model_dict, moment_inputs, run_moments and run_search.  Whoever edits
one of them changes what that test replays: record the file again at the commit it freezes, or leave them alone."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "contour_parent.npz")

# sizes 1, 4, 11 and 0, interleaved; matrix 5 (exactly singular) is in the group of 11 (tests/test_gpu_contour_sets.py)
GROUP = np.array([2, 1, 2, 2, 1, 2, 0, 2, 2, 1, 2, 2, 2, 1, 2, 2], dtype=np.int32)
MOMENT_N, MOMENT_L = (5, 64), (1, 8, 64)
# the suite's contexts (tests/conftest.py): the node cache serves calls of any size
OPTIONS = dict(cache_min_batch=1)
# name: (model, circle, context options, contour settings).  b forces midpoint rounds (a count >= 1 cannot resolve on 4
# nodes) and L doublings (one probe, four roots inside); c stays unresolved at its cap; e has a node cache, which
# serves its nodes, f has none, so that its nodes go through the tile fill
SEARCH_CASES = {
    "a": ("tokamak", "tokamak", {}, {}),
    "b": ("tokamak", "tokamak", {}, dict(points=4, probes=1)),
    "c": ("tokamak", "tokamak", {}, dict(points=4, max_points=8)),
    "d": ("stellarator", "stellarator", {}, {}),
    "e": ("tokamak", "tokamak", dict(tile_uncached=1), {}),
    "f": ("tokamak", "tokamak", dict(tile_uncached=1, node_cache_gb=0), {}),
}
SEARCH_KEYS = ("roots", "iters", "info", "n_roots", "winding", "points_used", "complete")
LATTICE = {"tokamak": (np.linspace(-1.2, -0.4, 8), np.linspace(-0.3, 0.4, 8)),
           "stellarator": (np.linspace(-2.2, -1.1, 8), np.linspace(1.9, 3.1, 8))}


def model_dict(model):
    from oracle.binding import example_stellarator, example_tokamak
    return example_tokamak(npoints=32) if model == "tokamak" else example_stellarator(npoints=32)


def moment_inputs(n):
    rng = np.random.default_rng(n)
    nq = 16
    M = (rng.standard_normal((nq, n, n)) + 1j * rng.standard_normal((nq, n, n))) / np.sqrt(n)
    M += np.eye(n)[None]
    M[5, :, 0] = 0.0  # exactly singular: factorisation stops at column 1
    z = rng.standard_normal(nq) + 1j * rng.standard_normal(nq)
    w = rng.standard_normal(nq) + 1j * rng.standard_normal(nq)
    return M, z, w


def run_moments(emme, n, L, call):
    """{name: array} of one moments case: call = "batch" (contour_moments on all 16 matrices) or "groups" """
    import bench
    M, z, w = moment_inputs(n)
    with emme.Context(emme.params_from_dict(bench.workload_dict(32)), device=0, **OPTIONS) as ctx:
        if call == "batch":
            A0, A1, ld, info = ctx.contour_moments(M, z, w, L)
        else:
            A0, A1, ld, info = ctx.contour_moments_groups(M, GROUP, 4, z, w, L)
    stem = f"moments_n{n}_L{L}_{call}_"
    return {stem + "A0": A0, stem + "A1": A1, stem + "logdet": ld, stem + "info": info}


def run_search(emme, name, center, radius):
    """{name: array} of one search case on the circle (center, radius)"""
    model, _, options, settings = SEARCH_CASES[name]
    with emme.Context(emme.params_from_dict(model_dict(model)), device=0, **{**OPTIONS, **options}) as ctx:
        res = ctx.find_roots_in_contour(complex(center), (float(radius), float(radius)), **settings)
    return {f"search_{name}_{k}": np.asarray(res[k]) for k in SEARCH_KEYS}


def circles(emme):
    """The circle of every model: the pair circle of its lattice roots, else around the most isolated lattice root a
    circle of half the distance to its neighbour (test_contour_matches_own_lattice_small)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_contour import _lattice_roots, _pair_circle
    out = {}
    for model, (re, im) in LATTICE.items():
        with emme.Context(emme.params_from_dict(model_dict(model)), device=0, **OPTIONS) as ctx:
            lat = _lattice_roots(ctx, re, im)
        assert len(lat) >= 1, f"the lattice found no root of {model}"
        circ = _pair_circle(lat)
        if circ is None:
            near = [np.sort(np.abs(lat - x))[1] if len(lat) > 1 else np.inf for x in lat]
            k = int(np.argmax(near))
            circ = (lat[k], min(0.5 * near[k], 0.9 * abs(lat[k].real), 0.3))
        out[f"circle_{model}_center"] = np.complex128(circ[0])
        out[f"circle_{model}_radius"] = np.float64(circ[1])
    return out


def record(emme, out):
    data = circles(emme)
    for n in MOMENT_N:
        for L in MOMENT_L:
            for call in ("batch", "groups"):
                data.update(run_moments(emme, n, L, call))
    for name, (_, circle, _, settings) in SEARCH_CASES.items():
        got = run_search(emme, name, data[f"circle_{circle}_center"], data[f"circle_{circle}_radius"])
        print(name, settings, {k: got[f"search_{name}_{k}"].tolist() for k in SEARCH_KEYS}, flush=True)
        data.update(got)
    b = SEARCH_CASES["b"][3]
    data["search_b_points"], data["search_b_probes"] = np.int32(b["points"]), np.int32(b["probes"])
    assert data["search_b_points_used"] > b["points"], "case b took no midpoint round: lower its points"
    np.savez_compressed(out, **data)


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
            path = os.path.join(tmp, f"run{k}.npz")
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", "--out", path])
            with np.load(path) as f:
                runs.append({k: f[k] for k in f.files})
    first, second = runs
    assert first.keys() == second.keys()
    differ = [k for k in first
              if first[k].shape != second[k].shape or np.ascontiguousarray(first[k]).tobytes() != np.ascontiguousarray(second[k]).tobytes()]
    for k in differ:
        print("the two runs differ in", k, flush=True)
    print(f"{len(first) - len(differ)} of {len(first)} arrays agree bit for bit between the two runs")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, not_reproduced=np.array(differ, dtype="U64"), **first)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
