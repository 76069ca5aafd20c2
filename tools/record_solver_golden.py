#!/usr/bin/env python3
"""Record what the kernels that solve on the factors of an in-place LU return (k_null_iterate, the two eigenpair step
kernels, k_fold_solve / k_fold_combine, k_eigpair_fold_half / k_eigpair_fold_combine: tri_solve.hpp and its readers) into
tests/golden/solver_parent.json, the file tests/test_gpu_solver_frozen.py replays.  Run it at the commit whose results
are to be frozen (the parent of a change to those files or to the host drivers above them), never at the commit under
test; EMME_LIB may name a library built elsewhere.

A case is one call on the seeded inputs of tests/linalg_cases.py; what is kept of it is the SHA-256 digest of the bytes
of every array it returns, and the info codes and counters themselves (a few small integers).  Batch 3, item 1 made
exactly singular where the family has a construction for it (a zero column; linalg_cases.with_singular_half):
  null_vectors, eigenpair_step, eigenpair_secant_step   n = 1, 2, 17, 33, 65, 514, 530 -- one row, the 16-row block edge,
      the 32-row snapshot edge, the 64-lane edge, the 512-thread stride, the chunked factorisation's maps; the two steps
      with v given ("v") and with v = None ("s": the step makes v_0 = M^-1 s / |M^-1 s| first)
  eigenpair_step n = 1026, one item, v = None           the unblocked factorisation's single snapshot
  trace_secant_folded, eigenpair_secant_folded_step     n = 2, 4, 34, 66, 130, 1030 (n = 2: no singular item, a half of
      order 1 has no row to spare)
  solve_eigenpairs(secant=True) with eigpair_fold on, solve_roots with lu_fold on     N = 24, six guesses: roots, vectors,
      residuals, iteration counts, info and the two folded-step counters (the live-list staging, the residual-only launch)

Without --child the tool starts itself twice as a child process (two processes: two independent runs), compares the two
and writes the first together with `not_reproduced`, the "case.key" names whose two runs differ.

FROZEN WITH THE FILE: the test loads this module by path and replays the cases through CASES and run_case.  Whoever edits
one of them changes what that test replays: record the file again, or leave them alone."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "solver_parent.json")

STEP_ORDERS = [1, 2, 17, 33, 65, 514, 530]
FOLD_ORDERS = [2, 4, 34, 66, 130, 1030]
DOMEGA = np.array([1e-2 * np.exp(0.7j), 1e-7 * np.exp(-2.1j), 3e-3 * np.exp(2.9j)])
# the first six guesses of the 16-guess secant search of tests/test_gpu_fold.py
GUESSES = np.array([-0.7249 + 0.1803j, -0.5617 + 0.3641j, -0.6346 + 0.2529j, -0.9649 + 0.3541j, -0.9199 + 0.2919j,
                    -0.5759 + 0.3225j])
# the suite's contexts (tests/conftest.py): the node cache serves calls of any size
OPTIONS = dict(cache_min_batch=1)

# (call, order, variant)
CASES = ([("null_vectors", n, "") for n in STEP_ORDERS] +
         [(call, n, v) for call in ("eigenpair_step", "eigenpair_secant_step") for n in STEP_ORDERS for v in ("v", "s")] +
         [("eigenpair_step", 1026, "s")] +
         [(call, n, "") for call in ("trace_secant_folded", "eigenpair_secant_folded_step") for n in FOLD_ORDERS] +
         [("solve_eigenpairs_secant", 24, "fold"), ("solve_roots", 24, "fold")])


def case_id(case):
    call, n, variant = case
    return f"{call}-n{n}" + (f"-{variant}" if variant else "")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _unit_vectors(n, nb):
    """nb unit vectors: the start vector s of include/emme_hip.h, rolled by the item's index"""
    import linalg_cases as lc
    v = np.array([np.roll(lc.start_vector(n), b) for b in range(nb)])
    return v / np.linalg.norm(v, axis=1)[:, None]


def _step_inputs(n):
    """(M with column min(5, n - 1) of item 1 zero, the second operand, the singular item) of the three-item batches; the
    one item of n = 1026 is regular"""
    import linalg_cases as lc
    nb = 1 if n == 1026 else 3
    A, B, _ = lc.shifted_symmetric(n, nb=nb)
    M = A.copy()
    if nb == 3:
        M[1][:, min(5, n - 1)] = 0.0
    return M, B, (1 if nb == 3 else None)


def _fold_inputs(n):
    """(M, M_old, domega, the singular item): fold_inputs(n, 3), the even half of item 1 with row and column
    min(5, n / 2 - 1) exactly zero (n >= 4)"""
    import linalg_cases as lc
    M, Mo, dw, _ = lc.fold_inputs(n, 3)
    M = M.copy()
    if n < 4:
        return M, Mo, dw, None
    M[1] = lc.with_singular_half(M[1], min(5, n // 2 - 1), False)
    return M, Mo, dw, 1


def run_case(emme, ctx, case):
    """{key: value} of one case.  ctx: a context for the calls on caller matrices (any model; the searches make their
    own).  `singular` is the item made singular (or None), `info` the codes as they came back."""
    from oracle.binding import example_tokamak
    call, n, variant = case
    if call == "null_vectors":
        M, _, sing = _step_inputs(n)
        vecs, info = ctx.null_vectors(M)
        return {"vecs_sha256": _sha(vecs), "info": info.tolist(), "singular": sing}
    if call in ("eigenpair_step", "eigenpair_secant_step"):
        M, B, sing = _step_inputs(n)
        v = _unit_vectors(n, len(M)) if variant == "v" else None
        if call == "eigenpair_step":
            out = ctx.eigenpair_step(M, B, v)
        else:
            out = ctx.eigenpair_secant_step(M, B, DOMEGA[:len(M)], v)
        return {"vecs_sha256": _sha(out[0]), "tau_sha256": _sha(out[1]), "resid_sha256": _sha(out[2]),
                "info": out[3].tolist(), "singular": sing}
    if call == "trace_secant_folded":
        M, Mo, dw, sing = _fold_inputs(n)
        tr, info = ctx.trace_secant_folded(M, Mo, dw)
        return {"tr_sha256": _sha(tr), "info": info.tolist(), "singular": sing}
    if call == "eigenpair_secant_folded_step":
        M, Mo, dw, sing = _fold_inputs(n)
        out = ctx.eigenpair_secant_folded_step(M, Mo, dw, _unit_vectors(n, 3))
        return {"vecs_sha256": _sha(out[0]), "tau_sha256": _sha(out[1]), "resid_sha256": _sha(out[2]),
                "info": out[3].tolist(), "singular": sing}
    params = emme.params_from_dict(example_tokamak(npoints=n))
    if call == "solve_eigenpairs_secant":
        with emme.Context(params, device=0, eigpair_fold=1, **OPTIONS) as c:
            roots, vecs, resid, iters, info = c.solve_eigenpairs(GUESSES, secant=True)
            counters = [int(c.last_folded_steps()), int(c.last_folded_eigpair_steps())]
        return {"roots_sha256": _sha(roots), "vecs_sha256": _sha(vecs), "resid_sha256": _sha(resid),
                "iters": iters.tolist(), "info": info.tolist(), "folded_steps": counters, "singular": None}
    assert call == "solve_roots"
    with emme.Context(params, device=0, lu_fold=1, **OPTIONS) as c:
        roots, iters, info = c.solve_roots(GUESSES)
        counters = [int(c.last_folded_steps()), int(c.last_folded_eigpair_steps())]
    return {"roots_sha256": _sha(roots), "iters": iters.tolist(), "info": info.tolist(), "folded_steps": counters,
            "singular": None}


def record(emme, out):
    from oracle.binding import example_tokamak
    data = {}
    with emme.Context(emme.params_from_dict(example_tokamak(npoints=16)), device=0, **OPTIONS) as ctx:
        for case in CASES:
            got = run_case(emme, ctx, case)
            print(case_id(case), got, flush=True)
            data[case_id(case)] = got
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
    differ = [f"{case}.{k}" for case in first for k in first[case] if first[case][k] != second[case][k]]
    for k in differ:
        print("the two runs differ in", k, flush=True)
    total = sum(len(v) for v in first.values())
    print(f"{total - len(differ)} of {total} values agree between the two runs")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(first, not_reproduced=differ), f, indent=1)
        f.write("\n")
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
