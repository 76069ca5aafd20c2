#!/usr/bin/env python3
"""Secant (emme_solve_roots) against Newton with the exact M' (emme_solve_roots_newton) on the headline workload
(BASELINE configs[2]: tokamak ES, npoints 256, dim 256).  Development tool, not the bench.  DESIGN.md §12.

Three ways of running the bench's 128-guess lattice:
  cached    one call on a default context (node cache built on the first call; ms is the best of --repeat warm calls)
  uncached  one call on a node_cache_gb = 0 context (every fill from scratch, omega-lane kernels)
  scan      32 single-guess calls (every fourth lattice point) on a default context: below cache_min_batch no cache is
            built, so every fill is a from-scratch lanes-are-nodes fill -- the reference's parameter-scan workload
For each: fills (matrices assembled) per converged chain, ms per call (per guess for `scan`), converged chains and the
distinct roots reached.  Also the cost of one fill: plain against derivative, per kernel.
--deriv-cached adds the option deriv_cached = 1 (derivative fills through the node cache, k_assemble_dense_deriv): the
cached rows are then printed for both settings (`cached` = 0, `cached+dc` = 1, one context each, same process and
device), and the fill-cost table gets the cached derivative fill of the 128 omegas.
--out FILE writes the numbers as JSON."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import emme_amd  # noqa: E402


def distinct(roots, tol=1e-6):
    out = []
    for x in roots:
        if np.isfinite(x) and all(abs(x - y) > 10 * tol * abs(x) for y in out):
            out.append(complex(x))
    return sorted(out, key=lambda x: -x.imag)


def run(ctx, method, guesses):
    """One call; returns (roots, converged mask, fills, ms)."""
    ctx.profile_read(reset=True)
    t0 = time.perf_counter()
    f = ctx.solve_roots if method == "secant" else ctx.solve_roots_newton
    roots, iters, info = f(guesses)
    ms = (time.perf_counter() - t0) * 1e3
    fills = ctx.profile_read(reset=True).matrices
    conv = (info == 0) & (iters <= ctx.params.iteration_step_limit)
    return roots, conv, fills, ms


def fill_cost(ctx, omegas, repeat, deriv):
    best = None
    for _ in range(repeat):
        ctx.profile_read(reset=True)
        if deriv:
            ctx.assemble_derivative(omegas)
        else:
            ctx.assemble(omegas)
        ms = ctx.profile_read(reset=True).assemble_ms
        best = ms if best is None else min(best, ms)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--deriv-cached", action="store_true")
    a = ap.parse_args()
    d = bench.workload_dict(256)
    lattice = bench.lattice(1, 0, 128)
    scan = lattice[::4]
    res = {"workload": "BASELINE configs[2], npoints 256, 128-guess lattice", "modes": {}, "fill_ms": {}}
    reached = {}

    runs = [("cached", {}), ("uncached", {"node_cache_gb": 0.0})]
    if a.deriv_cached:
        runs.insert(1, ("cached+dc", {"deriv_cached": 1}))
    for mode, opt in runs:
        with emme_amd.Context(emme_amd.params_from_dict(d), device=0, **opt) as ctx:
            ctx.profile(True)
            for method in ("secant", "newton"):
                first = None
                best = None
                for k in range(a.repeat):
                    roots, conv, fills, ms = run(ctx, method, lattice)
                    first = ms if first is None else first
                    best = ms if best is None else min(best, ms)
                rs = distinct(roots[conv])
                reached[(mode, method)] = rs
                res["modes"][f"{mode}/{method}"] = {
                    "fills": int(fills), "converged": int(conv.sum()),
                    "fills_per_converged": fills / max(int(conv.sum()), 1),
                    "ms_first_call": first, "ms_per_call": best, "distinct_roots": len(rs)}
            if mode == "uncached":
                for name, om in (("omega-lane, 128 omegas", lattice), ("lanes-are-nodes, 1 omega", lattice[:1])):
                    p = fill_cost(ctx, om, a.repeat, False)
                    q = fill_cost(ctx, om, a.repeat, True)
                    res["fill_ms"][name] = {"plain": p, "derivative": q, "ratio": q / p}
            elif mode == "cached":
                p = fill_cost(ctx, lattice, a.repeat, False)
                res["fill_ms"]["cached plain, 128 omegas"] = {"plain": p}
            else:
                p = fill_cost(ctx, lattice, a.repeat, False)
                q = fill_cost(ctx, lattice, a.repeat, True)
                res["fill_ms"]["cached derivative (k_assemble_dense_deriv), 128 omegas"] = {
                    "plain": p, "derivative": q, "ratio": q / p}

    with emme_amd.Context(emme_amd.params_from_dict(d), device=0) as ctx:
        ctx.profile(True)
        for method in ("secant", "newton"):
            tot_fills, tot_ms, ok, allr = 0, 0.0, 0, []
            for g in scan:
                roots, conv, fills, ms = run(ctx, method, np.array([g]))
                tot_fills += fills
                tot_ms += ms
                ok += int(conv.sum())
                allr += list(roots[conv])
            rs = distinct(allr)
            reached[("scan", method)] = rs
            res["modes"][f"scan/{method}"] = {
                "fills": int(tot_fills), "converged": ok, "fills_per_converged": tot_fills / max(ok, 1),
                "ms_per_call": tot_ms / len(scan), "calls": len(scan), "distinct_roots": len(rs)}
        assert ctx.cache_state()[0] == -1, "the scan built a node cache"

    for mode in [m for m, _ in runs] + ["scan"]:
        s, n = reached[(mode, "secant")], reached[(mode, "newton")]
        only_s = [x for x in s if all(abs(x - y) > 1e-5 * abs(x) for y in n)]
        only_n = [x for x in n if all(abs(x - y) > 1e-5 * abs(x) for y in s)]
        res["modes"][f"{mode}/roots"] = {"secant_only": [[x.real, x.imag] for x in only_s],
                                         "newton_only": [[x.real, x.imag] for x in only_n],
                                         "both": len(s) - len(only_s)}

    for k, v in res["modes"].items():
        print(f"{k:18s} " + "  ".join(f"{kk} {vv:.4g}" if isinstance(vv, float) else f"{kk} {vv}" for kk, vv in v.items()))
    for k, v in res["fill_ms"].items():
        print(f"fill {k:60s} " + "  ".join(f"{kk} {vv:.4g}" for kk, vv in v.items()))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
