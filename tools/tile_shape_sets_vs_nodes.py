#!/usr/bin/env python3
"""The tile fill over parameter sets on electromagnetic and GK31 contexts (tile shapes ALL, option tile_uncached = 1:
k_assemble_tile_shape_sets<PTS, NM>, a set per omega chunk) against the lanes-are-nodes fill over sets (option off:
k_assemble_sets, the path every such sets call took before).  Development tool, not the bench.  DESIGN.md §13.8;
modelled on tools/tile_sets_vs_nodes.py.

One process, pairs of bound contexts that differ in tile_uncached alone (node_cache_gb = 0, wl_min = 1, tile shapes ALL,
deriv_cached = 1 on both, which the option-off context ignores for sets).  The two variants alternate: one warm-up of
each, then --repeat (3) synchronised runs each, and every value is printed so that the spread is visible.
Shapes: the stellarator input (electromagnetic, GK31), the same with integration_start_points = 15, the tokamak
workload with integration_start_points = 31.  Cells: P sets of a k_rho sweep x G guesses per set (an electromagnetic
chunk holds 5 omegas), at N = 64 and 256.
  plain / deriv   assemble_ms + deferred_ms (device time of the fill kernels and of the work list) of one
                  assemble_sets call without / with the exact derivative
  search          wall ms of one solve_roots_sets call (secant search)
Per cell also: whether the interval counts of the fills are equal item by item, and the largest entry difference
between the two variants, relative to max|M| of the item; for the searches, how many chains converged within the step
limit in each variant, the largest root difference among those, and whether their iteration counts are equal.
--out STEM writes STEM.txt (what is printed) and STEM.json."""
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

LINES = []
VARIANTS = ("nodes", "tile")
SHAPES = ("stellarator", "stellarator-gk15", "tokamak-gk31")


def say(s):
    print(s, flush=True)
    LINES.append(s)


def sweep(shape, n, p):
    if shape == "tokamak-gk31":
        ds = [bench.workload_dict(n, integration_start_points=31, k_rho=float(k)) for k in np.linspace(0.25, 0.45, p)]
    else:
        over = {"integration_start_points": 15} if shape == "stellarator-gk15" else {}
        ds = [dict(bench.STELLARATOR, npoints=n, k_rho=float(k), **over) for k in np.linspace(0.2, 0.3, p)]
    return [emme_amd.params_from_dict(d) for d in ds]


def guesses(shape, g):
    """G guesses around the input's initial guess (that guess first), all on the Re omega < 0 side"""
    if shape == "tokamak-gk31":
        re, im = np.meshgrid(np.linspace(-0.8, -0.65, 4), np.linspace(0.25, 0.10, 4))
    else:
        re, im = np.meshgrid(np.linspace(-1.656, -1.5, 4), np.linspace(2.49, 2.25, 4))
    return (re + 1j * im).reshape(-1)[:g].copy()


def fill_ms(ctx, st, w, deriv):
    ctx.profile_read(reset=True)
    out = ctx.assemble_sets(st, w, want_derivative=deriv, want_intervals=True)
    pr = ctx.profile_read(reset=True)
    return pr.assemble_ms + pr.deferred_ms, out


def search_ms(ctx, st, w):
    t0 = time.perf_counter()
    roots, iters, info = ctx.solve_roots_sets(st, w)
    return (time.perf_counter() - t0) * 1e3, roots, iters, info


def fmt(v):
    return "[" + ", ".join(f"{x:.2f}" for x in v) + "]"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=SHAPES)
    ap.add_argument("--npoints", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--sets", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--guesses", type=int, nargs="+", default=[1, 2, 5, 10, 15])
    ap.add_argument("--what", nargs="+", default=["plain", "deriv", "search"], choices=["plain", "deriv", "search"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    emme_amd.load()
    res = {"repeat": a.repeat, "cells": []}
    say(f"tile fill over sets, tile shapes ALL (tile_uncached = 1) vs lanes-are-nodes over sets (0): {a.repeat} runs each "
        "after a warm-up, alternating; fills: device ms (assemble + deferred), search: wall ms of solve_roots_sets")
    for shape in a.shapes:
        for n in a.npoints:
            for p in a.sets:
                sets = sweep(shape, n, p)
                ctxs = {}
                for name in VARIANTS:
                    c = emme_amd.Context(sets[0], device=0, node_cache_gb=0.0, wl_min=1, deriv_cached=1,
                                         tile_uncached=int(name == "tile"))
                    c.set_tile_shapes(emme_amd.TILE_SHAPES_ALL)
                    c.bind_param_sets(sets)
                    c.profile(True)
                    ctxs[name] = c
                for g in a.guesses:
                    # a lattice of guesses per scan point: guess-major, so that the items of a set are not neighbours
                    st = np.tile(np.arange(p, dtype=np.int32), g)
                    w = np.repeat(guesses(shape, g), p)
                    cell = {"shape": shape, "npoints": n, "sets": p, "guesses": g, "items": int(p * g)}
                    for what in a.what:
                        t = {v: [] for v in VARIANTS}
                        keep = {}
                        for r in range(a.repeat + 1):  # (run 0: the warm-up of both)
                            for v in VARIANTS:
                                if what == "search":
                                    ms, roots, iters, info = search_ms(ctxs[v], st, w)
                                    keep[v] = (roots, iters, info, ctxs[v].lib.emme_ctx_fill_mode(ctxs[v].h))
                                else:
                                    ms, out = fill_ms(ctxs[v], st, w, what == "deriv")
                                    keep[v] = (out, ctxs[v].lib.emme_ctx_fill_mode(ctxs[v].h), ctxs[v].last_deferred())
                                if r > 0:
                                    t[v].append(ms)
                        ratio = min(t["nodes"]) / min(t["tile"])
                        row = {"nodes_ms": t["nodes"], "tile_ms": t["tile"], "nodes_over_tile": ratio}
                        line = (f"{shape:16s} N = {n:3d} P = {p:2d} G = {g:2d} {what:6s} nodes {fmt(t['nodes'])} tile "
                                f"{fmt(t['tile'])} nodes / tile = {ratio:5.2f}")
                        if what == "search":
                            (r0, i0, f0, m0), (r1, i1, f1, m1) = keep["nodes"], keep["tile"]
                            # (a chain that runs into the step limit ends with info 0 too, wherever it is then: not a root)
                            limit = ctxs["tile"].params.iteration_step_limit
                            ok = (f0 == 0) & (f1 == 0) & (i0 <= limit) & (i1 <= limit)
                            worst = float(np.max(np.abs(r0[ok] - r1[ok]) / np.abs(r0[ok]))) if ok.any() else float("nan")
                            row.update(converged=[int(((f0 == 0) & (i0 <= limit)).sum()), int(((f1 == 0) & (i1 <= limit)).sum())],
                                       worst_rel_root_diff=worst, iterations_equal=bool(np.array_equal(i0[ok], i1[ok])),
                                       modes=[int(m0), int(m1)])
                            line += (f"  modes {m0}/{m1}, converged {row['converged'][0]}/{row['converged'][1]} of {p * g}, "
                                     f"worst |dw|/|w| of those {worst:.1e}, their iterations equal: {row['iterations_equal']}")
                        else:
                            (o0, m0, h0), (o1, m1, h1) = keep["nodes"], keep["tile"]
                            M0, M1, iv0, iv1 = o0[0], o1[0], o0[-1], o1[-1]
                            diff = max(float(np.abs(M0[k] - M1[k]).max() / np.abs(M0[k]).max()) for k in range(len(st)))
                            row.update(same_intervals=bool(np.array_equal(iv0, iv1)), max_rel_diff=diff,
                                       modes=[int(m0), int(m1)], handed_over=int(h1))
                            if what == "deriv":
                                row["max_rel_diff_deriv"] = max(
                                    float(np.abs(o0[1][k] - o1[1][k]).max() / np.abs(o0[1][k]).max()) for k in range(len(st)))
                            line += (f"  modes {m0}/{m1}, interval counts equal: {row['same_intervals']}, max entry difference "
                                     f"{diff:.1e} of max|M|" +
                                     (f", {row['max_rel_diff_deriv']:.1e} of max|M'|" if what == "deriv" else "") +
                                     f", handed over {h1}")
                        say(line)
                        cell[what] = row
                    res["cells"].append(cell)
                    if a.out:  # (kept up to date cell by cell)
                        with open(a.out + ".txt", "w") as f:
                            f.write("\n".join(LINES) + "\n")
                for c in ctxs.values():
                    c.close()
    if a.out:
        with open(a.out + ".json", "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
