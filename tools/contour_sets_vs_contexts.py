#!/usr/bin/env python3
"""P parameter sets x 1 ellipse on ONE context (bind_param_sets + find_roots_in_contours_sets) against a context per
set (Context(...) + find_roots_in_contour + destroy).  Development tool, not the bench.  DESIGN.md §13.9.

The sets are a k_rho sweep of the tokamak example, the ellipse of every set the unstable-mode ellipse of DESIGN.md §11.
Both variants run in THIS process and alternate (a number from another run, on another box, is no partner); each is
run --repeat (3) times after one warm-up of each, context creation, binding and destruction counted in both, every
wall time ends behind the call's own stream synchronisation, and every wall time is printed so that the spread is
visible.  Cells: N = 64 and 256, P = 8 and 32, once with default options and once with tile_uncached = 1 (both
variants get the option).  --out STEM writes STEM.txt (what is printed) and STEM.json."""
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
CENTER, AXES = -0.80 + 0.25j, (0.25, 0.20)


def say(s):
    print(s, flush=True)
    LINES.append(s)


def sweep(n, p):
    return [emme_amd.params_from_dict(bench.workload_dict(n, k_rho=float(k))) for k in np.linspace(0.25, 0.45, p)]


def one_context(sets, options):
    t0 = time.perf_counter()
    with emme_amd.Context(sets[0], **options) as ctx:
        ctx.bind_param_sets(sets)
        res = ctx.find_roots_in_contours_sets(np.arange(len(sets)), [CENTER] * len(sets), [AXES] * len(sets))
    return (time.perf_counter() - t0) * 1e3, res


def context_per_set(sets, options):
    t0 = time.perf_counter()
    res = []
    for p in sets:
        with emme_amd.Context(p, **options) as ctx:
            res.append(ctx.find_roots_in_contour(CENTER, AXES))
    return (time.perf_counter() - t0) * 1e3, res


def fmt(v):
    return "[" + ", ".join(f"{x:.1f}" for x in v) + "]"


def agreement(one, per):
    """items with the same count, node number and number of roots; the worst relative distance of paired roots"""
    same, worst = 0, 0.0
    for a, b in zip(one, per):
        ok = a["winding"] == b["winding"] and a["points_used"] == b["points_used"] and a["n_roots"] == b["n_roots"]
        same += ok
        if ok and len(b["roots"]):
            worst = max(worst, max(float(np.min(np.abs(a["roots"] - x)) / abs(x)) for x in b["roots"]))
    return same, worst


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--npoints", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--sets", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    emme_amd.load()
    res = {"center": [CENTER.real, CENTER.imag], "semi_axes": list(AXES), "repeat": a.repeat, "cells": []}
    say(f"region search over sets on one context vs a context per set: wall ms of P searches (1 ellipse each, "
        f"centre {CENTER}, semi-axes {AXES}), {a.repeat} runs each, alternating; context creation and binding counted in both")
    for name, options in (("default options", {}), ("tile_uncached = 1", {"tile_uncached": 1})):
        say(name)
        for n in a.npoints:
            for p in a.sets:
                sets = sweep(n, p)
                one_context(sets, options), context_per_set(sets, options)  # warm-up of both
                t_one, t_per = [], []
                for _ in range(a.repeat):
                    ms, r1 = one_context(sets, options)
                    t_one.append(ms)
                    ms, r2 = context_per_set(sets, options)
                    t_per.append(ms)
                same, worst = agreement(r1, r2)
                ratio = min(t_per) / min(t_one)
                nodes = sum(r["points_used"] for r in r1)
                say(f"N = {n:4d}  P = {p:3d}   one context {fmt(t_one)} best {min(t_one):8.1f}   context per set {fmt(t_per)} "
                    f"best {min(t_per):8.1f}   per-set / one = {ratio:5.2f}   nodes {nodes}, roots {sum(r['n_roots'] for r in r1)}, "
                    f"complete {sum(r['complete'] for r in r1)}/{p}, same count / nodes / roots {same}/{p}, worst |dw|/|w| {worst:.1e}")
                res["cells"].append({"options": name, "npoints": n, "sets": p, "one_context_ms": t_one, "context_per_set_ms": t_per,
                                     "ratio_best": ratio, "nodes": nodes, "items_agreeing": same, "worst_rel_root_diff": worst})
    if a.out:
        with open(a.out + ".txt", "w") as f:
            f.write("\n".join(LINES) + "\n")
        with open(a.out + ".json", "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
