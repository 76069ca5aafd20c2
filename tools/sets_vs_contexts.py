#!/usr/bin/env python3
"""P parameter sets x 1 guess on ONE context (bind_param_sets + solve_roots_sets) against a context per set
(Context(...) + solve_roots([g]) + destroy, the scan driver's way).  Development tool, not the bench.  DESIGN.md §13.5.

The sets are a k_rho sweep of the tokamak example.  Both variants run in THIS process and alternate (a number from
another run, on another box, is no partner); each is run --repeat (3) times after one warm-up of each, context
creation and destruction counted in both, and every wall time is printed so that the spread is visible.  Cells:
N = 64 and 256, P = 8 and 32.  --out STEM writes STEM.txt (what is printed) and STEM.json."""
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
GUESS = -0.8 + 0.25j


def say(s):
    print(s, flush=True)
    LINES.append(s)


def sweep(n, p):
    return [emme_amd.params_from_dict(bench.workload_dict(n, k_rho=float(k))) for k in np.linspace(0.25, 0.45, p)]


def one_context(sets):
    t0 = time.perf_counter()
    with emme_amd.Context(sets[0]) as ctx:
        ctx.bind_param_sets(sets)
        roots, iters, info = ctx.solve_roots_sets(np.arange(len(sets)), [GUESS] * len(sets))
    return (time.perf_counter() - t0) * 1e3, roots, iters, info


def context_per_set(sets):
    t0 = time.perf_counter()
    roots, iters, info = [], [], []
    for p in sets:
        with emme_amd.Context(p) as ctx:
            r, i, f = ctx.solve_roots([GUESS])
        roots.append(r[0]), iters.append(i[0]), info.append(f[0])
    return (time.perf_counter() - t0) * 1e3, np.array(roots), np.array(iters), np.array(info)


def fmt(v):
    return "[" + ", ".join(f"{x:.1f}" for x in v) + "]"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--npoints", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--sets", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    emme_amd.load()
    res = {"guess": [GUESS.real, GUESS.imag], "repeat": a.repeat, "cells": []}
    say(f"sets on one context vs a context per set: wall ms of P root searches (1 guess each), {a.repeat} runs each, "
        "alternating; context creation counted in both")
    for n in a.npoints:
        for p in a.sets:
            sets = sweep(n, p)
            one_context(sets), context_per_set(sets)  # warm-up of both
            t_one, t_per = [], []
            for _ in range(a.repeat):
                ms, r1, i1, f1 = one_context(sets)
                t_one.append(ms)
                ms, r2, i2, f2 = context_per_set(sets)
                t_per.append(ms)
            ok = (f1 == 0) & (f2 == 0)
            worst = float(np.max(np.abs(r1[ok] - r2[ok]) / np.abs(r2[ok]))) if ok.any() else float("nan")
            same_iters = bool(np.array_equal(i1[ok], i2[ok]))
            ratio = min(t_per) / min(t_one)
            say(f"N = {n:4d}  P = {p:3d}   one context {fmt(t_one)} best {min(t_one):8.1f}   context per set {fmt(t_per)} "
                f"best {min(t_per):8.1f}   per-set / one = {ratio:5.2f}   converged {int(ok.sum())}/{p}, "
                f"worst |dw|/|w| {worst:.1e}, iterations equal: {same_iters}")
            res["cells"].append({"npoints": n, "sets": p, "one_context_ms": t_one, "context_per_set_ms": t_per,
                                 "ratio_best": ratio, "converged": int(ok.sum()), "worst_rel_root_diff": worst,
                                 "iterations_equal": same_iters})
    if a.out:
        with open(a.out + ".txt", "w") as f:
            f.write("\n".join(LINES) + "\n")
        with open(a.out + ".json", "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
