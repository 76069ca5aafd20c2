#!/usr/bin/env python3
"""Region searches that return eigenpairs (emme_find_eigenpairs_in_contour[s_sets]) against what a
caller had to do before for the same answer: find_roots_* , then assemble at the roots, then null_vectors.

Cells: the three ellipses of DESIGN.md §11 on the headline context (npoints 256, default options, mirrored cache), and one
32-item sets call at npoints 64.  Both routes alternate in one process after a warm-up, three runs each, wall time of the
whole calls, best of three.  Also reported: polish steps per candidate from the Beyn seed against the same search
started from the fixed s (the chains of the root form's polish stand for the latter's candidates: same candidates, no
seed), and the K_LIN / K_NULL spans per polish step of the secant eigenpair route against the trace route.

    python3 tools/contour_eigenpairs.py [--out profiles/contour_eigenpairs.txt]

One GPU, one process; what is printed is appended to --out."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import emme_amd as emme  # noqa: E402

ELLIPSES = [(-0.80 + 0.25j, (0.25, 0.20)), (-0.641 - 0.232j, (0.085, 0.05)), (-0.60 + 0.10j, (0.15, 0.12))]


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def spans(ctx):
    p = ctx.profile_read(reset=True)
    return p.linstep_ms, p.nullspace_ms


def cell_single(ctx, say, name, c, ab, exact):
    def new():
        return ctx.find_eigenpairs_in_contour(c, ab, exact=exact)

    def old():
        r = ctx.find_roots_in_contour(c, ab)
        if len(r["roots"]):
            M = ctx.assemble(r["roots"])
            r["vecs"], _ = ctx.null_vectors(M)
        return r

    new(), old()  # warm-up: the cache settles
    runs = {"pairs": [], "roots+assemble+null": []}
    keep = {}
    for _ in range(3):
        for label, fn in (("pairs", new), ("roots+assemble+null", old)):
            ctx.profile_read(reset=True)
            ms, out = timed(fn)
            runs[label].append((ms,) + spans(ctx))
            keep[label] = out
    for label, rs in runs.items():
        say(f"{name:10s} exact {int(exact)} {label:20s} wall ms {[round(r[0], 2) for r in rs]}  K_LIN ms {[round(r[1], 2) for r in rs]}  "
            f"K_NULL ms {[round(r[2], 2) for r in rs]}  roots {keep[label]['n_roots']} winding {keep[label]['winding']} "
            f"polish steps per root {np.mean(keep[label]['iters']) if len(keep[label]['iters']) else 0:.2f}")
    bn, bo = min(r[0] for r in runs["pairs"]), min(r[0] for r in runs["roots+assemble+null"])
    say(f"{name:10s} exact {int(exact)} best wall: pairs {bn:.2f} ms, roots+assemble+null {bo:.2f} ms: x{bo / bn:.2f}"
        f"{' (loses)' if bn > bo else ''}")
    p = keep["pairs"]
    if len(p["roots"]):
        say(f"{name:10s} exact {int(exact)} pairs resid max {p['resid'].max():.2e}; seeded polish against the fixed s on the same roots x (1 + 1e-3): "
            f"{np.mean(ctx.solve_eigenpairs(p['roots'] * (1 + 1e-3), v0=p['vecs'], secant=not exact)[3]):.2f} against "
            f"{np.mean(ctx.solve_eigenpairs(p['roots'] * (1 + 1e-3), secant=not exact)[3]):.2f} steps per chain")


def cell_sets(say, nitems=32, npoints=64):
    base = bench.workload_dict(npoints)
    dicts = [dict(base, k_rho=base["k_rho"] * (1.0 + 0.01 * k)) for k in range(nitems)]
    with emme.Context(emme.params_from_dict(dicts[0]), device=0) as ctx:
        ctx.bind_param_sets([emme.params_from_dict(d) for d in dicts])
        ctx.profile(True)
        sets = list(range(nitems))
        c, ab = ELLIPSES[0]
        args = (sets, [c] * nitems, [ab] * nitems)

        def new():
            return ctx.find_eigenpairs_in_contours_sets(*args)

        def old():
            rs = ctx.find_roots_in_contours_sets(*args)
            st = [k for k, r in enumerate(rs) for _ in r["roots"]]
            w = [x for r in rs for x in r["roots"]]
            if w:
                ctx.null_vectors(ctx.assemble_sets(st, w))
            return rs

        new(), old()
        runs = {"pairs": [], "roots+assemble+null": []}
        for _ in range(3):
            for label, fn in (("pairs", new), ("roots+assemble+null", old)):
                ms, out = timed(fn)
                runs[label].append(ms)
        for label, rs in runs.items():
            say(f"sets x{nitems} N{npoints} {label:20s} wall ms {[round(r, 2) for r in rs]}")
        bn, bo = min(runs["pairs"]), min(runs["roots+assemble+null"])
        say(f"sets x{nitems} N{npoints} best wall: pairs {bn:.2f} ms, roots+assemble+null {bo:.2f} ms: x{bo / bn:.2f}"
            f"{' (loses)' if bn > bo else ''}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contour_eigenpairs.txt"))
    a = ap.parse_args()
    lines = ["$ python3 tools/contour_eigenpairs.py"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    emme.load()
    with emme.Context(emme.params_from_dict(bench.workload_dict(256)), device=0) as ctx:
        ctx.profile(True)
        for k, (c, ab) in enumerate(ELLIPSES):
            for exact in (False, True):
                cell_single(ctx, say, f"ellipse {k}", c, ab, exact)
    cell_sets(say)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
