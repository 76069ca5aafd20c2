#!/usr/bin/env python3
"""Region search against the lattice search on the headline workload (BASELINE configs[2]: tokamak ES, npoints 256,
dim 256), one context.  Development tool, not the bench.

(a) the bench's 128-guess lattice (Re w in [-1.2, -0.4] x Im w in [0.05, 0.40]) through solve_roots;
(b) find_roots_in_contour over an ellipse that covers the lattice region.
Prints for each: omega-points (fills), wall ms (both calls return after a stream synchronisation), the distinct roots, and W for (b).
--sigma also prints, for the test contours of tests/test_gpu_contour.py, the node count the argument principle needed
and the singular values of A0 (EMME_DEBUG lines of the library), the measurements behind the emme_contour_t defaults."""
import argparse
import os
import subprocess
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
            out.append(x)
    return sorted(out, key=lambda x: -x.imag)


def fills(ctx):
    return ctx.profile_read(reset=True).matrices


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--sigma", action="store_true", help="print sigma(A0) and N of the test contours (child process)")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.sigma:
        # the library prints its per-stage lines with EMME_DEBUG: in a child process of its own
        env = dict(os.environ, EMME_DEBUG="1")
        for spec in ("-0.80,0.25,0.25,0.20", "-0.641,-0.232,0.085,0.05", "-0.80,0.125,0.40,0.175"):
            print(f"--- contour {spec}", flush=True)
            r = subprocess.run([sys.executable, __file__, f"--child={spec}"], env=env, capture_output=True, text=True)
            print(r.stdout.strip())
            print("\n".join(l for l in r.stderr.splitlines() if "contour" in l))
            if r.returncode != 0:
                print(r.stderr[-2000:])
                return r.returncode
        return 0
    with emme_amd.Context(emme_amd.params_from_dict(bench.workload_dict(256)), device=0) as ctx:
        if a.child:
            cx, cy, ea, eb = (float(v) for v in a.child.split(","))
            for pts in (8, 16, 32, 64, 128):
                res = ctx.find_roots_in_contour(complex(cx, cy), (ea, eb), points=pts, max_points=pts, probes=8)
                print(f"points {pts}: W {res['winding']} roots {len(res['roots'])} complete {res['complete']}", flush=True)
            return 0
        ctx.profile(True)
        g = bench.lattice(1, 0)
        # the headline lattice covers Re [-1.2, -0.4] x Im [0.05, 0.40]: the ellipse through its corners
        c = -0.8 + 0.225j
        ea, eb = 0.4 * np.sqrt(2), 0.175 * np.sqrt(2)
        # |Re c| must exceed a: shrink a to stay left of Re omega = 0
        ea = min(ea, 0.79)
        ctx.solve_roots(g)  # warm: node cache
        ctx.find_roots_in_contour(c, (ea, eb))
        fills(ctx)
        for name in ("lattice", "contour"):
            best = None
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                if name == "lattice":
                    roots, iters, info = ctx.solve_roots(g)
                    found, W, N = distinct(roots[info == 0]), None, None
                else:
                    res = ctx.find_roots_in_contour(c, (ea, eb))
                    found, W, N = list(res["roots"]), res["winding"], res["points_used"]
                ms = 1e3 * (time.perf_counter() - t0)
                nf = fills(ctx)
                best = ms if best is None else min(best, ms)
            print(f"({'a' if name == 'lattice' else 'b'}) {name}: omega-points (fills) {nf}, wall {best:.1f} ms "
                  f"(best of {a.repeat}), {len(found)} distinct roots" + (f", W {W}, N {N}" if W is not None else ""))
            for x in found:
                print(f"    {x.real:+.10f}{x.imag:+.10f}i")
        if name == "contour":
            print(f"ellipse c {c}, a {ea:.4f}, b {eb:.4f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
