#!/usr/bin/env python3
"""Newton on the eigenpair (emme_solve_eigenpairs) against what it replaces: emme_solve_roots_newton
followed by emme_null_vectors_batch(M = NULL).  Development tool, not the bench.

Both run in THIS process on ONE context (deriv_cached = 1, node cache settled on the cell's guesses), alternating, every
call synchronising; three recorded runs after one warm-up of each, ALL of them printed.  Per run: wall ms of the whole
call(s), steps per chain, and the K_LIN / K_NULL spans of emme_profile_t (linstep_ms: the trace step's LU with n
right-hand sides, or the eigenpair search's work copies and residual launch; nullspace_ms: emme_null_vectors_batch, or
the eigenpair search's factorisations and step kernels).
Cells:
  golden    headline parameters at N = 256, the distinct golden roots x (1 + 1e-3)
  lattice   the same context, the bench's 128-guess lattice; also the distinct roots reached with resid below 100 x the
            median resid of the golden cell, against Newton's distinct roots (info = 0, simple root by the sigma rule is
            NOT applied here: both counts are of distinct end points)
  stell     the stellarator shape at N = 256 (dim 512, GK31 electromagnetic, derivative cache shapes ALL), 128 guesses
            around (-1.656, 2.490), step limit 20
--out FILE appends what is printed to FILE (default profiles/eigenpairs_vs_newton.txt)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import emme_amd  # noqa: E402

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def fmt(v, p=2):
    return "[" + ", ".join(f"{x:.{p}f}" for x in v) + "]"


def golden_roots():
    g = np.load(bench.GOLDEN_CFG3)
    out = []
    for x in g["roots"][g["converged"].astype(bool)]:
        if all(abs(x - y) > 1e-7 * abs(x) for y in out):
            out.append(x)
    return np.array(out)


def distinct(roots):
    out = []
    for x in roots:
        if np.isfinite(x) and all(abs(x - y) > 1e-6 * abs(x) for y in out):
            out.append(x)
    return out


def cell(name, ctx, guesses, repeat, step_limit=None, resid_bar=None):
    kw = {} if step_limit is None else {"step_limit": step_limit}
    runs = {"eigenpairs": [], "newton+null": []}
    keep = {}

    def one(label, record):
        ctx.profile_read(reset=True)
        t0 = time.perf_counter()
        if label == "eigenpairs":
            roots, vecs, resid, iters, info = ctx.solve_eigenpairs(guesses, **kw)
        else:
            roots, iters, info = ctx.solve_roots_newton(guesses, **kw)
            vecs, _ = ctx.null_vectors(nbatch=len(guesses))
            resid = None
        ms = (time.perf_counter() - t0) * 1e3
        pr = ctx.profile_read(reset=True)
        if record:
            runs[label].append((ms, pr.linstep_ms, pr.nullspace_ms, pr.assemble_ms + pr.deferred_ms))
            keep[label] = (roots, vecs, resid, iters, info)

    for label in runs:
        one(label, False)  # warm-up
    for _ in range(repeat):
        for label in runs:
            one(label, True)
    for label, v in runs.items():
        roots, vecs, resid, iters, info = keep[label]
        ok = info == 0
        say(f"{name:8s} {label:12s} wall ms {fmt([r[0] for r in v])}  K_LIN ms {fmt([r[1] for r in v])}  K_NULL ms "
            f"{fmt([r[2] for r in v])}  fills ms {fmt([r[3] for r in v])}  chains {len(guesses)}, info = 0: {int(ok.sum())}, "
            f"steps per chain mean {iters.mean():.2f} max {int(iters.max())}, total {int(iters.sum())}")
    be, bn = min(r[0] for r in runs["eigenpairs"]), min(r[0] for r in runs["newton+null"])
    spread = max(max(r[0] for r in v) - min(r[0] for r in v) for v in runs.values())
    say(f"{name:8s} best wall: eigenpairs {be:.2f} ms, newton+null {bn:.2f} ms: x{bn / be:.2f} (newton+null - eigenpairs = "
        f"{bn - be:+.2f} ms, 3 x spread {3 * spread:.2f} ms)")
    re, ve, resid, ie, fe = keep["eigenpairs"]
    rn, vn, _, inn, fn = keep["newton+null"]
    okr = (fe == 0) & np.isfinite(resid)
    say(f"{name:8s} eigenpairs resid: median {np.median(resid[okr]):.2e}, min {resid[okr].min():.2e}, max {resid[okr].max():.2e}")
    both = (fe == 0) & (fn == 0)
    with np.errstate(invalid="ignore"):
        same = both & (np.abs(re - rn) <= 1e-9 * np.abs(rn))
    ov = [abs(np.vdot(ve[b], vn[b])) for b in np.nonzero(same)[0]]
    say(f"{name:8s} chains with info = 0 in both {int(both.sum())}, the same root within 1e-9 relative {int(same.sum())}"
        + (f", worst 1 - |<v_eig, v_null>| there {max(1 - o for o in ov):.1e}" if ov else ""))
    if resid_bar is not None:
        good = okr & (resid < resid_bar)
        say(f"{name:8s} distinct roots: eigenpairs with resid < {resid_bar:.1e}: {len(distinct(re[good]))} "
            f"(chains {int(good.sum())}; info = 0 but resid above the bar: {int((okr & ~good).sum())}); "
            f"newton, info = 0: {len(distinct(rn[fn == 0]))} (chains {int((fn == 0).sum())})")
    return float(np.median(resid[okr]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="golden,lattice,stell")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eigenpairs_vs_newton.txt"))
    a = ap.parse_args()
    cells = a.cells.split(",")
    say("one run on one device; every run of every cell is listed")
    if "golden" in cells or "lattice" in cells:
        lat = bench.lattice(1, 0, 128)
        ctx = emme_amd.Context(emme_amd.params_from_dict(bench.workload_dict(256)), device=0, deriv_cached=1)
        ctx.profile(True)
        ctx.cache_settle(lat)
        g = golden_roots() * (1 + 1e-3)
        med = cell("golden", ctx, g, a.repeat)
        if "lattice" in cells:
            cell("lattice", ctx, lat, a.repeat, resid_bar=100.0 * med)
        ctx.close()
    if "stell" in cells:
        cfg4 = bench.lattice_cfg4(0)
        ctx = emme_amd.Context(emme_amd.params_from_dict(dict(bench.STELLARATOR, npoints=256)), device=0, deriv_cached=1)
        ctx.set_deriv_cache_shapes(emme_amd.DERIV_CACHE_SHAPES_ALL)
        ctx.profile(True)
        ctx.cache_settle(cfg4)
        cell("stell", ctx, cfg4, a.repeat, step_limit=20)
        ctx.close()
    with open(a.out, "a") as f:
        f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
