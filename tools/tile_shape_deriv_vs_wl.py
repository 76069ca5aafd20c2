#!/usr/bin/env python3
"""The derivative tile fill of electromagnetic and GK31 contexts (tile_uncached = 1 + deriv_cached = 1 with tile shapes
ALL, k_assemble_tile_shape_deriv<PTS, NM>) against the omega-lane derivative kernel (shapes at their default,
k_assemble_wl_deriv) on contexts without a node cache.  Development tool, not the bench.  DESIGN.md §12.4; after
tools/tile_deriv_vs_wl.py (§12.3), rows as tools/tile_shapes_vs_wl.py's (§5.3c).

Both settings run in THIS process, on a pair of node_cache_gb = 0, deriv_cached = 1, tile_uncached = 1 contexts of the
same parameter set: one with shapes off (the partner), one with shapes ALL.  The two alternate inside every repeat;
every call synchronises; each figure is the best of --repeat (3) calls after one warm-up, and all of them are printed so
that the spread is visible.  A difference counts when it exceeds three times the spread of the repeats.
  fill rows    assemble_ms + deferred_ms of one derivative fill (device time of the fill kernel and of the work list)
  search row   wall ms of one emme_solve_roots_newton call and matrices filled per second
One row per invocation (--row), one GPU step each:
  stell1024        stellarator N = 1024 (dim 2048, GK31 EM), 4 lattice omegas: M and M'
  stell256         stellarator N = 256 (dim 512), 128 lattice omegas around (-1.656, 2.490): M and M'
  stell256-newton  the same context's whole emme_solve_roots_newton on those guesses
  tok-em15         tokamak beta_e = 0.02 (GK15 EM) N = 256, the bench's 128 lattice omegas: M and M'
  tok-es31         tokamak GK31 (electrostatic) N = 256, the bench's 128 lattice omegas: M and M'
--out FILE appends what is printed to FILE (default profiles/tile_shape_deriv_vs_wl.txt)."""
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
ENUMERIC = -6


def say(s):
    print(s, flush=True)
    LINES.append(s)


def fmt(v):
    return "[" + ", ".join(f"{x:.3f}" for x in v) + "]"


def pair_for(d):
    p = emme_amd.params_from_dict(d)
    off = emme_amd.Context(p, device=0, node_cache_gb=0.0, deriv_cached=1, tile_uncached=1)
    on = emme_amd.Context(p, device=0, node_cache_gb=0.0, deriv_cached=1, tile_uncached=1)
    on.set_tile_shapes(emme_amd.TILE_SHAPES_ALL)
    off.profile(True), on.profile(True)
    return [("omega-lane", off), ("tile-shape", on)]


def deriv(ctx, omegas):
    """emme_assemble_derivative_batch with its return code (EMME_ENUMERIC: a matrix holds a non-finite integral)"""
    w = np.ascontiguousarray(omegas, dtype=np.complex128)
    nb = w.shape[0]
    iv = np.zeros(nb, dtype=np.int64)
    M = np.zeros((nb, ctx.dim, ctx.dim), dtype=np.complex128)
    Mp = np.zeros_like(M)
    rc = ctx.lib.emme_assemble_derivative_batch(ctx.h, w.ctypes.data, nb, M.ctypes.data, Mp.ctypes.data, iv.ctypes.data)
    if rc not in (0, ENUMERIC):
        raise RuntimeError(f"emme_assemble_derivative_batch: {rc}")
    return M, Mp, iv


def rel_diff(A, B):
    """per matrix max|A - B| / max|B|, over the matrices that are finite in both"""
    ok = np.isfinite(A).all(axis=(1, 2)) & np.isfinite(B).all(axis=(1, 2))
    return np.array([np.abs(A[k] - B[k]).max() / np.abs(B[k]).max() if ok[k] else 0.0 for k in range(len(B))]), ok


def fill_row(name, pair, omegas, repeat):
    vals = {label: [] for label, _ in pair}
    keep = {}
    for _, ctx in pair:
        deriv(ctx, omegas)  # warm-up
    for _ in range(repeat):
        for label, ctx in pair:
            ctx.profile_read(reset=True)
            M, Mp, iv = deriv(ctx, omegas)
            pr = ctx.profile_read(reset=True)
            vals[label].append(pr.assemble_ms + pr.deferred_ms)
            keep[label] = (iv, M, Mp, pr.tile_tasks, ctx.last_deferred())
    for label, _ in pair:
        v = vals[label]
        iv, _, _, tasks, handed = keep[label]
        say(f"{name:30s} {label:10s} best {min(v):10.3f} ms  {len(omegas) / (min(v) * 1e-3):9.1f} omega-points/s"
            f"  all {fmt(v)}  spread {max(v) - min(v):.3f}  intervals {int(iv.sum())}  tile tasks {tasks}  handed over {handed}")
    (iv0, M0, Mp0, _, _), (iv1, M1, Mp1, _, _) = keep["omega-lane"], keep["tile-shape"]
    dm, ok = rel_diff(M1, M0)
    dp, _ = rel_diff(Mp1, Mp0)
    kw = int(dp.argmax())
    b0, b1 = min(vals["omega-lane"]), min(vals["tile-shape"])
    spread = max(max(v) - min(v) for v in vals.values())
    say(f"{name:30s} tile-shape / omega-lane: x{b0 / b1:.2f} (difference {b0 - b1:+.3f} ms, 3 x spread {3 * spread:.3f} ms); "
        f"interval totals equal omega by omega: {bool(np.array_equal(iv0, iv1))}; worst difference M {dm.max():.2e} of max|M|, "
        f"M' {dp.max():.2e} of max|M'| (worst at omega {complex(omegas[kw]):.6g}; {int((dp > 1e-10).sum())} omegas above 1e-10; "
        f"{int(ok.sum())} finite in both)")


def search_row(name, pair, guesses, repeat):
    vals = {label: [] for label, _ in pair}
    keep = {}
    for _, ctx in pair:
        ctx.solve_roots_newton(guesses)  # warm-up
    for _ in range(repeat):
        for label, ctx in pair:
            ctx.profile_read(reset=True)
            t0 = time.perf_counter()
            roots, iters, info = ctx.solve_roots_newton(guesses)
            ms = (time.perf_counter() - t0) * 1e3
            pr = ctx.profile_read(reset=True)
            keep[label] = (roots, iters, info, pr.matrices, pr.tile_tasks)
            vals[label].append(ms)
    for label, ctx in pair:
        v = vals[label]
        roots, iters, info, fills, tasks = keep[label]
        conv = (info == 0) & (iters <= ctx.params.iteration_step_limit)
        say(f"{name:30s} {label:10s} best {min(v):10.3f} ms  {fills / (min(v) * 1e-3):9.1f} omega-points/s"
            f"  all {fmt(v)}  spread {max(v) - min(v):.3f}  converged {int(conv.sum())}  iterations {int(iters.sum())}"
            f"  matrices {fills}  tile tasks {tasks}")
    (r0, i0, f0, _, _), (r1, i1, f1, _, _) = keep["omega-lane"], keep["tile-shape"]
    limit = pair[0][1].params.iteration_step_limit
    # converged = info 0 inside the step limit; a chain that runs into the limit has info 0 too and no root to compare
    both = (f0 == 0) & (f1 == 0) & (i0 <= limit) & (i1 <= limit)
    b0, b1 = min(vals["omega-lane"]), min(vals["tile-shape"])
    spread = max(max(v) - min(v) for v in vals.values())
    say(f"{name:30s} tile-shape / omega-lane: x{b0 / b1:.2f} (difference {b0 - b1:+.3f} ms, 3 x spread {3 * spread:.3f} ms); "
        f"chains converged in both: {int(both.sum())}, same iteration counts among them: {int((i0[both] == i1[both]).sum())} "
        f"(among all {len(i0)} chains: {int((i0 == i1).sum())}), "
        f"largest |root difference| of a chain converged in both {np.abs(r0[both] - r1[both]).max() if both.any() else 0.0:.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--row", required=True, choices=["stell1024", "stell256", "stell256-newton", "tok-em15", "tok-es31"])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_shape_deriv_vs_wl.txt"))
    a = ap.parse_args()
    cfg4 = bench.lattice_cfg4(0)  # 128 guesses around (-1.656, 2.490)
    lat = bench.lattice(1, 0, 128)
    if a.row == "stell1024":
        pair = pair_for(dict(bench.STELLARATOR, npoints=1024))
        fill_row("stellarator N=1024, 4 w", pair, np.ascontiguousarray(cfg4[::32]), a.repeat)
    elif a.row == "stell256":
        pair = pair_for(dict(bench.STELLARATOR, npoints=256))
        fill_row("stellarator N=256, 128 w", pair, cfg4, a.repeat)
    elif a.row == "stell256-newton":
        pair = pair_for(dict(bench.STELLARATOR, npoints=256))
        search_row("stellarator N=256 Newton", pair, cfg4, a.repeat)
    elif a.row == "tok-em15":
        pair = pair_for(bench.workload_dict(256, beta_e=0.02))
        fill_row("tokamak EM GK15 N=256, 128 w", pair, lat, a.repeat)
    else:
        pair = pair_for(bench.workload_dict(256, integration_start_points=31))
        fill_row("tokamak ES GK31 N=256, 128 w", pair, lat, a.repeat)
    for _, ctx in pair:
        ctx.close()
    with open(a.out, "a") as f:
        f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
