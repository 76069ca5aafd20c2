#!/usr/bin/env python3
"""The table-free derivative tile fill (options tile_uncached = 1 + deriv_cached = 1, k_assemble_tile_deriv) against the
omega-lane derivative kernel (tile_uncached = 0, k_assemble_wl_deriv) on contexts without a node cache.  Development
tool, not the bench.  DESIGN.md §12.3; the plain fills' counterpart is tools/tile_vs_wl.py.

Both settings run in THIS process, on a pair of node_cache_gb = 0, deriv_cached = 1 contexts of the same parameter set
(boxes differ by up to 15 %, so a number from another run is no partner).  Every call synchronises; each figure is the
best of --repeat (3) calls after one warm-up, and all of them are printed so that the spread is visible.
  fill rows    assemble_ms + deferred_ms of one derivative fill (device time of the fill kernel and of the work list)
  search rows  wall ms of one emme_solve_roots_newton call and matrices filled per second (omega-points/s)
Rows: N = 256, the bench's 128 lattice omegas; the whole Newton search on those guesses; the omegas still live at step 10
of the secant search (tools/tile_vs_wl.py's set); N = 1024, 32 lattice omegas and a Newton search on them.
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
ENUMERIC = -6


def say(s):
    print(s, flush=True)
    LINES.append(s)


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


def fill_ms(ctx, omegas, repeat):
    deriv(ctx, omegas)  # warm-up
    vals = []
    for _ in range(repeat):
        ctx.profile_read(reset=True)
        M, Mp, iv = deriv(ctx, omegas)
        pr = ctx.profile_read(reset=True)
        vals.append(pr.assemble_ms + pr.deferred_ms)
    return vals, iv, pr.tile_tasks, ctx.last_deferred(), M, Mp


def search_ms(ctx, guesses, repeat):
    ctx.solve_roots_newton(guesses)  # warm-up
    vals, rate = [], []
    for _ in range(repeat):
        ctx.profile_read(reset=True)
        t0 = time.perf_counter()
        roots, iters, info = ctx.solve_roots_newton(guesses)
        ms = (time.perf_counter() - t0) * 1e3
        pr = ctx.profile_read(reset=True)
        vals.append(ms)
        rate.append(pr.matrices / (ms * 1e-3))
    return vals, rate, roots, iters, info, pr.tile_tasks, pr.matrices


def fmt(v):
    return "[" + ", ".join(f"{x:.3f}" for x in v) + "]"


def guarded(fn):
    def run(res, name, *a):
        try:
            fn(res, name, *a)
        except Exception as e:  # (a row that cannot be measured is reported as such; the others still are)
            say(f"{name:36s} UNMEASURED: {e}")
            res["rows"][name] = {"unmeasured": str(e)}
    return run


def rel_diff(A, B):
    """per matrix max|A - B| / max|B|, over the matrices that are finite in both"""
    ok = np.isfinite(A).all(axis=(1, 2)) & np.isfinite(B).all(axis=(1, 2))
    return np.array([np.abs(A[k] - B[k]).max() / np.abs(B[k]).max() if ok[k] else 0.0 for k in range(len(B))]), ok


@guarded
def fill_row(res, name, pair, omegas, repeat):
    row = {"omegas": int(len(omegas))}
    keep = {}
    for label, ctx in pair:
        vals, iv, tasks, handed, M, Mp = fill_ms(ctx, omegas, repeat)
        keep[label] = (iv, M, Mp)
        row[label] = {"ms": vals, "best_ms": min(vals), "omega_points_per_s": len(omegas) / (min(vals) * 1e-3),
                      "tile_tasks": int(tasks), "handed_over": int(handed), "intervals": int(iv.sum())}
        say(f"{name:36s} {label:10s} best {min(vals):9.3f} ms  {len(omegas) / (min(vals) * 1e-3):9.1f} omega-points/s"
            f"  all {fmt(vals)}  tile tasks {tasks}  handed over {handed}")
    (iv0, M0, Mp0), (iv1, M1, Mp1) = keep["omega-lane"], keep["tile"]
    row["same_intervals"] = bool(np.array_equal(iv0, iv1))
    dm, ok = rel_diff(M1, M0)
    dp, _ = rel_diff(Mp1, Mp0)
    row["finite_in_both"] = int(ok.sum())
    row["max_rel_diff_M"], row["max_rel_diff_Mp"] = float(dm.max()), float(dp.max())
    row["median_rel_diff_Mp"] = float(np.median(dp))
    kw = int(dp.argmax())
    row["worst_omega_Mp"] = [float(np.real(omegas[kw])), float(np.imag(omegas[kw]))]
    row["over_1e-10_Mp"] = [[float(np.real(omegas[k])), float(np.imag(omegas[k])), float(dp[k])] for k in np.flatnonzero(dp > 1e-10)]
    row["speedup"] = row["omega-lane"]["best_ms"] / row["tile"]["best_ms"]
    say(f"{name:36s} tile / omega-lane: x{row['speedup']:.2f}; same interval counts: {row['same_intervals']}; worst difference "
        f"M {row['max_rel_diff_M']:.2e} of max|M|, M' {row['max_rel_diff_Mp']:.2e} of max|M'| (median {row['median_rel_diff_Mp']:.2e}; "
        f"worst at omega {complex(omegas[kw]):.6g}; {len(row['over_1e-10_Mp'])} omegas above 1e-10; {row['finite_in_both']} finite in both)")
    res["rows"][name] = row


@guarded
def search_row(res, name, pair, guesses, repeat):
    row = {"guesses": int(len(guesses))}
    keep = {}
    for label, ctx in pair:
        vals, rate, roots, iters, info, tasks, fills = search_ms(ctx, guesses, repeat)
        conv = (info == 0) & (iters <= ctx.params.iteration_step_limit)
        keep[label] = (roots, iters, conv)
        row[label] = {"ms": vals, "best_ms": min(vals), "omega_points_per_s": max(rate), "tile_tasks": int(tasks),
                      "fills": int(fills), "converged": int(conv.sum())}
        say(f"{name:36s} {label:10s} best {min(vals):9.3f} ms  {max(rate):9.1f} omega-points/s  all {fmt(vals)}"
            f"  tile tasks {tasks}  matrices {fills}  converged {int(conv.sum())}")
    (r0, i0, c0), (r1, i1, c1) = keep["omega-lane"], keep["tile"]
    both = c0 & c1
    row["converged_in_both"] = int(both.sum())
    row["same_iterations_in_both"] = int((i0[both] == i1[both]).sum())
    row["max_rel_root_diff"] = float((np.abs(r0[both] - r1[both]) / np.abs(r0[both])).max()) if both.any() else 0.0
    row["speedup"] = row["omega-lane"]["best_ms"] / row["tile"]["best_ms"]
    say(f"{name:36s} tile / omega-lane: x{row['speedup']:.2f}; converged in both {row['converged_in_both']}, same iteration "
        f"count {row['same_iterations_in_both']}, worst root difference {row['max_rel_root_diff']:.2e} relative")
    res["rows"][name] = row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-1024", action="store_true")
    a = ap.parse_args()
    res = {"rows": {}}
    lattice = bench.lattice(1, 0, 128)

    def pair_for(n):
        p = emme_amd.params_from_dict(bench.workload_dict(n))
        off = emme_amd.Context(p, device=0, node_cache_gb=0.0, deriv_cached=1, tile_uncached=0)
        on = emme_amd.Context(p, device=0, node_cache_gb=0.0, deriv_cached=1, tile_uncached=1)
        off.profile(True), on.profile(True)
        return [("omega-lane", off), ("tile", on)]

    pair = pair_for(256)
    fill_row(res, "N=256, 128 lattice omegas: M, M'", pair, lattice, a.repeat)
    search_row(res, "N=256, Newton, 128 guesses", pair, lattice, a.repeat)
    # the late-search shape of tools/tile_vs_wl.py: the omegas of the secant search still live at its step 10
    _, it2, _, its = pair[0][1].solve_roots(lattice, want_iterates=True)
    w10 = np.ascontiguousarray(its[np.flatnonzero(it2 > 10), 10])
    fill_row(res, f"N=256, {len(w10)} omegas live at step 10", pair, w10, a.repeat)
    for _, ctx in pair:
        ctx.close()
    if not a.skip_1024:
        pair = pair_for(1024)
        w32 = np.ascontiguousarray(lattice[::4])
        fill_row(res, "N=1024, 32 lattice omegas: M, M'", pair, w32, a.repeat)
        search_row(res, "N=1024, Newton, 32 guesses", pair, w32, a.repeat)
        for _, ctx in pair:
            ctx.close()
    if a.out:
        with open(a.out + ".txt", "w") as f:
            f.write("\n".join(LINES) + "\n")
        with open(a.out + ".json", "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
