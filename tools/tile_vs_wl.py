#!/usr/bin/env python3
"""The table-free tile fill (option tile_uncached = 1, k_assemble_tile) against the omega-lane kernel (option off) on
batches without a node cache.  Development tool, not the bench.  DESIGN.md §5.3b.

Both settings run in THIS process, on a pair of node_cache_gb = 0 contexts of the same parameter set (boxes differ by
up to 15 %, so a number from another run is no partner).  Every call synchronises; each figure is the best of --repeat
(3) calls after one warm-up, and all of them are printed so that the spread is visible.
  fill rows    assemble_ms + deferred_ms of one plain fill (device time of the fill kernel and of the work list)
  search row   wall ms of one emme_solve_roots call and matrices filled per second (omega-points/s)
Rows: N = 256, the bench's 128 lattice omegas; the whole root search on those guesses; the omegas still live at step 10
of that search (tools/fill_probe.py's set); N = 1024, 32 lattice omegas.
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


def say(s):
    print(s, flush=True)
    LINES.append(s)


def fill_ms(ctx, omegas, repeat):
    """(the `repeat` values of assemble_ms + deferred_ms, interval counts, fill kernel, integrals handed over)"""
    ctx.assemble(omegas)  # warm-up
    vals = []
    for _ in range(repeat):
        ctx.profile_read(reset=True)
        M, iv = ctx.assemble(omegas, want_intervals=True)
        pr = ctx.profile_read(reset=True)
        vals.append(pr.assemble_ms + pr.deferred_ms)
    return vals, iv, ctx.fill_kernel().split()[0], ctx.last_deferred(), M


def search_ms(ctx, guesses, repeat):
    ctx.solve_roots(guesses)  # warm-up
    vals, rate = [], []
    for _ in range(repeat):
        ctx.profile_read(reset=True)
        t0 = time.perf_counter()
        roots, iters, info = ctx.solve_roots(guesses)
        ms = (time.perf_counter() - t0) * 1e3
        fills = ctx.profile_read(reset=True).matrices
        vals.append(ms)
        rate.append(fills / (ms * 1e-3))
    return vals, rate, roots, iters, info, ctx.fill_kernel().split()[0]


def fmt(v):
    return "[" + ", ".join(f"{x:.3f}" for x in v) + "]"


def fill_row(res, name, pair, omegas, repeat):
    try:
        fill_row_(res, name, pair, omegas, repeat)
    except Exception as e:  # (a row that cannot be measured is reported as such; the others still are)
        say(f"{name:34s} UNMEASURED: {e}")
        res["rows"][name] = {"unmeasured": str(e)}


def fill_row_(res, name, pair, omegas, repeat):
    row = {"omegas": int(len(omegas))}
    keep = {}
    for label, ctx in pair:
        vals, iv, kern, handed, M = fill_ms(ctx, omegas, repeat)
        keep[label] = (iv, M)
        row[label] = {"ms": vals, "best_ms": min(vals), "omega_points_per_s": len(omegas) / (min(vals) * 1e-3),
                      "kernel": kern, "handed_over": int(handed), "intervals": int(iv.sum())}
        say(f"{name:34s} {label:10s} {kern:16s} best {min(vals):9.3f} ms  {len(omegas) / (min(vals) * 1e-3):9.1f} omega-points/s"
            f"  all {fmt(vals)}  handed over {handed}")
    (iv0, M0), (iv1, M1) = keep["omega-lane"], keep["tile"]
    row["same_intervals"] = bool(np.array_equal(iv0, iv1))
    ok = np.isfinite(M0).all(axis=(1, 2))
    diff = np.array([np.abs(M0[k] - M1[k]).max() / np.abs(M0[k]).max() if ok[k] else 0.0 for k in range(len(omegas))])
    row["max_rel_diff"] = float(diff.max())
    row["median_rel_diff"] = float(np.median(diff))
    kw = int(diff.argmax())
    row["worst_omega"] = [float(np.real(omegas[kw])), float(np.imag(omegas[kw]))]
    row["worst_omega_max_entry"] = float(np.abs(M0[kw]).max())
    row["over_1e-10"] = [[float(np.real(omegas[k])), float(np.imag(omegas[k])), float(diff[k])] for k in np.flatnonzero(diff > 1e-10)]
    row["speedup"] = row["omega-lane"]["best_ms"] / row["tile"]["best_ms"]
    say(f"{name:34s} tile / omega-lane: x{row['speedup']:.2f}; same interval counts: {row['same_intervals']}; "
        f"max entry difference {row['max_rel_diff']:.2e} of max|M| (median {row['median_rel_diff']:.2e}; worst at omega "
        f"{complex(omegas[kw]):.6g}, max|M| {row['worst_omega_max_entry']:.3g}; {len(row['over_1e-10'])} omegas above 1e-10)")
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
        off = emme_amd.Context(p, device=0, node_cache_gb=0.0, tile_uncached=0)
        on = emme_amd.Context(p, device=0, node_cache_gb=0.0, tile_uncached=1)
        off.profile(True), on.profile(True)
        return [("omega-lane", off), ("tile", on)]

    pair = pair_for(256)
    fill_row(res, "N=256, 128 lattice omegas: fill", pair, lattice, a.repeat)
    row = {}
    its = None
    for label, ctx in pair:
        vals, rate, roots, iters, info, kern = search_ms(ctx, lattice, a.repeat)
        row[label] = {"ms": vals, "best_ms": min(vals), "omega_points_per_s": max(rate), "kernel": kern,
                      "converged": int((info == 0).sum())}
        say(f"{'N=256, solve_roots, 128 guesses':34s} {label:10s} {kern:16s} best {min(vals):9.3f} ms  {max(rate):9.1f} omega-points/s"
            f"  all {fmt(vals)}  converged {int((info == 0).sum())}")
        if its is None:
            _, it2, _, its = ctx.solve_roots(lattice, want_iterates=True)
            live = np.flatnonzero(it2 > 10)
    row["speedup"] = row["omega-lane"]["best_ms"] / row["tile"]["best_ms"]
    say(f"{'N=256, solve_roots, 128 guesses':34s} tile / omega-lane: x{row['speedup']:.2f}")
    res["rows"]["N=256, solve_roots, 128 guesses"] = row
    w10 = np.ascontiguousarray(its[live, 10])
    fill_row(res, f"N=256, {len(w10)} omegas live at step 10", pair, w10, a.repeat)
    for _, ctx in pair:
        ctx.close()
    if not a.skip_1024:
        pair = pair_for(1024)
        fill_row(res, "N=1024, 32 lattice omegas: fill", pair, np.ascontiguousarray(lattice[::4]), a.repeat)
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
