#!/usr/bin/env python3
"""The table-free tile fill of electromagnetic and GK31 contexts (tile_uncached = 1 with tile shapes ALL,
k_assemble_tile_shape<PTS, NM>) against the omega-lane kernel (shapes at their default) on batches without a node cache.
Development tool, not the bench.  DESIGN.md §5.3c; measured the way §5.3b was (tools/tile_vs_wl.py).

Both settings run in THIS process, on a pair of node_cache_gb = 0, tile_uncached = 1 contexts of the same parameter set:
one with shapes off (the partner), one with shapes ALL.  The two alternate inside every repeat; every call
synchronises; each figure is the best of --repeat (3) calls after one warm-up, and all of them are printed so that the
spread is visible.  A difference counts when it exceeds three times the spread of the repeats.
  fill rows    assemble_ms + deferred_ms of one plain fill (device time of the fill kernel and of the work list)
  search row   wall ms of one emme_solve_roots call and matrices filled per second
One row per invocation (--row), one GPU step each:
  stell256      stellarator N = 256 (dim 512, GK31 EM), 128 lattice omegas around (-1.656, 2.490): one plain fill
  stell256-roots   the same context's whole emme_solve_roots on those guesses
  tok-em15      tokamak beta_e = 0.02 (GK15 EM) N = 256, the bench's 128 lattice omegas
  tok-es31      tokamak GK31 (electrostatic) N = 256, the bench's 128 lattice omegas
  stell1024     stellarator N = 1024 (dim 2048), 4 lattice omegas: one plain fill
--out FILE appends what is printed to FILE."""
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


def fmt(v):
    return "[" + ", ".join(f"{x:.3f}" for x in v) + "]"


def pair_for(d):
    p = emme_amd.params_from_dict(d)
    off = emme_amd.Context(p, device=0, node_cache_gb=0.0, tile_uncached=1)
    on = emme_amd.Context(p, device=0, node_cache_gb=0.0, tile_uncached=1)
    on.set_tile_shapes(emme_amd.TILE_SHAPES_ALL)
    off.profile(True), on.profile(True)
    return [("omega-lane", off), ("tile-shape", on)]


def fill_row(name, pair, omegas, repeat):
    vals = {label: [] for label, _ in pair}
    keep = {}
    for _, ctx in pair:
        ctx.assemble(omegas)  # warm-up
    for _ in range(repeat):
        for label, ctx in pair:
            ctx.profile_read(reset=True)
            M, iv = ctx.assemble(omegas, want_intervals=True)
            pr = ctx.profile_read(reset=True)
            vals[label].append(pr.assemble_ms + pr.deferred_ms)
            keep[label] = (iv, M, ctx.fill_kernel_symbol(), ctx.last_deferred())
    for label, _ in pair:
        v = vals[label]
        iv, _, kern, handed = keep[label]
        say(f"{name:28s} {label:10s} {kern:30s} best {min(v):10.3f} ms  {len(omegas) / (min(v) * 1e-3):9.1f} omega-points/s"
            f"  all {fmt(v)}  spread {max(v) - min(v):.3f}  intervals {int(iv.sum())}  handed over {handed}")
    (iv0, M0, _, _), (iv1, M1, _, _) = keep["omega-lane"], keep["tile-shape"]
    ok = np.isfinite(M0).all(axis=(1, 2))
    diff = np.array([np.abs(M0[k] - M1[k]).max() / np.abs(M0[k]).max() if ok[k] else 0.0 for k in range(len(omegas))])
    kw = int(diff.argmax())
    b0, b1 = min(vals["omega-lane"]), min(vals["tile-shape"])
    spread = max(max(v) - min(v) for v in vals.values())
    say(f"{name:28s} tile-shape / omega-lane: x{b0 / b1:.2f} (difference {b0 - b1:+.3f} ms, 3 x spread {3 * spread:.3f} ms); "
        f"interval totals equal omega by omega: {bool(np.array_equal(iv0, iv1))}; max entry difference {diff.max():.2e} of max|M| "
        f"(worst at omega {complex(omegas[kw]):.6g}; {int((diff > 1e-10).sum())} omegas above 1e-10)")


def search_row(name, pair, guesses, repeat):
    vals = {label: [] for label, _ in pair}
    keep = {}
    for _, ctx in pair:
        ctx.solve_roots(guesses)  # warm-up
    for _ in range(repeat):
        for label, ctx in pair:
            ctx.profile_read(reset=True)
            t0 = time.perf_counter()
            roots, iters, info = ctx.solve_roots(guesses)
            ms = (time.perf_counter() - t0) * 1e3
            keep[label] = (roots, iters, info, ctx.profile_read(reset=True).matrices, ctx.fill_kernel_symbol())
            vals[label].append(ms)
    for label, _ in pair:
        v = vals[label]
        roots, iters, info, fills, kern = keep[label]
        say(f"{name:28s} {label:10s} {kern:30s} best {min(v):10.3f} ms  {fills / (min(v) * 1e-3):9.1f} omega-points/s"
            f"  all {fmt(v)}  spread {max(v) - min(v):.3f}  converged {int((info == 0).sum())}  matrices {fills}")
    (r0, i0, f0, _, _), (r1, i1, f1, _, _) = keep["omega-lane"], keep["tile-shape"]
    both = (f0 == 0) & (f1 == 0)
    b0, b1 = min(vals["omega-lane"]), min(vals["tile-shape"])
    spread = max(max(v) - min(v) for v in vals.values())
    say(f"{name:28s} tile-shape / omega-lane: x{b0 / b1:.2f} (difference {b0 - b1:+.3f} ms, 3 x spread {3 * spread:.3f} ms); "
        f"chains converged in both: {int(both.sum())}, same step counts: {int((i0[both] == i1[both]).sum())}, "
        f"largest |root difference| {np.abs(r0[both] - r1[both]).max() if both.any() else 0.0:.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--row", required=True, choices=["stell256", "stell256-roots", "tok-em15", "tok-es31", "stell1024"])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg4 = bench.lattice_cfg4(0)  # 128 guesses around (-1.656, 2.490)
    lat = bench.lattice(1, 0, 128)
    if a.row == "stell256":
        pair = pair_for(dict(bench.STELLARATOR, npoints=256))
        fill_row("stellarator N=256, 128 w", pair, cfg4, a.repeat)
    elif a.row == "stell256-roots":
        pair = pair_for(dict(bench.STELLARATOR, npoints=256))
        search_row("stellarator N=256 solve_roots", pair, cfg4, a.repeat)
    elif a.row == "tok-em15":
        pair = pair_for(bench.workload_dict(256, beta_e=0.02))
        fill_row("tokamak EM GK15 N=256, 128 w", pair, lat, a.repeat)
    elif a.row == "tok-es31":
        pair = pair_for(bench.workload_dict(256, integration_start_points=31))
        fill_row("tokamak ES GK31 N=256, 128 w", pair, lat, a.repeat)
    else:
        pair = pair_for(dict(bench.STELLARATOR, npoints=1024))
        fill_row("stellarator N=1024, 4 w", pair, np.ascontiguousarray(cfg4[::32]), a.repeat)
    for _, ctx in pair:
        ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
