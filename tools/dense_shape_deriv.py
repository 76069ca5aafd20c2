#!/usr/bin/env python3
"""The cached derivative fill of electromagnetic and GK31 contexts (deriv_cached = 1 with derivative cache shapes ALL,
k_assemble_dense_shape_deriv<PTS, NM>) against what such a context runs without the switch.  Development tool, not the
bench.  DESIGN.md §12.5; method of tools/tile_shape_deriv_vs_wl.py (§12.4).

All variants run in THIS process on ONE context that has a settled node cache; a variant is a setting of the context's
switches, put in place before its call.  The variants alternate inside every repeat; every call synchronises; each
figure is the best of --repeat (3) calls after one warm-up of every variant, and all of them are printed so that the
spread is visible.  A difference counts when it exceeds three times the spread of the repeats.
  fill rows    device ms of one fill of M and M' (assemble_ms + deferred_ms + other_ms: the fill kernel, the work list,
               the phase table and list staging) of
                 cached        k_assemble_dense_shape_deriv (switch on; the task order the launcher picks)
                 cached-cm     the same, chunk-major task order   (EMME_EXP_SHAPE_DERIV_ORDER = 0)
                 cached-xcd    the same, XCD-grouped task order   (EMME_EXP_SHAPE_DERIV_ORDER = 1)
                 omega-lane    k_assemble_wl_deriv (switch off)
                 tile-shape    k_assemble_tile_shape_deriv (tile_uncached = 1, tile shapes ALL, switch off)
                 plain-cached  the plain cached fill of M alone, for scale
  search row   wall ms of one root search on the 128 guesses: emme_solve_roots_newton with the switch on (newton-cached),
               off (newton-wl), the tile triple (newton-tile), and emme_solve_roots (secant) on the same cached context
One row per invocation (--row), one GPU step each:
  stell256         stellarator N = 256 (dim 512, GK31 EM), 128 lattice omegas around (-1.656, 2.490)
  stell256-search  the same context's root searches on those guesses
  tok-em15         tokamak beta_e = 0.02 (GK15 EM) N = 256, the bench's 128 lattice omegas
  tok-es31         tokamak GK31 (electrostatic) N = 256, the bench's 128 lattice omegas
--out FILE appends what is printed to FILE (default profiles/dense_shape_deriv.txt)."""
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
ORDER_ENV = "EMME_EXP_SHAPE_DERIV_ORDER"


def say(s):
    print(s, flush=True)
    LINES.append(s)


def fmt(v):
    return "[" + ", ".join(f"{x:.3f}" for x in v) + "]"


def switches(ctx, cached, tile, order=None):
    """deriv_cached stays 1; `cached`: derivative cache shapes ALL; `tile`: the tile pair (tile_uncached, tile shapes ALL)"""
    ctx.set_deriv_cache_shapes(emme_amd.DERIV_CACHE_SHAPES_ALL if cached else emme_amd.DERIV_CACHE_SHAPES_ES15)
    ctx.set_options(tile_uncached=1 if tile else 0)
    ctx.set_tile_shapes(emme_amd.TILE_SHAPES_ALL if tile else emme_amd.TILE_SHAPES_ES15)
    if order is None:
        os.environ.pop(ORDER_ENV, None)
    else:
        os.environ[ORDER_ENV] = str(order)


FILL_VARIANTS = [("cached", (True, False, None)), ("cached-cm", (True, False, 0)), ("cached-xcd", (True, False, 1)),
                 ("omega-lane", (False, False, None)), ("tile-shape", (False, True, None))]


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


def context_for(d, omegas):
    ctx = emme_amd.Context(emme_amd.params_from_dict(d), device=0, deriv_cached=1)
    ctx.profile(True)
    fills = ctx.cache_settle(omegas)
    say(f"context: {ctx.fill_kernel_symbol()}, cache settled in {fills} fills: depth / subtrees / GiB {ctx.cache_state()}")
    return ctx


def device_ms(pr):
    return pr.assemble_ms + pr.deferred_ms + pr.other_ms


def fill_row(name, ctx, omegas, repeat):
    labels = [v[0] for v in FILL_VARIANTS] + ["plain-cached"]
    vals = {label: [] for label in labels}
    keep = {}

    def one(label, record):
        if label == "plain-cached":
            switches(ctx, True, False)
            ctx.profile_read(reset=True)
            ctx.assemble(omegas)
            pr = ctx.profile_read(reset=True)
            out = None
        else:
            switches(ctx, *dict(FILL_VARIANTS)[label])
            ctx.profile_read(reset=True)
            out = deriv(ctx, omegas)
            pr = ctx.profile_read(reset=True)
        if record:
            vals[label].append(device_ms(pr))
            keep[label] = (out, pr.tile_tasks, pr.dense_rounds, pr.sparse_rounds, ctx.last_deferred(), pr.assemble_ms,
                           pr.deferred_ms, pr.other_ms)

    for label in labels:
        one(label, False)  # warm-up
    state = ctx.cache_state()
    for _ in range(repeat):
        for label in labels:
            one(label, True)
    say(f"{name}: cache state unchanged over the row: {ctx.cache_state() == state}")
    for label in labels:
        v = vals[label]
        out, tasks, dr, sr, handed, a_ms, d_ms, o_ms = keep[label]
        iv = f"intervals {int(out[2].sum())}  " if out else ""
        say(f"{name:30s} {label:12s} best {min(v):10.3f} ms  {len(omegas) / (min(v) * 1e-3):9.1f} omega-points/s"
            f"  all {fmt(v)}  spread {max(v) - min(v):.3f}  {iv}tile tasks {tasks}  rounds {dr} MFMA / {sr} vector"
            f"  handed over {handed}  (last call: fill {a_ms:.3f} + list {d_ms:.3f} + other {o_ms:.3f})")
    spread = max(max(v) - min(v) for v in vals.values())
    b = {label: min(vals[label]) for label in labels}
    for other in labels[1:]:
        say(f"{name:30s} cached against {other:12s}: x{b[other] / b['cached']:.2f} ({other} - cached = "
            f"{b[other] - b['cached']:+.3f} ms, 3 x spread {3 * spread:.3f} ms)")
    (M1, Mp1, iv1) = keep["cached"][0]
    for other in ("omega-lane", "tile-shape"):
        (M0, Mp0, iv0) = keep[other][0]
        dm, ok = rel_diff(M1, M0)
        dp, _ = rel_diff(Mp1, Mp0)
        kw = int(dp.argmax())
        say(f"{name:30s} cached against {other:12s}: interval totals equal omega by omega: {bool(np.array_equal(iv0, iv1))}; "
            f"worst difference M {dm.max():.2e} of max|M|, M' {dp.max():.2e} of max|M'| (worst at omega "
            f"{complex(omegas[kw]):.6g}; {int((dp > 1e-10).sum())} omegas above 1e-10; {int(ok.sum())} finite in both)")
    for other in ("cached-cm", "cached-xcd"):
        (M0, Mp0, iv0) = keep[other][0]
        say(f"{name:30s} cached against {other:12s}: bit-identical M, M', counts: "
            f"{bool(np.array_equal(M0.view(np.float64), M1.view(np.float64)) and np.array_equal(Mp0.view(np.float64), Mp1.view(np.float64)) and np.array_equal(iv0, iv1))}")


SEARCH_VARIANTS = [("newton-cached", (True, False, None)), ("newton-wl", (False, False, None)),
                   ("newton-tile", (False, True, None)), ("secant", (True, False, None))]


def search_row(name, ctx, guesses, repeat):
    labels = [v[0] for v in SEARCH_VARIANTS]
    vals = {label: [] for label in labels}
    keep = {}
    limit = ctx.params.iteration_step_limit

    def one(label, record):
        switches(ctx, *dict(SEARCH_VARIANTS)[label])
        ctx.profile_read(reset=True)
        t0 = time.perf_counter()
        roots, iters, info = (ctx.solve_roots if label == "secant" else ctx.solve_roots_newton)(guesses)
        ms = (time.perf_counter() - t0) * 1e3
        pr = ctx.profile_read(reset=True)
        if record:
            vals[label].append(ms)
            keep[label] = (roots, iters, info, pr.matrices, pr.tile_tasks, pr.assemble_ms + pr.deferred_ms, pr.linstep_ms)

    for label in labels:
        one(label, False)  # warm-up
    for _ in range(repeat):
        for label in labels:
            one(label, True)
    for label in labels:
        v = vals[label]
        roots, iters, info, fills, tasks, fill_ms, lin_ms = keep[label]
        conv = (info == 0) & (iters <= limit)
        say(f"{name:30s} {label:14s} best {min(v):10.3f} ms  all {fmt(v)}  spread {max(v) - min(v):.3f}  converged "
            f"{int(conv.sum())}  iterations {int(iters.sum())}  matrices {fills}  tile tasks {tasks}"
            f"  (last call: fills {fill_ms:.3f} ms, linear steps {lin_ms:.3f} ms on the device)")
    spread = max(max(v) - min(v) for v in vals.values())
    b = {label: min(vals[label]) for label in labels}
    for other in labels[1:]:
        say(f"{name:30s} newton-cached against {other:12s}: x{b[other] / b['newton-cached']:.2f} ({other} - newton-cached = "
            f"{b[other] - b['newton-cached']:+.3f} ms, 3 x spread {3 * spread:.3f} ms)")
    (r1, i1, f1) = keep["newton-cached"][:3]
    (r0, i0, f0) = keep["newton-wl"][:3]
    both = (f0 == 0) & (f1 == 0) & (i0 <= limit) & (i1 <= limit)
    with np.errstate(invalid="ignore"):
        same = both & (i0 == i1) & (np.abs(r0 - r1) <= 1e-9 * np.abs(r0))
    say(f"{name:30s} switch on against off: chains converged in both {int(both.sum())}; with equal iteration counts and roots "
        f"within 1e-9 relative {int(same.sum())} of {len(i0)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--row", required=True, choices=["stell256", "stell256-search", "tok-em15", "tok-es31"])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_shape_deriv.txt"))
    a = ap.parse_args()
    cfg4 = bench.lattice_cfg4(0)  # 128 guesses around (-1.656, 2.490)
    lat = bench.lattice(1, 0, 128)
    if a.row == "stell256":
        ctx = context_for(dict(bench.STELLARATOR, npoints=256), cfg4)
        fill_row("stellarator N=256, 128 w", ctx, cfg4, a.repeat)
    elif a.row == "stell256-search":
        ctx = context_for(dict(bench.STELLARATOR, npoints=256), cfg4)
        search_row("stellarator N=256 search", ctx, cfg4, a.repeat)
    elif a.row == "tok-em15":
        ctx = context_for(bench.workload_dict(256, beta_e=0.02), lat)
        fill_row("tokamak EM GK15 N=256, 128 w", ctx, lat, a.repeat)
    else:
        ctx = context_for(bench.workload_dict(256, integration_start_points=31), lat)
        fill_row("tokamak ES GK31 N=256, 128 w", ctx, lat, a.repeat)
    ctx.close()
    with open(a.out, "a") as f:
        f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
