#!/usr/bin/env python3
"""A/B of mirror-image pairs for electromagnetic and GK31 contexts (emme_ctx_set_mirror_shapes): the
parent commit's library, this library at its default (MIRROR_SHAPES_ES15), and this library with MIRROR_SHAPES_ALL.

Cells (N = 256 each, 128 omegas):
  cfg4   BASELINE configs[3] as tools/run_configs.py runs it: the stellarator example (electromagnetic, GK31, dim 512),
         share 0 of the 32 x 32 lattice, solve_roots(step_limit=7, tol=0): 8 steps per chain
  em15   the tokamak example with beta_e = 0.02 (electromagnetic, GK15, dim 512), the bench lattice, default search
  gk31   the tokamak example with integration_start_points = 31 (electrostatic, GK31), the bench lattice, default search

Every figure comes from a fresh process (the variants alternate, `--rounds` rounds): one fill of the 128 omegas that
builds the cache, three timed fills, a warm-up search, three timed searches; best of three each.  A fill is timed by
its spans (dense fill + deferred pass: the host copy of 128 matrices is not the subject), a search by its wall time.
Per cell and variant the rounds' bests are printed with their spread (max - min); the parent's spread stands beside
every difference.  Then, chain by chain, info, iteration counts and roots of the last search, parent against both.
Last, unless --no-bench, `python bench.py --gpus 1 --steps 10 --warmup 3` alternating on the parent's library and this
one, `--rounds` times each.

    python3 tools/mirror_shapes_ab.py --parent-lib /path/to/parent/libemme_hip.so [--out profiles/mirror_shapes_ab.txt]

One GPU, one process at a time; what is printed is appended to --out."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CELLS = ["cfg4", "em15", "gk31"]
VARIANTS = ["parent", "default", "all"]


def worker(cell, shapes_all):
    import bench
    import emme_amd as emme

    emme.load()
    if cell == "cfg4":
        d, g, kw = dict(bench.STELLARATOR, npoints=256), bench.lattice_cfg4(0), dict(step_limit=7, tol=0.0)
    elif cell == "em15":
        d, g, kw = bench.workload_dict(256, beta_e=0.02), bench.lattice(1, 0), {}
    elif cell == "gk31":
        d, g, kw = bench.workload_dict(256, integration_start_points=31), bench.lattice(1, 0), {}
    else:
        sys.exit(f"unknown cell {cell!r}")
    with emme.Context(emme.params_from_dict(d), device=0) as ctx:
        if shapes_all:
            ctx.set_mirror_shapes(emme.MIRROR_SHAPES_ALL)
        ctx.profile(True)
        ctx.assemble(g)  # builds the cache
        cache_gib, build_ms = ctx.node_cache_gib(), ctx.profile_read(reset=True).cache_build_ms
        fills = []
        for _ in range(3):
            ctx.assemble(g)
            p = ctx.profile_read(reset=True)
            fills.append((p.assemble_ms + p.deferred_ms, p.assemble_ms, p.deferred_ms, p.assemble_launches))
        ctx.solve_roots(g, **kw)  # warm-up: the cache settles
        runs = []
        for _ in range(3):
            ctx.profile_read(reset=True)
            t0 = time.perf_counter()
            roots, iters, info = ctx.solve_roots(g, **kw)
            ms = (time.perf_counter() - t0) * 1e3
            p = ctx.profile_read(reset=True)
            runs.append((ms, p.assemble_ms, p.assemble_launches, p.deferred_ms, p.linstep_ms))
        f, s = min(fills), min(runs)
        res = {"fill_ms": f[0], "fill_dense_ms": f[1], "fill_deferred_ms": f[2], "fill_launches": f[3],
               "search_ms": s[0], "dense_ms": s[1], "dense_launches": s[2], "deferred_ms": s[3], "linstep_ms": s[4],
               "cache_gib": cache_gib, "cache_gib_end": ctx.node_cache_gib(), "cache_build_ms": build_ms,
               "mirror": ctx.mirror_pairs() if hasattr(ctx.lib, "emme_ctx_get_mirror_pairs") else 0,
               "folded": ctx.last_folded_steps() if hasattr(ctx.lib, "emme_ctx_last_folded_steps") else 0,
               "steps": int(iters.sum()), "info": [int(x) for x in info], "iters": [int(x) for x in iters],
               "roots": [[float(r.real), float(r.imag)] for r in roots]}
    print("RESULT " + json.dumps(res), flush=True)


def fresh(cmd, env_lib, timeout):
    env = dict(os.environ)
    for k in ("EMME_MIRROR_SHAPES", "EMME_MIRROR", "EMME_LU_FOLD", "EMME_LIB"):
        env.pop(k, None)
    if env_lib:
        env["EMME_LIB"] = os.path.abspath(env_lib)
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=os.environ.get("EMME_PARENT_LIB"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mirror_shapes_ab.txt"))
    ap.add_argument("--cells", default=",".join(CELLS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--chain-detail", action="store_true", help="only: the chains that differ, parent against all")
    ap.add_argument("--worker", nargs=2, metavar=("CELL", "ALL"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], int(a.worker[1]))
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the parent commit's libemme_hip.so is needed")
    lines = ["$ python3 tools/mirror_shapes_ab.py --cells " + a.cells + (" --chain-detail" if a.chain_detail else f" --rounds {a.rounds}"),
             "parent = the parent commit's library through EMME_LIB; default = this library as it comes "
             "(MIRROR_SHAPES_ES15); all = this library after set_mirror_shapes(MIRROR_SHAPES_ALL).",
             "Every figure from a fresh process, variants alternating; best of three timed calls after a warm-up call.",
             "fill: dense fill + deferred pass spans of one 128-omega assemble call; search: wall ms of one solve_roots; "
             "dense / launch, deferred, LU: spans of the best search; cache: GiB after the first fill -> at the end."]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        del lines[:]

    cells = [c for c in a.cells.split(",") if c]  # (--cells "": the bench alone)
    if a.chain_detail:
        # one more process each for parent and all: which chains differ by more than 1e-9, and what they are
        for cell in cells:
            got = {}
            for v in ("parent", "all"):
                r = fresh([sys.executable, os.path.abspath(__file__), "--worker", cell, "1" if v == "all" else "0"],
                          a.parent_lib if v == "parent" else None, 400)
                res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not res:
                    say(f"{cell} {v}: the worker failed (exit {r.returncode}): {r.stderr[-400:]}")
                    flush()
                    sys.exit(1)
                got[v] = json.loads(res[-1][7:])
            rp = np.array([complex(*z) for z in got["parent"]["roots"]])
            ra = np.array([complex(*z) for z in got["all"]["roots"]])
            rel = np.abs(ra - rp) / np.abs(rp)
            it, limit = np.array(got["parent"]["iters"]), max(got["parent"]["iters"])
            far = np.flatnonzero(~(rel <= 1e-9))
            say(f"{cell}: chains whose roots differ by more than 1e-9 relative, parent against all: {len(far)} of {len(rp)}; "
                f"the largest iteration count of the search is {limit}, reached by {int((it == limit).sum())} chains")
            for k in far:
                say(f"  chain {int(k):3d}: {int(it[k]):2d} iterations (all: {got['all']['iters'][k]}), info {got['parent']['info'][k]} / "
                    f"{got['all']['info'][k]}, parent root {rp[k]:.6g}, difference {rel[k]:.3g}")
            rest = rel[rel <= 1e-9]
            say(f"  the other {len(rest)} chains: max {rest.max() if rest.size else 0.0:.3g}, median {np.median(rest) if rest.size else 0.0:.3g}")
            flush()
        return
    for cell in cells:
        got = {v: [] for v in VARIANTS}
        for _ in range(a.rounds):
            for v in VARIANTS:
                r = fresh([sys.executable, os.path.abspath(__file__), "--worker", cell, "1" if v == "all" else "0"],
                          a.parent_lib if v == "parent" else None, 400)
                res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not res:
                    say(f"{cell} {v}: the worker failed (exit {r.returncode}): {r.stderr[-400:]}")
                    flush()
                    sys.exit(1)  # (nothing more is started on the device after a failure)
                got[v].append(json.loads(res[-1][7:]))
        say(f"{cell}: {a.rounds} rounds, variants alternating")
        stat = {}
        for what, key in (("search", "search_ms"), ("fill", "fill_ms")):
            say(f"  {what:6s} {'variant':8s} {'ms per round':28s} {'mean':>8s} {'spread':>7s}")
            for v in VARIANTS:
                w = [x[key] for x in got[v]]
                stat[what, v] = (float(np.mean(w)), max(w) - min(w))
                say(f"  {'':6s} {v:8s} {str([round(t, 2) for t in w]):28s} {stat[what, v][0]:8.2f} {stat[what, v][1]:7.2f}")
            sp = stat[what, "parent"][1]
            for v in ("default", "all"):
                dms = stat[what, v][0] - stat[what, "parent"][0]
                say(f"  {what} {v} against parent: {dms:+.2f} ms ({100.0 * dms / stat[what, 'parent'][0]:+.1f} %); the parent's "
                    f"spread is {sp:.2f} ms" + (": inside it" if abs(dms) <= sp else (": a loss" if dms > 0 else ": a win")))
        say(f"  {'variant':8s} {'dense ms':>9s} {'launches':>8s} {'ms/launch':>9s} {'deferred':>9s} {'LU':>8s} "
            f"{'fill dense':>10s} {'fill defer':>10s}  cache GiB      build ms  mirror folded steps")
        for v in VARIANTS:
            m = lambda k: float(np.mean([x[k] for x in got[v]]))  # noqa: E731
            x = got[v][-1]
            say(f"  {v:8s} {m('dense_ms'):9.2f} {x['dense_launches']:8d} {m('dense_ms') / max(x['dense_launches'], 1):9.3f} "
                f"{m('deferred_ms'):9.2f} {m('linstep_ms'):8.2f} {m('fill_dense_ms'):10.2f} {m('fill_deferred_ms'):10.2f}  "
                f"{x['cache_gib']:.2f} -> {x['cache_gib_end']:.2f}  {m('cache_build_ms'):8.1f}  {x['mirror']:6d} {x['folded']:6d} "
                f"{x['steps']:5d}")
        ref = got["parent"][-1]
        rr = np.array([complex(*z) for z in ref["roots"]])
        for v in ("default", "all"):
            x = got[v][-1]
            rv = np.array([complex(*z) for z in x["roots"]])
            same_info = int(sum(p == q for p, q in zip(ref["info"], x["info"])))
            same_it = int(sum(p == q for p, q in zip(ref["iters"], x["iters"])))
            both = np.array([p == 0 and q == 0 for p, q in zip(ref["info"], x["info"])]) & np.isfinite(rr) & np.isfinite(rv)
            rel = np.abs(rv - rr)[both] / np.abs(rr)[both]
            bits = int(sum(p == q for p, q in zip(ref["roots"], x["roots"])))
            say(f"  chains, parent against {v}: info equal {same_info} / {len(rr)}, iteration counts equal {same_it} / {len(rr)}, "
                f"roots bit-equal {bits} / {len(rr)}; of the {int(both.sum())} chains with info 0 in both, root difference "
                f"max {rel.max() if rel.size else 0.0:.3g}, median {np.median(rel) if rel.size else 0.0:.3g} relative; "
                f"worst chains {[int(k) for k in np.flatnonzero(both)[np.argsort(rel)[-3:]]] if rel.size else []}")
        flush()
    if not a.no_bench:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3"]
        say(f"$ python bench.py --gpus 1 --steps 10 --warmup 3   (EMME_LIB = the parent's, then this library: {a.rounds} rounds)")
        ms = {"parent": [], "new": []}
        for _ in range(a.rounds):
            for v in ("parent", "new"):
                r = fresh(cmd, a.parent_lib if v == "parent" else None, 600)
                out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                if r.returncode != 0 or not out:
                    say(f"bench {v}: failed (exit {r.returncode}): {r.stderr[-400:]}")
                    flush()
                    sys.exit(1)
                ms[v].append(json.loads(out[-1])["ms_per_step"])
        for v in ("parent", "new"):
            say(f"  bench {v:7s} {[round(t, 2) for t in ms[v]]} mean {np.mean(ms[v]):.2f} spread {max(ms[v]) - min(ms[v]):.2f} ms per search")
        dms = float(np.mean(ms["new"]) - np.mean(ms["parent"]))
        sp = max(ms["parent"]) - min(ms["parent"])
        say(f"  new against parent: {dms:+.2f} ms; the parent's spread is {sp:.2f} ms" + (": inside it" if abs(dms) <= sp else ""))
        flush()


if __name__ == "__main__":
    main()
