#!/usr/bin/env python3
"""A/B of the folded secant eigenpair step (option eigpair_fold): the parent commit's library, this
library with the option off, and this library with it on.

Cells:
  golden256  solve_eigenpairs(secant=True) on the distinct golden roots x (1 + 1e-3), headline parameters, N = 256
  golden512  the same starts at N = 512 (config 5's parameters: bench.workload_dict(512, k_rho = its first k_rho))
  contour    find_eigenpairs_in_contour(exact=0) on the first two ellipses of tools/contour_eigenpairs.py, N = 256

Every figure comes from a fresh process (the variants alternate, `--rounds` rounds): a warm-up call, then three timed
calls, best of three -- wall time of the whole call, and its K_LIN / K_NULL spans.  Per cell and variant the rounds'
bests are printed with their spread (max - min); the parent's spread stands beside every difference.  Last, unless
--no-bench, `python bench.py --gpus 1 --steps 10 --warmup 3` once on this library and once on the parent's (the bench
runs no eigenpair search: it shows that nothing else moved).

    python3 tools/eigpair_fold_ab.py --parent-lib /path/to/parent/libemme_hip.so [--out profiles/eigpair_fold_ab.txt]

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

ELLIPSES = [(-0.80 + 0.25j, (0.25, 0.20)), (-0.641 - 0.232j, (0.085, 0.05))]
CELLS = ["golden256", "contour", "golden512"]
VARIANTS = ["parent", "off", "on"]


def worker(cell, fold):
    import bench
    import emme_amd as emme
    from tools.eigenpairs_vs_newton import golden_roots

    emme.load()
    if cell == "golden512":
        krs, _ = bench.sweep_cfg5(0)
        d = bench.workload_dict(512, k_rho=float(krs[0]))
    else:
        d = bench.workload_dict(256)
    g = golden_roots() * (1 + 1e-3)
    with emme.Context(emme.params_from_dict(d), device=0) as ctx:
        if fold:
            ctx.set_eigpair_fold(1)
        ctx.profile(True)

        def call():
            if cell == "contour":
                return [ctx.find_eigenpairs_in_contour(c, ab, exact=False) for c, ab in ELLIPSES]
            return ctx.solve_eigenpairs(g, secant=True)

        call()  # warm-up: the cache settles
        runs = []
        for _ in range(3):
            ctx.profile_read(reset=True)
            t0 = time.perf_counter()
            out = call()
            ms = (time.perf_counter() - t0) * 1e3
            p = ctx.profile_read(reset=True)
            runs.append((ms, p.linstep_ms, p.nullspace_ms))
        best = min(runs)
        res = {"wall_ms": best[0], "k_lin_ms": best[1], "k_null_ms": best[2],
               "folded_steps": ctx.last_folded_eigpair_steps() if fold else 0}
        if cell == "contour":
            res["roots"] = sum(r["n_roots"] for r in out)
            res["iters"] = int(sum(r["iters"].sum() for r in out))
        else:
            res["roots"] = int((out[4] == 0).sum())
            res["iters"] = int(out[3].sum())
            res["resid_max"] = float(np.nanmax(out[2]))
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=os.environ.get("EMME_PARENT_LIB"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eigpair_fold_ab.txt"))
    ap.add_argument("--cells", default=",".join(CELLS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--worker", nargs=2, metavar=("CELL", "FOLD"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], int(a.worker[1]))
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the parent commit's libemme_hip.so is needed")
    lines = ["$ python3 tools/eigpair_fold_ab.py --cells " + a.cells + f" --rounds {a.rounds}",
             "parent = the parent commit's library through EMME_LIB; off = this library, eigpair_fold = 0 (the default); "
             "on = this library after set_eigpair_fold(1).",
             "Every figure from a fresh process, variants alternating; in a process a warm-up call, then three timed calls, "
             "best of three: wall ms of the whole call;",
             "K_LIN / K_NULL: those spans of the best call, mean over the rounds; steps: the chains' iteration counts summed; "
             "folded: folded steps of the last call."]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for cell in a.cells.split(","):
        got = {v: [] for v in VARIANTS}
        for _ in range(a.rounds):
            for v in VARIANTS:
                env = dict(os.environ)
                env.pop("EMME_EIGPAIR_FOLD", None)
                env.pop("EMME_LIB", None)
                if v == "parent":
                    env["EMME_LIB"] = os.path.abspath(a.parent_lib)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", cell, "1" if v == "on" else "0"],
                                   env=env, capture_output=True, text=True, timeout=300)
                res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not res:
                    say(f"{cell} {v}: the worker failed (exit {r.returncode}): {r.stderr[-400:]}")
                    sys.exit(1)  # (nothing more is started on the device after a failure)
                got[v].append(json.loads(res[-1][7:]))
        say(f"{cell}: best of three per fresh process, {a.rounds} rounds, variants alternating")
        say(f"  {'variant':8s} {'wall ms per round':28s} {'mean':>8s} {'spread':>7s}  {'K_LIN':>7s} {'K_NULL':>7s}  roots  steps  folded")
        stat = {}
        for v in VARIANTS:
            w = [x["wall_ms"] for x in got[v]]
            stat[v] = (float(np.mean(w)), max(w) - min(w))
            x = got[v][-1]
            say(f"  {v:8s} {str([round(t, 2) for t in w]):28s} {stat[v][0]:8.2f} {stat[v][1]:7.2f}  "
                f"{np.mean([y['k_lin_ms'] for y in got[v]]):7.2f} {np.mean([y['k_null_ms'] for y in got[v]]):7.2f}  "
                f"{x['roots']:5d}  {x['iters']:5d}  {x['folded_steps']:6d}"
                + (f"  resid max {x['resid_max']:.1e}" if "resid_max" in x else ""))
        sp = stat["parent"][1]
        for v in ("off", "on"):
            dms = stat[v][0] - stat["parent"][0]
            say(f"  {v} against parent: {dms:+.2f} ms ({100.0 * dms / stat['parent'][0]:+.1f} %); the parent's spread is {sp:.2f} ms"
                + (": inside it" if abs(dms) <= sp else (": a loss" if dms > 0 else ": a win")))
    if not a.no_bench:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3"]
        say("$ python bench.py --gpus 1 --steps 10 --warmup 3   (this library, then EMME_LIB = the parent's)")
        for v in ("new", "parent"):
            env = dict(os.environ)
            env.pop("EMME_EIGPAIR_FOLD", None)
            env.pop("EMME_LIB", None)
            if v == "parent":
                env["EMME_LIB"] = os.path.abspath(a.parent_lib)
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not out:
                say(f"bench {v}: failed (exit {r.returncode}): {r.stderr[-400:]}")
                sys.exit(1)
            line = json.loads(out[-1])
            say(f"  bench {v:7s} {line['ms_per_step']:.3f} ms per search, {line['value']:.0f} {line['unit']}")
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
