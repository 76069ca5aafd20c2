#!/usr/bin/env python3
"""Root sensitivities from eigenpairs (emme_root_sensitivities_sets) against what a user did before for
the same numbers: solve_eigenpairs(set=+-, guesses=root, v0=v) on all 2 ndir neighbour sets of every root, then
differences of the roots.

Cells: the headline parameters at N = 256 with 6 parameters, for 1 root and for 9 roots (9 base sets along k_rho, one
root each); the stellarator shape at N = 256 (dim 512) with 3 parameters; N = 64 with 32 base sets x 1 root x 2
parameters.  Both routes alternate in one process after a warm-up, three runs each, wall time of the whole calls, best
of three; the re-solve runs at tol 1e-10 (at the default 1e-6 its difference of two roots carries 1e-2 of a 1e-4 step).
Also: the forms kernel's time (the K_OTHER span of emme_sym_forms_batch on device matrices: k_sym_forms +
k_sym_forms_finish) with and without the 64-row block split, at dim 512 with 6 and with 300 items.

    python3 tools/sensitivities_vs_resolve.py [--out profiles/sensitivities.txt]

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

REL_STEP = 1e-4
TOL = 1e-10


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def cell(say, name, bases, names):
    params, st, sp, sm, dp = emme.neighbour_sets(bases, names, rel_step=REL_STEP)
    nb, nd = len(bases), len(names)
    with emme.Context(params[0], device=0) as ctx:
        ctx.bind_param_sets(params)
        guess = complex(*bases[0]["initial_guess"])
        r0, _, info = ctx.solve_roots_sets(st, [guess] * nb)
        w, v, resid, _, info2 = ctx.solve_eigenpairs(r0, set=st, tol=TOL)
        if (info != 0).any() or (info2 != 0).any() or not (resid < 1e-4).all():
            say(f"{name}: no eigenpair from the example's guess (info {info} {info2}, resid {resid}): cell left out")
            return
        if not (resid < 1e-10).all():
            say(f"{name}: the eigenpair search stopped at resid {resid.max():.1e} (root {w[int(np.argmax(resid))]:.6f}): "
                f"the roots of this cell are defined no better than that, and so is a difference of two of them")
        both = np.concatenate([sp.ravel(), sm.ravel()])
        g = np.tile(np.repeat(w, nd), 2)
        v0 = np.tile(np.repeat(v, nd, axis=0), (2, 1))

        def new():
            return ctx.root_sensitivities(st, w, v, sp, sm, dp)

        def old():
            wpm, _, rs, its, inf = ctx.solve_eigenpairs(g, set=both, v0=v0, tol=TOL)
            return ((wpm[:nb * nd] - wpm[nb * nd:]) / dp.ravel()).reshape(nb, nd), its, inf

        new(), old()  # warm-up
        runs = {"sensitivities": [], "re-solve": []}
        keep = {}
        for _ in range(3):
            for label, fn in (("sensitivities", new), ("re-solve", old)):
                ms, keep[label] = timed(fn)
                runs[label].append(ms)
        for label, rs in runs.items():
            say(f"{name:28s} {label:14s} wall ms {[round(r, 2) for r in rs]}")
        bn, bo = min(runs["sensitivities"]), min(runs["re-solve"])
        dwdp, denom, corr, cond, inf = keep["sensitivities"]
        fd, its, inf_o = keep["re-solve"]
        say(f"{name:28s} best wall: sensitivities {bn:.2f} ms, re-solve {bo:.2f} ms ({2 * nb * nd} chains, "
            f"{np.mean(its):.1f} steps each): x{bo / bn:.2f}{' (loses)' if bn > bo else ''};  dim {ctx.dim}, "
            f"{2 * nb} + {2 * nb * nd} matrices filled;  info {sorted(set(inf.tolist()))};  largest relative "
            f"disagreement of the two answers {np.nanmax(np.abs(dwdp - fd) / np.abs(dwdp)):.1e};  cond "
            f"{cond.min():.3g} .. {cond.max():.3g}, |corr| max {np.abs(corr).max():.1e}")


def forms_split(say, n=512):
    import ctypes as C

    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rng = np.random.default_rng(1)
    block = rng.normal(size=(6, n, n)) + 1j * rng.normal(size=(6, n, n))  # (dealt round-robin into the device tables)
    v = rng.normal(size=(1, n)) + 0j
    with emme.Context(emme.params_from_dict(bench.workload_dict(16)), device=0) as ctx:
        ctx.profile(True)
        for nitems in (6, 300):
            dA, dB = C.c_void_p(), C.c_void_p()
            nbytes = nitems * n * n * 16
            assert hip.hipMalloc(C.byref(dA), nbytes) == 0 and hip.hipMalloc(C.byref(dB), nbytes) == 0
            for base, shift in ((dA, 0), (dB, 1)):
                for k in range(0, nitems, 6):
                    src = np.ascontiguousarray(np.roll(block, shift, axis=0))
                    assert hip.hipMemcpy(base.value + k * n * n * 16, src.ctypes.data, min(6, nitems - k) * n * n * 16, 1) == 0
            idx = np.arange(nitems)

            def run():
                ctx.profile_read(reset=True)
                out = ctx.sym_forms((nitems, n), None, v, idx, idx, np.zeros(nitems, dtype=int),
                                    a_device_ptr=dA.value, b_device_ptr=dB.value)
                return ctx.profile_read(reset=True).other_ms, out

            res = {}
            for split in ("1", "0", "1", "0"):
                os.environ["EMME_SYM_FORMS_SPLIT"] = split
                run()
                res.setdefault(split, []).extend(run()[0] for _ in range(5))
            os.environ.pop("EMME_SYM_FORMS_SPLIT")
            hip.hipFree(dA), hip.hipFree(dB)
            b1, b0 = min(res["1"]), min(res["0"])
            gb = 2 * nitems * n * n * 16 / 1e9
            say(f"forms kernel dim {n} {nitems:3d} items ({gb:.2f} GB read): 64-row blocks ({nitems * (n // 64)} workgroups) "
                f"{b1 * 1e3:.1f} us = {gb / b1:.2f} TB/s;  one workgroup per item {b0 * 1e3:.1f} us = {gb / b0:.2f} TB/s: "
                f"the split is x{b0 / b1:.2f}{' (loses)' if b1 > b0 else ''}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensitivities.txt"))
    a = ap.parse_args()
    lines = ["$ python3 tools/sensitivities_vs_resolve.py"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    emme.load()
    six = ["eta_i", "k_rho", "shat", "q", "tau", "epsilon_n"]
    head = bench.workload_dict(256)
    cell(say, "headline N256 1 root x 6", [head], six)
    cell(say, "headline N256 9 roots x 6", [dict(head, k_rho=head["k_rho"] * (1 + 0.01 * k)) for k in range(9)], six)
    cell(say, "stellarator N256 1 root x 3", [dict(bench.STELLARATOR)], ["eta_i", "k_rho", "beta_e"])
    small = bench.workload_dict(64)
    cell(say, "N64 32 sets x 1 root x 2", [dict(small, k_rho=small["k_rho"] * (1 + 0.01 * k)) for k in range(32)],
         ["eta_i", "k_rho"])
    forms_split(say)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
