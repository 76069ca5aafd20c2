"""Root sensitivities from eigenpairs, host side: the two new symbols with their argtypes and wrappers,
the argument errors that are found before any device is looked for, neighbour_sets, and the chunk plan's self-test
under the sanitizers.  No GPU.

Without a device there is no context, so the calls below pass a context pointer that is never dereferenced: every
pointer, count and dp is checked, and a negative set index refused, before the context is read (the pattern of
tests/test_eigenpairs_host.py).  The errors that need a real context -- no binding, an index beyond the binding, a
zero vector row (its length is the context's dim), n or dim above 2048 -- are in tests/test_gpu_sensitivities.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle.binding import example_stellarator, example_tokamak

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "emme_amd", "csrc")
EMME_EINVAL = -1


def test_symbols_argtypes_and_wrappers_exist(emme):
    lib = emme.load()
    assert lib.emme_version() == 4
    want = {"emme_sym_forms_batch": 14, "emme_root_sensitivities_sets": 15}
    hdr = open(os.path.join(ROOT, "include", "emme_hip.h")).read()
    for name, nargs in want.items():
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, (name, fn.argtypes)
        assert name in hdr
    forms, sens = lib.emme_sym_forms_batch.argtypes, lib.emme_root_sensitivities_sets.argtypes
    # counts travel as ints, everything else as pointers: n, nmat, nvec, nitems / nroots, ndir, max_items
    assert [k for k, t in enumerate(forms) if t is C.c_int] == [1, 2, 5, 7]
    assert [k for k, t in enumerate(sens) if t is C.c_int] == [1, 5, 9]
    assert all(t is C.c_void_p for k, t in enumerate(forms) if k not in (1, 2, 5, 7))  # form, fro2, ...
    assert all(t is C.c_void_p for k, t in enumerate(sens) if k not in (1, 5, 9))      # dp, dwdp, ...
    for name in ("sym_forms", "root_sensitivities"):
        assert callable(getattr(emme.Context, name))
    assert callable(emme.neighbour_sets) and "neighbour_sets" in emme.__all__
    # the formula and the symmetry it rests on are in the header
    assert "v^T (dM/dp) v / (v^T M' v)" in hdr and "M = M^T" in hdr
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = mk.split("SRCS =")[1].split("HDRS =")[0]
    assert "sym_forms.hip" in srcs and "sens_plan.cpp" in srcs
    assert "sens_plan_selftest" in mk.split("host-sanitize:")[1]
    assert "launch_sym_forms" in open(os.path.join(CSRC, "launch.hpp")).read()


def test_sym_forms_argument_errors_come_before_the_device(emme):
    lib = emme.load()
    fake = C.c_void_p(1)  # (never dereferenced: every call below fails on another argument first)
    buf = np.zeros(64)
    idx = np.zeros(2, dtype=np.int32)
    p, pi = buf.ctypes.data, idx.ctypes.data

    def call(ctx=fake, n=2, nmat=1, A=p, B=p, nvec=1, vecs=p, nitems=2, a=pi, b=pi, x=pi, y=pi, form=p, fro2=p):
        return lib.emme_sym_forms_batch(ctx, n, nmat, A, B, nvec, vecs, nitems, a, b, x, y, form, fro2)

    assert call(ctx=None) == EMME_EINVAL
    for kw in ("A", "vecs", "a", "x", "form"):
        assert call(**{kw: None}) == EMME_EINVAL, kw
    for kw in ("n", "nmat", "nvec", "nitems"):
        assert call(**{kw: 0}) == EMME_EINVAL, kw
    assert call(B=None) == EMME_EINVAL  # b names second matrices that do not exist
    assert "emme_sym_forms_batch" in emme.last_error()
    for kw, bad in (("a", 1), ("a", -1), ("b", 1), ("b", -2), ("x", 1), ("x", -1), ("y", 1), ("y", -1)):
        arr = np.array([0, bad], dtype=np.int32)
        assert call(**{kw: arr.ctypes.data}) == EMME_EINVAL, (kw, bad)
        assert "emme_sym_forms_batch" in emme.last_error() and kw + "[1]" in emme.last_error()


def test_root_sensitivities_argument_errors_come_before_the_device(emme):
    lib = emme.load()
    fake = C.c_void_p(1)
    buf = np.ones(64)
    idx = np.zeros(4, dtype=np.int32)
    p, pi = buf.ctypes.data, idx.ctypes.data

    def call(ctx=fake, nroots=2, set=pi, roots=p, vecs=p, ndir=2, set_plus=pi, set_minus=pi, dp=p, max_items=0, dwdp=p,
             denom=p, corr=p, cond=p, info=pi):
        return lib.emme_root_sensitivities_sets(ctx, nroots, set, roots, vecs, ndir, set_plus, set_minus, dp, max_items,
                                                dwdp, denom, corr, cond, info)

    assert call(ctx=None) == EMME_EINVAL
    for kw in ("set", "roots", "vecs", "set_plus", "set_minus", "dp", "dwdp", "denom", "corr", "cond", "info"):
        assert call(**{kw: None}) == EMME_EINVAL, kw
    for kw, bad in (("nroots", 0), ("nroots", -1), ("ndir", -1), ("max_items", -1)):
        assert call(**{kw: bad}) == EMME_EINVAL, (kw, bad)
    assert "emme_root_sensitivities_sets" in emme.last_error()
    for bad in (0.0, float("nan"), float("inf")):
        d = np.array([1e-4, 1e-4, bad, 1e-4])
        assert call(dp=d.ctypes.data) == EMME_EINVAL, bad
        assert "emme_root_sensitivities_sets" in emme.last_error() and "dp[2]" in emme.last_error()
    neg = np.array([0, -1, 0, 0], dtype=np.int32)
    for kw in ("set", "set_plus", "set_minus"):
        assert call(**{kw: neg.ctypes.data}) == EMME_EINVAL, kw
        assert "emme_root_sensitivities_sets" in emme.last_error()


def test_neighbour_sets_counts_indices_and_dp(emme):
    base = example_tokamak(npoints=16)
    bases = [base, dict(base, k_rho=base["k_rho"] * 1.05)]
    names = ["eta_i", "k_rho", "shat"]
    params, st, sp, sm, dp = emme.neighbour_sets(bases, names, rel_step=1e-4)
    assert len(params) == 2 + 2 * 2 * 3
    assert st.tolist() == [0, 1] and sp.shape == sm.shape == dp.shape == (2, 3)
    assert sorted(sp.ravel().tolist() + sm.ravel().tolist()) == list(range(2, 14))
    for b, d in enumerate(bases):
        assert all(getattr(params[b], k) == d[k] for k in names)
        for k, name in enumerate(names):
            plus, minus = params[sp[b, k]], params[sm[b, k]]
            assert getattr(plus, name) == d[name] * (1 + 1e-4) or getattr(plus, name) == d[name] + d[name] * 1e-4
            assert dp[b, k] == getattr(plus, name) - getattr(minus, name)
            assert abs(dp[b, k] / (2e-4 * d[name]) - 1) < 1e-12
            # only the named parameter moved
            for other in ("eta_i", "k_rho", "shat", "q", "tau", "epsilon_n"):
                if other != name:
                    assert getattr(plus, other) == d[other] and getattr(minus, other) == d[other]
            assert emme.params_same_shape(params[0], plus) and emme.params_same_shape(params[0], minus)
    # one base given as a dict
    params, st, sp, sm, dp = emme.neighbour_sets(base, ["q"])
    assert len(params) == 3 and st.tolist() == [0] and sp.tolist() == [[1]] and sm.tolist() == [[2]]


def test_neighbour_sets_absolute_step_for_a_zero_parameter(emme):
    base = example_tokamak(npoints=16)
    assert base["theta"] == 0.0
    params, _, sp, sm, dp = emme.neighbour_sets(base, ["theta"], rel_step=1e-3)
    assert params[sp[0, 0]].theta == 1e-3 and params[sm[0, 0]].theta == -1e-3 and dp[0, 0] == 2e-3


def test_neighbour_sets_refuses_shape_changes(emme):
    es = example_tokamak(npoints=16)
    em = example_stellarator(npoints=8)
    for base, name, kw in ((es, "npoints", {}), (es, "integration_start_points", {}), (es, "iteration_method", {}),
                           (es, "beta_e", {}),                 # 0 -> +-rel_step: electrostatic to electromagnetic
                           (em, "beta_e", {"rel_step": 2.0}),  # 0.02 -> -0.02 .. 0.06: across 0
                           (em, "beta_e", {"rel_step": 1.0})):  # reaches 0
        with pytest.raises(ValueError):
            emme.neighbour_sets(base, [name], **kw)
    emme.neighbour_sets(em, ["beta_e"])  # a small step of a non-zero beta_e is fine
    with pytest.raises(ValueError):
        emme.neighbour_sets([es, em], ["eta_i"])  # bases of two shapes


def test_chunk_plan_selftest_under_the_sanitizers(tmp_path):
    """The stand-alone self-test of the chunk plan, as `make host-sanitize` builds it (the whole target takes minutes;
    its other programs have tests of their own)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "sens_plan_selftest")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(CSRC, "sens_plan.cpp"),
                    os.path.join(CSRC, "sens_plan_selftest.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "sens_plan_selftest: ok" in r.stdout
