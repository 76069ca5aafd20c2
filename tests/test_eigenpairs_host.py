"""Newton on the eigenpair, host side: the two new symbols with their argtypes and wrappers, and the
argument errors that are found before any device is looked for.  No GPU.

Without a device there is no context, so the calls below pass a context pointer that is never dereferenced: every
pointer and range is checked before the context is read (the pattern of tests/test_contour_sets_host.py).  The errors
that need a real context -- dim or n above 2048, a bad v0 row, a set without a binding -- are in
tests/test_gpu_eigenpairs.py."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMME_EINVAL = -1


def test_symbols_argtypes_and_wrappers_exist(emme):
    lib = emme.load()
    assert lib.emme_version() == 4
    want = {"emme_solve_eigenpairs": 13, "emme_eigenpair_step_batch": 10}
    hdr = open(os.path.join(ROOT, "include", "emme_hip.h")).read()
    for name, nargs in want.items():
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, (name, fn.argtypes)
        assert name in hdr
    # tol travels as a double, the counts as ints: a float passed where ctypes would guess an int is the classic slip
    assert lib.emme_solve_eigenpairs.argtypes[5] is C.c_double
    assert lib.emme_solve_eigenpairs.argtypes[3] is C.c_int and lib.emme_solve_eigenpairs.argtypes[6] is C.c_int
    assert lib.emme_eigenpair_step_batch.argtypes[6] is C.c_int
    for name in ("solve_eigenpairs", "eigenpair_step"):
        assert callable(getattr(emme.Context, name))
    # the start vector's formula is in the header, for callers who want to reproduce v_0
    assert "0.37 sin(1 + i)" in hdr and "0.21 cos(2 i)" in hdr
    mk = open(os.path.join(ROOT, "emme_amd", "csrc", "Makefile")).read()
    assert "eigpair.hip" in mk and "tri_solve.hpp" in mk


def _solve(lib, ctx, n=2, tol=1e-6, step_limit=20, drop=()):
    g = np.zeros(2 * max(n, 1))
    a = {"guesses": g, "roots": np.zeros(2 * max(n, 1)), "vecs": np.zeros(8), "resid": np.zeros(max(n, 1)),
         "iters": np.zeros(max(n, 1), dtype=np.int32), "info": np.zeros(max(n, 1), dtype=np.int32)}
    p = {k: (None if k in drop else v.ctypes.data) for k, v in a.items()}
    return lib.emme_solve_eigenpairs(ctx, None, p["guesses"], n, None, tol, step_limit, p["roots"], p["vecs"], p["resid"],
                                     p["iters"], p["info"], None)


def test_solve_eigenpairs_argument_errors_come_before_the_device(emme):
    lib = emme.load()
    fake = C.c_void_p(1)  # (never dereferenced: every call below fails on another argument first)
    assert _solve(lib, None) == EMME_EINVAL
    for name in ("guesses", "roots", "vecs", "resid", "iters", "info"):
        assert _solve(lib, fake, drop=(name,)) == EMME_EINVAL, name
    for n in (0, -3):
        assert _solve(lib, fake, n=n) == EMME_EINVAL
    assert _solve(lib, fake, step_limit=-1) == EMME_EINVAL
    for tol in (0.0, -1e-6, float("nan")):
        assert _solve(lib, fake, tol=tol) == EMME_EINVAL
    assert "emme_solve_eigenpairs" in emme.last_error()


def test_eigenpair_step_argument_errors_come_before_the_device(emme):
    lib = emme.load()
    fake = C.c_void_p(1)
    buf = np.zeros(16)
    inf = np.zeros(2, dtype=np.int32)
    p, pi = buf.ctypes.data, inf.ctypes.data

    def call(ctx=fake, n=2, nbatch=1, M=p, Mp=p, v=p, tau=p, resid=p, info=pi):
        return lib.emme_eigenpair_step_batch(ctx, n, nbatch, M, Mp, v, 1, tau, resid, info)

    assert call(ctx=None) == EMME_EINVAL
    for kw in ("M", "Mp", "v", "tau", "resid", "info"):
        assert call(**{kw: None}) == EMME_EINVAL, kw
    assert call(n=0) == EMME_EINVAL
    assert call(nbatch=0) == EMME_EINVAL
    assert "emme_eigenpair_step_batch" in emme.last_error()
