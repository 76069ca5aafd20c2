"""Region search over parameter sets, host side: the new symbols and wrappers, the argument errors
that are found before any device is looked for, and the stand-alone self-test of the round plan.  No GPU.

Without a device there is no context, so the calls below pass a context pointer that is never dereferenced: nitems and
every contour are checked before the context is read.  The two errors that need a real context -- no binding, a set[k]
out of range -- are in tests/test_gpu_contour_sets.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "emme_amd", "csrc")
EMME_EINVAL = -1


def test_symbols_and_wrappers_exist(emme):
    lib = emme.load()
    for name in ("emme_find_roots_in_contours_sets", "emme_contour_moments_groups"):
        assert hasattr(lib, name), name
    assert lib.emme_version() == 4
    for name in ("find_roots_in_contours_sets", "contour_moments_groups"):
        assert callable(getattr(emme.Context, name))
    hdr = open(os.path.join(ROOT, "include", "emme_hip.h")).read()
    assert "emme_find_roots_in_contours_sets" in hdr and "emme_contour_moments_groups" in hdr


def _search(emme, ctx, nitems, set_, cts, tol=1e-6, step_limit=20, max_roots=4, status=True):
    n = max(nitems, 1)
    roots = np.zeros(2 * n * max_roots)
    ints = [np.zeros(n * max_roots, dtype=np.int32) for _ in range(2)] + [np.zeros(n, dtype=np.int32) for _ in range(4)]
    ptrs = [a.ctypes.data for a in ints]
    if not status:
        ptrs[-1] = None
    return emme.load().emme_find_roots_in_contours_sets(ctx, nitems, set_.ctypes.data if set_ is not None else None,
                                                        C.cast(cts, C.c_void_p), 0, tol, step_limit, max_roots,
                                                        roots.ctypes.data, *ptrs)


def test_argument_errors_come_before_the_device(emme):
    fake = C.c_void_p(1)  # (never dereferenced: every call below fails on another argument first)
    st = np.zeros(3, dtype=np.int32)
    good = lambda: emme.contour_default(center=-0.8 + 0.2j, semi_axes=(0.1, 0.1))
    cts = (emme.Contour * 3)(good(), good(), good())
    for nitems in (0, -2):
        assert _search(emme, fake, nitems, st, cts) == EMME_EINVAL
        assert "nitems" in emme.last_error()
    assert _search(emme, None, 3, st, cts) == EMME_EINVAL
    assert _search(emme, fake, 3, None, cts) == EMME_EINVAL
    assert _search(emme, fake, 3, st, cts, tol=0.0) == EMME_EINVAL
    assert _search(emme, fake, 3, st, cts, step_limit=-1) == EMME_EINVAL
    assert _search(emme, fake, 3, st, cts, max_roots=0) == EMME_EINVAL
    assert _search(emme, fake, 3, st, cts, status=False) == EMME_EINVAL
    # every argument rule of the single call, on item 1 or 2; the message names the item
    bad = [(dict(semi_axes=(0.0, 0.1)), "semi-axes"), (dict(semi_axes=(0.1, -0.1)), "semi-axes"),
           (dict(semi_axes=(0.1, float("inf"))), "semi-axes"), (dict(center=complex("nan"), semi_axes=(0.1, 0.1)), "semi-axes"),
           (dict(center=-0.2 + 0.1j, semi_axes=(0.3, 0.1)), "Re omega = 0"), (dict(points=12), "powers of two"),
           (dict(points=2), "powers of two"), (dict(points=64, max_points=32), "powers of two"),
           (dict(max_points=48), "powers of two"), (dict(probes=0), "probes"), (dict(probes=65), "probes"),
           (dict(rank_tol=0.0), "rank_tol"), (dict(rank_tol=1.0), "rank_tol")]
    for q, (over, word) in enumerate(bad):
        k = 1 + q % 2
        items = [good(), good(), good()]
        items[k] = emme.contour_default(**dict(dict(center=-0.8 + 0.2j, semi_axes=(0.1, 0.1)), **over))
        assert _search(emme, fake, 3, st, (emme.Contour * 3)(*items)) == EMME_EINVAL, over
        msg = emme.last_error()
        assert "emme_find_roots_in_contours_sets" in msg and f"item {k}" in msg and word in msg, (over, msg)
    items = [good(), good(), good()]
    items[2].size = 8
    assert _search(emme, fake, 3, st, (emme.Contour * 3)(*items)) == EMME_EINVAL
    assert "item 2" in emme.last_error() and "wrong size" in emme.last_error()
    # the building block
    lib = emme.load()
    one = np.zeros(8)
    p = one.ctypes.data
    g = np.array([0, 2], dtype=np.int32)
    call = lambda ctx, n, nq, grp, ng, L: lib.emme_contour_moments_groups(ctx, n, nq, p, grp, ng, p, p, L, None, p, p, p, p)
    assert call(None, 1, 2, g.ctypes.data, 2, 1) == EMME_EINVAL
    assert call(fake, 1, 2, None, 2, 1) == EMME_EINVAL
    assert call(fake, 0, 2, g.ctypes.data, 3, 1) == EMME_EINVAL
    assert call(fake, 1, 0, g.ctypes.data, 3, 1) == EMME_EINVAL
    assert call(fake, 1, 2, g.ctypes.data, 0, 1) == EMME_EINVAL
    assert call(fake, 1, 2, g.ctypes.data, 3, 65) == EMME_EINVAL
    assert call(fake, 1, 2, g.ctypes.data, 2, 1) == EMME_EINVAL  # group[1] = 2 is outside [0, 2)
    assert "group[1]" in emme.last_error()
    g[1] = -1
    assert call(fake, 1, 2, g.ctypes.data, 2, 1) == EMME_EINVAL


def test_wrapper_checks_its_lists(emme):
    class Stub(emme.Context):
        def __init__(self):  # no device, no handle: the wrapper's own checks come first
            pass

        def __del__(self):
            pass

    with pytest.raises(ValueError):
        emme.Context.find_roots_in_contours_sets(Stub(), [0, 1], [-0.8 + 0.2j], [(0.1, 0.1)])
    with pytest.raises(ValueError):
        emme.Context.find_roots_in_contours_sets(Stub(), [0], [-0.8 + 0.2j], [(0.1, 0.1)], contours=[{}, {}])


def test_round_plan_selftest(tmp_path):
    """Built as `make host-sanitize` builds it: a stand-alone program, nothing loaded into Python under a sanitizer."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    mk = open(os.path.join(SRC, "Makefile")).read()
    assert "host_contour_rounds_selftest" in mk[mk.index("host-sanitize:"):]
    exe = str(tmp_path / "host_contour_rounds_selftest")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(SRC, "host_contour.cpp"),
                    os.path.join(SRC, "host_contour_rounds_selftest.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "contour round-plan self-test ok" in r.stdout
