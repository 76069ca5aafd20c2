"""The host side of the option deriv_cached, without a GPU: the options struct carries the new field,
struct sizes that do not match the library are still rejected, and the fill planner gives a derivative request chunks
of at most 8 omegas and never a wide chunk (emme_amd/csrc/host_plan_deriv_selftest.cpp under ASan + UBSan)."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_options_struct_round_trips_deriv_cached(emme):
    o = emme.default_options()
    assert o.deriv_cached == 0
    assert o.size == ctypes.sizeof(emme.Options)
    assert emme.Options._fields_[-1][0] == "deriv_cached"  # grown at its end: every earlier field keeps its offset
    assert emme.default_options(deriv_cached=1).deriv_cached == 1
    with pytest.raises(TypeError):
        emme.default_options(deriv_cache=1)
    assert emme.load().emme_version() == 4


def test_a_struct_of_another_size_is_still_rejected(emme):
    from oracle.binding import example_tokamak
    lib = emme.load()
    p = emme.params_from_dict(example_tokamak(npoints=8))
    for size in (ctypes.sizeof(emme.Options) - 4, ctypes.sizeof(emme.Options) + 8):
        o = emme.default_options()
        o.size = size  # (the struct of a caller built against another header)
        h = ctypes.c_void_p()
        rc = lib.emme_ctx_create_ex(ctypes.byref(p), 0, ctypes.byref(o), ctypes.byref(h))
        assert rc == -1 and not h.value  # EMME_EINVAL, before any device is touched
        assert b"size" in lib.emme_last_error()
    o = emme.default_options(deriv_cached=2)
    h = ctypes.c_void_p()
    assert lib.emme_ctx_create_ex(ctypes.byref(p), 0, ctypes.byref(o), ctypes.byref(h)) == -1
    assert b"range" in lib.emme_last_error()


def test_planner_gives_derivative_requests_chunks_of_eight():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "emme_amd", "csrc"), "host-sanitize"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "host_plan_deriv_selftest ok" in r.stdout
