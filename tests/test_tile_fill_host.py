"""The host side of the option tile_uncached, without a GPU: the options struct carries the new field
without moving any other, out-of-range values and structs of another size are rejected as for every option (deriv_cached is handled
the same way: the size must match the library's), fill mode 5 has a name, and the tile fill's chunk planner passes its
self-test (emme_amd/csrc/host_plan_tile_selftest.cpp under ASan + UBSan)."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_options_struct_round_trips_tile_uncached(emme):
    o = emme.default_options()
    assert o.tile_uncached == 0
    assert o.size == ctypes.sizeof(emme.Options)
    # the field sits in what was alignment padding in front of dense_cost_ratio: no other field moved (deriv_cached is
    # still the last one, test_deriv_cached_host.py) and the size is what it was
    O = emme.Options
    assert O.tile_uncached.offset == O.dense_min_tasks.offset + 4 == O.dense_cost_ratio.offset - 4
    assert (O.size.offset, O.node_cache_gb.offset, O.dense_cost_ratio.offset, O.deriv_cached.offset) == (0, 8, 72, 104)
    assert ctypes.sizeof(O) == 112
    assert emme.default_options(tile_uncached=1).tile_uncached == 1
    with pytest.raises(TypeError):
        emme.default_options(tile_uncache=1)
    assert emme.load().emme_version() == 4


def test_out_of_range_and_other_sizes_are_rejected(emme):
    from oracle.binding import example_tokamak
    lib = emme.load()
    p = emme.params_from_dict(example_tokamak(npoints=8))
    h = ctypes.c_void_p()
    o = emme.default_options(tile_uncached=2)
    assert lib.emme_ctx_create_ex(ctypes.byref(p), 0, ctypes.byref(o), ctypes.byref(h)) == -1  # EMME_EINVAL
    assert b"range" in lib.emme_last_error() and not h.value
    o = emme.default_options(tile_uncached=-1)
    assert lib.emme_ctx_create_ex(ctypes.byref(p), 0, ctypes.byref(o), ctypes.byref(h)) == -1
    # a struct of another size (the size check is exact, as it is for deriv_cached)
    o = emme.default_options()
    o.size = ctypes.sizeof(emme.Options) - 4
    assert lib.emme_ctx_create_ex(ctypes.byref(p), 0, ctypes.byref(o), ctypes.byref(h)) == -1
    assert b"size" in lib.emme_last_error() and not h.value


def test_fill_mode_five_has_a_name(emme):
    assert emme.Context.FILL_KERNELS[5].startswith("k_assemble_tile")
    assert sorted(emme.Context.FILL_KERNELS) == [0, 1, 2, 3, 4, 5]


def test_tile_chunk_planner_selftest(tmp_path):
    """The planner's stand-alone self-test, built as `make host-sanitize` builds it (that target, which
    test_deriv_cached_host.py runs whole, includes it too)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "emme_amd", "csrc")
    assert "host_plan_tile_selftest" in open(os.path.join(src, "Makefile")).read()
    exe = str(tmp_path / "host_plan_tile_selftest")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(src, "fill_plan.cpp"),
                    os.path.join(src, "host_plan_tile_selftest.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "host_plan_tile_selftest ok" in r.stdout
