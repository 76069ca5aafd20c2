"""The host side of the tile fill's shape switch (emme_ctx_set_tile_shapes / _get_tile_shapes),
without a GPU: the two entry points exist beside an unchanged emme_options_t and version, reject a NULL context before
any device is looked for, have Python wrappers and constants, and the chunk planner passes its self-test for
electromagnetic contexts (chunks of 5 omegas; emme_amd/csrc/host_plan_tile_shape_selftest.cpp under ASan + UBSan)."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMME_EINVAL = -1


def test_tile_shape_symbols_are_exported(emme):
    lib = emme.load()
    assert hasattr(lib, "emme_ctx_set_tile_shapes") and hasattr(lib, "emme_ctx_get_tile_shapes")


def test_null_context_is_rejected_before_any_device(emme):
    lib = emme.load()
    assert lib.emme_ctx_set_tile_shapes(None, 1) == EMME_EINVAL
    assert lib.emme_ctx_get_tile_shapes(None) < 0


def test_python_face_and_frozen_abi(emme):
    assert (emme.TILE_SHAPES_ES15, emme.TILE_SHAPES_ALL) == (0, 1)
    assert callable(emme.Context.set_tile_shapes) and callable(emme.Context.tile_shapes)
    O = emme.Options
    assert ctypes.sizeof(O) == 112
    last = max((getattr(O, name).offset, name) for name, _ in O._fields_)
    assert last == (104, "deriv_cached")
    assert emme.load().emme_version() == 4
    assert sorted(emme.Context.FILL_KERNELS) == [0, 1, 2, 3, 4, 5]


def test_tile_shape_chunk_planner_selftest(tmp_path):
    """The planner's stand-alone self-test for chunks of 16 / nm omegas, built as `make host-sanitize` builds it."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "emme_amd", "csrc")
    assert "host_plan_tile_shape_selftest" in open(os.path.join(src, "Makefile")).read()
    exe = str(tmp_path / "host_plan_tile_shape_selftest")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(src, "fill_plan.cpp"),
                    os.path.join(src, "host_plan_tile_shape_selftest.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "host_plan_tile_shape_selftest ok" in r.stdout
