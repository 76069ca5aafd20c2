"""The host side of the derivative tile fill for electromagnetic and GK31 contexts (k_assemble_tile_shape_deriv<PTS, NM>,
DESIGN.md §12.4), without a GPU: the kernel file is part of the build and of the resource-usage / device-asm lists, the
built library holds the kernel, the public surface is what it was (no new option, no new version, no new fill kernel
code), and the chunk planner -- unchanged: the derivative fill takes the plain tile-shape fill's chunks of 16 / nm
omegas -- still passes its stand-alone self-test under ASan + UBSan."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "emme_amd", "csrc")


def _make_list(name):
    """The words of `NAME = ...` in the Makefile, continuation lines included."""
    text = open(os.path.join(SRC, "Makefile")).read().replace("\\\n", " ")
    m = re.search(r"^%s\s*=(.*)$" % name, text, re.M)
    assert m, name
    return m.group(1).split()


def test_makefile_lists_the_kernel_file():
    assert os.path.exists(os.path.join(SRC, "assemble_tile_shape_deriv.hip"))
    assert "assemble_tile_shape_deriv.hip" in _make_list("SRCS")
    assert "assemble_tile_shape_deriv" in _make_list("KERNELS")


def test_library_holds_the_kernel(emme):
    """(the host half of the library names every kernel it registers)"""
    data = open(emme.lib_path(), "rb").read()
    assert b"k_assemble_tile_shape_deriv" in data
    assert b"k_assemble_deriv_list_shape" in data


def test_public_surface_is_unchanged(emme):
    O = emme.Options
    assert ctypes.sizeof(O) == 112
    last = max((getattr(O, name).offset, name) for name, _ in O._fields_)
    assert last == (104, "deriv_cached")
    assert emme.load().emme_version() == 4
    assert sorted(emme.Context.FILL_KERNELS) == [0, 1, 2, 3, 4, 5]


def test_tile_shape_chunk_planner_selftest_still_passes(tmp_path):
    """Built as `make host-sanitize` builds it: a stand-alone program, nothing loaded into Python under a sanitizer."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "host_plan_tile_shape_selftest")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(SRC, "fill_plan.cpp"),
                    os.path.join(SRC, "host_plan_tile_shape_selftest.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "host_plan_tile_shape_selftest ok" in r.stdout
