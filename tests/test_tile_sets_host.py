"""The host side of the tile fill over parameter sets (k_assemble_tile_sets / k_assemble_tile_sets_deriv and the list
kernels of their hand-over), without a GPU: the kernel files are part of the build and of the
resource-usage / device-asm lists, the built library holds the four kernels, the public surface is what it was (no new
option, no new version; fill mode 7 has a name of its own beside an unchanged FILL_KERNELS), and the chunk planner's
sets form passes its stand-alone self-test under ASan + UBSan."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "emme_amd", "csrc")
UNITS = ["assemble_tile_sets", "assemble_tile_sets_deriv", "assemble_sets_list", "assemble_sets_list_deriv"]


def _make_list(name):
    """The words of `NAME = ...` in the Makefile, continuation lines included."""
    text = open(os.path.join(SRC, "Makefile")).read().replace("\\\n", " ")
    m = re.search(r"^%s\s*=(.*)$" % name, text, re.M)
    assert m, name
    return m.group(1).split()


def test_makefile_lists_the_kernel_files():
    for unit in UNITS:
        assert os.path.exists(os.path.join(SRC, unit + ".hip")), unit
        assert unit + ".hip" in _make_list("SRCS"), unit
        assert unit in _make_list("KERNELS"), unit
    assert "assemble_sets_list_text.hpp" in _make_list("HDRS")


def test_library_holds_the_kernels(emme):
    """(the host half of the library names every kernel it registers)"""
    data = open(emme.lib_path(), "rb").read()
    for name in (b"k_assemble_tile_sets", b"k_assemble_tile_sets_deriv", b"k_assemble_sets_list",
                 b"k_assemble_sets_deriv_list"):
        # (the mangled name: length prefix, so that k_assemble_tile_sets is not found inside k_assemble_tile_sets_deriv)
        assert b"%d%s" % (len(name), name) in data, name


def test_public_surface_is_unchanged(emme):
    O = emme.Options
    assert ctypes.sizeof(O) == 112
    last = max((getattr(O, name).offset, name) for name, _ in O._fields_)
    assert last == (104, "deriv_cached")
    assert emme.load().emme_version() == 4
    assert sorted(emme.Context.FILL_KERNELS) == [0, 1, 2, 3, 4, 5]
    assert emme.Context.TILE_SETS_FILL_KERNEL == "k_assemble_tile_sets (table-free tile fill, a parameter set per chunk)"
    hdr = open(os.path.join(ROOT, "include", "emme_hip.h")).read()
    assert "7 table-free" in hdr and "k_assemble_tile_sets" in hdr


def test_tile_sets_chunk_planner_selftest(tmp_path):
    """Built as `make host-sanitize` builds it: a stand-alone program, nothing loaded into Python under a sanitizer."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    assert "host_plan_tile_sets_selftest" in open(os.path.join(SRC, "Makefile")).read()
    exe = str(tmp_path / "host_plan_tile_sets_selftest")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(SRC, "fill_plan.cpp"),
                    os.path.join(SRC, "host_plan_tile_sets_selftest.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "host_plan_tile_sets_selftest ok" in r.stdout
