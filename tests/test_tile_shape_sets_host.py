"""The host side of the tile fill over parameter sets for electromagnetic and GK31 contexts
(k_assemble_tile_shape_sets<PTS, NM> / k_assemble_tile_shape_sets_deriv<PTS, NM> and the list kernels of their hand-over,
DESIGN.md §13.8), without a GPU: the four new kernel files are part of the build and of the resource-usage / device-asm
lists, all eight tile units and all four list units set exactly their texts' selectors, the built library holds the new
kernels, the public surface is what it was, and the chunk planner's electromagnetic sets form passes its stand-alone
self-test under ASan + UBSan."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "emme_amd", "csrc")
UNITS = ["assemble_tile_shape_sets", "assemble_tile_shape_sets_deriv", "assemble_sets_list_shape",
         "assemble_sets_list_shape_deriv"]
TILE_UNITS = ["assemble_tile", "assemble_tile_deriv", "assemble_tile_sets", "assemble_tile_sets_deriv",
              "assemble_tile_shape", "assemble_tile_shape_deriv", "assemble_tile_shape_sets",
              "assemble_tile_shape_sets_deriv"]
LIST_UNITS = ["assemble_sets_list", "assemble_sets_list_deriv", "assemble_sets_list_shape",
              "assemble_sets_list_shape_deriv"]


def _make_list(name):
    """The words of `NAME = ...` in the Makefile, continuation lines included."""
    text = open(os.path.join(SRC, "Makefile")).read().replace("\\\n", " ")
    m = re.search(r"^%s\s*=(.*)$" % name, text, re.M)
    assert m, name
    return m.group(1).split()


def _selectors(unit, text, prefix):
    """{selector: value} of the `#define NAME 0|1` lines before the unit reads `text`; none of the text's selectors
    (`prefix`) is defined behind it"""
    lines = [line.split("//")[0] for line in open(os.path.join(SRC, unit + ".hip")).read().splitlines()]
    inc = next(k for k, line in enumerate(lines) if re.match(r'\s*#\s*include\s+"%s"' % re.escape(text), line))
    defs = [m.groups() for line in lines[:inc] for m in [re.match(r"\s*#\s*define\s+(\w+)\s+([01])\s*$", line)] if m]
    assert len(defs) == len(dict(defs)), (unit, defs)  # each once
    assert not any(re.match(r"\s*#\s*define\s+" + prefix, line) for line in lines[inc:]), unit
    return {k: int(v) for k, v in defs}


def test_makefile_lists_the_kernel_files():
    for unit in UNITS:
        assert os.path.exists(os.path.join(SRC, unit + ".hip")), unit
        assert unit + ".hip" in _make_list("SRCS"), unit
        assert unit in _make_list("KERNELS"), unit
    assert "host_plan_tile_shape_sets_selftest" in open(os.path.join(SRC, "Makefile")).read()


def test_the_eight_tile_units_are_the_eight_readings():
    seen = set()
    for unit in TILE_UNITS:
        d = _selectors(unit, "assemble_tile_text.hpp", "EMME_TILE_")
        assert sorted(d) == ["EMME_TILE_DERIV", "EMME_TILE_SETS", "EMME_TILE_SHAPE"], (unit, d)
        assert d["EMME_TILE_SHAPE"] == ("shape" in unit) and d["EMME_TILE_SETS"] == ("sets" in unit), (unit, d)
        assert d["EMME_TILE_DERIV"] == unit.endswith("_deriv"), (unit, d)
        seen.add(tuple(sorted(d.items())))
    assert len(seen) == 8
    # the new units are thin: the three defines and the include
    for unit in UNITS[:2]:
        code = [line for line in open(os.path.join(SRC, unit + ".hip")).read().splitlines()
                if line.strip() and not line.lstrip().startswith("//")]
        assert len(code) == 4, (unit, code)
    text = open(os.path.join(SRC, "assemble_tile_text.hpp")).read()
    assert text.count("#error") == 1


def test_the_four_list_units_are_the_four_readings():
    seen = set()
    for unit in LIST_UNITS:
        d = _selectors(unit, "assemble_sets_list_text.hpp", "EMME_SETS_LIST_")
        assert sorted(d) == ["EMME_SETS_LIST_DERIV", "EMME_SETS_LIST_SHAPE"], (unit, d)
        assert d["EMME_SETS_LIST_SHAPE"] == ("shape" in unit) and d["EMME_SETS_LIST_DERIV"] == unit.endswith("_deriv")
        seen.add(tuple(sorted(d.items())))
    assert len(seen) == 4


def test_library_holds_the_kernels(emme):
    """(the host half of the library names every kernel it registers; templates: the mangled name's length prefix and
    the template arguments that follow it)"""
    data = open(emme.lib_path(), "rb").read()
    for name, args in ((b"k_assemble_tile_shape_sets", (b"ILi15ELi3EE", b"ILi31ELi1EE", b"ILi31ELi3EE")),
                       (b"k_assemble_tile_shape_sets_deriv", (b"ILi15ELi3EE", b"ILi31ELi1EE", b"ILi31ELi3EE")),
                       (b"k_assemble_sets_list_shape", (b"ILi15EE", b"ILi31EE")),
                       (b"k_assemble_sets_deriv_list_shape", (b"ILi15EE", b"ILi31EE"))):
        for a in args:
            assert b"%d%s%s" % (len(name), name, a) in data, (name, a)


def test_public_surface_is_unchanged(emme):
    O = emme.Options
    assert ctypes.sizeof(O) == 112
    last = max((getattr(O, name).offset, name) for name, _ in O._fields_)
    assert last == (104, "deriv_cached")
    assert emme.load().emme_version() == 4
    assert sorted(emme.Context.FILL_KERNELS) == [0, 1, 2, 3, 4, 5]
    assert emme.Context.TILE_SETS_FILL_KERNEL == "k_assemble_tile_sets (table-free tile fill, a parameter set per chunk)"
    assert (emme.TILE_SHAPES_ES15, emme.TILE_SHAPES_ALL) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "emme_hip.h")).read()
    assert "7 table-free" in hdr and "k_assemble_tile_sets" in hdr and "k_assemble_tile_shape_sets" in hdr
    assert "k_assemble_tile_shape_sets" in emme.Context.set_tile_shapes.__doc__


def test_tile_shape_sets_chunk_planner_selftest(tmp_path):
    """Built as `make host-sanitize` builds it: a stand-alone program, nothing loaded into Python under a sanitizer."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "host_plan_tile_shape_sets_selftest")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(SRC, "fill_plan.cpp"),
                    os.path.join(SRC, "host_plan_tile_shape_sets_selftest.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "host_plan_tile_shape_sets_selftest ok" in r.stdout
