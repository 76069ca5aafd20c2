"""The host side of the cached derivative fill for electromagnetic and GK31 contexts (k_assemble_dense_shape_deriv<PTS, NM>
behind emme_ctx_set_deriv_cache_shapes), without a GPU: the setter and getter are exported and check
their arguments before any device is looked for, the options struct and the version are what they were, the kernel file is
part of the build and of the resource-usage / device-asm lists, and the planner's stand-alone self-tests -- the new one
for these shapes and the electrostatic GK15 one, which must not notice -- pass under ASan + UBSan.  (That an out-of-range
value leaves the earlier one in place needs a context, so a device: tests/test_gpu_dense_shape_deriv.py, routing.)"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "emme_amd", "csrc")
EMME_EINVAL = -1


def _make_list(name):
    """The words of `NAME = ...` in the Makefile, continuation lines included."""
    text = open(os.path.join(SRC, "Makefile")).read().replace("\\\n", " ")
    m = re.search(r"^%s\s*=(.*)$" % name, text, re.M)
    assert m, name
    return m.group(1).split()


def test_symbols_are_exported(emme):
    lib = emme.load()
    assert hasattr(lib, "emme_ctx_set_deriv_cache_shapes") and hasattr(lib, "emme_ctx_get_deriv_cache_shapes")
    assert lib.emme_ctx_set_deriv_cache_shapes.argtypes is not None
    assert lib.emme_ctx_get_deriv_cache_shapes.argtypes is not None
    assert (emme.DERIV_CACHE_SHAPES_ES15, emme.DERIV_CACHE_SHAPES_ALL) == (0, 1)
    assert callable(emme.Context.set_deriv_cache_shapes) and callable(emme.Context.deriv_cache_shapes)
    assert "k_assemble_dense_shape_deriv" in emme.Context.set_deriv_cache_shapes.__doc__


def test_null_context_is_einval(emme):
    """No device is looked for: this runs on a machine without one."""
    lib = emme.load()
    for shapes in (0, 1, 2, -1):
        assert lib.emme_ctx_set_deriv_cache_shapes(None, shapes) == EMME_EINVAL
    assert "NULL context" in emme.last_error()
    assert lib.emme_ctx_get_deriv_cache_shapes(None) == EMME_EINVAL


def test_header_documents_the_switch():
    h = open(os.path.join(ROOT, "include", "emme_hip.h")).read()
    assert re.search(r"#define\s+EMME_DERIV_CACHE_SHAPES_ES15\s+0\b", h)
    assert re.search(r"#define\s+EMME_DERIV_CACHE_SHAPES_ALL\s+1\b", h)
    assert "int emme_ctx_set_deriv_cache_shapes(emme_ctx_t* ctx, int shapes);" in h
    assert "int emme_ctx_get_deriv_cache_shapes(const emme_ctx_t* ctx);" in h


def test_public_surface_is_unchanged(emme):
    O = emme.Options
    assert ctypes.sizeof(O) == 112
    last = max((getattr(O, name).offset, name) for name, _ in O._fields_)
    assert last == (104, "deriv_cached")
    assert emme.load().emme_version() == 4
    assert sorted(emme.Context.FILL_KERNELS) == [0, 1, 2, 3, 4, 5]


def test_makefile_lists_the_kernel_file():
    assert os.path.exists(os.path.join(SRC, "assemble_dense_shape_deriv.hip"))
    assert "assemble_dense_shape_deriv.hip" in _make_list("SRCS")
    assert "assemble_dense_shape_deriv" in _make_list("KERNELS")


def test_library_holds_the_kernels(emme):
    """(the host half of the library names every kernel it registers)"""
    data = open(emme.lib_path(), "rb").read()
    assert b"k_assemble_dense_shape_deriv" in data
    assert b"k_btab_shape_deriv" in data


@pytest.mark.parametrize("name", ["host_plan_dense_shape_deriv_selftest", "host_plan_deriv_selftest"])
def test_planner_selftests_pass_under_sanitizers(tmp_path, name):
    """Built as `make host-sanitize` builds them: stand-alone programs, nothing loaded into Python under a sanitizer.
    The electrostatic GK15 self-test is the unmodified one: a derivative request there keeps its chunks of 8."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    mk = open(os.path.join(SRC, "Makefile")).read()
    assert "../%s\n" % name in mk[mk.index("host-sanitize:"):]
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(SRC, "fill_plan.cpp"),
                    os.path.join(SRC, name + ".cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert name + " ok" in r.stdout
