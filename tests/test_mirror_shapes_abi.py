"""The host side of the mirror shapes switch (emme_ctx_set_mirror_shapes / _get_mirror_shapes),
without a GPU: the header declares the two entry points and the two constants beside an unchanged emme_options_t and
version, the library exports them, a NULL context is rejected before any device is looked for, and the Python names
exist."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMME_EINVAL = -1


def test_header_declares_functions_and_constants():
    text = open(os.path.join(ROOT, "include", "emme_hip.h")).read()
    assert re.search(r"^#define\s+EMME_MIRROR_SHAPES_ES15\s+0\b", text, re.M)
    assert re.search(r"^#define\s+EMME_MIRROR_SHAPES_ALL\s+1\b", text, re.M)
    assert re.search(r"^int\s+emme_ctx_set_mirror_shapes\(emme_ctx_t\*\s*ctx,\s*int\s+shapes\);", text, re.M)
    assert re.search(r"^int\s+emme_ctx_get_mirror_shapes\(const\s+emme_ctx_t\*\s*ctx\);", text, re.M)


def test_mirror_shape_symbols_are_exported(emme):
    lib = emme.load()
    assert hasattr(lib, "emme_ctx_set_mirror_shapes") and hasattr(lib, "emme_ctx_get_mirror_shapes")


def test_null_context_is_rejected_before_any_device(emme):
    lib = emme.load()
    assert lib.emme_ctx_set_mirror_shapes(None, 1) == EMME_EINVAL
    assert lib.emme_ctx_set_mirror_shapes(None, 0) == EMME_EINVAL
    assert lib.emme_ctx_get_mirror_shapes(None) == EMME_EINVAL


def test_python_face_and_frozen_abi(emme):
    assert (emme.MIRROR_SHAPES_ES15, emme.MIRROR_SHAPES_ALL) == (0, 1)
    assert callable(emme.Context.set_mirror_shapes) and callable(emme.Context.mirror_shapes)
    assert "MIRROR_SHAPES_ES15" in emme.__all__ and "MIRROR_SHAPES_ALL" in emme.__all__
    O = emme.Options
    assert ctypes.sizeof(O) == 112
    assert emme.load().emme_version() == 4
