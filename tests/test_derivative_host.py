"""The exact-derivative fill and the true Newton search without a device: the symbols, the Python
wrappers and the argument checks that come before any device work."""
import ctypes as C

import numpy as np

EINVAL = -1


def test_symbols_and_wrappers_exist(emme):
    lib = emme.load()
    for name in ("emme_assemble_derivative_batch", "emme_solve_roots_newton"):
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert callable(getattr(emme.Context, "assemble_derivative", None))
    assert callable(getattr(emme.Context, "solve_roots_newton", None))
    assert lib.emme_version() == 4


def test_bad_arguments_are_rejected_without_a_device(emme):
    lib = emme.load()
    # a stand-in context: every check below fails before the context is looked at
    fake = C.create_string_buffer(64)
    ctx = C.cast(fake, C.c_void_p)
    w = np.array([-0.8, 0.25])
    M = np.zeros(8)
    Mp = np.zeros(8)
    ad = lib.emme_assemble_derivative_batch
    assert ad(None, w.ctypes.data, 1, M.ctypes.data, Mp.ctypes.data, None) == EINVAL
    assert ad(ctx, None, 1, M.ctypes.data, Mp.ctypes.data, None) == EINVAL
    assert ad(ctx, w.ctypes.data, 1, None, Mp.ctypes.data, None) == EINVAL
    assert ad(ctx, w.ctypes.data, 1, M.ctypes.data, None, None) == EINVAL
    assert ad(ctx, w.ctypes.data, 0, M.ctypes.data, Mp.ctypes.data, None) == EINVAL
    assert ad(ctx, w.ctypes.data, -3, M.ctypes.data, Mp.ctypes.data, None) == EINVAL

    roots = np.zeros(2)
    iters = np.zeros(1, dtype=np.int32)
    info = np.zeros(1, dtype=np.int32)
    sr = lib.emme_solve_roots_newton
    args = (w.ctypes.data, 1, 1e-6, 20, roots.ctypes.data, iters.ctypes.data, info.ctypes.data, None)
    assert sr(None, *args) == EINVAL
    assert sr(ctx, None, *args[1:]) == EINVAL
    assert sr(ctx, w.ctypes.data, 0, *args[2:]) == EINVAL
    assert sr(ctx, w.ctypes.data, 1, 1e-6, -1, *args[4:]) == EINVAL
    assert sr(ctx, *args[:4], None, *args[5:]) == EINVAL
    assert sr(ctx, *args[:5], None, *args[6:]) == EINVAL
    assert sr(ctx, *args[:6], None, None) == EINVAL
