"""The folded secant eigenpair step and mode parity, host side: the new symbols with their argtypes
and wrappers, the argument errors that are found before any device is looked for, emme_vector_parity (plain host
arithmetic), and the numpy restatement of the folded formulas (eigpair_fold_reference.py) against np.linalg.solve.  No
GPU.

Without a device there is no context, so the calls below pass a context pointer that is never dereferenced: every
pointer and range is checked before the context is read (the pattern of tests/test_eigenpairs_host.py).

Measured (restatement against the direct step, relative error of tau / of u): structured n = 2 .. 34: 3e-16 .. 7e-15;
oracle tokamak N = 24 at omega = -0.8 + 0.25i: 1.6e-13 / 1.7e-14 with the rank-2 terms, 2.5e-2 / 1.8e-2 without them."""
import ctypes as C
import os

import numpy as np
import pytest

from eigpair_fold_reference import direct_step, folded_step, parity
from fold_reference import structured_pair
from oracle.binding import example_tokamak

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMME_EINVAL = -1
W = -0.8 + 0.25j


def test_symbols_argtypes_and_wrappers_exist(emme):
    lib = emme.load()
    assert lib.emme_version() == 4
    want = {"emme_eigenpair_secant_folded_step_batch": 10, "emme_ctx_set_eigpair_fold": 2, "emme_ctx_get_eigpair_fold": 1,
            "emme_ctx_last_folded_eigpair_steps": 1, "emme_vector_parity": 4}
    hdr = open(os.path.join(ROOT, "include", "emme_hip.h")).read()
    for name, nargs in want.items():
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, (name, fn.argtypes)
        assert name in hdr
    assert lib.emme_eigenpair_secant_folded_step_batch.argtypes[1] is C.c_int
    assert lib.emme_eigenpair_secant_folded_step_batch.argtypes[2] is C.c_int
    assert lib.emme_ctx_set_eigpair_fold.argtypes[1] is C.c_int
    for name in ("set_eigpair_fold", "eigpair_fold", "last_folded_eigpair_steps", "eigenpair_secant_folded_step"):
        assert callable(getattr(emme.Context, name)), name
    assert callable(emme.vector_parity)
    assert "EMME_EIGPAIR_FOLD" in hdr
    mk = open(os.path.join(ROOT, "emme_amd", "csrc", "Makefile")).read()
    assert mk.count("eigpair_fold") == 2  # the sources and the kernel files of resource-usage / device-asm


def test_step_argument_errors_come_before_the_device(emme):
    lib = emme.load()
    fake = C.c_void_p(1)  # (never dereferenced: every call below fails on another argument first)
    buf = np.zeros(64)
    inf = np.zeros(2, dtype=np.int32)
    p, pi = buf.ctypes.data, inf.ctypes.data

    def call(ctx=fake, n=2, nbatch=1, M=p, Mo=p, dw=p, v=p, tau=p, resid=p, info=pi):
        return lib.emme_eigenpair_secant_folded_step_batch(ctx, n, nbatch, M, Mo, dw, v, tau, resid, info)

    assert call(ctx=None) == EMME_EINVAL
    for name in ("M", "Mo", "dw", "v", "tau", "resid", "info"):
        assert call(**{name: None}) == EMME_EINVAL, name
    for n in (1, 0, -2, 3, 5, 25):  # below 2, or odd
        assert call(n=n) == EMME_EINVAL, n
    assert "emme_eigenpair_secant_folded_step_batch" in emme.last_error()
    for nb in (0, -1):
        assert call(nbatch=nb) == EMME_EINVAL


def test_setter_and_getters_on_null(emme):
    lib = emme.load()
    assert lib.emme_ctx_set_eigpair_fold(None, 1) == EMME_EINVAL
    assert "emme_ctx_set_eigpair_fold" in emme.last_error()
    assert lib.emme_ctx_get_eigpair_fold(None) == EMME_EINVAL
    assert lib.emme_ctx_last_folded_eigpair_steps(None) == EMME_EINVAL


def test_vector_parity_argument_errors(emme):
    lib = emme.load()
    v, out = np.zeros(8), np.zeros(2)
    assert lib.emme_vector_parity(2, 1, None, out.ctypes.data) == EMME_EINVAL
    assert lib.emme_vector_parity(2, 1, v.ctypes.data, None) == EMME_EINVAL
    assert lib.emme_vector_parity(0, 1, v.ctypes.data, out.ctypes.data) == EMME_EINVAL
    assert lib.emme_vector_parity(2, 0, v.ctypes.data, out.ctypes.data) == EMME_EINVAL
    assert "emme_vector_parity" in emme.last_error()
    with pytest.raises(ValueError):
        emme.vector_parity(np.zeros((2, 2, 2)))


@pytest.mark.parametrize("n", [2, 5, 24])
def test_vector_parity_on_constructed_vectors(emme, n):
    rng = np.random.default_rng(50 + n)
    k = n // 2
    h = rng.standard_normal(k) + 1j * rng.standard_normal(k)
    mid = [0.7 - 0.2j] if n % 2 else []
    even = np.concatenate([h, mid, h[::-1]])
    odd = np.concatenate([h, [0.0] * len(mid), -h[::-1]])
    e0 = np.zeros(n, dtype=complex)
    e0[0] = 1.0
    got = emme.vector_parity(np.array([even, odd, e0]))
    assert got.tolist() == [1.0, 0.0, 0.5], got
    # phase and scale leave it alone, exactly on these and to rounding on a mixed vector
    s = 3.0 * np.exp(0.7j)
    assert emme.vector_parity(s * even) == 1.0 and emme.vector_parity(s * odd) == 0.0
    mixed = even + 0.3 * odd + 0.1 * e0
    p0, p1 = emme.vector_parity(mixed), emme.vector_parity(s * mixed)
    assert 0.0 < p0 < 1.0 and abs(p1 - p0) <= 4e-16, (p0, p1)
    assert abs(p0 - parity(mixed)) <= 4e-16
    # a zero and a non-finite vector have none
    bad = np.zeros((2, n), dtype=complex)
    bad[1, 0] = np.inf
    assert np.isnan(emme.vector_parity(bad)).all()
    assert np.isnan(emme.vector_parity(np.zeros(n)))


def _errors(M, Mo, dw, v, rank2=True):
    vn, tau, res, uh, _ = folded_step(M, Mo, dw, v, rank2=rank2)
    vd, tau_d, res_d, uh_d = direct_step(M, Mo, dw, v)
    return (abs(tau - tau_d) / abs(tau_d), np.linalg.norm(uh - uh_d) / np.linalg.norm(uh_d), abs(res - res_d),
            1.0 - abs(np.vdot(vn, vd)))


@pytest.mark.parametrize("n", [2, 4, 30, 34])
def test_restatement_on_structured_matrices(n):
    rng = np.random.default_rng(7000 * n + 5)
    for _ in range(5):
        M, Mo = structured_pair(rng, n)
        v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        v /= np.linalg.norm(v)
        dw = (0.2 + 0.3 * rng.random()) * np.exp(2j * np.pi * rng.random())
        e_tau, e_u, e_res, e_ov = _errors(M, Mo, dw, v)
        print(f"restatement n={n}: tau {e_tau:.3g}, u {e_u:.3g}, resid {e_res:.3g}, 1 - overlap {e_ov:.3g}")
        assert e_tau <= 1e-12 and e_u <= 1e-12, (n, e_tau, e_u)
        assert e_res <= 1e-13 and e_ov <= 1e-13, (n, e_res, e_ov)


def test_restatement_on_oracle_matrices(oracle):
    """Far from a root the mirror noise of the oracle's separately rounded pairs is not magnified: M and M_old as the
    oracle gives them.  Without u and u' the step must miss, so the first check exercises the rank-2 terms."""
    n = 24
    po = oracle.params(example_tokamak(npoints=n))
    dw = 0.01 * W
    Mo, _ = oracle.assemble(po, W)
    M, _ = oracle.assemble(po, W + dw)
    rng = np.random.default_rng(24)
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    v /= np.linalg.norm(v)
    e_tau, e_u, e_res, _ = _errors(M, Mo, dw, v)
    b_tau, b_u, _, _ = _errors(M, Mo, dw, v, rank2=False)
    print(f"restatement on the oracle N={n}: tau {e_tau:.3g}, u {e_u:.3g}, resid {e_res:.3g}; "
          f"without the rank-2 terms tau {b_tau:.3g}, u {b_u:.3g}")
    assert e_tau <= 1e-12 and e_u <= 1e-12, (e_tau, e_u)
    assert e_res <= 1e-13
    assert b_tau > 1e-6 and b_u > 1e-6, (b_tau, b_u)
