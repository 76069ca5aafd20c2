"""Region searches that return eigenpairs and the secant eigenpair step, host side: the new symbols
with their argtypes and wrappers, emme_contour_eigpairs on exact moments of a non-normal linear pencil, the argument
errors of the four search and step entry points (found before any device is looked for), and the stand-alone self-test
of the Beyn step with vectors.  No GPU; the device side is tests/test_gpu_contour_eigenpairs.py.

Without a device there is no context, so the calls below pass a context pointer that is never dereferenced."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "emme_amd", "csrc")
EPS = np.finfo(np.float64).eps
EMME_EINVAL, EMME_ECONFIG = -1, -5


def test_symbols_argtypes_and_wrappers_exist(emme):
    lib = emme.load()
    want = {"emme_eigenpair_secant_step_batch": 11, "emme_solve_eigenpairs_secant": 13, "emme_contour_eigpairs": 10,
            "emme_find_eigenpairs_in_contour": 14, "emme_find_eigenpairs_in_contours_sets": 17}
    hdr = open(os.path.join(ROOT, "include", "emme_hip.h")).read()
    for name, nargs in want.items():
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
        assert name in hdr
    assert lib.emme_version() == 4
    assert lib.emme_solve_eigenpairs_secant.argtypes == lib.emme_solve_eigenpairs.argtypes
    assert lib.emme_eigenpair_secant_step_batch.argtypes[7] is C.c_int
    assert lib.emme_contour_eigpairs.argtypes[4] is C.c_double
    assert lib.emme_find_eigenpairs_in_contour.argtypes[2] is C.c_int and lib.emme_find_eigenpairs_in_contour.argtypes[3] is C.c_double
    for name in ("eigenpair_secant_step", "solve_eigenpairs", "contour_eigpairs", "find_eigenpairs_in_contour",
                 "find_eigenpairs_in_contours_sets"):
        assert callable(getattr(emme.Context, name)), name
    import inspect
    sig = inspect.signature(emme.Context.solve_eigenpairs)
    assert sig.parameters["secant"].default is False  # the existing call keeps its defaults
    mk = open(os.path.join(SRC, "Makefile")).read()
    assert "host_contour_eigpairs_selftest" in mk[mk.index("host-sanitize:"):]


# ---- emme_contour_eigpairs on exact moments of M(omega) = omega I - A, A non-normal ----------------------------------
def _pencil(n, L, inside, seed):
    """A = X diag(lam) X^-1 with X far from unitary; the moments of a contour that holds lam[:inside]:
    A0 = sum_inside x_i y_i^H V, A1 = sum lam_i x_i y_i^H V (y_i^H: rows of X^-1), V the probes."""
    rng = np.random.default_rng(seed)
    cplx = lambda *s: rng.normal(size=s) + 1j * rng.normal(size=s)
    A = cplx(n, n) + np.triu(3.0 * cplx(n, n), 1)  # a heavy strict upper triangle: non-normal
    lam, X = np.linalg.eig(A)
    Y = np.linalg.inv(X)
    V = cplx(n, L)
    P = X[:, :inside] @ Y[:inside, :] @ V
    A0 = P
    A1 = (X[:, :inside] * lam[:inside]) @ Y[:inside, :] @ V
    return np.ascontiguousarray(A0), np.ascontiguousarray(A1), lam[:inside], X[:, :inside], np.linalg.cond(X)


def _eigs(emme, A0, A1, rank_tol, max_eigs=64):
    lib = emme.load()
    n, L = A0.shape
    mu = np.full(max_eigs, 7.0 + 7.0j)
    sig = np.zeros(L)
    k = C.c_int(-1)
    assert lib.emme_contour_eigs(n, L, A0.ctypes.data, A1.ctypes.data, rank_tol, max_eigs, mu.ctypes.data, C.byref(k),
                                 sig.ctypes.data) == 0
    return mu, k.value, sig


def _eigpairs(emme, A0, A1, rank_tol, max_eigs=64, vecs=True):
    lib = emme.load()
    n, L = A0.shape
    mu = np.full(max_eigs, 7.0 + 7.0j)
    v = np.full((max_eigs, n), 7.0 + 7.0j)
    sig = np.zeros(L)
    k = C.c_int(-1)
    assert lib.emme_contour_eigpairs(n, L, A0.ctypes.data, A1.ctypes.data, rank_tol, max_eigs, mu.ctypes.data,
                                     v.ctypes.data if vecs else None, C.byref(k), sig.ctypes.data) == 0
    return mu, v, k.value, sig


# (n, L, eigenvalues inside): 1 and 3 inside at every size, and k = L at (5, 4, 4)
@pytest.mark.parametrize("n,L,inside", [(5, 4, 1), (5, 4, 3), (5, 4, 4), (24, 4, 3), (24, 8, 1), (24, 8, 3), (65, 4, 1),
                                        (65, 8, 3)])
def test_contour_eigpairs_on_a_non_normal_pencil(emme, n, L, inside):
    A0, A1, lam, X, cond = _pencil(n, L, inside, 100 * n + 10 * L + inside)
    mu0, k0, sig0 = _eigs(emme, A0, A1, 1e-8)
    mu, v, k, sig = _eigpairs(emme, A0, A1, 1e-8)
    assert k == k0 == inside
    assert mu.tobytes() == mu0.tobytes() and sig.tobytes() == sig0.tobytes()  # bit for bit, unwritten slots included
    bound = 1e3 * n * EPS * cond
    for c in range(k):
        i = int(np.argmin(np.abs(lam - mu[c])))
        assert abs(mu[c] - lam[i]) <= 1e-9 * max(1.0, np.abs(lam).max()) * cond
        x = X[:, i]
        ov = abs(np.vdot(x, v[c])) / np.linalg.norm(x)
        nrm = np.linalg.norm(v[c])
        print(f"n {n} L {L} inside {inside} c {c}: 1 - overlap {1 - ov / nrm:.2e} (bound {bound:.2e}), |v| - 1 {nrm - 1:.1e}")
        assert abs(nrm - 1.0) <= 1e-13
        assert 1.0 - ov / nrm <= bound, (n, L, inside, c, 1.0 - ov / nrm, bound)
    assert (v[k:] == 7.0 + 7.0j).all()  # rows beyond the rank are not written
    # vecs = NULL is accepted and is the old function
    mu2, _, k2, sig2 = _eigpairs(emme, A0, A1, 1e-8, vecs=False)
    assert k2 == k and mu2.tobytes() == mu0.tobytes() and sig2.tobytes() == sig0.tobytes()
    # the wrapper
    class Stub(emme.Context):
        def __init__(self):  # no device, no handle: the Beyn step is host code
            self.lib = emme.load()

        def __del__(self):
            pass

    wmu, wv, wk, wsig = emme.Context.contour_eigpairs(Stub(), A0, A1, rank_tol=1e-8)
    assert wk == k and wmu.tobytes() == mu[:k].tobytes() and wv.tobytes() == v[:k].tobytes()


def test_contour_eigpairs_bad_arguments(emme):
    lib = emme.load()
    A = np.zeros((4, 3), dtype=np.complex128)
    mu, v, k = np.zeros(64, dtype=np.complex128), np.zeros((64, 4), dtype=np.complex128), C.c_int(0)
    call = lambda n, L, a0, a1, tol, me, m, kk: lib.emme_contour_eigpairs(n, L, a0, a1, tol, me, m, v.ctypes.data, kk, None)
    p = A.ctypes.data
    assert call(0, 3, p, p, 1e-8, 64, mu.ctypes.data, C.byref(k)) == EMME_EINVAL
    assert "emme_contour_eigpairs" in emme.last_error()
    assert call(4, 65, p, p, 1e-8, 64, mu.ctypes.data, C.byref(k)) == EMME_EINVAL
    assert call(4, 3, None, p, 1e-8, 64, mu.ctypes.data, C.byref(k)) == EMME_EINVAL
    assert call(4, 3, p, p, 0.0, 64, mu.ctypes.data, C.byref(k)) == EMME_EINVAL
    assert call(4, 3, p, p, 1e-8, 0, mu.ctypes.data, C.byref(k)) == EMME_EINVAL
    assert call(4, 3, p, p, 1e-8, 64, None, C.byref(k)) == EMME_EINVAL
    assert call(4, 3, p, p, 1e-8, 64, mu.ctypes.data, None) == EMME_EINVAL


# ---- argument errors of the search and step entry points, before the device ----------------------------------------
def test_secant_step_argument_errors_come_before_the_device(emme):
    lib = emme.load()
    fake = C.c_void_p(1)  # (never dereferenced: every call below fails on another argument first)
    buf = np.zeros(64)
    p = buf.ctypes.data

    def call(ctx=fake, n=2, nbatch=1, M=p, Mo=p, dw=p, v=p, tau=p, resid=p, info=p):
        return lib.emme_eigenpair_secant_step_batch(ctx, n, nbatch, M, Mo, dw, v, 1, tau, resid, info)

    for kw in (dict(ctx=None), dict(n=0), dict(nbatch=0), dict(M=None), dict(Mo=None), dict(dw=None), dict(v=None),
               dict(tau=None), dict(resid=None), dict(info=None)):
        assert call(**kw) == EMME_EINVAL, kw
        assert "emme_eigenpair_secant_step_batch" in emme.last_error(), kw
    assert call(n=2049) == EMME_ECONFIG


def test_secant_search_argument_errors_come_before_the_device(emme):
    lib = emme.load()
    fake = C.c_void_p(1)
    buf = np.zeros(64)
    p = buf.ctypes.data

    def call(ctx=fake, g=p, n=1, tol=1e-8, steps=5, roots=p, vecs=p, resid=p, iters=p, info=p):
        return lib.emme_solve_eigenpairs_secant(ctx, None, g, n, None, tol, steps, roots, vecs, resid, iters, info, None)

    for kw in (dict(ctx=None), dict(g=None), dict(n=0), dict(tol=0.0), dict(tol=float("nan")), dict(steps=-1),
               dict(roots=None), dict(vecs=None), dict(resid=None), dict(iters=None), dict(info=None)):
        assert call(**kw) == EMME_EINVAL, kw
        assert "emme_solve_eigenpairs_secant" in emme.last_error(), kw


def _outs(n, max_roots, dim=4):
    roots = np.zeros(2 * n * max_roots)
    vecs = np.zeros(2 * n * max_roots * dim)
    resid = np.zeros(n * max_roots)
    ints = [np.zeros(n * max_roots, dtype=np.int32) for _ in range(2)] + [np.zeros(n, dtype=np.int32) for _ in range(4)]
    return roots, vecs, resid, ints


def test_region_search_argument_errors_come_before_the_device(emme):
    lib = emme.load()
    fake = C.c_void_p(1)
    good = lambda **o: emme.contour_default(**dict(dict(center=-0.8 + 0.2j, semi_axes=(0.1, 0.1)), **o))

    def one(ctx=fake, ct=None, tol=1e-6, steps=20, max_roots=4, drop=None, no_ct=False):
        roots, vecs, resid, ints = _outs(1, max(max_roots, 1))
        ptrs = [roots.ctypes.data, vecs.ctypes.data, resid.ctypes.data] + [a.ctypes.data for a in ints[:5]]
        if drop is not None:
            ptrs[drop] = None
        c = ct if ct is not None else good()
        return lib.emme_find_eigenpairs_in_contour(ctx, None if no_ct else C.byref(c), 0, tol, steps, max_roots, *ptrs)

    assert one(ctx=None) == EMME_EINVAL
    assert one(no_ct=True) == EMME_EINVAL
    assert one(tol=0.0) == EMME_EINVAL and one(steps=-1) == EMME_EINVAL and one(max_roots=0) == EMME_EINVAL
    for drop in range(8):  # roots, vecs, resid, iters, info, n_roots, winding, points_used
        assert one(drop=drop) == EMME_EINVAL, drop
        assert "emme_find_eigenpairs_in_contour" in emme.last_error()
    for over, word in [(dict(semi_axes=(0.0, 0.1)), "semi-axes"), (dict(center=-0.2 + 0.1j, semi_axes=(0.3, 0.1)), "Re omega = 0"),
                       (dict(points=12), "powers of two"), (dict(probes=65), "probes"), (dict(rank_tol=1.0), "rank_tol")]:
        assert one(ct=good(**over)) == EMME_EINVAL, over
        assert "emme_find_eigenpairs_in_contour" in emme.last_error() and word in emme.last_error(), over

    st = np.zeros(3, dtype=np.int32)

    def many(ctx=fake, nitems=3, set_=st, cts=None, tol=1e-6, steps=20, max_roots=4, drop=None):
        roots, vecs, resid, ints = _outs(3, max(max_roots, 1))
        ptrs = [roots.ctypes.data, vecs.ctypes.data, resid.ctypes.data] + [a.ctypes.data for a in ints]
        if drop is not None:
            ptrs[drop] = None
        cts = cts if cts is not None else (emme.Contour * 3)(good(), good(), good())
        return lib.emme_find_eigenpairs_in_contours_sets(ctx, nitems, set_.ctypes.data if set_ is not None else None,
                                                         C.cast(cts, C.c_void_p), 0, tol, steps, max_roots, *ptrs)

    for nitems in (0, -2, 65536):
        assert many(nitems=nitems) == EMME_EINVAL
        assert "nitems" in emme.last_error()
    assert many(ctx=None) == EMME_EINVAL and many(set_=None) == EMME_EINVAL
    assert many(tol=0.0) == EMME_EINVAL and many(steps=-1) == EMME_EINVAL and many(max_roots=0) == EMME_EINVAL
    for drop in range(9):  # ... and status
        assert many(drop=drop) == EMME_EINVAL, drop
    items = (emme.Contour * 3)(good(), good(), good(probes=0))
    assert many(cts=items) == EMME_EINVAL
    msg = emme.last_error()
    assert "emme_find_eigenpairs_in_contours_sets" in msg and "item 2" in msg and "probes" in msg


def test_wrappers_check_their_lists(emme):
    class Stub(emme.Context):
        def __init__(self):  # no device, no handle: the wrappers' own checks come first
            pass

        def __del__(self):
            pass

    with pytest.raises(ValueError):
        emme.Context.find_eigenpairs_in_contours_sets(Stub(), [0, 1], [-0.8 + 0.2j], [(0.1, 0.1)])
    with pytest.raises(ValueError):
        emme.Context.eigenpair_secant_step(Stub(), np.zeros((2, 3, 3)), np.zeros((2, 3, 3)), [1e-3])
    with pytest.raises(ValueError):
        emme.Context.eigenpair_secant_step(Stub(), np.zeros((2, 3, 3)), np.zeros((2, 4, 4)), [1e-3, 1e-3])


def test_beyn_eigenpair_selftest(tmp_path):
    """Built as `make host-sanitize` builds it: a stand-alone program, nothing loaded into Python under a sanitizer."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "host_contour_eigpairs_selftest")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(SRC, "host_contour.cpp"),
                    os.path.join(SRC, "host_contour_eigpairs_selftest.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "contour eigenpair self-test ok" in r.stdout
