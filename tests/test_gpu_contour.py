"""Region search on the device: emme_contour_moments_batch against numpy on every factorisation
branch, emme_find_roots_in_contour against the golden lattice search of the headline workload and against a lattice
search of its own at small size, determinism and the rejections."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_CFG3 = os.path.join(ROOT, "tests", "golden", "cfg3_chains.npz")

EINVAL, ECONFIG = -1, -5
SEED = 0x454D4D45
GOLDEN_UNSTABLE = -0.79908943835746860 + 0.26916836098937963j
# a damped mode inside the second test ellipse that no chain of the golden 128-guess lattice reached: Newton converges
# on it from the contour's candidate, sigma_min / sigma_max of M there is 3e-10, and the count W = 3 agrees
MISSED_DAMPED = -0.6497855437578175 - 0.2619896194079743j


def probes(n, L):
    """The internal probes of DESIGN.md §11: splitmix64 of counter 2 (64 i + l) (+1 for Im), seed 0x454D4D45."""
    k = (2 * (64 * np.arange(n, dtype=np.uint64)[:, None] + np.arange(L, dtype=np.uint64)[None, :]))
    out = []
    with np.errstate(over="ignore"):
        for kk in (k, k + np.uint64(1)):
            z = np.uint64(SEED) + (kk + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
            out.append(2.0 * (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 - 1.0)
    return out[0] + 1j * out[1]


def norm_radius(w, c, a, b):
    w = np.asarray(w)
    return np.hypot((w.real - c.real) / a, (w.imag - c.imag) / b)


@pytest.fixture(scope="module")
def ctx256(emme):
    import bench
    ctx = emme.Context(emme.params_from_dict(bench.workload_dict(256)), device=0)
    yield ctx
    ctx.close()


def golden_roots():
    g = np.load(GOLDEN_CFG3)
    r = g["roots"][g["converged"].astype(bool)]
    out = []
    for x in r:
        if all(abs(x - y) > 1e-7 * abs(x) for y in out):
            out.append(x)
    return np.array(out)


class _DeviceCopy:
    """A device copy of a host array through the HIP runtime (hipMalloc / hipMemcpy / hipFree)."""

    def __init__(self, a):
        import ctypes as C
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.ptr = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), a.nbytes) == 0
        assert self.hip.hipMemcpy(self.ptr, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice

    def __enter__(self):
        return self.ptr.value

    def __exit__(self, *exc):
        self.hip.hipFree(self.ptr)


# ---- 1. the building block against numpy ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 64, 256, 600, 1100])
def test_contour_moments_match_numpy(emme, n):
    import bench
    rng = np.random.default_rng(n)
    nq = 16
    M = (rng.standard_normal((nq, n, n)) + 1j * rng.standard_normal((nq, n, n))) / np.sqrt(n)
    M += np.eye(n)[None]
    M[5, :, 0] = 0.0  # exactly singular: factorisation stops at column 1
    z = rng.standard_normal(nq) + 1j * rng.standard_normal(nq)
    w = rng.standard_normal(nq) + 1j * rng.standard_normal(nq)
    with emme.Context(emme.params_from_dict(bench.workload_dict(32)), device=0) as ctx:
        for L in (1, 8, 64):
            for src in ("host", "device", "probes"):
                V = probes(n, L) if src == "probes" else rng.standard_normal((n, L)) + 1j * rng.standard_normal((n, L))
                if src == "device":
                    with _DeviceCopy(M) as dptr, _DeviceCopy(np.ascontiguousarray(V)) as vptr:
                        A0, A1, ld, info = ctx.contour_moments((nq, n), z, w, L, device_ptr=dptr, v_device_ptr=vptr)
                else:
                    A0, A1, ld, info = ctx.contour_moments(M, z, w, L, V=None if src == "probes" else V)
                assert info[5] > 0
                assert np.all(info[np.arange(nq) != 5] == 0)
                ok = np.arange(nq) != 5
                X = np.linalg.solve(M[ok], np.broadcast_to(V, (ok.sum(), n, L)))
                R0 = np.einsum("j,jil->il", w[ok], X)
                R1 = np.einsum("j,jil->il", w[ok] * z[ok], X)
                assert np.linalg.norm(A0 - R0) <= 1e-11 * np.linalg.norm(R0), (L, src)
                assert np.linalg.norm(A1 - R1) <= 1e-11 * np.linalg.norm(R1), (L, src)
                sgn, lab = np.linalg.slogdet(M[ok])
                assert np.all(np.abs(ld[ok].real - lab) <= 1e-10 * np.maximum(1.0, np.abs(lab)))
                dang = np.angle(np.exp(1j * (ld[ok].imag - np.angle(sgn))))
                assert np.all(np.abs(dang) <= 1e-10)
                assert np.isneginf(ld[5].real)


# ---- 2./3. the headline workload against its golden lattice search -------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["unstable", "damped"])
def test_contour_finds_the_golden_roots(emme, ctx256, case):
    c, a, b = {"unstable": (-0.80 + 0.25j, 0.25, 0.20), "damped": (-0.641 - 0.232j, 0.085, 0.05)}[case]
    gold = golden_roots()
    r = norm_radius(gold, c, a, b)
    expect = gold[r < 1.0]
    # the ellipse is well separated from every other golden root
    assert not np.any((r >= 1.0) & (r < 1.3))
    if case == "unstable":
        assert len(expect) == 1 and abs(expect[0] - GOLDEN_UNSTABLE) < 1e-11
    else:
        assert len(expect) == 2
        assert np.allclose(np.sort_complex(expect), np.sort_complex([-0.6061208629 - 0.2144014141j,
                                                                      -0.6758368581 - 0.2495217212j]), atol=1e-9)
        assert norm_radius(MISSED_DAMPED, c, a, b) < 1.0
        assert np.min(np.abs(gold - MISSED_DAMPED)) > 1e-3  # not a golden root
        sv = np.linalg.svd(ctx256.assemble([MISSED_DAMPED])[0], compute_uv=False)
        assert sv[-1] < 1e-8 * sv[0] and sv[-2] > 1e-4 * sv[0]  # a simple root of M, checked here on its own
        expect = np.append(expect, MISSED_DAMPED)
    res = ctx256.find_roots_in_contour(c, (a, b))
    assert res["winding"] == len(expect), res
    assert res["complete"], res
    assert len(res["roots"]) == len(expect)
    for x in expect:
        assert np.min(np.abs(res["roots"] - x)) <= 1e-9 * abs(x), (res["roots"], expect)
    assert np.all(res["info"] == 0)
    assert np.all(np.diff(res["roots"].imag) <= 0)


# ---- 4. self-consistency at small size against a lattice search of its own -----------------------------------------
def _lattice_roots(ctx, re, im):
    """Distinct converged roots of the lattice search that are simple roots: a chain can also stop where the step is
    below tol without M being singular (at npoints 32 several end at sigma_min / sigma_max ~ 1e-2)."""
    g = (re[None, :] + 1j * im[:, None]).reshape(-1)
    roots, iters, info = ctx.solve_roots(g)
    out = []
    for x in roots[info == 0]:
        if np.isfinite(x) and x.real < 0 and all(abs(x - y) > 1e-6 * abs(x) for y in out):
            s = np.linalg.svd(ctx.assemble([x])[0], compute_uv=False)
            # singular, and a simple root: not a point where M collapses to a few huge directions (there every
            # singular value but the largest is ~1e-17 of it: the exponentials run into the safe_exp clamp)
            if s[-1] < 1e-6 * s[0] and s[-2] > 1e-4 * s[0]:
                out.append(x)
    return np.array(out)


def _pair_circle(roots):
    """The smallest circle around the midpoint of two lattice roots that holds both at normalised radius < 0.8, has no
    other lattice root below 1.25 and stays inside Re omega < 0; None if no pair allows one."""
    best = None
    for i in range(len(roots)):
        for j in range(i + 1, len(roots)):
            c = 0.5 * (roots[i] + roots[j])
            others = np.delete(roots, [i, j])
            r_lo = 0.5 * abs(roots[i] - roots[j]) / 0.8
            r_hi = np.min(np.abs(others - c)) / 1.25 if len(others) else np.inf
            r = min(np.sqrt(r_lo * r_hi), 1.5 * r_lo, 0.9 * abs(c.real))
            if r_lo < r <= r_hi and (best is None or r < best[1]):
                best = (c, r)
    return best


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["tokamak_es", "stellarator_em"])
def test_contour_matches_own_lattice_small(emme, model):
    from oracle.binding import example_stellarator, example_tokamak
    if model == "tokamak_es":
        d = example_tokamak(npoints=32)
        re, im = np.linspace(-1.2, -0.4, 8), np.linspace(-0.3, 0.4, 8)
    else:
        d = example_stellarator(npoints=32)
        assert d["beta_e"] > 0
        re, im = np.linspace(-2.2, -1.1, 8), np.linspace(1.9, 3.1, 8)
    with emme.Context(emme.params_from_dict(d), device=0) as ctx:
        if model == "stellarator_em":
            assert ctx.dim == 64
        lat = _lattice_roots(ctx, re, im)
        assert len(lat) >= 1, "the lattice found no root"
        circ = _pair_circle(lat)
        if model == "tokamak_es":
            assert circ is not None, lat  # (this lattice has several close pairs of roots)
        if circ is None:  # one lattice root: a circle of half the distance to its nearest neighbour
            near = [np.sort(np.abs(lat - x))[1] if len(lat) > 1 else np.inf for x in lat]
            k = int(np.argmax(near))
            circ = (lat[k], min(0.5 * near[k], 0.9 * abs(lat[k].real), 0.3))
        c, r = circ
        rad = norm_radius(lat, c, r, r)
        assert not np.any((rad >= 0.8) & (rad < 1.25))
        res = ctx.find_roots_in_contour(c, (r, r))  # the default contour settings
        assert res["winding"] >= 0 and res["n_roots"] == res["winding"] and res["complete"], res
        got = res["roots"]
        assert np.all(res["info"] == 0)
        assert np.all(norm_radius(got, c, r, r) < 1.0)
        for x in got:  # every returned root is a root: M(x) singular
            sv = np.linalg.svd(ctx.assemble([x])[0], compute_uv=False)
            assert sv[-1] < 1e-6 * sv[0], (x, sv[-1] / sv[0])
        tol = ctx.params.iteration_precision
        inside = lat[rad < 0.8]
        if model == "tokamak_es":
            assert len(inside) >= 2
        for x in inside:
            assert np.min(np.abs(got - x)) <= 1e3 * tol * abs(x), (got, x)


# ---- 5. determinism ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_contour_is_deterministic_on_a_settled_context(emme, ctx256):
    c, a, b = -0.80 + 0.25j, 0.25, 0.20
    first = ctx256.find_roots_in_contour(c, (a, b))
    N = first["points_used"]
    t = 2 * np.pi * np.arange(N) / N
    ctx256.cache_settle(c + a * np.cos(t) + 1j * b * np.sin(t))
    ctx256.find_roots_in_contour(c, (a, b))
    r1 = ctx256.find_roots_in_contour(c, (a, b))
    r2 = ctx256.find_roots_in_contour(c, (a, b))
    assert r1["roots"].tobytes() == r2["roots"].tobytes()
    assert r1["winding"] == r2["winding"] and r1["points_used"] == r2["points_used"]


# ---- 6. rejections -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_contour_rejections(emme, ctx256):
    def code(fn):
        with pytest.raises(emme.EmmeError) as e:
            fn()
        return e.value.code, e.value.reason

    k, msg = code(lambda: ctx256.find_roots_in_contour(-0.2 + 0.1j, (0.3, 0.1)))
    assert k == EINVAL and "Re omega = 0" in msg
    k, msg = code(lambda: ctx256.find_roots_in_contour(-0.8 + 0.1j, (0.0, 0.1)))
    assert k == EINVAL and "semi-axes" in msg
    k, msg = code(lambda: ctx256.find_roots_in_contour(-0.8 + 0.1j, (0.1, -0.1)))
    assert k == EINVAL and "semi-axes" in msg
    k, msg = code(lambda: ctx256.find_roots_in_contour(-0.8 + 0.1j, (0.1, 0.1), probes=65))
    assert k == EINVAL and "probes" in msg
    from oracle.binding import example_stellarator
    with emme.Context(emme.params_from_dict(example_stellarator(npoints=1100)), device=0) as big:
        assert big.dim == 2200
        k, msg = code(lambda: big.find_roots_in_contour(-1.6 + 2.5j, (0.1, 0.1)))
        assert k == ECONFIG and "2048" in msg


# ---- 7. a caller stream that does not synchronise with the null stream ----------------------------------------------
@pytest.mark.gpu
def test_contour_on_a_non_blocking_stream(emme, ctx256):
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    st = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(st), 1) == 0  # hipStreamNonBlocking
    try:
        ctx256.set_stream(st.value)
        for case in ("unstable", "damped"):
            c, a, b, expect = {"unstable": (-0.80 + 0.25j, 0.25, 0.20, [GOLDEN_UNSTABLE]),
                               "damped": (-0.641 - 0.232j, 0.085, 0.05,
                                          [-0.6061208629 - 0.2144014141j, -0.6758368581 - 0.2495217212j,
                                           MISSED_DAMPED])}[case]
            res = ctx256.find_roots_in_contour(c, (a, b))
            assert res["complete"] and res["winding"] == len(expect), res
            for x in expect:
                assert np.min(np.abs(res["roots"] - x)) <= 1e-9, (res["roots"], x)
        rng = np.random.default_rng(5)
        n, nq, L = 64, 8, 8
        M = (rng.standard_normal((nq, n, n)) + 1j * rng.standard_normal((nq, n, n))) / np.sqrt(n) + np.eye(n)[None]
        zw = rng.standard_normal(nq) + 1j * rng.standard_normal(nq)
        A0, A1, ld, info = ctx256.contour_moments(M, zw, zw, L)
        sgn, lab = np.linalg.slogdet(M)
        assert np.all(info == 0) and np.allclose(ld.real, lab, rtol=1e-10, atol=1e-10)
    finally:
        ctx256.set_stream(0)
        hip.hipStreamDestroy(st)
