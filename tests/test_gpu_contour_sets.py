"""Region search over parameter sets: emme_contour_moments_groups against numpy and against
emme_contour_moments_batch on each group alone, emme_find_roots_in_contours_sets against emme_find_roots_in_contour on a
context of each item's own set (electrostatic GK15, electromagnetic, GK31), the exact polish, the tile route,
determinism, the errors that need a context, a non-blocking stream.

The `emme` fixture sets cache_min_batch = 1, so the per-set comparison contexts are created with node_cache_gb = 0, as
in tests/test_gpu_param_sets.py: their fills are then the lanes-are-nodes kernel, whose bits k_assemble_sets has.

A failing node fill cannot be provoked through a legal contour: the path that takes an item out of the call in
mid-flight (status EMME_ENUMERIC, winding -1, no roots, the others go on) is covered by the host self-test of the round
plan (emme_amd/csrc/host_contour_rounds_selftest.cpp, tests/test_contour_sets_host.py)."""
import numpy as np
import pytest

from oracle.binding import example_stellarator, example_tokamak

pytestmark = pytest.mark.gpu

EINVAL, ECONFIG = -1, -5
SEED = 0x454D4D45
OUT_KEYS = ("roots", "iters", "info", "n_roots", "winding", "points_used", "status")


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


def _ctx(emme, d, **options):
    return emme.Context(emme.params_from_dict(d), **options)


def _bound(emme, dicts, **options):
    ctx = _ctx(emme, dicts[0], **options)
    ctx.bind_param_sets([emme.params_from_dict(d) for d in dicts])
    return ctx


def _bits(a):
    return np.ascontiguousarray(a).view(np.float64)


# ---- 1. the building block against numpy and against the ungrouped call -------------------------------------------
# sizes 1, 4, 11 and 0, interleaved; matrix 5 (exactly singular) is in the group of 11
GROUP = np.array([2, 1, 2, 2, 1, 2, 0, 2, 2, 1, 2, 2, 2, 1, 2, 2], dtype=np.int32)


@pytest.mark.parametrize("n", [5, 64, 256])
def test_moments_groups_match_numpy_and_the_ungrouped_call(emme, n):
    import bench
    assert [int((GROUP == g).sum()) for g in range(4)] == [1, 4, 11, 0] and GROUP[5] == 2
    rng = np.random.default_rng(n)
    nq = 16
    M = (rng.standard_normal((nq, n, n)) + 1j * rng.standard_normal((nq, n, n))) / np.sqrt(n)
    M += np.eye(n)[None]
    M[5, :, 0] = 0.0  # exactly singular: factorisation stops at column 1
    z = rng.standard_normal(nq) + 1j * rng.standard_normal(nq)
    w = rng.standard_normal(nq) + 1j * rng.standard_normal(nq)
    bit_equal = True
    with emme.Context(emme.params_from_dict(bench.workload_dict(32)), device=0) as ctx:
        for L in (1, 8, 64):
            for src in ("host", "probes"):
                V = probes(n, L) if src == "probes" else rng.standard_normal((n, L)) + 1j * rng.standard_normal((n, L))
                Varg = None if src == "probes" else V
                A0, A1, ld, info = ctx.contour_moments_groups(M, GROUP, 4, z, w, L, V=Varg)
                assert A0.shape == (4, n, L)
                assert info[5] > 0 and np.all(info[np.arange(nq) != 5] == 0)
                ok = np.arange(nq) != 5
                X = np.linalg.solve(M[ok], np.broadcast_to(V, (ok.sum(), n, L)))
                Xall = np.zeros((nq, n, L), complex)
                Xall[ok] = X
                for g in range(3):
                    sel = (GROUP == g) & ok
                    R0 = np.einsum("j,jil->il", w[sel], Xall[sel])
                    R1 = np.einsum("j,jil->il", w[sel] * z[sel], Xall[sel])
                    assert np.linalg.norm(A0[g] - R0) <= 1e-11 * np.linalg.norm(R0), (L, src, g)
                    assert np.linalg.norm(A1[g] - R1) <= 1e-11 * np.linalg.norm(R1), (L, src, g)
                    # the group's matrices alone through emme_contour_moments_batch
                    mem = np.flatnonzero(GROUP == g)
                    B0, B1, bld, binfo = ctx.contour_moments(M[mem], z[mem], w[mem], L, V=Varg)
                    same = np.array_equal(_bits(A0[g]), _bits(B0)) and np.array_equal(_bits(A1[g]), _bits(B1))
                    bit_equal &= same
                    print(f"n {n} L {L} {src} group {g}: bit-equal to the ungrouped call: {same}, "
                          f"|dA0|/|A0| = {np.linalg.norm(A0[g] - B0) / np.linalg.norm(B0):.2e}")
                    assert np.linalg.norm(A0[g] - B0) <= 1e-13 * np.linalg.norm(B0), (L, src, g)
                    assert np.linalg.norm(A1[g] - B1) <= 1e-13 * np.linalg.norm(B1), (L, src, g)
                    assert np.array_equal(binfo, info[mem])
                assert not A0[3].any() and not A1[3].any()  # the empty group: exact zeros
                assert not np.signbit(_bits(A0[3])).any()
                sgn, lab = np.linalg.slogdet(M[ok])
                assert np.all(np.abs(ld[ok].real - lab) <= 1e-10 * np.maximum(1.0, np.abs(lab)))
                dang = np.angle(np.exp(1j * (ld[ok].imag - np.angle(sgn))))
                assert np.all(np.abs(dang) <= 1e-10)
                assert np.isneginf(ld[5].real)
    # the two calls share one kernel (k_contour_moments_groups; the ungrouped call is one group), so this holds by
    # construction; the comparison with the ungrouped kernel that used to be is tests/test_gpu_contour_frozen.py
    assert bit_equal


# ---- 2. the whole search against per-set contexts, electrostatic GK15 ---------------------------------------------
K_RHO, ETA_I = 0.3182, 3.13  # example_tokamak's own values
ES = [example_tokamak(npoints=32), example_tokamak(npoints=32, k_rho=K_RHO * 1.2),
      example_tokamak(npoints=32, eta_i=ETA_I * 0.9)]
LATTICE = (np.linspace(-1.2, -0.4, 8), np.linspace(-0.3, 0.4, 8))  # test_contour_matches_own_lattice_small


def _lattice_roots(ctx, s, re, im):
    """Distinct converged roots of the lattice search on set s that are simple roots (the filter of
    tests/test_gpu_contour.py: a chain can also stop where the step is below tol without M being singular, or where M
    collapses to a few huge directions)."""
    g = (re[None, :] + 1j * im[:, None]).reshape(-1)
    roots, iters, info = ctx.solve_roots_sets([s] * len(g), g)
    out = []
    for x in roots[info == 0]:
        if np.isfinite(x) and x.real < 0 and all(abs(x - y) > 1e-6 * abs(x) for y in out):
            sv = np.linalg.svd(ctx.assemble_sets([s], [x])[0], compute_uv=False)
            if sv[-1] < 1e-6 * sv[0] and sv[-2] > 1e-4 * sv[0]:
                out.append(x)
    return np.array(out)


def _pair_circle(roots):
    """The smallest circle around the midpoint of two lattice roots that holds both at normalised radius < 0.8, has no
    other lattice root below 1.25 and stays inside Re omega < 0; None if no pair allows one (tests/test_gpu_contour.py)."""
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


def _circle(lat):
    """The pair circle, or around the most isolated lattice root a circle of half the distance to its neighbour."""
    circ = _pair_circle(lat)
    if circ is None:
        near = [np.sort(np.abs(lat - x))[1] if len(lat) > 1 else np.inf for x in lat]
        k = int(np.argmax(near))
        circ = (lat[k], min(0.5 * near[k], 0.9 * abs(lat[k].real), 0.3))
    return circ


def _freeze(results):
    for r in results:
        for k in ("roots", "iters", "info"):
            r[k].setflags(write=False)
    return results


def _per_set(emme, dicts, items):
    """find_roots_in_contour for every item on a context of the item's own set, same settings"""
    out = []
    for s, c, r, kw in items:
        with _ctx(emme, dicts[s], node_cache_gb=0) as one:
            out.append(one.find_roots_in_contour(c, (r, r), **kw))
    return _freeze(out)


def _search(ctx, items, **kw):
    return _freeze(ctx.find_roots_in_contours_sets([it[0] for it in items], [it[1] for it in items],
                                                   [(it[2], it[2]) for it in items], contours=[it[3] for it in items], **kw))


@pytest.fixture(scope="module")
def es_case(emme):
    """The five items of the electrostatic case, the batched search (default options) and the per-set searches:
    computed once, shared, never modified"""
    with _bound(emme, ES) as ctx:
        tol = ctx.params.iteration_precision
        lat = [_lattice_roots(ctx, s, *LATTICE) for s in range(3)]
        for s in range(3):
            assert len(lat[s]) >= 1, f"the lattice found no root of set {s}"
        a = _pair_circle(lat[0])
        assert a is not None, lat[0]
        b, c = _circle(lat[1]), _circle(lat[2])
        items = [(0, a[0], a[1], {}), (1, b[0], b[1], dict(points=4)), (2, c[0], c[1], dict(probes=1)),
                 (0, 0.6 + 0.1j, 0.2, {}), (1, b[0], b[1], {})]
        got = _search(ctx, items)
        again = _search(ctx, items)
        mats = {(k, q): ctx.assemble_sets([items[k][0]], [x])[0] for k in range(5) for q, x in enumerate(got[k]["roots"])}
    return dict(items=items, lat=lat, tol=tol, got=got, again=again, mats=mats, ref=_per_set(emme, ES, items))


def _compare(got, ref, tol, what):
    """winding, points_used, n_roots equal; roots paired within the call's own duplicate distance.  Returns whether the
    roots are bit-equal."""
    bits = True
    for k, (g, r) in enumerate(zip(got, ref)):
        same = np.array_equal(_bits(g["roots"]), _bits(r["roots"]))
        bits &= same
        d = max((np.min(np.abs(g["roots"] - x)) / abs(x) for x in r["roots"]), default=0.0) if g["n_roots"] else 0.0
        print(f"{what} item {k}: winding {g['winding']} / {r['winding']}, points {g['points_used']} / {r['points_used']}, "
              f"roots {g['n_roots']} / {r['n_roots']}, bit-equal {same}, max |dw|/|w| = {d:.2e}")
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g["status"] == 0
        assert g["winding"] == r["winding"] and g["points_used"] == r["points_used"] and g["n_roots"] == r["n_roots"], k
        assert g["complete"] == r["complete"]
        assert len(g["roots"]) == len(r["roots"])
        for x in r["roots"]:
            assert np.min(np.abs(g["roots"] - x)) <= 10 * tol * abs(x), (k, g["roots"], r["roots"])
        assert np.all(np.diff(g["roots"].imag) <= 0)
    return bits


def test_search_matches_per_set_contexts_es15(es_case):
    items, got, ref, tol = es_case["items"], es_case["got"], es_case["ref"], es_case["tol"]
    bits = _compare(got, ref, tol, "es15")
    # what keeps the comparison from passing on nothing
    assert got[0]["winding"] >= 2
    # a count >= 1 cannot resolve on 4 nodes with every step <= pi / 2: item b doubles by itself, from 4 nodes, while
    # the other items start at 32
    assert got[1]["points_used"] > 4
    for k in (0, 1, 2, 4):
        assert got[k]["winding"] >= 1, k
        assert np.all(np.abs(got[k]["roots"] - items[k][1]) < items[k][2])
    # the pair circle of set 0 (tests/test_gpu_contour.py asserts the same of the single search): both lattice roots
    rad = np.abs(es_case["lat"][0] - items[0][1]) / items[0][2]
    assert (rad < 0.8).sum() >= 2
    for x in es_case["lat"][0][rad < 0.8]:
        assert np.min(np.abs(got[0]["roots"] - x)) <= 1e3 * tol * abs(x), x
    for (k, q), M in es_case["mats"].items():
        sv = np.linalg.svd(M, compute_uv=False)
        assert sv[-1] < 1e-6 * sv[0], (k, q, sv[-1] / sv[0])
    # Bit equality of the roots was measured and does not hold (items a, b, c, e differ by 3e-17 .. 6e-16 relative, item d
    # has no roots): a one-item call returns the bits of the five-item call, so the company of an item plays no part;
    # the per-set context fills through its own kernel family, the sets call through k_assemble_sets
    print("roots bit-equal to the per-set searches on all items:", bits)


# ---- 3. other shapes ------------------------------------------------------------------------------------------
SHAPES = {"em": ([example_stellarator(npoints=16), example_stellarator(npoints=16, beta_e=0.03, eta_k=0.2)], -1.656 + 2.49j),
          "es31": ([example_tokamak(npoints=16, integration_start_points=31),
                    example_tokamak(npoints=16, integration_start_points=31, k_rho=K_RHO * 1.7)], -0.8 + 0.25j)}


@pytest.mark.parametrize("shape", ["em", "es31"])
def test_search_matches_per_set_contexts_other_shapes(emme, shape):
    dicts, guess = SHAPES[shape]
    with _bound(emme, dicts) as ctx:
        if shape == "em":
            assert ctx.dim == 32
        tol = ctx.params.iteration_precision
        roots, iters, info = ctx.solve_roots_sets([0, 1], [guess, guess])
        assert np.all(info == 0)
        items = [(s, roots[s], 0.3 * abs(roots[s].real), {}) for s in range(2)]
        got = _search(ctx, items)
    ref = _per_set(emme, dicts, items)
    _compare(got, ref, tol, shape)
    # (at npoints 16 the GK31 circles hold a dozen roots and one count stays unresolved at max_points: the comparison
    # above covers that path too; where a search is complete, the root its circle was drawn around is among its roots)
    for k in range(2):
        assert got[k]["n_roots"] >= 1
        if got[k]["complete"]:
            assert np.min(np.abs(got[k]["roots"] - roots[k])) <= 1e3 * tol * abs(roots[k])


# ---- 4. the exact polish ------------------------------------------------------------------------------------------
def test_exact_polish(emme, es_case):
    items, plain, tol = es_case["items"], es_case["got"], es_case["tol"]
    with _bound(emme, ES) as ctx:
        got = _search(ctx, items, exact=True)
    for k, (g, p) in enumerate(zip(got, plain)):
        assert g["status"] == 0 and g["winding"] == p["winding"] and g["n_roots"] == p["n_roots"], k
        assert g["points_used"] == p["points_used"]
        for x in p["roots"]:
            assert np.min(np.abs(g["roots"] - x)) <= 1e3 * tol * abs(x), (k, g["roots"], p["roots"])


# ---- 5. the tile route --------------------------------------------------------------------------------------------
def test_tile_route(emme, es_case):
    items, plain, tol = es_case["items"], es_case["got"], es_case["tol"]
    with _bound(emme, ES, tile_uncached=1) as ctx:
        ctx.profile(True)
        got = _search(ctx, items)
        assert ctx.profile_read(reset=True).tile_tasks > 0  # the nodes went through the tile fill over sets
    for k, (g, p) in enumerate(zip(got, plain)):
        assert g["status"] == 0 and g["winding"] == p["winding"] and g["n_roots"] == p["n_roots"], k
        for x in p["roots"]:
            assert np.min(np.abs(g["roots"] - x)) <= 1e3 * tol * abs(x), (k, g["roots"], p["roots"])


# ---- 6. determinism -----------------------------------------------------------------------------------------------
def test_two_calls_return_the_same_bytes(es_case):
    for k, (a, b) in enumerate(zip(es_case["got"], es_case["again"])):
        for key in OUT_KEYS:
            assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (k, key)


# ---- 7. errors that need a context --------------------------------------------------------------------------------
def test_errors_with_a_device(emme):
    def code(fn):
        with pytest.raises(emme.EmmeError) as e:
            fn()
        return e.value.code, e.value.reason

    with _ctx(emme, ES[0], node_cache_gb=0) as ctx:
        k, msg = code(lambda: ctx.find_roots_in_contours_sets([0], [-0.8 + 0.2j], [(0.1, 0.1)]))
        assert k == EINVAL and "no parameter sets" in msg
        ctx.bind_param_sets([emme.params_from_dict(d) for d in ES[:2]])
        for bad in (2, -1):
            k, msg = code(lambda: ctx.find_roots_in_contours_sets([0, bad], [-0.8 + 0.2j] * 2, [(0.1, 0.1)] * 2))
            assert k == EINVAL and "set[1]" in msg
        k, msg = code(lambda: ctx.find_roots_in_contours_sets([0, 1], [-0.8 + 0.2j, -0.05 + 0.2j], [(0.1, 0.1)] * 2))
        assert k == EINVAL and "item 1" in msg and "Re omega = 0" in msg
        ctx.bind_param_sets([])
        k, msg = code(lambda: ctx.find_roots_in_contours_sets([0], [-0.8 + 0.2j], [(0.1, 0.1)]))
        assert k == EINVAL
    d = example_stellarator(npoints=1100)
    with _bound(emme, [d]) as big:
        assert big.dim == 2200
        k, msg = code(lambda: big.find_roots_in_contours_sets([0], [-1.6 + 2.5j], [(0.1, 0.1)]))
        assert k == ECONFIG and "2048" in msg


# ---- 8. a caller stream that does not synchronise with the null stream ----------------------------------------------
def test_on_a_non_blocking_stream(emme, es_case):
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    st = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(st), 1) == 0  # hipStreamNonBlocking
    item, want = es_case["items"][0], es_case["got"][0]
    with _bound(emme, ES) as ctx:
        try:
            ctx.set_stream(st.value)
            got = _search(ctx, [item])[0]
            rng = np.random.default_rng(5)
            n, nq, L = 64, 8, 8
            M = (rng.standard_normal((nq, n, n)) + 1j * rng.standard_normal((nq, n, n))) / np.sqrt(n) + np.eye(n)[None]
            zw = rng.standard_normal(nq) + 1j * rng.standard_normal(nq)
            A0, A1, ld, info = ctx.contour_moments_groups(M, [0, 1] * 4, 2, zw, zw, L)
            sgn, lab = np.linalg.slogdet(M)
            assert np.all(info == 0) and np.allclose(ld.real, lab, rtol=1e-10, atol=1e-10)
        finally:
            ctx.set_stream(0)
            hip.hipStreamDestroy(st)
    assert got["status"] == 0 and got["complete"] and got["winding"] == want["winding"] >= 2
    assert got["n_roots"] == want["n_roots"]
    for x in want["roots"]:
        assert np.min(np.abs(got["roots"] - x)) <= 10 * es_case["tol"] * abs(x)
