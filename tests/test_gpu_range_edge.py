"""Every fill route near EMME_MAX_ENTRY = 1e150 and beside a lost matrix (assemble_common.hpp: "the same two numbers in
every kernel, so that the flag does not depend on which kernel served the integral"; a lost matrix costs its own item
only), the searches beside a lost chain, and the linear-algebra kernels on matrices of that size.

The omegas and their premises are tests/range_edge_cases.py, checked from the oracle alone by test_range_edge_host.py.
Every bar is one the project already uses: TOL_M = 1e-10 max|M| or 10 x the oracle's own spread under omega (1 + 1e-13)
(test_damped_omegas_full_size_match_reference_checksums), 1e-13 max|M| for the same omega in another batch
(test_every_fill_kernel_matches_oracle), 1e-9 |root| and +-1 step for a search.  The bar of M' is measured from the
oracle in the test.  Every context is fresh, and every test asserts that the kernel its route names ran.
"""
import functools

import numpy as np
import pytest

import range_edge_cases as rc

pytestmark = pytest.mark.gpu

ENUMERIC = -6
SAME_OMEGA_OTHER_BATCH = 1e-13  # test_every_fill_kernel_matches_oracle
TOL_ROOT = 1e-9
WORST = {}                      # section -> (largest error / bar, where)


def _note(section, ratio, where):
    if ratio > WORST.get(section, (-1.0, None))[0]:
        WORST[section] = (float(ratio), where)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for section in sorted(WORST):
        print(f"\nrange edge, section {section}: worst error / bar = {WORST[section][0]:.3g} at {WORST[section][1]}")


# ---- routes ----------------------------------------------------------------------------------------------------------
ALL = ("es15", "es31", "em15", "em31")
ES, EM, SHAPED = ("es15", "es31"), ("em15", "em31"), ("es31", "em15", "em31")
CACHE = dict(node_cache_gb=8.0, wl_min=1)
# (the 0.002 GB of _modes holds no cache on any grid: such a context falls back to the omega-lane kernel without a word.
# The budgets below are the smallest of 0.003, 0.005, 0.01 and 0.02 GB that hold a cache -- of depth 3 -- for the shape
# on its grid; the ordinary omegas' trees are deeper, so their integrals are handed over)
TINY = dict(wl_min=1, cache_min_depth=1)
TINY_TILED_GB = dict(es15=0.005, es31=0.01, em15=0.003, em31=0.005)
TINY_LANES_GB = dict(es15=0.01, es31=0.02, em15=0.003, em31=0.005)
NO_CACHE = dict(node_cache_gb=0.0, wl_min=1)
TILE = dict(node_cache_gb=0.0, wl_min=1, tile_uncached=1)
# the options under which the tile fill over sets runs (test_gpu_tile_sets.py, test_gpu_device_forms.py)
TILE_SETS = dict(node_cache_gb=0.0, wl_min=1, tile_uncached=1, dense_min_tasks=0, deriv_cached=1)
UNION, LANES = 1, 2  # EMME_FILL_UNION, EMME_FILL_LANES
DENSE, TILE_MODE, SETS_MODE, TILE_SETS_MODE = 4, 5, 6, 7

# name -> opt: context options; shapes; mode: emme_ctx_fill_mode after the fill (a dict: per shape); symbol: prefix of
# fill_kernel_symbol(); deferred: last_deferred() must be > 0 after a fill that holds an ordinary omega; cache_gb:
# node_cache_gb per shape; gemm: omegas sit side by side as columns of one GEMM; sets: two bound parameter sets, the
# ordinary omegas on the second
PLAIN = {
    # the fifteen option sets of _modes (test_gpu_parity.py).  Every shape is tiled under the default fill option, so
    # the dense fill serves all four; fill = UNION walks the union on electrostatic GK15 and takes the independent
    # lanes elsewhere
    "cached": dict(opt=CACHE, shapes=ALL, mode=DENSE, symbol="k_assemble_dense<", gemm=True),
    "cached-dense-all-sparse": dict(opt=dict(CACHE, dense_min_cols=17), shapes=ALL, mode=DENSE, gemm=True,
                                    rounds="sparse"),
    "cached-dense-all-mfma": dict(opt=dict(CACHE, dense_min_cols=1), shapes=ALL, mode=DENSE, gemm=True, rounds="mfma"),
    "cached-dense-narrow": dict(opt=dict(CACHE, dense_min_tasks=100000000), shapes=ALL, mode=DENSE, gemm=True),
    "cached-dense-tiny": dict(opt=TINY, cache_gb=TINY_TILED_GB, shapes=ALL, mode=DENSE, deferred=True, gemm=True),
    "cached-dense-wide": dict(opt=dict(CACHE, dense_wide=1), shapes=ES, mode=DENSE, gemm=True),
    "cached-union": dict(opt=dict(CACHE, fill=UNION), shapes=ALL, mode=dict(es15=3, es31=2, em15=2, em31=2)),
    "cached-union-tiny": dict(opt=dict(TINY, fill=UNION), cache_gb=TINY_LANES_GB, shapes=ALL,
                              mode=dict(es15=3, es31=2, em15=2, em31=2), deferred=True),
    "cached-independent": dict(opt=dict(CACHE, fill=LANES), shapes=ALL, mode=2, symbol="k_assemble_cached"),
    "cached-unfolded": dict(opt=dict(CACHE, phase_table=0), shapes=ALL, mode=2, symbol="k_assemble_cached"),
    # (under the default fill option an electromagnetic context is tiled whatever em_shared says: the dense fill again;
    # the per-moment records are reached with the independent lanes, the row below)
    "cached-em-per-moment": dict(opt=dict(CACHE, em_shared=0), shapes=EM, mode=DENSE, gemm=True),
    "independent-em-per-moment": dict(opt=dict(CACHE, fill=LANES, em_shared=0), shapes=EM, mode=2),
    # (cached-tiny of _modes is the same option set as cached-dense-tiny since every shape is tiled: one row)
    "cached-tiny-independent": dict(opt=dict(TINY, fill=LANES), cache_gb=TINY_LANES_GB, shapes=ALL, mode=2,
                                    deferred=True),
    "omega-lane": dict(opt=NO_CACHE, shapes=ALL, mode=1, symbol="k_assemble_wl<"),
    "nodes": dict(opt=dict(node_cache_gb=0.0, wl_min=100000), shapes=ALL, mode=0, symbol="k_assemble<"),
    "dense-unmirrored": dict(opt=CACHE, shapes=("es15",), mode=DENSE, symbol="k_assemble_dense<", mirror=False,
                             gemm=True),
    "tile": dict(opt=TILE, shapes=("es15",), mode=TILE_MODE, symbol="k_assemble_tile", gemm=True),
    "tile-shape": dict(opt=TILE, shapes=SHAPED, mode=TILE_MODE, symbol="k_assemble_tile_shape<", tile_shapes=1,
                       gemm=True),
    "sets": dict(opt={}, shapes=ALL, mode=SETS_MODE, symbol="k_assemble_sets<", sets=True),
    "tile-sets": dict(opt=TILE_SETS, shapes=("es15",), mode=TILE_SETS_MODE, symbol="k_assemble_tile_sets", sets=True,
                      gemm=True),
    "tile-shape-sets": dict(opt=TILE_SETS, shapes=SHAPED, mode=TILE_SETS_MODE, symbol="k_assemble_tile_shape_sets<",
                            tile_shapes=1, sets=True, gemm=True),
}


# The library names no kernel for a derivative fill (emme_ctx_fill_mode keeps naming the last plain fill): the routes
# tell themselves apart in the profile's counters and the cache state, as test_gpu_derivative_cached.py,
# test_gpu_tile_deriv.py and test_gpu_dense_shape_deriv.py read them.
def _ran_uncached(pr, ctx):
    return pr.tile_tasks == 0 and pr.sparse_rounds == 0 and pr.cache_build_launches == 0 and ctx.cache_state()[2] == 0.0


def _ran_omega_lane(pr, ctx):
    # (the omega-lane kernel counts its own rounds in the first round counter: test_gpu_derivative_cached.py)
    return _ran_uncached(pr, ctx) and pr.dense_rounds > 0


def _ran_nodes(pr, ctx):
    return _ran_uncached(pr, ctx) and pr.dense_rounds == 0


def _ran_dense_deriv(pr, ctx):
    return pr.tile_tasks > 0 and pr.dense_rounds + pr.sparse_rounds > 0 and ctx.cache_state()[2] > 0.0


def _ran_tile_deriv(pr, ctx):
    return pr.tile_tasks > 0 and ctx.cache_state()[2] == 0.0


# plain: the plain route whose M the header promises bit for bit (include/emme_hip.h: the uncached kernels and
# k_assemble_tile_deriv)
DERIV = {
    "deriv-omega-lane": dict(opt=NO_CACHE, shapes=ALL, ran=_ran_omega_lane, plain="omega-lane"),
    "deriv-nodes": dict(opt=dict(node_cache_gb=0.0, wl_min=100000), shapes=ALL, ran=_ran_nodes, plain="nodes"),
    "deriv-dense": dict(opt=dict(CACHE, deriv_cached=1), shapes=("es15",), ran=_ran_dense_deriv, gemm=True),
    "deriv-dense-shape": dict(opt=dict(CACHE, deriv_cached=1), shapes=SHAPED, ran=_ran_dense_deriv, deriv_shapes=1,
                              gemm=True),
    "deriv-tile": dict(opt=dict(TILE, deriv_cached=1), shapes=("es15",), ran=_ran_tile_deriv, plain="tile", gemm=True),
    "deriv-tile-shape": dict(opt=dict(TILE, deriv_cached=1), shapes=SHAPED, ran=_ran_tile_deriv, tile_shapes=1,
                             gemm=True),
    "deriv-sets": dict(opt={}, shapes=ALL, ran=_ran_uncached, sets=True, mode=SETS_MODE),
    "deriv-tile-sets": dict(opt=TILE_SETS, shapes=("es15",), ran=_ran_tile_deriv, sets=True, mode=TILE_SETS_MODE,
                            gemm=True),
    "deriv-tile-shape-sets": dict(opt=TILE_SETS, shapes=SHAPED, ran=_ran_tile_deriv, tile_shapes=1, sets=True,
                                  mode=TILE_SETS_MODE, gemm=True),
}
for _r in DERIV.values():
    _r["deriv"] = True
ROUTES = {**PLAIN, **DERIV}

def _pairs(table):
    return [(name, shape) for name, r in table.items() for shape in r["shapes"]]


def _npoints(route, shape):
    return ROUTES[route].get("npoints", {}).get(shape, rc.grids(shape)[0])


def _ctx(emme, route, shape, **extra):
    r = ROUTES[route]
    n = _npoints(route, shape)
    opt = dict(r["opt"], **extra)
    if "cache_gb" in r:
        opt["node_cache_gb"] = r["cache_gb"][shape]
    ctx = emme.Context(emme.params_from_dict(rc.shape_dict(shape, n)), **opt)
    try:
        if r.get("mirror") is not None:
            ctx.set_mirror_pairs(r["mirror"])
        if r.get("tile_shapes"):
            ctx.set_tile_shapes(r["tile_shapes"])
        if r.get("deriv_shapes"):
            ctx.set_deriv_cache_shapes(r["deriv_shapes"])
        if r.get("sets"):
            ctx.bind_param_sets([emme.params_from_dict(rc.shape_dict(shape, n, second)) for second in (False, True)])
        if r.get("deriv") or r.get("rounds"):
            ctx.profile(True)
    except Exception:
        ctx.close()
        raise
    return ctx


def _second(route, role):
    """Does the item sit on the second bound parameter set?"""
    return bool(ROUTES[route].get("sets")) and role.startswith("ordinary")


def _fill(emme, route, shape, roles, **extra):
    """One raw fill of the shape's omegas of these roles on a fresh context, with the check that the route's kernel
    ran: dict(rc, M, Mp (None on a plain route), iv)."""
    r = ROUTES[route]
    ws = np.array([rc.OMEGAS[shape][role] for role in roles], dtype=np.complex128)
    st = np.array([int(_second(route, role)) for role in roles], dtype=np.int32) if r.get("sets") else None
    with _ctx(emme, route, shape, **extra) as ctx:
        if r.get("deriv"):
            code, M, Mp, iv = ctx.assemble_derivative_raw(ws, set=st)
            pr = ctx.profile_read()
            counters = dict(tile_tasks=pr.tile_tasks, dense=pr.dense_rounds, sparse=pr.sparse_rounds,
                            union=pr.union_rounds, deferred_launches=pr.deferred_launches,
                            cache_builds=pr.cache_build_launches, cache=ctx.cache_state())
            assert pr.matrices == len(ws) and r["ran"](pr, ctx), (route, shape, roles, counters)
        else:
            code, M, iv = ctx.assemble_raw(ws, set=st)
            Mp = None
        if r.get("rounds") and any(role.startswith("ordinary") for role in roles):
            # the dense fill's rounds on the vector path / on the matrix cores (test_gpu_dense_shape_deriv.py); the
            # omega-lane kernel, which takes the minority contour class of the call, counts its own in the first counter
            pr = ctx.profile_read()
            print(f"{route} {shape} {roles}: rounds {pr.dense_rounds} MFMA / {pr.sparse_rounds} vector, tasks {pr.tile_tasks}")
            assert pr.tile_tasks > 0
            assert pr.sparse_rounds > 0 if r["rounds"] == "sparse" else pr.sparse_rounds == 0, (route, shape, roles)
        if "mode" in r:
            mode, want = ctx.lib.emme_ctx_fill_mode(ctx.h), r["mode"]
            want = want[shape] if isinstance(want, dict) else want
            assert mode == want, (route, shape, roles, mode, ctx.fill_kernel_symbol())
        if "symbol" in r:
            assert ctx.fill_kernel_symbol().startswith(r["symbol"]), (route, shape, ctx.fill_kernel_symbol())
        if r.get("deferred") and any(role.startswith("ordinary") for role in roles):
            assert ctx.last_deferred() > 0, (route, shape, roles)  # (a bad item alone may end inside the cache)
        if r.get("mirror") is not None:
            assert ctx.mirror_pairs() == int(r["mirror"])
    return dict(rc=code, M=M, Mp=Mp, iv=iv)


def _against_oracle(section, route, shape, roles, got, only=None):
    """Every item (only: these positions) is finite, symmetric (include/emme_hip.h: every fill kernel writes an entry
    with its mirror), walked the oracle's tree and is within the bar of range_edge_cases.bar."""
    n = _npoints(route, shape)
    for k, role in enumerate(roles):
        if only is not None and k not in only:
            continue
        w = complex(rc.OMEGAS[shape][role])
        Mo, tot = rc.oracle_fill(shape, n, _second(route, role), w)
        M = got["M"][k]
        assert np.isfinite(M.view(np.float64)).all(), (route, shape, role)
        bar = rc.bar(shape, n, _second(route, role), w)
        err = np.abs(M - Mo).max()
        print(f"{section} {route} {shape} {role} {w}: |M - oracle| / bar = {err / bar:.3g} "
              f"(bar {bar / np.abs(Mo).max():.3g} max|M|), intervals {got['iv'][k]} / {tot}")
        assert got["iv"][k] == tot, (route, shape, role, got["iv"][k], tot)
        assert err <= bar, (route, shape, role, err / np.abs(Mo).max(), bar / np.abs(Mo).max())
        assert np.array_equal(M, M.T), (route, shape, role)
        _note(section, err / bar, (route, shape, role))


# ---- A. in range -----------------------------------------------------------------------------------------------------
def _in_range_lists(shape):
    """[ordinary, large, ordinary, edge], with "large" the sharp and the deep point in turn (GK31 has no edge: its two
    large points share a list); the majority contour class of every list is that of its large and edge items, so that
    they go through the route's own kernel (the minority class of a cached call takes the omega-lane kernel)."""
    o = rc.OMEGAS[shape]
    if "sharp_edge" not in o:
        return [["ordinary_a", "sharp_large", "ordinary_b", "deep_large"]]
    return [["ordinary_a", "sharp_large", "ordinary_b", "sharp_edge"],
            [role for role in ("ordinary_a", "deep_large", "ordinary_b", "deep_edge") if role in o]]


def _in_range_cases():
    return [pytest.param(route, shape, k, id=f"{route}-{shape}-{'sharp' if k == 0 else 'deep'}")
            for route, shape in _pairs(PLAIN) for k in range(len(_in_range_lists(shape)))]


@pytest.mark.parametrize("route,shape,which", _in_range_cases())
def test_in_range_fill_matches_oracle(emme, route, shape, which):
    """rc = 0, finite entries, the oracle's interval totals and |M - M_oracle|.max() <= max(1e-10, 10 x spread) max|M|
    for [ordinary, large, ordinary, edge] in one call.  On the sharp points the bar is about 1.5e-9; on the deep ones
    (spread 1e-8 .. 2e-3 in the oracle itself) it only guards finiteness and gross error, while the interval totals
    stay exact.  The edge omegas of the GK15 shapes, 0.5 - 5i and -0.1 - 4i, are where the accept / split rule used to
    square an interval's Kronrod sum into infinity (gk_modulus, assemble_common.hpp): every route
    answered them with EMME_ENUMERIC."""
    roles = _in_range_lists(shape)[which]
    got = _fill(emme, route, shape, roles)
    assert got["rc"] == 0, (route, shape, roles, got["rc"], emme.last_error())
    _against_oracle("A", route, shape, roles, got)


# ---- B. derivative in range ------------------------------------------------------------------------------------------
DERIV_ROLES = ["ordinary_a", "sharp_large", "ordinary_b"]


@pytest.mark.parametrize("route,shape", _pairs(DERIV))
def test_in_range_derivative_matches_richardson(emme, route, shape):
    """M and M' at the sharp large omega between the two ordinary ones (M' is about 300 M: at the edge omega it would
    legitimately leave the range).  M is held to A's bar and, where the header promises it, to the bits of the plain
    fill of the same route.  M' is held to the Richardson-extrapolated central difference of the oracle's M,
    (4 D(h/2) - D(h)) / 3 with h = 1e-5 |omega|; the bar is 10 x the disagreement of that extrapolation along Re omega
    and along Im omega, measured here from the oracle alone: 1.8e-11 .. 6.5e-11 of max|M'| when this was written, so the
    bar lands near 1e-9 -- three decades under the 1e-6 of test_mp_is_the_complex_derivative."""
    n = _npoints(route, shape)
    got = _fill(emme, route, shape, DERIV_ROLES)
    assert got["rc"] == 0, (route, shape, got["rc"], emme.last_error())
    _against_oracle("B (M)", route, shape, DERIV_ROLES, got)
    Mp_ref, disagreement, same_tree = rc.oracle_derivative(shape, n)
    assert same_tree
    scale = np.abs(Mp_ref).max()
    bar = 10.0 * disagreement
    err = np.abs(got["Mp"][1] - Mp_ref).max() / scale
    print(f"B {route} {shape}: Richardson disagreement {disagreement:.3g} -> bar {bar:.3g}; |M' - reference| = {err:.3g} "
          f"max|M'|, max|M'| = {scale:.3g}")
    assert np.isfinite(got["Mp"].view(np.float64)).all()
    assert err <= bar, (route, shape, err, bar)
    assert np.array_equal(got["Mp"][1], got["Mp"][1].T)
    _note("B (M')", err / bar, (route, shape))
    plain = ROUTES[route].get("plain")
    if plain is not None:
        same = _fill(emme, plain, shape, DERIV_ROLES)
        assert same["rc"] == 0 and np.array_equal(same["iv"], got["iv"])
        assert same["M"].tobytes() == got["M"].tobytes(), (route, shape, np.abs(same["M"] - got["M"]).max())


# ---- C. beside a lost matrix -----------------------------------------------------------------------------------------
def _healthy_roles(route, shape):
    """ordinary a, the edge omega (the sharp large one where the shape has no edge, and on a derivative route, where M'
    of the edge omega leaves the range), ordinary b"""
    edge = "sharp_edge" if "sharp_edge" in rc.OMEGAS[shape] and not ROUTES[route].get("deriv") else "sharp_large"
    return ["ordinary_a", edge, "ordinary_b"]


def _beside(emme, route, shape, **extra):
    healthy = _healthy_roles(route, shape)
    without = _fill(emme, route, shape, healthy, **extra)
    assert without["rc"] == 0, (route, shape, without["rc"], emme.last_error())
    _against_oracle("C", route, shape, healthy, without)
    positions = [1] + ([0, 3] if ROUTES[route].get("gemm") else [])  # column position matters on the GEMM routes only
    for bad in rc.BAD:
        alone = _fill(emme, route, shape, [bad], **extra)
        assert alone["rc"] == ENUMERIC, (route, shape, bad, alone["rc"])
        for pos in positions:
            roles = healthy[:pos] + [bad] + healthy[pos:]
            keep = [k for k in range(4) if k != pos]
            got = _fill(emme, route, shape, roles, **extra)
            assert got["rc"] == ENUMERIC, (route, shape, bad, pos, got["rc"])
            assert np.array_equal(got["iv"][keep], without["iv"]), (route, shape, bad, pos, got["iv"], without["iv"])
            for name in ("M", "Mp"):
                if got[name] is None:
                    continue
                for k, k0 in zip(keep, range(3)):
                    diff = np.abs(got[name][k] - without[name][k0]).max() / np.abs(without[name][k0]).max()
                    print(f"C {route} {shape} {bad} at {pos}: {name} of {roles[k]} beside it vs without it {diff:.3g}")
                    assert diff <= SAME_OMEGA_OTHER_BATCH, (route, shape, bad, pos, name, roles[k], diff)
                    _note("C (beside / without)", diff / SAME_OMEGA_OTHER_BATCH, (route, shape, bad, pos, roles[k]))
            _against_oracle("C", route, shape, roles, got, only=keep)
    return without


@pytest.mark.parametrize("route,shape", _pairs(ROUTES))
def test_healthy_items_beside_a_lost_one(emme, route, shape):
    """[ordinary a, bad, edge, ordinary b] for the omega beyond the range and the one that is lost at once: the call
    and the bad item alone return EMME_ENUMERIC, the call without it 0; the three healthy matrices have the interval
    totals of the call without the bad item, agree with it to 1e-13 max|M| and with the oracle at A's bar.  On the GEMM
    routes (dense, tile, tile over sets) the bad item also goes first and last: its column position differs.  Nothing
    is asserted about the bad item's own entries."""
    _beside(emme, route, shape)


# ---- D. searches beside a lost chain ---------------------------------------------------------------------------------
SEARCH_ROUTES = {
    "cached": CACHE,
    "omega-lane": NO_CACHE,
    "tile": dict(TILE, deriv_cached=1),
}
SEARCH_SYMBOL = {"cached": "k_assemble_dense<", "omega-lane": "k_assemble_wl<", "tile": "k_assemble_tile"}
SETS_SEARCH_ROUTES = {"nodes": {}, "tile": TILE_SETS}
RESID = 1e-12


def _search_dict(**over):
    return rc.shape_dict(rc.SEARCH_SHAPE, rc.SEARCH_NPOINTS) | over


@functools.lru_cache(maxsize=None)
def _guesses():
    """The converged simple roots of a preliminary Newton search x (1 + 1e-3), as test_gpu_eigenpairs.py takes them."""
    import emme_amd
    import test_gpu_eigenpairs as ep
    with emme_amd.Context(emme_amd.params_from_dict(_search_dict())) as ctx:
        roots = ep._simple_roots(ctx, ep.LAT_ES)
    assert len(roots) >= 2
    g = roots * (1 + 1e-3)
    g.setflags(write=False)
    return g


SEARCHES = {
    "secant-trace": lambda ctx, g: ctx.solve_roots(g, tol=1e-10, step_limit=20),
    "secant-qr": lambda ctx, g: ctx.solve_roots(g, tol=1e-10, step_limit=20),
    "newton": lambda ctx, g: ctx.solve_roots_newton(g, tol=1e-10, step_limit=20),
    "eigenpairs": lambda ctx, g: ctx.solve_eigenpairs(g, tol=1e-10, step_limit=20),
    "eigenpairs-secant": lambda ctx, g: ctx.solve_eigenpairs(g, tol=1e-10, step_limit=20, secant=True),
}


def _compare_search(label, out, ref, lost, pair, lost_code=ENUMERIC):
    """out: the search with the lost guess at position `lost`; ref: without it.  (roots, iters, info), or with pair
    (roots, vecs, resid, iters, info)."""
    roots, iters, info = (out[0], out[3], out[4]) if pair else out
    roots0, iters0, info0 = (ref[0], ref[3], ref[4]) if pair else ref
    print(f"D {label}: the lost chain ends with info {info[lost]}")
    assert info[lost] == lost_code if lost_code is not None else info[lost] != 0, (label, info)
    keep = np.arange(len(roots)) != lost
    assert np.array_equal(info[keep], info0), (label, info, info0)
    assert (info0 == 0).any(), (label, info0)  # (a search that converged nowhere shows nothing)
    done = info0 == 0
    rel = np.abs(roots[keep][done] - roots0[done]) / np.abs(roots0[done])
    print(f"D {label}: |d root| / |root| <= {rel.max():.3g}, steps {iters[keep].tolist()} / {iters0.tolist()}")
    assert (rel <= TOL_ROOT).all(), (label, rel)
    assert (np.abs(iters[keep] - iters0) <= 1).all(), (label, iters[keep], iters0)
    _note("D (root)", rel.max() / TOL_ROOT, label)
    if pair:
        resid = out[2][keep][done]
        assert (resid <= RESID).all() and (ref[2][done] <= RESID).all(), (label, resid, ref[2])


@pytest.mark.parametrize("skip_lost", [1, 0], ids=["skip-lost", "no-skip-lost"])
@pytest.mark.parametrize("route", sorted(SEARCH_ROUTES))
@pytest.mark.parametrize("search", sorted(SEARCHES))
def test_searches_beside_a_lost_chain(emme, search, route, skip_lost):
    """One guess whose first fill is lost (0.5 - 9.2i) among the healthy ones: its chain ends with EMME_ENUMERIC, every
    other chain with the info, the root (1e-9 |root|) and the step count (+-1, as test_search_matches_the_restatement
    allows) of the search without it; the eigenpair searches keep residuals <= 1e-12 on the healthy chains.  skip_lost
    acts in the searches alone (a plain fill call never sets it): with it off the lost matrix is filled to the end, and
    its chain may end with the Newton step's own code instead (test_lost_matrix_is_left_alone_and_its_chain_retires) --
    not with 0; the healthy chains are held to the same bars."""
    g0 = _guesses()
    lost = 1
    g = np.insert(g0, lost, rc.SEARCH_LOST_GUESS)
    d = _search_dict(iteration_method="QRSecant") if search == "secant-qr" else _search_dict()
    plain_fills = search in ("secant-trace", "secant-qr", "eigenpairs-secant")  # (the others fill M and M' together)
    runs = []
    for guesses in (g, g0):
        with emme.Context(emme.params_from_dict(d), skip_lost=skip_lost, **SEARCH_ROUTES[route]) as ctx:
            ctx.profile(True)
            runs.append(SEARCHES[search](ctx, guesses))
            pr = ctx.profile_read()
            counters = dict(tile_tasks=pr.tile_tasks, dense=pr.dense_rounds, sparse=pr.sparse_rounds)
            if plain_fills:
                assert ctx.fill_kernel_symbol().startswith(SEARCH_SYMBOL[route]), (search, route, ctx.fill_kernel_symbol())
            # (a derivative fill names no kernel: tile tasks without a cache are the tile fill's, test_gpu_tile_deriv.py;
            # without deriv_cached a derivative search keeps the uncached kernels on a context that has a cache too)
            if route == "omega-lane" or (route == "cached" and not plain_fills):
                assert pr.tile_tasks == 0 and pr.sparse_rounds == 0, (search, route, counters)
            else:
                assert pr.tile_tasks > 0, (search, route, counters)
    _compare_search(f"{search} {route} skip_lost={skip_lost}", runs[0], runs[1], lost,
                    pair=search.startswith("eigenpairs"), lost_code=ENUMERIC if skip_lost else None)


@pytest.mark.parametrize("route", sorted(SETS_SEARCH_ROUTES))
@pytest.mark.parametrize("exact", [0, 1])
def test_sets_searches_beside_a_lost_chain(emme, exact, route):
    """solve_roots_sets over two bound sets (the same physics twice, so that the healthy guesses serve both), the lost
    guess on the first."""
    g0 = _guesses()
    g0 = np.concatenate([g0, g0])
    st0 = np.repeat([0, 1], len(g0) // 2).astype(np.int32)
    lost = 1
    g, st = np.insert(g0, lost, rc.SEARCH_LOST_GUESS), np.insert(st0, lost, 0)
    p = emme.params_from_dict(_search_dict())
    runs = []
    for guesses, sets in ((g, st), (g0, st0)):
        with emme.Context(p, **SETS_SEARCH_ROUTES[route]) as ctx:
            ctx.bind_param_sets([p, p])
            runs.append(ctx.solve_roots_sets(sets, guesses, exact=exact, tol=1e-10, step_limit=20))
            assert ctx.lib.emme_ctx_fill_mode(ctx.h) == (TILE_SETS_MODE if route == "tile" else SETS_MODE)
    _compare_search(f"sets exact={exact} {route}", runs[0], runs[1], lost, pair=False)


# ---- E. linear algebra at the same range -----------------------------------------------------------------------------
SCALE_EXP = 490  # an even power of two: exact, and it commutes with every +, *, / and sqrt that neither overflows nor
SCALE = 2.0 ** SCALE_EXP  # underflows; entries become about 3e147


@pytest.fixture(scope="module")
def small_ctx(emme):
    ctx = emme.Context(emme.params_from_dict(rc.shape_dict("es15", 16)))
    yield ctx
    ctx.close()


def _same_bits(label, scaled, plain):
    """Output by output the same bits; a NaN (the exactly singular item of a batch) is a NaN, whatever its payload."""
    for k, (a, b) in enumerate(zip(scaled, plain)):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (label, k)
        if a.dtype.kind in "fc":
            same = np.array_equal(a.view(np.float64), b.view(np.float64), equal_nan=True)
            assert same, (label, k, np.nanmax(np.abs(a - b)))
        else:
            assert np.array_equal(a, b), (label, k, a, b)


@pytest.mark.parametrize("n", [17, 64, 300])
def test_linear_algebra_on_matrices_scaled_to_the_edge(small_ctx, n):
    """trace_solve, qr_secant, null_vectors, eigenpair_step, eigenpair_secant_step and sym_forms on the constructed
    matrices of their own tests, as they are and with every input matrix multiplied by 2^490: tr, q, the vectors, tau and
    the residuals are unchanged, the forms scale by 2^490 and the squared norms by 2^980.  After unscaling: the same info
    and the same bits -- no kernel squares an entry without scaling it first, and none compares against an absolute
    threshold."""
    import test_gpu_device_forms as df
    import test_gpu_sensitivities as sens
    ctx = small_ctx
    A, B = df._symmetric_batch(n)
    M, Mp, v = df._constructed_batch(n)
    dw = np.array([0.01 - 0.002j, -0.003 + 0.004j, 0.002 + 0.001j])
    assert np.isfinite((A * SCALE).view(np.float64)).all() and np.abs(A * SCALE).max() > 1e147
    _same_bits(("trace_solve", n), ctx.trace_solve(A * SCALE, B * SCALE), ctx.trace_solve(A, B))
    _same_bits(("qr_secant", n), ctx.qr_secant(A * SCALE, B * SCALE), ctx.qr_secant(A, B))
    _same_bits(("null_vectors", n), ctx.null_vectors(A * SCALE), ctx.null_vectors(A))
    for have_v in (v, None):
        _same_bits(("eigenpair_step", n, have_v is not None), ctx.eigenpair_step(M * SCALE, Mp * SCALE, have_v),
                   ctx.eigenpair_step(M, Mp, have_v))
        _same_bits(("eigenpair_secant_step", n, have_v is not None),
                   ctx.eigenpair_secant_step(M * SCALE, Mp * SCALE, dw, have_v), ctx.eigenpair_secant_step(M, Mp, dw, have_v))
    d = sens._forms_data(n)
    items = sens.ITEMS
    f, s = ctx.sym_forms(d["A"], d["B"], d["v"], items[:, 0], items[:, 1], items[:, 2], items[:, 3])
    fs, ss = ctx.sym_forms(d["A"] * SCALE, d["B"] * SCALE, d["v"], items[:, 0], items[:, 1], items[:, 2], items[:, 3])
    assert np.isfinite(fs.view(np.float64)).all() and np.isfinite(ss).all()
    _same_bits(("sym_forms", n), (fs / SCALE, ss / SCALE / SCALE), (f, s))
