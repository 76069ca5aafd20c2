"""M and the exact dM/domega from the tiled node cache for electromagnetic and GK31 contexts
(k_assemble_dense_shape_deriv<PTS, NM>): the option deriv_cached beside
set_deriv_cache_shapes(DERIV_CACHE_SHAPES_ALL).  The kernel is k_assemble_dense<1, PTS, NM>'s walk with K' of every column
as its twin column (8 electrostatic omegas, or 2 omegas x 3 moments per chunk); integrals that leave the cache are finished
by k_assemble_deriv_list_shape<PTS>.

Bars: the project's own, as tests/test_gpu_tile_shape_deriv.py states them.
  * Interval counts equal the CPU oracle's, omega by omega.
  * M is within 1e-10 max|M| of the plain cached fill and of the oracle.
  * M' is within 1e-10 max|M'| of the partner: the uncached derivative fill on the same context after
    set_deriv_cache_shapes(DERIV_CACHE_SHAPES_ES15).  At strongly damped omegas the bar is the larger of that and 10 x the
    PARTNER's own change under omega (1 + 1e-13) -- never computed from the code under test.
Every test asserts tile_tasks > 0 after the derivative fill: without the kernel a derivative fill of these shapes on a
context with a cache runs no tile task.
"""
import os

import numpy as np
import pytest

from oracle.binding import example_stellarator, example_tokamak

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-10
OPTS = dict(node_cache_gb=8.0, deriv_cached=1)
W_DAMPED = -0.142 - 1.469j
W_DAMPED_POS = 0.153 - 0.316j
# the ten omegas of test_dense_fill_every_shape_matches_oracle: both contour classes, a damped one
WS10 = np.array([-0.8 + 0.25j, -0.6 - 0.21j, 0.5 + 0.1j, -1.656 + 2.49j, W_DAMPED_POS, -0.7 + 0.3j, -0.9 + 0.1j, -0.5 + 0.2j,
                 -0.65 + 0.27j, -1.0 + 0.05j])
# ... and its shapes
SHAPES = {
    "em31": lambda **kw: example_stellarator(**dict(dict(npoints=14), **kw)),
    "em15": lambda **kw: example_stellarator(**dict(dict(npoints=14, integration_start_points=15), **kw)),
    "es31": lambda **kw: example_tokamak(**dict(dict(npoints=28, integration_start_points=31), **kw)),
}
CAPACITY = {"em31": 2, "em15": 2, "es31": 8}  # omegas of a chunk: 8 K columns beside their 8 twins


def _ctx(emme, d, shapes=None, **options):
    ctx = emme.Context(emme.params_from_dict(d), **options)
    ctx.set_deriv_cache_shapes(emme.DERIV_CACHE_SHAPES_ALL if shapes is None else shapes)
    return ctx


def _bits(a):
    return np.ascontiguousarray(a).view(np.float64)


def _ntiles(n):
    return (n * (n - 1) // 2 + 15) // 16


def _cached_deriv(ctx, ws):
    """One derivative fill with the profile's counters: ((M, Mp, iv), profile)."""
    ctx.profile(True)
    ctx.profile_read(reset=True)
    out = ctx.assemble_derivative(ws, want_intervals=True)
    pr = ctx.profile_read(reset=True)
    assert pr.tile_tasks > 0, "the derivative fill did not go through k_assemble_dense_shape_deriv"
    return out, pr


def _partner(emme, ctx, ws, spread=True):
    """The uncached derivative fill of the same omegas on the same context (switch off), and of omega (1 + 1e-13)."""
    ctx.set_deriv_cache_shapes(emme.DERIV_CACHE_SHAPES_ES15)
    try:
        ctx.profile(True)
        ctx.profile_read(reset=True)
        u = ctx.assemble_derivative(ws, want_intervals=True)
        assert ctx.profile_read(reset=True).tile_tasks == 0
        u2 = ctx.assemble_derivative(np.asarray(ws) * (1 + 1e-13)) if spread else None
    finally:
        ctx.set_deriv_cache_shapes(emme.DERIV_CACHE_SHAPES_ALL)
    return u, u2


def _check_structure(d, Mp):
    """M' has the block structure of M (include/solver.h:461-511) and no diagonal: the diagonals are constant in omega"""
    N = d["npoints"]
    for Pk in Mp:
        if d["beta_e"] == 0.0:
            assert np.array_equal(Pk, Pk.T) and np.abs(np.diag(Pk)).max() == 0.0
            continue
        A, B, C, D = Pk[:N, :N], Pk[:N, N:], Pk[N:, :N], Pk[N:, N:]
        assert np.array_equal(A, A.T) and np.array_equal(D, D.T)
        assert np.array_equal(B, -B.T) and np.array_equal(C, -B)
        for blk in (A, B, C, D):
            assert np.abs(np.diag(blk)).max() == 0.0


def _check_against_partner(d, ws, got, u, u2, damped=()):
    M, Mp, iv = got
    assert np.array_equal(iv, u[2]), (iv, u[2])
    for b, w in enumerate(ws):
        sm, sp = np.abs(u[0][b]).max(), np.abs(u[1][b]).max()
        bar_m, bar_p, which = TOL * sm, TOL * sp, "1e-10"
        if complex(w) in damped:  # 10 x the partner's own spread, same floor
            bar_m = max(bar_m, 10.0 * np.abs(u[0][b] - u2[0][b]).max())
            bar_p = max(bar_p, 10.0 * np.abs(u[1][b] - u2[1][b]).max())
            which = "spread"
        em, ep = np.abs(M[b] - u[0][b]).max(), np.abs(Mp[b] - u[1][b]).max()
        print(f"omega {complex(w)}: M {em / sm:.3e} of max|M| (bar {bar_m / sm:.3e}), "
              f"M' {ep / sp:.3e} of max|M'| (bar {bar_p / sp:.3e}, {which})")
        assert em <= bar_m, (w, em, bar_m)
        assert ep <= bar_p, (w, ep, bar_p)
    _check_structure(d, Mp)


_ORACLE = {}


def _oracle_fill(oracle, shape, d, w):
    """(M, interval total) of the CPU oracle, computed once per (parameters, omega) of this module."""
    key = (shape, d["npoints"], complex(w))
    if key not in _ORACLE:
        _ORACLE[key] = oracle.assemble(oracle.params(d), complex(w))
    return _ORACLE[key]


def _check_counts(oracle, shape, d, ws, iv, M=None):
    for k, w in enumerate(ws):
        Mo, tot = _oracle_fill(oracle, shape, d, w)
        print(f"omega {complex(w)}: intervals {iv[k]} (oracle {tot})")
        assert iv[k] == tot, (w, iv[k], tot)
        if M is not None:
            assert np.abs(M[k] - Mo).max() <= TOL * np.abs(Mo).max(), (w, np.abs(M[k] - Mo).max() / np.abs(Mo).max())


# ---- 1. routing --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_routing_follows_the_switch(emme, shape):
    d = SHAPES[shape]()
    with _ctx(emme, d, **OPTS) as ctx:
        assert ctx.deriv_cache_shapes() == emme.DERIV_CACHE_SHAPES_ALL
        ctx.cache_settle(WS10)
        mode, state = ctx.fill_kernel(), ctx.cache_state()
        assert mode.startswith("k_assemble_dense") and state[0] >= 0
        on, pr = _cached_deriv(ctx, WS10)
        assert pr.dense_rounds + pr.sparse_rounds > 0 and pr.matrices == 10 and pr.deferred_launches >= 1
        assert ctx.fill_kernel() == mode  # emme_ctx_fill_mode keeps naming the last plain fill
        assert ctx.cache_state() == state  # (settled on these omegas)
        # an out-of-range value is rejected and the earlier value kept
        for bad in (-1, 2):
            with pytest.raises(Exception):
                ctx.set_deriv_cache_shapes(bad)
        assert ctx.deriv_cache_shapes() == emme.DERIV_CACHE_SHAPES_ALL
        # not a layout setting: it changes on the live context, from the next call on
        ctx.set_deriv_cache_shapes(emme.DERIV_CACHE_SHAPES_ES15)
        assert ctx.deriv_cache_shapes() == emme.DERIV_CACHE_SHAPES_ES15
        ctx.profile_read(reset=True)
        off = ctx.assemble_derivative(WS10, want_intervals=True)
        pr = ctx.profile_read(reset=True)
        assert pr.tile_tasks == 0 and pr.matrices == 10
        assert ctx.cache_state() == state
        # no effect while deriv_cached = 0
        ctx.set_deriv_cache_shapes(emme.DERIV_CACHE_SHAPES_ALL)
        ctx.set_options(deriv_cached=0)
        off0 = ctx.assemble_derivative(WS10, want_intervals=True)
        assert ctx.profile_read(reset=True).tile_tasks == 0
        assert ctx.cache_state() == state
    # what such a context computes today: neither switch, on a fresh context with a cache
    with _ctx(emme, d, emme.DERIV_CACHE_SHAPES_ES15, node_cache_gb=8.0) as ctx:
        ctx.cache_settle(WS10)
        today = ctx.assemble_derivative(WS10, want_intervals=True)
    for got in (off, off0):
        assert np.array_equal(_bits(got[0]), _bits(today[0])) and np.array_equal(_bits(got[1]), _bits(today[1]))
        assert np.array_equal(got[2], today[2])
    assert np.array_equal(on[2], today[2])


# ---- 2. per shape: counts, M, M' ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_counts_m_and_mp(emme, oracle, shape):
    d = SHAPES[shape]()
    with _ctx(emme, d, **OPTS) as ctx:
        ctx.cache_settle(WS10)
        M0, iv0 = ctx.assemble(WS10, want_intervals=True)
        (M, Mp, iv), pr = _cached_deriv(ctx, WS10)
        (M2, Mp2, iv2), _ = _cached_deriv(ctx, WS10)
        (M1, Mp1, iv1), _ = _cached_deriv(ctx, WS10[1:2])  # a single-omega call after the cache exists
        u, u2 = _partner(emme, ctx, WS10)
    nchunks = -(-10 // CAPACITY[shape])
    print(f"tile tasks {pr.tile_tasks}, rounds {pr.dense_rounds} MFMA / {pr.sparse_rounds} vector")
    assert pr.tile_tasks >= nchunks * _ntiles(d["npoints"]) and pr.tile_tasks % _ntiles(d["npoints"]) == 0
    _check_counts(oracle, shape, d, WS10, iv, M)
    assert np.array_equal(iv, iv0)
    for b in range(10):  # M: the plain cached fill's within the bar
        assert np.abs(M[b] - M0[b]).max() <= TOL * np.abs(M0[b]).max(), b
    _check_against_partner(d, WS10, (M, Mp, iv), u, u2, damped=(W_DAMPED_POS,))
    # M' of the first omega is the complex derivative of the oracle's M
    po = oracle.params(d)
    h = 1e-6
    Mh, _ = oracle.assemble(po, complex(WS10[0]) + h)
    Ml, _ = oracle.assemble(po, complex(WS10[0]) - h)
    fd = np.abs(Mp[0] - (Mh - Ml) / (2 * h)).max() / np.abs(Mp[0]).max()
    print(f"M' against the oracle's central difference: {fd:.3e} of max|M'|")
    assert fd <= 1e-6
    # two fills of a settled context
    assert np.array_equal(iv, iv2) and np.array_equal(_bits(M), _bits(M2)) and np.array_equal(_bits(Mp), _bits(Mp2))
    # the single-omega call
    assert iv1[0] == iv[1]
    assert np.abs(M1[0] - M[1]).max() <= 1e-13 * np.abs(M[1]).max()
    assert np.abs(Mp1[0] - Mp[1]).max() <= 1e-13 * np.abs(Mp[1]).max()


# ---- 3. several chunks and a partial last one ----------------------------------------------------------------------------
def _batch15():
    rng = np.random.default_rng(3)
    return np.concatenate([rng.uniform(-1.2, -0.4, 13) + 1j * rng.uniform(0.05, 0.4, 13), [0.6 + 0.1j, W_DAMPED_POS]])


CHUNKING = {
    # (parameters, options): chunks of 2 (7 full ones and a single omega); chunks of 8 (dense_min_tasks = 0 keeps the
    # planner from halving them on so small a grid: one full chunk and one of 7) and the planned halving to 2
    "em31": (lambda: example_stellarator(npoints=8), {}),
    "em15": (lambda: example_stellarator(npoints=8, integration_start_points=15), {}),
    "es31": (lambda: example_tokamak(npoints=12, integration_start_points=31), {"dense_min_tasks": 0}),
    "es31-halved": (lambda: example_tokamak(npoints=12, integration_start_points=31), {}),
}


@pytest.mark.parametrize("case", sorted(CHUNKING))
def test_several_chunks_and_a_partial_one(emme, oracle, case):
    """13 omegas with Re omega < 0 and 2 with Re omega > 0 (each class has its cache): more chunks than one, the last one
    partial, both classes' roots on the level-0 list of the chunks that mix them."""
    make, opts = CHUNKING[case]
    d, ws = make(), _batch15()
    cap = 2 if case != "es31" else 8
    with _ctx(emme, d, **dict(OPTS, **opts)) as ctx:
        ctx.cache_settle(ws)
        M0, iv0 = ctx.assemble(ws, want_intervals=True)
        (M, Mp, iv), pr = _cached_deriv(ctx, ws)
        u, u2 = _partner(emme, ctx, ws)
    ntiles = _ntiles(d["npoints"])
    print(f"tile tasks {pr.tile_tasks} on {ntiles} tiles")
    assert pr.tile_tasks == -(-15 // cap) * ntiles
    _check_counts(oracle, case, d, ws, iv, M)
    assert np.array_equal(iv, iv0)
    _check_against_partner(d, ws, (M, Mp, iv), u, u2, damped=(W_DAMPED_POS,))


# ---- 4. round mixes ------------------------------------------------------------------------------------------------------
# (tests/test_gpu_derivative_cached.py: the planned mix, one chunk, every round on the matrix cores / on the vector ALU)
ROUND_MIXES = {"planned": {}, "one-chunk": {"dense_min_tasks": 0}, "all-mfma": {"dense_min_tasks": 0, "dense_min_cols": 1},
               "all-vector": {"dense_min_tasks": 0, "dense_min_cols": 17}}
WS_MIX = {"em31": np.array([-1.656 + 2.49j, -0.85 - 0.32j, 0.4 - 0.2j, W_DAMPED_POS]),
          "em15": np.array([-1.656 + 2.49j, -0.85 - 0.32j, 0.4 - 0.2j, W_DAMPED_POS]),
          "es31": np.array([-0.8 + 0.25j, -0.6 - 0.21j, 0.5 + 0.1j, W_DAMPED_POS, -0.7 + 0.3j, -0.9 + 0.1j])}


@pytest.mark.parametrize("mix", sorted(ROUND_MIXES))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_round_mixes(emme, oracle, shape, mix):
    d = SHAPES[shape](npoints=10 if shape != "es31" else 12)
    ws = WS_MIX[shape]
    with _ctx(emme, d, **dict(OPTS, **ROUND_MIXES[mix])) as ctx:
        ctx.cache_settle(ws)
        (M, Mp, iv), pr = _cached_deriv(ctx, ws)
        u, u2 = _partner(emme, ctx, ws)
    print(f"rounds {pr.dense_rounds} MFMA / {pr.sparse_rounds} vector, tile tasks {pr.tile_tasks}")
    if mix == "all-mfma":
        assert pr.dense_rounds > 0 and pr.sparse_rounds == 0
    if mix == "all-vector":
        assert pr.dense_rounds == 0 and pr.sparse_rounds > 0
    _check_counts(oracle, shape, d, ws, iv, M)
    _check_against_partner(d, ws, (M, Mp, iv), u, u2, damped=(W_DAMPED_POS,))


# ---- 5. small and odd grids ----------------------------------------------------------------------------------------------
GRIDS = [("em31", n) for n in (2, 3, 6, 7, 17)] + [("em15", n) for n in (2, 3, 6, 7, 17)] + [("es31", n) for n in (2, 5, 17)]


@pytest.mark.parametrize("shape,n", GRIDS, ids=[f"{s}-{n}" for s, n in GRIDS])
def test_small_and_odd_grids(emme, oracle, shape, n):
    """One pair, fewer pairs than a tile, 15 pairs (one partial tile), two tiles, nine tiles (the last workgroup with
    idle waves, its last tile partial); one omega and three.  The cache is built by a first plain call."""
    d = SHAPES[shape](npoints=n)
    ws3 = WS10[[0, 2, 1]]
    with _ctx(emme, d, **OPTS) as ctx:
        ctx.assemble(WS10[:3])
        assert ctx.cache_state()[0] >= 0
        for ws in (ws3[:1], ws3):
            M0, iv0 = ctx.assemble(ws, want_intervals=True)
            got, _ = _cached_deriv(ctx, ws)
            u, _u2 = _partner(emme, ctx, ws, spread=False)
            _check_counts(oracle, shape, d, ws, got[2], got[0])
            assert np.array_equal(got[2], iv0)
            _check_against_partner(d, ws, got, u, None)


# ---- 6. leaving the cache --------------------------------------------------------------------------------------------------
def _leave_the_cache(emme, ctx, d, ws, damped=()):
    """The first cached derivative fill of a fresh context (it builds the cache itself) against the partner."""
    got, pr = _cached_deriv(ctx, ws)
    handed = ctx.last_deferred()
    assert ctx.cache_state()[0] >= 0
    u, u2 = _partner(emme, ctx, ws)
    print(f"handed over: {handed} integrals; cache state {ctx.cache_state()}")
    assert pr.deferred_launches >= 1 and handed > 0  # nothing handed over = the test shows nothing
    _check_against_partner(d, ws, got, u, u2, damped=damped)
    return got


# budgets (GiB) that hold the shallowest cache shape only, the full tree to depth 3 and the subtree below it (30
# intervals per class in the main buffer, a quarter of the budget at most): 6 tiles x 16 KB, 6 x 8 KB, 24 x 16 KB per interval
SHALLOW_GB = {"em31": 0.015, "em15": 0.008, "es31": 0.06}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_leaving_the_cache_shallow_cache(emme, oracle, shape):
    d = SHAPES[shape]()
    ws = np.array([-0.8 + 0.25j, -0.6 - 0.21j, 0.5 + 0.1j, W_DAMPED_POS])
    with _ctx(emme, d, node_cache_gb=SHALLOW_GB[shape], cache_min_depth=1, wl_min=1, deriv_cached=1) as ctx:
        got = _leave_the_cache(emme, ctx, d, ws, damped=(W_DAMPED_POS,))
        assert ctx.cache_state()[0] == 3
    _check_counts(oracle, shape, d, ws, got[2])


# The trees of the 15-point rule at the damped omega (about 26 intervals per integral) outgrow the deepest cache shape
# (full tree to depth 8), which a grid this small gets from any ordinary budget.  The 31-point rule needs about 20
# intervals per integral there (the oracle's counts) and stays inside that shape: its two contexts get the budget of the
# next-to-shallowest shape instead (full tree to depth 4, subtree to 7: 62 intervals per class in the main buffer), which
# the ordinary omegas of the call mostly fit and the damped one does not.
DAMPED_GB = {"em31": 0.03, "em15": 8.0, "es31": 0.12}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_leaving_the_cache_strongly_damped_omega(emme, oracle, shape):
    d = SHAPES[shape]()
    ws = np.array([-0.8 + 0.25j, -0.6 - 0.21j, W_DAMPED, 0.5 + 0.1j])
    with _ctx(emme, d, node_cache_gb=DAMPED_GB[shape], cache_min_depth=1, wl_min=1, deriv_cached=1) as ctx:
        got = _leave_the_cache(emme, ctx, d, ws, damped=(W_DAMPED,))
        assert ctx.cache_state()[0] == (8 if shape == "em15" else 4)
    _check_counts(oracle, shape, d, ws, got[2])


@pytest.fixture(scope="module")
def lattice():
    import bench
    return bench.lattice(1, 0, 128)


def test_leaving_the_cache_poisoned_tiles(emme, lattice):
    """Re omega > 0 on the headline lattice at N = 256 with the 31-point rule: tiles of that contour class hold poisoned
    blocks (a folded amplitude that is not representable), whose integrals all go to the list kernel."""
    import bench
    d = dict(bench.workload_dict(256), integration_start_points=31)
    ws = (-lattice.real + 1j * lattice.imag)[::8]
    with _ctx(emme, d, node_cache_gb=40.0, deriv_cached=1) as ctx:
        _leave_the_cache(emme, ctx, d, ws)


# ---- 7. Newton -------------------------------------------------------------------------------------------------------------
NEWTON = {
    "stellarator": (lambda: example_stellarator(npoints=24), -1.656 + 2.49j),
    "tokamak-es31": (lambda: example_tokamak(npoints=32, integration_start_points=31), -0.8 + 0.25j),
}


@pytest.mark.parametrize("case", sorted(NEWTON))
def test_newton_on_the_cache(emme, oracle, case):
    """Six guesses: four within 1e-3 of the oracle's root, two of the lattice's.  A chain is compared if it converges in
    the partner run (switch off) and in its omega (1 + 1e-13) twin to roots within 1e-9 relative; every compared chain
    then has the same iteration count, a root within 1e-9 relative and info 0 on the cache.  At least half the guesses
    must be compared (the printed line says how many were: the partner alone qualified all six on both inputs when the
    guesses were chosen, the two lattice guesses after 17-18 and 5-6 steps)."""
    make, guess = NEWTON[case]
    d = make()
    r_or, its_or, _, _ = oracle.solve_root(oracle.params(d), guess)
    print(f"oracle root {r_or!r} in {len(its_or)} steps")
    guesses = np.array([r_or * (1 + 1e-3), r_or * (1 - 1e-3), r_or * (1 + 1e-3j), r_or * (1 - 1e-3j), guess, guess - 0.1])
    limit = d["iteration_step_limit"]
    with _ctx(emme, d, **OPTS) as ctx:
        ctx.cache_settle(guesses)
        ctx.profile(True)
        ctx.set_deriv_cache_shapes(emme.DERIV_CACHE_SHAPES_ES15)
        ctx.profile_read(reset=True)
        ra, ita, ia = ctx.solve_roots_newton(guesses)
        rb, itb, ib = ctx.solve_roots_newton(guesses * (1 + 1e-13))
        assert ctx.profile_read(reset=True).tile_tasks == 0
        ctx.set_deriv_cache_shapes(emme.DERIV_CACHE_SHAPES_ALL)
        rc, itc, ic = ctx.solve_roots_newton(guesses)
        assert ctx.profile_read(reset=True).tile_tasks > 0  # the fills went through the cache
        v, vinfo = ctx.null_vectors(nbatch=len(guesses))
        assert np.isfinite(v[ic == 0]).all()
        assert np.isfinite(ctx.final_matrix(0)).all()
    conv_a, conv_b = (ia == 0) & (ita <= limit), (ib == 0) & (itb <= limit)
    with np.errstate(invalid="ignore"):
        cmp_ = conv_a & conv_b & (np.abs(ra - rb) <= 1e-9 * np.abs(ra))
    print(f"Newton: converged {conv_a.sum()} / {conv_b.sum()} in the partner runs, compared {cmp_.sum()} of {len(guesses)}; "
          f"iterations {itc} (partner {ita}); |root - partner| / |partner| {np.abs(rc - ra) / np.abs(ra)}")
    assert 2 * cmp_.sum() >= len(guesses)
    assert (ic[cmp_] == 0).all()
    assert np.array_equal(itc[cmp_], ita[cmp_])
    assert (np.abs(rc[cmp_] - ra[cmp_]) <= 1e-9 * np.abs(ra[cmp_])).all()


# ---- 8. precedence ---------------------------------------------------------------------------------------------------------
def test_the_cache_comes_before_the_tile_fill(emme, oracle):
    """The tile triple (tile_uncached, deriv_cached, TILE_SHAPES_ALL) and the switch together.  dense_min_cols = 17 makes
    the two kernels tell themselves apart in the profile: the cached kernel then runs vector rounds only (sparse_rounds),
    the tile-shape kernel has MFMA rounds only (dense_rounds).  16 omegas of one class on a context with a cache: the cache
    serves them all.  A 17th on the Re omega > 0 side, a minority class without a cache: the policy leaves it to the
    tile-shape kernel, in the same call.  Without a cache budget the same switches give the tile-shape kernel as today."""
    d = example_stellarator(npoints=10)
    major = np.linspace(-1.8, -1.0, 16) + 1.5j
    ws = np.concatenate([major, [0.4 + 0.3j]])
    triple = dict(tile_uncached=1, deriv_cached=1, dense_min_cols=17, wl_min=1)
    with _ctx(emme, d, node_cache_gb=8.0, **triple) as ctx:
        ctx.set_tile_shapes(emme.TILE_SHAPES_ALL)
        ctx.assemble(ws)  # (the plain fill builds the cache of the majority class)
        (M, Mp, iv), pr = _cached_deriv(ctx, major)
        assert pr.sparse_rounds > 0 and pr.dense_rounds == 0 and pr.tile_tasks == 8 * _ntiles(10)
        assert ctx.last_deferred() >= 0  # (the cached fill's work list)
        (Ma, Mpa, iva), pr = _cached_deriv(ctx, ws)
        # 8 chunks of 2 on the cache, one chunk of the tile-shape kernel for the minority omega
        assert pr.sparse_rounds > 0 and pr.dense_rounds > 0 and pr.tile_tasks == 9 * _ntiles(10) and pr.matrices == 17
        # the partner on this context is the tile-shape kernel: switch off, triple on, as today
        ctx.set_deriv_cache_shapes(emme.DERIV_CACHE_SHAPES_ES15)
        ctx.profile_read(reset=True)
        u = ctx.assemble_derivative(ws, want_intervals=True)
        pr = ctx.profile_read(reset=True)
        assert pr.tile_tasks > 0 and pr.dense_rounds > 0 and pr.sparse_rounds == 0
    assert np.array_equal(_bits(Ma[:16]), _bits(M)) and np.array_equal(_bits(Mpa[:16]), _bits(Mp))
    _check_counts(oracle, "precedence", d, ws[[0, 16]], iva[[0, 16]], Ma[[0, 16]])
    for b in range(17):
        assert iva[b] == u[2][b]
        assert np.abs(Ma[b] - u[0][b]).max() <= TOL * np.abs(u[0][b]).max()
        assert np.abs(Mpa[b] - u[1][b]).max() <= TOL * np.abs(u[1][b]).max()
    out = []
    for shapes in (emme.DERIV_CACHE_SHAPES_ES15, emme.DERIV_CACHE_SHAPES_ALL):
        with _ctx(emme, d, shapes, node_cache_gb=0.0, **triple) as ctx:
            ctx.set_tile_shapes(emme.TILE_SHAPES_ALL)
            ctx.profile(True)
            ctx.profile_read(reset=True)
            out.append(ctx.assemble_derivative(ws, want_intervals=True))
            pr = ctx.profile_read(reset=True)
            assert pr.tile_tasks > 0 and pr.dense_rounds > 0 and pr.sparse_rounds == 0
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(_bits(a) if a.dtype == np.complex128 else a, _bits(b) if b.dtype == np.complex128 else b)


# ---- 9. one full-size sample -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx256(emme, lattice):
    """BASELINE configs[3] (stellarator, electromagnetic, GK31, N = 256, dim 512) on a default context with
    deriv_cached = 1 and the switch on: one cache build, by the plain fill of the sample's omegas."""
    z = np.load(os.path.join(G, "cfg4_damped.npz"))
    ws = np.concatenate([lattice[::8], z["omegas"][[1, 3]]])
    ctx = _ctx(emme, example_stellarator(npoints=256), deriv_cached=1)
    ctx.cache_settle(ws)
    yield ctx, ws, z["intervals"][[1, 3]]
    ctx.close()


def test_full_size_sample(emme, ctx256):
    """16 lattice omegas and two of the reference's own damped iterates (cfg4_damped.npz): the interval totals of those two
    against the fixture, all counts, M and M' against the partner."""
    ctx, ws, ref_iv = ctx256
    assert ctx.fill_kernel_symbol() == "k_assemble_dense<1, 31, 3>"
    state = ctx.cache_state()
    (M, Mp, iv), pr = _cached_deriv(ctx, ws)
    assert ctx.cache_state() == state
    assert pr.matrices == 18 and pr.tile_tasks == 9 * _ntiles(256)
    u, u2 = _partner(emme, ctx, ws)
    print(f"intervals of the two damped omegas {iv[16:]} (fixture {ref_iv}); handed over {ctx.last_deferred()}")
    assert np.array_equal(iv[16:], ref_iv)
    _check_against_partner(example_stellarator(npoints=256), ws, (M, Mp, iv), u, u2, damped=tuple(complex(w) for w in ws[16:]))
