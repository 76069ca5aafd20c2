"""M and the exact dM/domega from the table-free tile fill (options tile_uncached + deriv_cached, k_assemble_tile_deriv,
DESIGN.md §12.3): a derivative fill on a context without a node cache builds the dense fill's operands in LDS, decides
on K and G exactly as k_assemble_tile does and takes K' from a second GEMM on the same operands.

The partner for M' is the omega-lane derivative fill (k_assemble_wl_deriv) on the same context after
set_options(tile_uncached=0); test_gpu_derivative.py pins that one against central differences and the argument
principle.  Bars: the project's own -- entries within 1e-10 max|.| per matrix, interval counts equal to the CPU oracle's
item by item; at strongly damped omegas 10 x the partner's own spread under omega (1 + 1e-13) with the 1e-10 floor
(_leave_the_cache of test_gpu_derivative_cached.py).  M must also be the plain tile fill's, bit for bit: the chunks are
the same and only K and G decide.  Every test asserts tile_tasks > 0 after the derivative fill: without the kernel a
derivative fill never runs a tile task on a context without a cache.
"""
import numpy as np
import pytest

from oracle.binding import example_stellarator, example_tokamak

pytestmark = pytest.mark.gpu

TOL = 1e-10
TOL_W = 1e-9
OPTS = dict(node_cache_gb=0.0, wl_min=1, tile_uncached=1, deriv_cached=1)
# more than 64 intervals on one bisection level (test_gpu_tile_fill.py)
W_WIDE = -0.00552674 - 0.73419159j
OMEGAS5 = [-0.8 + 0.25j, -0.6 - 0.21j, 0.5 + 0.1j, -0.142 - 1.469j, 0.153 - 0.316j]
DAMPED = (-0.142 - 1.469j, 0.153 - 0.316j)
ROOT32 = -0.5742270508974 + 0.2743044402209j  # the oracle's root at npoints 32 (6 secant steps from -0.8+0.25i)


def _ctx(emme, d, **options):
    return emme.Context(emme.params_from_dict(d), **options)


def _bits(a):
    return np.ascontiguousarray(a).view(np.float64)


def _tile_deriv(ctx, ws):
    """One derivative fill with the profile's tile-task count: ((M, Mp, iv), profile)."""
    ctx.profile(True)
    ctx.profile_read(reset=True)
    out = ctx.assemble_derivative(ws, want_intervals=True)
    pr = ctx.profile_read(reset=True)
    assert pr.tile_tasks > 0, "the derivative fill did not go through k_assemble_tile_deriv"
    return out, pr


def _partner(ctx, ws):
    """The omega-lane derivative fill of the same omegas on the same context, and of omega (1 + 1e-13)."""
    ctx.set_options(tile_uncached=0)
    try:
        ctx.profile_read(reset=True)
        u = ctx.assemble_derivative(ws, want_intervals=True)
        assert ctx.profile_read(reset=True).tile_tasks == 0
        u2 = ctx.assemble_derivative(np.asarray(ws) * (1 + 1e-13))
    finally:
        ctx.set_options(tile_uncached=1)
    return u, u2


def _check_against_partner(ws, got, u, u2, damped=(), check_m=True):
    M, Mp, iv = got
    assert np.array_equal(iv, u[2]), (iv, u[2])
    for b, w in enumerate(ws):
        bar_m, bar_p = TOL * np.abs(u[0][b]).max(), TOL * np.abs(u[1][b]).max()
        which = "1e-10"
        if complex(w) in damped:  # 10 x the partner's own spread, same floor
            bar_m = max(bar_m, 10.0 * np.abs(u[0][b] - u2[0][b]).max())
            bar_p = max(bar_p, 10.0 * np.abs(u[1][b] - u2[1][b]).max())
            which = "spread"
        em, ep = np.abs(M[b] - u[0][b]).max(), np.abs(Mp[b] - u[1][b]).max()
        print(f"omega {complex(w)}: M {em / np.abs(u[0][b]).max():.3e} of max|M| (bar {bar_m / np.abs(u[0][b]).max():.3e}), "
              f"M' {ep / np.abs(u[1][b]).max():.3e} of max|M'| (bar {bar_p / np.abs(u[1][b]).max():.3e}, {which})")
        if check_m:
            assert em <= bar_m, (w, em, bar_m)
        assert ep <= bar_p, (w, ep, bar_p)
        # the kernel writes an entry with its mirror; M' has no diagonal
        assert np.abs(Mp[b] - Mp[b].T).max() == 0.0 and np.abs(np.diag(Mp[b])).max() == 0.0


def _check_against_oracle(oracle, po, ws, M, iv, loose=()):
    for k, w in enumerate(ws):
        Mo, tot = oracle.assemble(po, complex(w))
        err = np.abs(M[k] - Mo).max() / np.abs(Mo).max()
        print(f"omega {complex(w)}: intervals {iv[k]} (oracle {tot}), max entry error {err:.3e} of max|M|")
        assert iv[k] == tot, (w, iv[k], tot)
        if complex(w) not in loose:
            assert err <= TOL, (w, err)


# ---- 1. both contour classes in one call ---------------------------------------------------------------------------------
def test_both_classes_in_one_call(emme, oracle):
    """npoints 40: 780 pairs, 49 tiles, the last one partial, 25 two-wave workgroups per chunk."""
    d = example_tokamak(npoints=40)
    po = oracle.params(d)
    ws = OMEGAS5
    with _ctx(emme, d, **OPTS) as ctx:
        M0, iv0 = ctx.assemble(ws, want_intervals=True)
        mode0 = ctx.fill_kernel()
        assert mode0.startswith("k_assemble_tile")
        (M, Mp, iv), pr = _tile_deriv(ctx, ws)
        assert pr.matrices == 5
        assert ctx.fill_kernel() == mode0  # emme_ctx_fill_mode keeps naming the last plain fill
        (M1, Mp1, iv1), _ = _tile_deriv(ctx, ws[1:2])
        u, u2 = _partner(ctx, ws)
    # counts: the oracle's, item by item (8 756, 17 384, 10 548, 70 192, 31 262)
    for k, w in enumerate(ws):
        _, tot = oracle.assemble(po, complex(w))
        print(f"omega {w}: intervals {iv[k]} (oracle {tot})")
        assert iv[k] == tot, (w, iv[k], tot)
    assert list(iv) == [8756, 17384, 10548, 70192, 31262]
    # M: the plain tile fill's, bit for bit
    assert np.array_equal(iv, iv0)
    assert np.array_equal(_bits(M), _bits(M0))
    # M': the partner's (M is held to the plain tile fill above, which test_gpu_tile_fill.py holds to the oracle)
    _check_against_partner(ws, (M, Mp, iv), u, u2, damped=DAMPED, check_m=False)
    # M' of the first omega is the complex derivative of the oracle's M
    h = 1e-6
    Mh, _ = oracle.assemble(po, complex(ws[0]) + h)
    Ml, _ = oracle.assemble(po, complex(ws[0]) - h)
    fd = np.abs(Mp[0] - (Mh - Ml) / (2 * h)).max() / np.abs(Mp[0]).max()
    print(f"M' against the oracle's central difference: {fd:.3e} of max|M'|")
    assert fd <= 1e-6
    # a single-omega call
    assert iv1[0] == iv[1]
    assert np.abs(M1[0] - M[1]).max() <= 1e-13 * np.abs(M[1]).max()
    assert np.abs(Mp1[0] - Mp[1]).max() <= 1e-13 * np.abs(Mp[1]).max()


# ---- 2. several chunks per class, repeatability ---------------------------------------------------------------------------
def _batch22():
    rng = np.random.default_rng(3)
    return np.concatenate([rng.uniform(-1.2, -0.4, 20) + 1j * rng.uniform(0.05, 0.4, 20), [0.6 + 0.1j, 0.153 - 0.316j]])


def test_several_chunks_per_class_and_repeatable(emme, oracle):
    d = example_tokamak(npoints=24)
    ws = _batch22()
    with _ctx(emme, d, **OPTS) as ctx:
        (M, Mp, iv), pr = _tile_deriv(ctx, ws)
        (M2, Mp2, iv2), _ = _tile_deriv(ctx, ws)
        u, u2 = _partner(ctx, ws)
    ntiles = (24 * 23 // 2 + 15) // 16
    assert ntiles == 18
    print(f"tile tasks {pr.tile_tasks}")
    assert pr.tile_tasks > 2 * ntiles and pr.tile_tasks % ntiles == 0
    _check_against_oracle(oracle, oracle.params(d), ws, M, iv)
    _check_against_partner(ws, (M, Mp, iv), u, u2, damped=DAMPED)
    assert np.array_equal(iv, iv2)
    assert np.array_equal(_bits(M), _bits(M2))
    assert np.array_equal(_bits(Mp), _bits(Mp2))


# ---- 3. small and odd grids -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 5, 17])
def test_small_and_odd_grids(emme, oracle, n):
    """One pair, a partial tile, and (17: 136 pairs, 9 tiles) a last workgroup with an idle wave."""
    d = example_tokamak(npoints=n)
    po = oracle.params(d)
    with _ctx(emme, d, **OPTS) as ctx:
        for ws in ([-0.8 + 0.25j], [-0.8 + 0.25j, 0.5 + 0.1j, -0.6 - 0.21j]):
            got, _ = _tile_deriv(ctx, ws)
            u, u2 = _partner(ctx, ws)
            _check_against_oracle(oracle, po, ws, got[0], got[2])
            _check_against_partner(ws, got, u, u2)


# ---- 4. hand-over ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ws", [[W_WIDE], [-0.8 + 0.25j, W_WIDE, -0.6 - 0.21j]], ids=["alone", "in-a-chunk"])
def test_hands_over_full_level_lists(emme, oracle, ws):
    """npoints 5 (10 pairs, one tile): every integral of W_WIDE (5 324 intervals) outgrows the 64-entry level list and
    goes, whole, to the tile fill's work list; launch_assemble_deriv_list gives M and M' of them from scratch."""
    d = example_tokamak(npoints=5)
    po = oracle.params(d)
    with _ctx(emme, d, **OPTS) as ctx:
        got, pr = _tile_deriv(ctx, ws)
        handed = ctx.last_deferred()
        u, u2 = _partner(ctx, ws)
    print(f"handed over: {handed} integrals; deferred launches {pr.deferred_launches}")
    assert pr.tile_tasks > 0 and pr.deferred_launches > 0
    assert 0 < handed <= 10  # nothing handed over = the test shows nothing
    for k, w in enumerate(ws):
        _, tot = oracle.assemble(po, complex(w))
        assert got[2][k] == tot, (w, got[2][k], tot)
        if complex(w) == W_WIDE:
            assert tot == 5324
    _check_against_partner(ws, got, u, u2, damped=(W_WIDE,))


# ---- 5. Newton ------------------------------------------------------------------------------------------------------------
def test_newton_through_the_tile_fill(emme, oracle):
    d = example_tokamak(npoints=32)
    po = oracle.params(d)
    r_or, its_or, _, _ = oracle.solve_root(po, -0.8 + 0.25j)
    assert len(its_or) == 6 and abs(r_or - ROOT32) <= 1e-11, (r_or, len(its_or))
    guesses = np.array([r_or * (1 + 1e-3), r_or * (1 - 1e-3), r_or * (1 + 1e-3j)])
    with _ctx(emme, d, **OPTS) as ctx:
        ctx.profile(True)
        ctx.profile_read(reset=True)
        roots, iters, info = ctx.solve_roots_newton(guesses)
        assert ctx.profile_read(reset=True).tile_tasks > 0
        v, vinfo = ctx.null_vectors(nbatch=3)
        assert (vinfo == 0).all() and np.isfinite(v).all()
        assert np.isfinite(ctx.final_matrix(0)).all()
        ctx.set_options(tile_uncached=0)
        roots_u, iters_u, info_u = ctx.solve_roots_newton(guesses)
        assert ctx.profile_read(reset=True).tile_tasks == 0
    print(f"Newton: iterations {iters} (omega-lane {iters_u}), |root - oracle| {np.abs(roots - r_or)}")
    assert (info == 0).all() and (info_u == 0).all(), (info, info_u)
    assert (np.abs(roots - r_or) <= TOL_W).all()
    assert np.array_equal(iters, iters_u)
    assert (np.abs(roots - roots_u) <= 1e-9 * np.abs(roots_u)).all()


# ---- 6. what it does not serve ----------------------------------------------------------------------------------------------
def _deriv_with(emme, d, ws, **opts):
    with _ctx(emme, d, node_cache_gb=0.0, wl_min=1, **opts) as ctx:
        ctx.profile(True)
        ctx.profile_read(reset=True)
        out = ctx.assemble_derivative(ws, want_intervals=True)
        return out, ctx.profile_read(reset=True).tile_tasks


def _same_bits(a, b):
    return np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(a[2], b[2])


def test_what_it_does_not_serve_keeps_its_kernel(emme):
    ws = [-0.8 + 0.25j, -0.6 - 0.21j, 0.5 + 0.1j]
    wem = [-1.656 + 2.49j, -0.85 - 0.32j, 0.4 - 0.2j]
    cases = [("electromagnetic", example_stellarator(npoints=10), wem),
             ("GK31", example_tokamak(npoints=12, integration_start_points=31), ws),
             ("accuracy 1e-12", example_tokamak(npoints=12, integration_accuracy=1e-12), ws)]
    for name, d, w in cases:
        off, t_off = _deriv_with(emme, d, w, tile_uncached=0, deriv_cached=0)
        on, t_on = _deriv_with(emme, d, w, tile_uncached=1, deriv_cached=1)
        assert t_off == 0 and t_on == 0, (name, t_off, t_on)
        assert _same_bits(off, on), name
    # each option alone
    d = example_tokamak(npoints=12)
    off, t_off = _deriv_with(emme, d, ws, tile_uncached=0, deriv_cached=0)
    assert t_off == 0
    for alone in (dict(tile_uncached=1, deriv_cached=0), dict(tile_uncached=0, deriv_cached=1)):
        got, t = _deriv_with(emme, d, ws, **alone)
        assert t == 0, alone
        assert _same_bits(off, got), alone
    # the pair: the tile fill, the same trees
    both, t = _deriv_with(emme, d, ws, tile_uncached=1, deriv_cached=1)
    assert t > 0
    assert np.array_equal(both[2], off[2])
    with _ctx(emme, d, **OPTS) as ctx:
        for bad in (dict(tile_uncached=2), dict(deriv_cached=2)):
            with pytest.raises(Exception):
                ctx.set_options(**bad)


# ---- 7. the minority class of a cached derivative call ---------------------------------------------------------------------
def test_serves_the_minority_class_of_a_cached_call(emme, oracle):
    """17 omegas, one on the Re omega > 0 side: the majority goes through the node cache (k_assemble_dense_deriv), the
    minority pass through k_assemble_tile_deriv -- two work lists, two list launches."""
    d = example_tokamak(npoints=12)
    ws = np.concatenate([np.linspace(-1.0, -0.5, 16) + 0.2j, [0.5 + 0.1j]])
    with _ctx(emme, d, node_cache_gb=8.0, tile_uncached=1, deriv_cached=1) as ctx:
        (M, Mp, iv), pr = _tile_deriv(ctx, ws)
        assert ctx.cache_state()[0] >= 0
    assert pr.deferred_launches >= 2
    with _ctx(emme, d, node_cache_gb=0.0, wl_min=1) as ctx:
        u = ctx.assemble_derivative(ws, want_intervals=True)
    _check_against_oracle(oracle, oracle.params(d), ws, M, iv)
    _check_against_partner(ws, (M, Mp, iv), u, None)


# ---- 8. full size ---------------------------------------------------------------------------------------------------------
def test_full_size_sample(emme, oracle):
    """npoints 1024, 2 omegas, against the omega-lane derivative fill on a second context (equal interval totals, M and
    M' within 1e-10) and, for M, 64 oracle pairs sampled as in test_tile_fill_full_size_sample."""
    d = example_tokamak(npoints=1024)
    ws = [-0.8 + 0.25j, -0.6 - 0.21j]
    with _ctx(emme, d, **OPTS) as ctx:
        (M, Mp, iv), _ = _tile_deriv(ctx, ws)
    with _ctx(emme, d, node_cache_gb=0.0, wl_min=1) as ctx:
        u = ctx.assemble_derivative(ws, want_intervals=True)
    print("interval totals:", iv, u[2])
    _check_against_partner(ws, (M, Mp, iv), u, None)
    po = oracle.params(d)
    eta, dx = oracle.grid(d["length"], 1024)
    W = lambda i, j: oracle.lib.oracle_weight(1024, i, j)
    for k, w in enumerate(ws):
        scale = np.abs(u[0][k]).max()
        worst = 0.0
        for s in range(64):
            off = 1 + (s * 1022) // 63
            i = (s * 37) % (1024 - off)
            kap, _ = oracle.kappa(po, 0, eta[i], eta[i + off], complex(w))
            want = -kap * W(i, i + off) * dx
            worst = max(worst, abs(M[k][i, i + off] - want), abs(M[k][i + off, i] - want))
        print(f"omega {w}: 64 sampled entries against the oracle, worst {worst / scale:.3e} of max|M|")
        assert worst <= TOL * scale
