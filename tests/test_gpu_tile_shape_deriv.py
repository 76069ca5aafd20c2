"""M and the exact dM/domega from the table-free tile fill for electromagnetic and GK31 contexts
(k_assemble_tile_shape_deriv<PTS, NM>): the option pair tile_uncached + deriv_cached beside
set_tile_shapes(TILE_SHAPES_ALL).  The kernel is k_assemble_tile_shape's walk with a second GEMM on the same operands for
K'; integrals it hands over are finished by k_assemble_deriv_list_shape<PTS>.

Bars: the project's own, as tests/test_gpu_tile_deriv.py states them.
  * M is the plain tile-shape fill's of the same omegas on the same context, bit for bit (only K and G decide; where the
    two fills hand integrals over to different list kernels -- test 4 -- M is held to the partner instead).
  * Interval counts equal the CPU oracle's item by item.
  * M' is within 1e-10 max|M'| of the partner: the omega-lane derivative fill (k_assemble_wl_deriv) on the same context
    after set_tile_shapes(TILE_SHAPES_ES15).  At strongly damped omegas the bar is the larger of that and 10 x the
    PARTNER's own change under omega (1 + 1e-13) -- never computed from the code under test.
Every test asserts tile_tasks > 0 after the derivative fill: without the kernel a derivative fill of these shapes runs no
tile task.
"""
import numpy as np
import pytest

from oracle.binding import example_stellarator, example_tokamak

pytestmark = pytest.mark.gpu

TOL = 1e-10
TOL_W = 1e-9
OPTS = dict(node_cache_gb=0.0, wl_min=1, tile_uncached=1, deriv_cached=1)
W_DAMPED = -0.142 - 1.469j
WS_EM = [-1.656 + 2.49j, -0.85 - 0.32j, 0.4 - 0.2j, W_DAMPED]
WS_ES = [-0.8 + 0.25j, -0.6 - 0.21j, 0.5 + 0.1j, W_DAMPED]
# (the shapes, omegas and hand-over inputs are tests/test_gpu_tile_shapes.py's)
SHAPES = {
    "em31": (lambda: example_stellarator(npoints=10), WS_EM),
    "em15": (lambda: example_stellarator(npoints=10, integration_start_points=15), WS_EM),
    "es31": (lambda: example_tokamak(npoints=12, integration_start_points=31), WS_ES),
}


def _ctx(emme, d, shapes=None, **options):
    ctx = emme.Context(emme.params_from_dict(d), **options)
    if shapes is not None:
        ctx.set_tile_shapes(shapes)
    return ctx


def _bits(a):
    return np.ascontiguousarray(a).view(np.float64)


def _ntiles(n):
    return (n * (n - 1) // 2 + 15) // 16


def _tile_deriv(ctx, ws):
    """One derivative fill with the profile's counters: ((M, Mp, iv), profile)."""
    ctx.profile(True)
    ctx.profile_read(reset=True)
    out = ctx.assemble_derivative(ws, want_intervals=True)
    pr = ctx.profile_read(reset=True)
    assert pr.tile_tasks > 0, "the derivative fill did not go through k_assemble_tile_shape_deriv"
    return out, pr


def _partner(emme, ctx, ws, spread=True):
    """The omega-lane derivative fill of the same omegas on the same context, and of omega (1 + 1e-13)."""
    ctx.set_tile_shapes(emme.TILE_SHAPES_ES15)
    try:
        ctx.profile(True)
        ctx.profile_read(reset=True)
        u = ctx.assemble_derivative(ws, want_intervals=True)
        assert ctx.profile_read(reset=True).tile_tasks == 0
        u2 = ctx.assemble_derivative(np.asarray(ws) * (1 + 1e-13)) if spread else None
    finally:
        ctx.set_tile_shapes(emme.TILE_SHAPES_ALL)
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


def _check_against_partner(d, ws, got, u, u2, damped=(), check_m=True):
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
        if check_m:
            assert em <= bar_m, (w, em, bar_m)
        assert ep <= bar_p, (w, ep, bar_p)
    _check_structure(d, Mp)


def _check_counts(oracle, po, ws, iv):
    for k, w in enumerate(ws):
        _, tot = oracle.assemble(po, complex(w))
        print(f"omega {complex(w)}: intervals {iv[k]} (oracle {tot})")
        assert iv[k] == tot, (w, iv[k], tot)


# ---- 1. both contour classes in one call -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_both_classes_in_one_call(emme, oracle, shape):
    make, ws = SHAPES[shape]
    d = make()
    po = oracle.params(d)
    with _ctx(emme, d, emme.TILE_SHAPES_ALL, **OPTS) as ctx:
        M0, iv0 = ctx.assemble(ws, want_intervals=True)
        mode0 = ctx.fill_kernel()
        assert mode0.startswith("k_assemble_tile")
        (M, Mp, iv), pr = _tile_deriv(ctx, ws)
        assert pr.matrices == 4
        assert ctx.fill_kernel() == mode0  # emme_ctx_fill_mode keeps naming the last plain fill
        (M1, Mp1, iv1), _ = _tile_deriv(ctx, ws[1:2])
        u, u2 = _partner(emme, ctx, ws)
    _check_counts(oracle, po, ws, iv)
    # M: the plain tile-shape fill's, bit for bit
    assert np.array_equal(iv, iv0)
    assert np.array_equal(_bits(M), _bits(M0))
    # M': the partner's (M is held to the plain fill above, which test_gpu_tile_shapes.py holds to the oracle)
    _check_against_partner(d, ws, (M, Mp, iv), u, u2, damped=(W_DAMPED,), check_m=False)
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


# ---- 2. several chunks per class, repeatability ------------------------------------------------------------------------
def _batch15():
    rng = np.random.default_rng(3)
    return np.concatenate([rng.uniform(-1.2, -0.4, 13) + 1j * rng.uniform(0.05, 0.4, 13), [0.6 + 0.1j, 0.153 - 0.316j]])


def test_several_chunks_and_repeatable(emme, oracle):
    """Stellarator npoints 8 (28 pairs, 2 tiles, one two-wave workgroup per chunk): the 13 omegas of Re omega < 0 need
    more than one chunk of 5."""
    d = example_stellarator(npoints=8)
    ws = _batch15()
    with _ctx(emme, d, emme.TILE_SHAPES_ALL, **OPTS) as ctx:
        M0, iv0 = ctx.assemble(ws, want_intervals=True)
        (M, Mp, iv), pr = _tile_deriv(ctx, ws)
        (M2, Mp2, iv2), _ = _tile_deriv(ctx, ws)
        u, u2 = _partner(emme, ctx, ws)
    ntiles = _ntiles(8)
    print(f"tile tasks {pr.tile_tasks}")
    assert pr.tile_tasks > 2 * ntiles and pr.tile_tasks % ntiles == 0
    _check_counts(oracle, oracle.params(d), ws, iv)
    assert np.array_equal(iv, iv0) and np.array_equal(_bits(M), _bits(M0))
    _check_against_partner(d, ws, (M, Mp, iv), u, u2, damped=(0.153 - 0.316j,), check_m=False)
    assert np.array_equal(iv, iv2)
    assert np.array_equal(_bits(M), _bits(M2))
    assert np.array_equal(_bits(Mp), _bits(Mp2))


# ---- 3. small and odd grids --------------------------------------------------------------------------------------------
GRIDS = [("em31", n) for n in (2, 3, 6, 7, 17)] + [("em15", n) for n in (2, 3, 6, 7, 17)] + [("es31", n) for n in (2, 5, 17)]


@pytest.mark.parametrize("shape,n", GRIDS, ids=[f"{s}-{n}" for s, n in GRIDS])
def test_small_and_odd_grids(emme, oracle, shape, n):
    """One pair (three integrals), fewer than 16 pairs, 15 pairs (one partial tile), two tiles (one full workgroup), nine
    tiles (the last workgroup with one idle wave, its tile of 8 pairs); one omega and three."""
    make, ws4 = SHAPES[shape]
    d = dict(make(), npoints=n)
    po = oracle.params(d)
    with _ctx(emme, d, emme.TILE_SHAPES_ALL, **OPTS) as ctx:
        for ws in (ws4[:1], [ws4[0], ws4[2], ws4[1]]):
            M0, iv0 = ctx.assemble(ws, want_intervals=True)
            got, _ = _tile_deriv(ctx, ws)
            u, _u2 = _partner(emme, ctx, ws, spread=False)
            _check_counts(oracle, po, ws, got[2])
            assert np.array_equal(_bits(got[0]), _bits(M0))
            _check_against_partner(d, ws, got, u, None)


# ---- 4. hand-over through the new list kernel --------------------------------------------------------------------------
# Inputs whose trees hold more than 64 intervals on one bisection level (tests/test_gpu_tile_shapes.py: found on the CPU
# with the oracle's interval trace): (parameters, the wide omega, two ordinary omegas)
W_WIDE15 = -0.00552674 - 0.73419159j
W_WIDE31 = -0.005 - 2j
HAND_OVER = {
    "em15-stellarator": (lambda: example_stellarator(npoints=4, integration_start_points=15), W_WIDE15, WS_EM[:2]),
    "em15-tokamak": (lambda: example_tokamak(npoints=4, beta_e=0.02), W_WIDE15, WS_ES[:2]),
    "em31-stellarator": (lambda: example_stellarator(npoints=3, integration_precision=1e-9), W_WIDE31, WS_EM[:2]),
    "es31-tokamak": (lambda: example_tokamak(npoints=3, integration_start_points=31, integration_accuracy=1e-9,
                                             integration_precision=1e-9), W_WIDE31, WS_ES[:2]),
}


@pytest.mark.parametrize("how", ["alone", "in-a-chunk"])
@pytest.mark.parametrize("case", sorted(HAND_OVER))
def test_hands_over_full_level_lists(emme, oracle, case, how):
    """An integral whose split does not fit the next 64-entry level list goes, whole, to the tile fill's work list
    ((b << 32) | (pair nm + moment)); k_assemble_deriv_list_shape gives M and M' of it from scratch, whatever its
    moment."""
    make, wide, ordinary = HAND_OVER[case]
    d = make()
    ws = [wide] if how == "alone" else [ordinary[0], wide, ordinary[1]]
    n = d["npoints"]
    nint = n * (n - 1) // 2 * (3 if d["beta_e"] != 0.0 else 1)  # integrals of one omega
    with _ctx(emme, d, emme.TILE_SHAPES_ALL, **OPTS) as ctx:
        got, pr = _tile_deriv(ctx, ws)
        handed = ctx.last_deferred()
        u, u2 = _partner(emme, ctx, ws)
    print(f"handed over: {handed} integrals of {nint}; deferred launches {pr.deferred_launches}")
    assert pr.deferred_launches > 0
    assert 0 < handed <= nint  # nothing handed over = the test shows nothing
    _check_counts(oracle, oracle.params(d), ws, got[2])
    _check_against_partner(d, ws, got, u, u2, damped=(wide,))


# ---- 5. Newton ---------------------------------------------------------------------------------------------------------
NEWTON = {
    # (parameters, guess of the oracle's secant search, roots held to the oracle's too)
    "stellarator": (lambda: example_stellarator(npoints=16), -1.656 + 2.49j, True),
    "tokamak-em15": (lambda: example_tokamak(npoints=16, beta_e=0.02), -0.8 + 0.25j, True),
    # the oracle's own restarts land up to 2.6e-10 apart on this input: its distance is printed, not asserted
    "tokamak-es31": (lambda: example_tokamak(npoints=16, integration_start_points=31), -0.8 + 0.25j, False),
}


@pytest.mark.parametrize("case", sorted(NEWTON))
def test_newton_through_the_tile_shapes(emme, oracle, case):
    make, guess, hold_to_oracle = NEWTON[case]
    d = make()
    r_or, its_or, _, _ = oracle.solve_root(oracle.params(d), guess)
    print(f"oracle root {r_or!r} in {len(its_or)} steps")
    guesses = np.array([r_or * (1 + 1e-3), r_or * (1 - 1e-3), r_or * (1 + 1e-3j)])
    with _ctx(emme, d, emme.TILE_SHAPES_ALL, **OPTS) as ctx:
        ctx.profile(True)
        ctx.profile_read(reset=True)
        roots, iters, info = ctx.solve_roots_newton(guesses)
        assert ctx.profile_read(reset=True).tile_tasks > 0
        v, vinfo = ctx.null_vectors(nbatch=3)
        assert np.isfinite(v).all()
        assert np.isfinite(ctx.final_matrix(0)).all()
        ctx.set_tile_shapes(emme.TILE_SHAPES_ES15)
        roots_u, iters_u, info_u = ctx.solve_roots_newton(guesses)
        assert ctx.profile_read(reset=True).tile_tasks == 0
    print(f"Newton: iterations {iters} (omega-lane {iters_u}), |root - oracle| {np.abs(roots - r_or)}, "
          f"|root - partner| / |partner| {np.abs(roots - roots_u) / np.abs(roots_u)}")
    assert (info == 0).all() and (info_u == 0).all(), (info, info_u)
    assert np.array_equal(iters, iters_u)
    assert (np.abs(roots - roots_u) <= 1e-9 * np.abs(roots_u)).all()
    if hold_to_oracle:
        assert (np.abs(roots - r_or) <= TOL_W).all()


# ---- 6. routing --------------------------------------------------------------------------------------------------------
def _deriv_with(emme, d, ws, shapes, cache_gb=0.0, **opts):
    with _ctx(emme, d, shapes, node_cache_gb=cache_gb, wl_min=1, **opts) as ctx:
        ctx.profile(True)
        ctx.profile_read(reset=True)
        out = ctx.assemble_derivative(ws, want_intervals=True)
        return out, ctx.profile_read(reset=True).tile_tasks


def _same_bits(a, b):
    return np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fewer_than_three_switches_keep_the_omega_lane_kernel(emme, shape):
    make, ws4 = SHAPES[shape]
    d, ws = make(), ws4[:3]
    off, t_off = _deriv_with(emme, d, ws, emme.TILE_SHAPES_ES15, tile_uncached=0, deriv_cached=0)
    assert t_off == 0
    for tu, dc, sh in [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)]:
        got, t = _deriv_with(emme, d, ws, emme.TILE_SHAPES_ALL if sh else emme.TILE_SHAPES_ES15, tile_uncached=tu,
                             deriv_cached=dc)
        assert t == 0, (tu, dc, sh)
        assert _same_bits(off, got), (tu, dc, sh)
    # the triple: the tile fill, the same trees
    on, t_on = _deriv_with(emme, d, ws, emme.TILE_SHAPES_ALL, tile_uncached=1, deriv_cached=1)
    assert t_on > 0
    assert np.array_equal(on[2], off[2])


def test_routing_preconditions(emme):
    # a quadrature goal below the dense formulation's keeps the omega-lane kernel with the triple set
    d = example_stellarator(npoints=10, integration_accuracy=1e-12)
    off, t_off = _deriv_with(emme, d, WS_EM[:3], emme.TILE_SHAPES_ES15, tile_uncached=0, deriv_cached=0)
    on, t_on = _deriv_with(emme, d, WS_EM[:3], emme.TILE_SHAPES_ALL, tile_uncached=1, deriv_cached=1)
    assert t_off == 0 and t_on == 0
    assert _same_bits(off, on)
    # electrostatic GK15 with shapes ALL: still k_assemble_tile_deriv, the same bits as with shapes at their default
    d = example_tokamak(npoints=12)
    dflt, t_d = _deriv_with(emme, d, WS_ES[:3], emme.TILE_SHAPES_ES15, tile_uncached=1, deriv_cached=1)
    allsh, t_a = _deriv_with(emme, d, WS_ES[:3], emme.TILE_SHAPES_ALL, tile_uncached=1, deriv_cached=1)
    assert t_d > 0 and t_a == t_d
    assert _same_bits(dflt, allsh)


def test_serves_contexts_that_have_a_cache(emme, oracle):
    """No derivative request of these shapes reads a node cache: with the triple set, 17 omegas (one on the
    Re omega > 0 side) of a context WITH a cache go through the new kernel, both contour classes in one call."""
    d = example_stellarator(npoints=10)
    ws = np.concatenate([np.linspace(-1.8, -1.0, 16) + 1.5j, [0.4 + 0.3j]])
    with _ctx(emme, d, emme.TILE_SHAPES_ALL, node_cache_gb=8.0, tile_uncached=1, deriv_cached=1) as ctx:
        ctx.assemble(ws)  # (the plain fill builds and reads the cache)
        assert ctx.fill_kernel().startswith("k_assemble_dense")
        (M, Mp, iv), pr = _tile_deriv(ctx, ws)
        assert pr.matrices == 17
        u, _u2 = _partner(emme, ctx, ws, spread=False)
    _check_counts(oracle, oracle.params(d), ws, iv)
    _check_against_partner(d, ws, (M, Mp, iv), u, None)


# ---- 7. full size ------------------------------------------------------------------------------------------------------
def test_full_size_sample(emme, oracle):
    """npoints 1024, the reference's shipped stellarator size (dim 2048), one omega, against the omega-lane derivative
    fill on a second context (equal interval totals, M and M' within 1e-10) and, for M, the 32 oracle pairs x 3 moments
    of test_tile_shapes_full_size_sample."""
    N = 1024
    d = example_stellarator(npoints=N)
    w = -1.656 + 2.49j
    with _ctx(emme, d, emme.TILE_SHAPES_ALL, **OPTS) as ctx:
        (M, Mp, iv), _ = _tile_deriv(ctx, [w])
    with _ctx(emme, d, node_cache_gb=0.0, wl_min=1) as ctx:
        ctx.profile(True)
        ctx.profile_read(reset=True)
        u = ctx.assemble_derivative([w], want_intervals=True)
        assert ctx.profile_read(reset=True).tile_tasks == 0
    print("interval totals:", iv, u[2])
    assert np.array_equal(iv, u[2])
    em = np.abs(M[0] - u[0][0]).max() / np.abs(u[0][0]).max()
    ep = np.abs(Mp[0] - u[1][0]).max() / np.abs(u[1][0]).max()
    print(f"difference from the omega-lane derivative fill: M {em:.3e} of max|M|, M' {ep:.3e} of max|M'|")
    assert em <= TOL and ep <= TOL
    M = M[0]
    scale = np.abs(u[0][0]).max()
    po = oracle.params(d)
    eta, dx = oracle.grid(d["length"], N)
    worst = 0.0
    for s in range(32):
        off = 1 + (s * (N - 2)) // 31
        i = (s * 37) % (N - off)
        j = i + off
        k = [oracle.kappa(po, m, eta[i], eta[j], w)[0] + oracle.kappa_e(po, m, eta[i], eta[j], w) for m in range(3)]
        a = -k[0] * oracle.lib.oracle_weight(N, i, j) * dx
        bb, dd = k[1] * dx, k[2] * dx
        got_want = [(M[i, j], a), (M[j, i], a), (M[i, j + N], bb), (M[j, i + N], -bb), (M[i + N, j], -bb),
                    (M[j + N, i], bb), (M[i + N, j + N], dd), (M[j + N, i + N], dd)]
        worst = max(worst, max(abs(g - t) for g, t in got_want))
    print(f"32 sampled pairs (8 entries each) against the oracle, worst {worst / scale:.3e} of max|M|")
    assert worst <= TOL * scale
