"""The table-free tile fill for electromagnetic and GK31 contexts (k_assemble_tile_shape<PTS, NM>, switched on by
emme_ctx_set_tile_shapes(EMME_TILE_SHAPES_ALL) beside the option tile_uncached) against the CPU oracle.

Bars: the project's own, as tests/test_gpu_tile_fill.py states them -- matrix entries 1e-10 * max|M|, roots 1e-9,
interval counts equal to the oracle's item by item.  At a strongly damped omega (entries that are remainders of integrand
values many orders larger) the bar is the larger of the entry bar and ten times the ORACLE's own change under
omega (1 + 1e-13), computed here from the oracle, never from the code under test.
"""
import numpy as np
import pytest

from oracle.binding import example_stellarator, example_tokamak

pytestmark = pytest.mark.gpu

TOL_M = 1e-10
TOL_W = 1e-9
TILE = dict(node_cache_gb=0.0, wl_min=1, tile_uncached=1)
W_DAMPED = -0.142 - 1.469j
WS_EM = [-1.656 + 2.49j, -0.85 - 0.32j, 0.4 - 0.2j, W_DAMPED]
WS_ES = [-0.8 + 0.25j, -0.6 - 0.21j, 0.5 + 0.1j, W_DAMPED]


def _ctx(emme, d, shapes=None, **options):
    ctx = emme.Context(emme.params_from_dict(d), **options)
    if shapes is not None:
        ctx.set_tile_shapes(shapes)
    return ctx


def _symbol(d):
    return "k_assemble_tile_shape<%d, %d>" % (d["integration_start_points"], 3 if d["beta_e"] != 0.0 else 1)


def _assert_tile_shape(ctx, d):
    assert ctx.fill_kernel().startswith("k_assemble_tile"), ctx.fill_kernel()
    assert ctx.fill_kernel_symbol() == _symbol(d), ctx.fill_kernel_symbol()


def _ntiles(n):
    return (n * (n - 1) // 2 + 15) // 16


def _check_against_oracle(oracle, po, ws, M, iv, sensitive=()):
    """entries and interval totals item by item; omegas in `sensitive` get the oracle-sensitivity bar"""
    for k, w in enumerate(ws):
        w = complex(w)
        Mo, tot = oracle.assemble(po, w)
        scale = np.abs(Mo).max()
        bar, which = TOL_M * scale, "TOL_M"
        if w in sensitive:
            Mo2, _ = oracle.assemble(po, w * (1 + 1e-13))
            sens = 10 * np.abs(Mo - Mo2).max()
            if sens > bar:
                bar, which = sens, "oracle sensitivity"
        err = np.abs(M[k] - Mo).max()
        print(f"omega {w}: intervals {iv[k]} (oracle {tot}), error {err / scale:.3e} of max|M|, bar {bar / scale:.3e} ({which})")
        assert iv[k] == tot, (w, iv[k], tot)
        assert err <= bar, (w, err / scale, bar / scale, which)


def _check_blocks(d, M):
    """include/solver.h:461-511: A and D symmetric, B antisymmetric, C = -B (electromagnetic); M symmetric (electrostatic)"""
    N = d["npoints"]
    for Mk in M:
        if d["beta_e"] == 0.0:
            assert np.array_equal(Mk, Mk.T)
            continue
        A, B, C, D = Mk[:N, :N], Mk[:N, N:], Mk[N:, :N], Mk[N:, N:]
        assert np.array_equal(A, A.T) and np.array_equal(D, D.T)
        assert np.array_equal(C, -B) and np.array_equal(B, -B.T)


SHAPES = {
    "em31": (lambda: example_stellarator(npoints=10), WS_EM),
    "em15": (lambda: example_stellarator(npoints=10, integration_start_points=15), WS_EM),
    "es31": (lambda: example_tokamak(npoints=12, integration_start_points=31), WS_ES),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_tile_shapes_match_oracle(emme, oracle, shape):
    """Both contour classes in one call.  Tasks: the three omegas of Re omega < 0 and the one of Re omega > 0 are far
    fewer tasks than dense_min_tasks, so the planner halves the chunk capacity to 2 (from 5 for the electromagnetic
    shapes, from 16 for the electrostatic one): 2 + 1 chunks, times 3 tiles (npoints 10: 45 pairs) or 5 (npoints 12: 66)."""
    make, ws = SHAPES[shape]
    d = make()
    with _ctx(emme, d, emme.TILE_SHAPES_ALL, **TILE) as ctx:
        assert ctx.tile_shapes() == emme.TILE_SHAPES_ALL
        ctx.profile(True)
        M, iv = ctx.assemble(ws, want_intervals=True)
        _assert_tile_shape(ctx, d)
        pr = ctx.profile_read(reset=True)
        assert pr.tile_tasks == 3 * _ntiles(d["npoints"]) and pr.dense_rounds > 0 and pr.matrices == 4
        M1, iv1 = ctx.assemble(ws[1:2], want_intervals=True)
        _assert_tile_shape(ctx, d)
    _check_against_oracle(oracle, oracle.params(d), ws, M, iv, sensitive=(W_DAMPED,))
    _check_blocks(d, M)
    assert iv1[0] == iv[1]
    assert np.abs(M1[0] - M[1]).max() <= 1e-13 * np.abs(M[1]).max()


def _batch15():
    rng = np.random.default_rng(3)
    return np.concatenate([rng.uniform(-1.2, -0.4, 13) + 1j * rng.uniform(0.05, 0.4, 13), [0.6 + 0.1j, 0.153 - 0.316j]])


def test_tile_shapes_several_chunks_and_repeatability(emme, oracle):
    """Stellarator npoints 8 (28 pairs, 2 tiles): 13 omegas of Re omega < 0 are more than one chunk of 5; two fills of
    the batch give the same bits."""
    d = example_stellarator(npoints=8)
    ws = _batch15()
    with _ctx(emme, d, emme.TILE_SHAPES_ALL, **TILE) as ctx:
        ctx.profile(True)
        M, iv = ctx.assemble(ws, want_intervals=True)
        _assert_tile_shape(ctx, d)
        pr = ctx.profile_read(reset=True)
        M2, iv2 = ctx.assemble(ws, want_intervals=True)
    ntiles = _ntiles(8)
    assert pr.tile_tasks > 2 * ntiles and pr.tile_tasks % ntiles == 0
    _check_against_oracle(oracle, oracle.params(d), ws, M, iv)
    _check_blocks(d, M)
    assert np.array_equal(iv, iv2)
    assert np.array_equal(M.view(np.float64), M2.view(np.float64))


GRIDS = [("em31", n) for n in (2, 3, 6, 7, 17)] + [("em15", n) for n in (2, 3, 6, 7, 17)] + [("es31", n) for n in (2, 5, 17)]


@pytest.mark.parametrize("shape,n", GRIDS, ids=[f"{s}-{n}" for s, n in GRIDS])
def test_tile_shapes_small_and_odd_grids(emme, oracle, shape, n):
    """One pair (three integrals), fewer than 16 pairs, 15 pairs (one partial tile), two tiles, nine tiles (the last
    workgroup with one wave at work on a tile of 8 pairs); one omega and three."""
    make, ws4 = SHAPES[shape]
    d = dict(make(), npoints=n)
    po = oracle.params(d)
    with _ctx(emme, d, emme.TILE_SHAPES_ALL, **TILE) as ctx:
        for ws in (ws4[:1], [ws4[0], ws4[2], ws4[1]]):
            M, iv = ctx.assemble(ws, want_intervals=True)
            _assert_tile_shape(ctx, d)
            _check_against_oracle(oracle, po, ws, M, iv)
            _check_blocks(d, M)


# Inputs whose trees hold more than 64 intervals on one bisection level (found on the CPU with the oracle's interval
# trace): (parameters, the wide omega, two ordinary omegas).  GK15 electromagnetic: the stellarator has an integral with
# 86 intervals on one level at this omega, the electromagnetic tokamak one with 114.  GK31: with the inputs' own
# tolerances no level exceeds 30 entries; with integration_precision 1e-9 every integral overflows at -0.005-2j (widest
# levels 84 .. 98).
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
def test_tile_shapes_hand_over_full_level_lists(emme, oracle, case, how):
    """An integral whose split does not fit the next 64-entry level list goes, whole, to the tile fill's work list; the
    other columns of its chunk go on in the tile kernel."""
    make, wide, ordinary = HAND_OVER[case]
    d = make()
    ws = [wide] if how == "alone" else [ordinary[0], wide, ordinary[1]]
    po = oracle.params(d)
    n = d["npoints"]
    nint = n * (n - 1) // 2 * (3 if d["beta_e"] != 0.0 else 1)  # integrals of one omega
    with _ctx(emme, d, emme.TILE_SHAPES_ALL, **TILE) as ctx:
        ctx.profile(True)
        M, iv = ctx.assemble(ws, want_intervals=True)
        _assert_tile_shape(ctx, d)
        handed = ctx.last_deferred()
        pr = ctx.profile_read(reset=True)
    print(f"handed over: {handed} integrals of {nint}; deferred launches {pr.deferred_launches}")
    assert pr.deferred_launches > 0
    assert 0 < handed <= nint  # nothing handed over = the test shows nothing
    _check_against_oracle(oracle, po, ws, M, iv, sensitive=(wide,))


def test_root_search_through_the_tile_shapes(emme, oracle):
    """The fused secant through the electromagnetic epilogue: guesses around the shipped one and one of Re omega > 0."""
    d = example_stellarator(npoints=16)
    po = oracle.params(d)
    guesses = np.array([-1.656 + 2.49j, -1.6 + 2.4j, -1.7 + 2.55j, 0.4 + 0.3j])
    with _ctx(emme, d, emme.TILE_SHAPES_ALL, **TILE) as ctx:
        roots, iters, info = ctx.solve_roots(guesses)
        _assert_tile_shape(ctx, d)
    for b in (0, 1):
        r_or, its_or, _, _ = oracle.solve_root(po, complex(guesses[b]))
        print(f"chain {b}: {iters[b]} steps (oracle {len(its_or)}), |root - oracle| {abs(roots[b] - r_or):.3e}")
        assert iters[b] == len(its_or) and abs(roots[b] - r_or) <= TOL_W


def test_tile_shapes_routing(emme, oracle):
    # shapes at their default: the omega-lane kernel on all three shapes
    for shape in sorted(SHAPES):
        make, ws = SHAPES[shape]
        d = make()
        with _ctx(emme, d, **TILE) as ctx:
            assert ctx.tile_shapes() == emme.TILE_SHAPES_ES15
            ctx.assemble(ws[:3])
            assert ctx.fill_kernel().startswith("k_assemble_wl"), shape
    # a quadrature goal below the dense formulation's keeps the omega-lane kernel with shapes ALL
    d = example_stellarator(npoints=10, integration_accuracy=1e-12)
    with _ctx(emme, d, emme.TILE_SHAPES_ALL, **TILE) as ctx:
        M, iv = ctx.assemble(WS_EM[:3], want_intervals=True)
        assert ctx.fill_kernel().startswith("k_assemble_wl")
    _check_against_oracle(oracle, oracle.params(d), WS_EM[:3], M, iv)
    d = example_stellarator(npoints=10)
    po = oracle.params(d)
    ws = WS_EM[:3]
    with _ctx(emme, d, emme.TILE_SHAPES_ALL, **TILE) as ctx:
        M0, iv0 = ctx.assemble(ws, want_intervals=True)
        _assert_tile_shape(ctx, d)
        ctx.profile(True)
        assert ctx.profile_read(reset=True).tile_tasks > 0
        # a derivative fill does not run the tile kernel
        M, Mp, iv = ctx.assemble_derivative(ws, want_intervals=True)
        pr = ctx.profile_read(reset=True)
        assert pr.tile_tasks == 0
        _check_against_oracle(oracle, po, ws, M, iv)
        # ... and its M' is the derivative: central differences of the oracle's matrix (h = 1e-6: truncation ~1e-12,
        # rounding ~1e-10 of the entries; the bar is tests/test_gpu_tile_fill.py's for the same check)
        h = 1e-6
        Mh, _ = oracle.assemble(po, complex(ws[0]) + h)
        Ml, _ = oracle.assemble(po, complex(ws[0]) - h)
        assert np.abs(Mp[0] - (Mh - Ml) / (2 * h)).max() <= 1e-6 * np.abs(Mp[0]).max()
        # not a layout setting: back to ES15 on the live context, the omega-lane kernel again
        ctx.set_tile_shapes(emme.TILE_SHAPES_ES15)
        assert ctx.tile_shapes() == emme.TILE_SHAPES_ES15
        M, iv = ctx.assemble(ws, want_intervals=True)
        assert ctx.fill_kernel().startswith("k_assemble_wl")
        assert ctx.last_deferred() == 0
        _check_against_oracle(oracle, po, ws, M, iv)
        for bad in (2, -1):
            with pytest.raises(emme.EmmeError):
                ctx.set_tile_shapes(bad)
        assert ctx.tile_shapes() == emme.TILE_SHAPES_ES15
    # no effect while tile_uncached = 0
    with _ctx(emme, d, emme.TILE_SHAPES_ALL, node_cache_gb=0.0, wl_min=1) as ctx:
        ctx.assemble(ws)
        assert ctx.fill_kernel().startswith("k_assemble_wl")
    # electrostatic GK15 with shapes ALL: still k_assemble_tile, the same bits as with shapes at their default
    d = example_tokamak(npoints=12)
    with _ctx(emme, d, **TILE) as ctx:
        Md = ctx.assemble(WS_ES[:3])
        assert ctx.fill_kernel_symbol() == "k_assemble_tile"
    with _ctx(emme, d, emme.TILE_SHAPES_ALL, **TILE) as ctx:
        Ma = ctx.assemble(WS_ES[:3])
        assert ctx.fill_kernel_symbol() == "k_assemble_tile"
    assert np.array_equal(Md.view(np.float64), Ma.view(np.float64))


def test_tile_shapes_serve_the_minority_class_of_a_cached_call(emme, oracle):
    """17 omegas, one of them on the Re omega > 0 side: the majority goes through the node cache, the minority pass
    through the tile fill; the call's fill kernel, as reported, stays the majority's."""
    d = example_stellarator(npoints=10)
    ws = np.concatenate([np.linspace(-1.8, -1.0, 16) + 1.5j, [0.4 + 0.3j]])
    with _ctx(emme, d, emme.TILE_SHAPES_ALL, node_cache_gb=8.0, tile_uncached=1) as ctx:
        ctx.profile(True)
        M, iv = ctx.assemble(ws, want_intervals=True)
        assert ctx.fill_kernel().startswith("k_assemble_dense")
        pr = ctx.profile_read(reset=True)
    assert pr.deferred_launches >= 2  # the cached fill's list and the tile fill's
    _check_against_oracle(oracle, oracle.params(d), ws, M, iv)


def test_tile_shapes_full_size_sample(emme, oracle):
    """npoints 1024, the reference's shipped stellarator size (dim 2048), one omega.  The oracle's whole matrix at this
    size takes minutes, so the partner is the omega-lane kernel on a second context (entries within TOL_M, the same
    interval total); the oracle is asked for 32 single pairs spread over |i - j|, all three moments, assembled into the
    A / B / D entries as the epilogue does (include/solver.h:472-509)."""
    N = 1024
    d = example_stellarator(npoints=N)
    w = -1.656 + 2.49j
    with _ctx(emme, d, emme.TILE_SHAPES_ALL, **TILE) as ctx:
        M, iv = ctx.assemble([w], want_intervals=True)
        _assert_tile_shape(ctx, d)
    with _ctx(emme, d, node_cache_gb=0.0, wl_min=1) as ctx:
        Mw, ivw = ctx.assemble([w], want_intervals=True)
        assert ctx.fill_kernel().startswith("k_assemble_wl")
    print("interval totals:", iv, ivw)
    assert np.array_equal(iv, ivw)
    M, Mw = M[0], Mw[0]
    scale = np.abs(Mw).max()
    err = np.abs(M - Mw).max() / scale
    print(f"max entry difference from the omega-lane fill {err:.3e} of max|M|")
    assert err <= TOL_M
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
    assert worst <= TOL_M * scale
