"""The table-free tile fill (option tile_uncached, k_assemble_tile) against the CPU oracle: a batch
without a node cache builds the dense fill's two GEMM operands in LDS and runs on the FP64 matrix cores.

Bars: the project's own -- matrix entries 1e-10 * max|M|, roots 1e-9, interval counts equal to the oracle's item by
item (the quadrature trees are the reference's; what differs is the order of the node sums and the safe_exp clamp,
<= 4e-14 absolute, assemble_dense.hip).
"""
import numpy as np
import pytest

from oracle.binding import example_stellarator, example_tokamak

pytestmark = pytest.mark.gpu

TOL_M = 1e-10
TOL_W = 1e-9
TILE = dict(node_cache_gb=0.0, wl_min=1, tile_uncached=1)
# a strongly damped point whose integrals hold more than 64 intervals on one bisection level (on this
# geometry 112 of one integral's 565 at npoints = 2 already: tests/analysis/level_width.py's count, taken with the oracle)
W_WIDE = -0.00552674 - 0.73419159j


def _ctx(emme, d, **options):
    return emme.Context(emme.params_from_dict(d), **options)


def _is_tile(ctx):
    return ctx.fill_kernel().startswith("k_assemble_tile")


def _check_against_oracle(oracle, po, ws, M, iv, loose=()):
    for k, w in enumerate(ws):
        Mo, tot = oracle.assemble(po, complex(w))
        err = np.abs(M[k] - Mo).max() / np.abs(Mo).max()
        print(f"omega {complex(w)}: intervals {iv[k]} (oracle {tot}), max entry error {err:.3e} of max|M|")
        assert iv[k] == tot, (w, iv[k], tot)
        assert err <= (1e-6 if complex(w) in loose else TOL_M), (w, err)


def test_tile_fill_matches_oracle(emme, oracle):
    """npoints 40: 780 pairs, the last tile is partial; both contour classes in one call: two partial chunks."""
    d = example_tokamak(npoints=40)
    ws = [-0.8 + 0.25j, -0.6 - 0.21j, 0.5 + 0.1j, -0.142 - 1.469j, 0.153 - 0.316j]
    with _ctx(emme, d, **TILE) as ctx:
        assert ctx.options().tile_uncached == 1
        ctx.profile(True)
        M, iv = ctx.assemble(ws, want_intervals=True)
        assert _is_tile(ctx), ctx.fill_kernel()
        assert ctx.fill_kernel_symbol() == "k_assemble_tile"
        pr = ctx.profile_read(reset=True)
        # 49 tiles; 3 + 2 omegas per class are few tasks, so the planner halves the chunks down to 2: 2 + 1 chunks
        assert pr.tile_tasks == 3 * 49 and pr.dense_rounds > 0 and pr.matrices == 5
        M1, iv1 = ctx.assemble(ws[1:2], want_intervals=True)
        assert _is_tile(ctx)
    # (-0.142-1.469j) is a strongly damped point: entries are ~1e38 and each is the remainder of integrand values
    # ~1e8 times larger, so BOTH implementations carry ~1e-8 relative rounding there (test_every_fill_kernel_matches_oracle)
    _check_against_oracle(oracle, oracle.params(d), ws, M, iv, loose=(-0.142 - 1.469j,))
    assert iv1[0] == iv[1]
    assert np.abs(M1[0] - M[1]).max() <= 1e-13 * np.abs(M[1]).max()


def _batch22():
    rng = np.random.default_rng(3)
    return np.concatenate([rng.uniform(-1.2, -0.4, 20) + 1j * rng.uniform(0.05, 0.4, 20), [0.6 + 0.1j, 0.153 - 0.316j]])


@pytest.fixture(scope="module")
def batch22_fills(emme):
    """Two fills of the 22-omega batch on one context (npoints 24: 18 tiles, so the task minimum halves the chunks)."""
    d = example_tokamak(npoints=24)
    with _ctx(emme, d, **TILE) as ctx:
        ctx.profile(True)
        first = ctx.assemble(_batch22(), want_intervals=True)
        tile = _is_tile(ctx)
        pr = ctx.profile_read(reset=True)
        second = ctx.assemble(_batch22(), want_intervals=True)
    return d, first, second, tile, pr


def test_tile_fill_several_chunks_per_class(emme, oracle, batch22_fills):
    d, (M, iv), _, tile, pr = batch22_fills
    assert tile
    ntiles = (24 * 23 // 2 + 15) // 16
    assert pr.tile_tasks > 2 * ntiles and pr.tile_tasks % ntiles == 0  # more than one chunk for the 20 of Re omega < 0
    _check_against_oracle(oracle, oracle.params(d), _batch22(), M, iv)


def test_tile_fill_is_repeatable(batch22_fills):
    _, (M, iv), (M2, iv2), _, _ = batch22_fills
    assert np.array_equal(iv, iv2)
    assert np.array_equal(M.view(np.float64), M2.view(np.float64))


@pytest.mark.parametrize("n", [2, 3, 5, 17])
def test_tile_fill_small_and_odd_grids(emme, oracle, n):
    """One pair, fewer than 16 pairs, and (17: 136 pairs) nine tiles -- three workgroups, the last with one wave at work
    on a tile of 8 pairs."""
    d = example_tokamak(npoints=n)
    po = oracle.params(d)
    with _ctx(emme, d, **TILE) as ctx:
        for ws in ([-0.8 + 0.25j], [-0.8 + 0.25j, 0.5 + 0.1j, -0.6 - 0.21j]):
            M, iv = ctx.assemble(ws, want_intervals=True)
            assert _is_tile(ctx)
            _check_against_oracle(oracle, po, ws, M, iv)


@pytest.mark.parametrize("ws", [[W_WIDE], [-0.8 + 0.25j, W_WIDE, -0.6 - 0.21j]], ids=["alone", "in-a-chunk"])
def test_tile_fill_hands_over_full_level_lists(emme, oracle, ws):
    """npoints 5 (10 pairs, one tile): every integral of W_WIDE outgrows the 64-entry level list and goes, whole, to the
    work list; the other columns of its chunk go on in the tile kernel."""
    d = example_tokamak(npoints=5)
    po = oracle.params(d)
    with _ctx(emme, d, **TILE) as ctx:
        ctx.profile(True)
        M, iv = ctx.assemble(ws, want_intervals=True)
        assert _is_tile(ctx)
        handed = ctx.last_deferred()
        pr = ctx.profile_read(reset=True)
    print(f"handed over: {handed} integrals; deferred launches {pr.deferred_launches}")
    assert pr.deferred_launches > 0
    assert 0 < handed <= 10  # nothing handed over = the test shows nothing
    for k, w in enumerate(ws):
        Mo, tot = oracle.assemble(po, complex(w))
        assert iv[k] == tot, (w, iv[k], tot)
        scale = np.abs(Mo).max()
        bar, which = TOL_M * scale, "TOL_M"
        if complex(w) == W_WIDE:
            # the oracle's own sensitivity to the last bits of omega, where that is larger
            Mo2, _ = oracle.assemble(po, complex(w) * (1 + 1e-13))
            sens = 10 * np.abs(Mo - Mo2).max()
            if sens > bar:
                bar, which = sens, "oracle sensitivity"
        err = np.abs(M[k] - Mo).max()
        print(f"omega {complex(w)}: error {err / scale:.3e} of max|M|, bar {bar / scale:.3e} ({which})")
        assert err <= bar, (w, err / scale, bar / scale, which)


def test_root_search_through_the_tile_fill(emme, oracle):
    """The guesses and checks of test_root_search_same_in_every_kernel_mode: the fused secant through the new epilogue."""
    d = example_tokamak(npoints=32)
    po = oracle.params(d)
    guesses = np.array([-0.8 + 0.25j, -0.7 + 0.3j, -0.9 + 0.2j, -0.5 + 0.1j, 0.6 + 0.2j])
    with _ctx(emme, d, **TILE) as ctx:
        roots, iters, info = ctx.solve_roots(guesses)
        assert _is_tile(ctx), ctx.fill_kernel()
    for b in (0, 3):
        r_or, its_or, _, _ = oracle.solve_root(po, complex(guesses[b]))
        print(f"chain {b}: {iters[b]} steps (oracle {len(its_or)}), |root - oracle| {abs(roots[b] - r_or):.3e}")
        assert iters[b] == len(its_or) and abs(roots[b] - r_or) <= TOL_W


def test_what_the_tile_fill_does_not_serve_keeps_its_kernel(emme, oracle):
    ws = [-0.8 + 0.25j, -0.6 - 0.21j, 0.5 + 0.1j]
    # electromagnetic
    d = example_stellarator(npoints=10)
    wem = [-1.656 + 2.49j, -0.85 - 0.32j, 0.4 - 0.2j]
    with _ctx(emme, d, **TILE) as ctx:
        M, iv = ctx.assemble(wem, want_intervals=True)
        assert ctx.fill_kernel().startswith("k_assemble_wl")
    _check_against_oracle(oracle, oracle.params(d), wem, M, iv)
    # GK31, and a quadrature goal below the dense formulation's
    for over in (dict(integration_start_points=31), dict(integration_accuracy=1e-12)):
        d = example_tokamak(npoints=12, **over)
        with _ctx(emme, d, **TILE) as ctx:
            M, iv = ctx.assemble(ws, want_intervals=True)
            assert ctx.fill_kernel().startswith("k_assemble_wl"), over
        _check_against_oracle(oracle, oracle.params(d), ws, M, iv)
    d = example_tokamak(npoints=12)
    po = oracle.params(d)
    with _ctx(emme, d, **TILE) as ctx:
        # a derivative fill: the omega-lane derivative kernel; the fill mode keeps naming the last plain fill
        M0, iv0 = ctx.assemble(ws, want_intervals=True)
        assert _is_tile(ctx)
        ctx.profile(True)
        assert ctx.profile_read(reset=True).tile_tasks > 0
        M, Mp, iv = ctx.assemble_derivative(ws, want_intervals=True)
        pr = ctx.profile_read(reset=True)
        assert pr.tile_tasks == 0 and pr.deferred_launches == 0  # not the tile kernel
        _check_against_oracle(oracle, po, ws, M, iv)
        h = 1e-6
        Mh, _ = oracle.assemble(po, complex(ws[0]) + h)
        Ml, _ = oracle.assemble(po, complex(ws[0]) - h)
        assert np.abs(Mp[0] - (Mh - Ml) / (2 * h)).max() <= 1e-6 * np.abs(Mp[0]).max()
        # not a layout option: off on the live context, the omega-lane kernel again
        ctx.set_options(tile_uncached=0)
        M, iv = ctx.assemble(ws, want_intervals=True)
        assert ctx.fill_kernel().startswith("k_assemble_wl")
        assert ctx.last_deferred() == 0
        _check_against_oracle(oracle, po, ws, M, iv)
        with pytest.raises(Exception):
            ctx.set_options(tile_uncached=2)
    with _ctx(emme, d, node_cache_gb=0.0, wl_min=1) as ctx:
        ctx.assemble(ws)
        assert ctx.fill_kernel().startswith("k_assemble_wl")


def test_tile_fill_serves_the_minority_class_of_a_cached_call(emme, oracle):
    """17 omegas, one of them on the Re omega > 0 side: the majority goes through the node cache, the minority pass
    (force_uncached) through the tile fill; the call's fill kernel, as reported, stays the majority's."""
    d = example_tokamak(npoints=12)
    ws = np.concatenate([np.linspace(-1.0, -0.5, 16) + 0.2j, [0.5 + 0.1j]])
    with _ctx(emme, d, node_cache_gb=8.0, tile_uncached=1) as ctx:
        ctx.profile(True)
        M, iv = ctx.assemble(ws, want_intervals=True)
        assert ctx.fill_kernel().startswith("k_assemble_dense")
        pr = ctx.profile_read(reset=True)
    assert pr.deferred_launches >= 2  # the cached fill's list and the tile fill's
    _check_against_oracle(oracle, oracle.params(d), ws, M, iv)


def test_tile_fill_full_size_sample(emme, oracle):
    """npoints 1024, the size of the reference's example inputs, 2 omegas.  The oracle's whole matrix at this size
    takes minutes, so the partner is the omega-lane kernel on a second context (entries within TOL_M, the same
    per-matrix interval totals: the device reports totals, not per-pair counts); the oracle is asked for 64 single
    pairs spread over |i - j|, whose entries are M_ij = -kappa W_ij dx."""
    d = example_tokamak(npoints=1024)
    ws = [-0.8 + 0.25j, -0.6 - 0.21j]
    with _ctx(emme, d, **TILE) as ctx:
        M, iv = ctx.assemble(ws, want_intervals=True)
        assert _is_tile(ctx)
    with _ctx(emme, d, node_cache_gb=0.0, wl_min=1) as ctx:
        Mw, ivw = ctx.assemble(ws, want_intervals=True)
        assert ctx.fill_kernel().startswith("k_assemble_wl")
    print("interval totals:", iv, ivw)
    assert np.array_equal(iv, ivw)
    for k in range(2):
        scale = np.abs(Mw[k]).max()
        err = np.abs(M[k] - Mw[k]).max() / scale
        print(f"omega {ws[k]}: max entry difference from the omega-lane fill {err:.3e} of max|M|")
        assert err <= TOL_M
    po = oracle.params(d)
    eta, dx = oracle.grid(d["length"], 1024)
    W = lambda i, j: oracle.lib.oracle_weight(1024, i, j)
    for k, w in enumerate(ws):
        scale = np.abs(Mw[k]).max()
        worst = 0.0
        for s in range(64):
            off = 1 + (s * 1022) // 63
            i = (s * 37) % (1024 - off)
            kap, _ = oracle.kappa(po, 0, eta[i], eta[i + off], complex(w))
            want = -kap * W(i, i + off) * dx
            worst = max(worst, abs(M[k][i, i + off] - want), abs(M[k][i + off, i] - want))
        print(f"omega {w}: 64 sampled entries against the oracle, worst {worst / scale:.3e} of max|M|")
        assert worst <= TOL_M * scale
