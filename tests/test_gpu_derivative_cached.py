"""Exact dM/domega from the tiled node cache (option deriv_cached, k_assemble_dense_deriv).

The comparison partner for M' is the existing uncached derivative fill (deriv_cached = 0), which test_gpu_derivative.py
pins against central differences and the argument principle; M is also held to the oracle and to the plain cached fill.
Bars: 1e-10 max|.| per matrix (the project's bar for M: M' is the same sums over the same records with another B
operand); at the strongly damped omegas of cfg3_damped.npz, 10 x the uncached fill's own spread under omega (1 + 1e-13)
with that floor, the fixture's margin and floor."""
import os

import numpy as np
import pytest

from oracle.binding import example_stellarator, example_tokamak

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
TOL = 1e-10
ENUMERIC = -6
OMEGAS_ES = np.array([-0.8 + 0.25j, -0.792 + 0.2475j, 0.6 + 0.1j, -0.3 - 0.05j])
ELLIPSES = [(-0.80 + 0.25j, 0.25, 0.20), (-0.641 - 0.232j, 0.085, 0.05)]
MISSED_DAMPED = -0.6497855437578175 - 0.2619896194079743j
SPURIOUS = 0.04680305249320635 + 0.0035554167215062246j
NEAR_DOUBLE = -0.4561423236079871 - 0.1966192121085958j


def _ctx(emme, d, **options):
    return emme.Context(emme.params_from_dict(d), **options)


def _deriv_rc(ctx, omegas):
    """emme_assemble_derivative_batch with its return code instead of an exception: (rc, M, Mp, intervals)."""
    w = np.ascontiguousarray(np.atleast_1d(omegas), dtype=np.complex128)
    nb = w.shape[0]
    iv = np.zeros(nb, dtype=np.int64)
    M = np.zeros((nb, ctx.dim, ctx.dim), dtype=np.complex128)
    Mp = np.zeros_like(M)
    rc = ctx.lib.emme_assemble_derivative_batch(ctx.h, w.ctypes.data, nb, M.ctypes.data, Mp.ctypes.data, iv.ctypes.data)
    return rc, M, Mp, iv


def _both(ctx, omegas):
    """(cached, uncached) derivative fills of the same omegas on one context: (M, Mp, iv) each."""
    ctx.set_options(deriv_cached=1)
    c = ctx.assemble_derivative(omegas, want_intervals=True)
    ctx.set_options(deriv_cached=0)
    u = ctx.assemble_derivative(omegas, want_intervals=True)
    ctx.set_options(deriv_cached=1)
    return c, u


def _worst(A, B):
    """max over the batch of max|A_b - B_b| / max|B_b|"""
    return max(np.abs(A[b] - B[b]).max() / np.abs(B[b]).max() for b in range(len(B)))


def _ellipse_nodes(ell, N=64):
    c, a, b = ELLIPSES[ell]
    t = 2 * np.pi * np.arange(N) / N
    return c + a * np.cos(t) + 1j * b * np.sin(t), -a * np.sin(t) + 1j * b * np.cos(t)


@pytest.fixture(scope="module")
def lattice():
    import bench
    return bench.lattice(1, 0, 128)


@pytest.fixture(scope="module")
def ctx256(emme, lattice):
    """The default context of the headline workload with deriv_cached = 1, its cache settled on the lattice."""
    import bench
    ctx = emme.Context(emme.params_from_dict(bench.workload_dict(256)), device=0, deriv_cached=1)
    ctx.profile(True)
    ctx.cache_settle(lattice)
    yield ctx
    ctx.close()


# ---- 1. routing ----------------------------------------------------------------------------------------------------
def test_routing_follows_the_option(ctx256, lattice):
    assert ctx256.options().deriv_cached == 1
    state = ctx256.cache_state()
    mode = ctx256.fill_kernel()
    ctx256.profile_read(reset=True)
    ctx256.assemble_derivative(lattice)
    pr = ctx256.profile_read(reset=True)
    assert pr.tile_tasks > 0 and pr.dense_rounds + pr.sparse_rounds > 0 and pr.matrices == 128
    assert pr.deferred_launches >= 1
    assert ctx256.fill_kernel() == mode  # emme_ctx_fill_mode keeps naming the last plain fill
    assert ctx256.cache_state() == state  # (settled on these omegas)
    ctx256.set_options(deriv_cached=0)  # not a layout option: it changes on the live context
    try:
        ctx256.assemble_derivative(lattice)
        pr = ctx256.profile_read(reset=True)
        # (no tile task: the omega-lane kernel counts its own rounds in the first round counter)
        assert pr.tile_tasks == 0 and pr.sparse_rounds == 0 and pr.matrices == 128
        assert ctx256.cache_state() == state
    finally:
        ctx256.set_options(deriv_cached=1)


def test_option_is_range_checked(ctx256):
    with pytest.raises(Exception):
        ctx256.set_options(deriv_cached=2)
    assert ctx256.options().deriv_cached == 1


# ---- 2., 3., 4., 7. the lattice: same trees, M, M', determinism -------------------------------------------------------
def test_lattice_trees_m_and_mp(ctx256, lattice):
    (Mc, Mpc, ivc), (Mu, Mpu, ivu) = _both(ctx256, lattice)
    Mplain, ivp = ctx256.assemble(lattice, want_intervals=True)
    assert np.array_equal(ivc, ivu) and np.array_equal(ivc, ivp)
    em_plain, em_unc, emp = _worst(Mc, Mplain), _worst(Mc, Mu), _worst(Mpc, Mpu)
    print(f"lattice: M cached-deriv vs plain cached {em_plain:.3g}, vs uncached deriv {em_unc:.3g}; M' vs uncached {emp:.3g}")
    assert em_plain <= TOL and em_unc <= TOL
    assert emp <= TOL
    for b in range(len(lattice)):
        assert np.abs(Mc[b] - Mc[b].T).max() == 0.0 and np.abs(Mpc[b] - Mpc[b].T).max() == 0.0
        assert np.abs(np.diag(Mpc[b])).max() == 0.0
    # determinism on the settled context
    M2, Mp2, iv2 = ctx256.assemble_derivative(lattice, want_intervals=True)
    assert np.array_equal(iv2, ivc)
    assert np.array_equal(M2.view(np.float64), Mc.view(np.float64))
    assert np.array_equal(Mp2.view(np.float64), Mpc.view(np.float64))


@pytest.mark.parametrize("ell", range(len(ELLIPSES)))
def test_ellipse_nodes_mp_and_argument_principle(ctx256, ell):
    z, dz = _ellipse_nodes(ell)
    (Mc, Mpc, ivc), (Mu, Mpu, ivu) = _both(ctx256, z)
    assert np.array_equal(ivc, ivu)
    em, emp = _worst(Mc, Mu), _worst(Mpc, Mpu)
    print(f"ellipse {ell}: M {em:.3g}, M' {emp:.3g} of the bar's 1e-10")
    assert em <= TOL and emp <= TOL
    # test_argument_principle_from_mp_matches_the_winding, on the cached M'
    res = ctx256.find_roots_in_contour(ELLIPSES[ell][0], ELLIPSES[ell][1:])
    assert res["winding"] >= 0
    tr, info = ctx256.trace_solve(Mc, Mpc)
    assert (info == 0).all()
    count = np.sum(tr * dz) / (1j * len(z))
    assert abs(count - res["winding"]) < 0.02, (count, res["winding"])


# (4 omegas on 18 / 71 tiles: the planner's halving below dense_min_tasks leaves chunks of 2, all vector rounds;
# dense_min_tasks = 0 keeps them in one chunk, dense_min_cols = 1 / 17 sends every round to the matrix cores / the vector ALU)
ROUND_MIXES = {"planned": {}, "one-chunk": {"dense_min_tasks": 0}, "all-mfma": {"dense_min_tasks": 0, "dense_min_cols": 1},
               "all-vector": {"dense_min_tasks": 0, "dense_min_cols": 17}}


@pytest.mark.parametrize("mix", sorted(ROUND_MIXES))
def test_m_matches_the_oracle(emme, oracle, mix):
    for npoints in (24, 48):
        d = example_tokamak(npoints=npoints)
        with _ctx(emme, d, cache_min_batch=1, deriv_cached=1, **ROUND_MIXES[mix]) as ctx:
            ctx.profile(True)
            ctx.cache_settle(OMEGAS_ES)
            ctx.profile_read(reset=True)
            M, Mp, iv = ctx.assemble_derivative(OMEGAS_ES, want_intervals=True)
            pr = ctx.profile_read(reset=True)
            assert pr.tile_tasks > 0
            if mix == "all-mfma":
                assert pr.dense_rounds > 0 and pr.sparse_rounds == 0
            if mix == "all-vector":
                assert pr.dense_rounds == 0 and pr.sparse_rounds > 0
            ctx.set_options(deriv_cached=0)
            Mu, Mpu, ivu = ctx.assemble_derivative(OMEGAS_ES, want_intervals=True)
        po = oracle.params(d)
        assert np.array_equal(iv, ivu)
        for b, w in enumerate(OMEGAS_ES):
            Mo, tot = oracle.assemble(po, complex(w))
            assert np.abs(M[b] - Mo).max() <= TOL * np.abs(Mo).max(), (npoints, b)
            assert iv[b] == tot
            assert np.abs(Mp[b] - Mpu[b]).max() <= TOL * np.abs(Mpu[b]).max(), (npoints, b)


def test_mp_is_the_complex_derivative(emme):
    """test_gpu_derivative.py::test_mp_is_the_complex_derivative (es-gk15) with the cached M'."""
    with _ctx(emme, example_tokamak(npoints=24), cache_min_batch=1, deriv_cached=1) as ctx:
        ctx.profile(True)
        ctx.cache_settle(OMEGAS_ES)
        ctx.profile_read(reset=True)
        _, Mp, iv = ctx.assemble_derivative(OMEGAS_ES, want_intervals=True)
        assert ctx.profile_read(reset=True).tile_tasks > 0
        for b, w in enumerate(OMEGAS_ES):
            h = 1e-6 * abs(w)
            scale = np.abs(Mp[b]).max()
            for step in (h, 1j * h):
                M2, iv2 = ctx.assemble(np.array([w + step, w - step]), want_intervals=True)
                assert (iv2 == iv[b]).all(), (b, step, iv2, iv[b])
                fd = (M2[0] - M2[1]) / (2 * step)
                err = np.abs(fd - Mp[b]).max()
                assert err <= 1e-6 * scale, (b, step, err / scale)


# ---- 2., 5. the damped omegas of the reference's wandering chains -----------------------------------------------------------
def test_damped_omegas_trees_and_mp(emme):
    """The 35 finite omegas of cfg3_damped.npz on a context settled on them.  M entries there are remainders of values
    up to 1e16 larger, so M' is held to the comparison partner's own sensitivity: spread = max|M'_unc(w) -
    M'_unc(w (1 + 1e-13))|, bar 10 x spread with the floor 1e-10 max|M'|.  Omegas whose uncached derivative fill reports
    EMME_ENUMERIC (at most 5) are compared on the code only."""
    import bench
    z = np.load(os.path.join(G, "cfg3_damped.npz"))
    fin = z["nonfinite"] == 0
    ws, ref_iv = z["omegas"][fin], z["intervals"][fin]
    assert len(ws) == 35
    with _ctx(emme, bench.workload_dict(256), cache_min_batch=8, deriv_cached=1) as ctx:
        ctx.cache_settle(ws)
        Mplain, ivp = ctx.assemble(ws, want_intervals=True)
        assert np.array_equal(ivp, ref_iv)
        ctx.set_options(deriv_cached=0)
        lost = np.array([_deriv_rc(ctx, ws[k:k + 1])[0] == ENUMERIC for k in range(len(ws))])
        print(f"damped omegas: the uncached derivative fill loses {lost.sum()} of {len(ws)}: {ws[lost]}")
        assert lost.sum() <= 5
        keep = ws[~lost]
        rc_u, Mu, Mpu, ivu = _deriv_rc(ctx, keep)
        _, _, Mpu2, _ = _deriv_rc(ctx, keep * (1 + 1e-13))
        ctx.set_options(deriv_cached=1)
        rc_c, Mc, Mpc, ivc = _deriv_rc(ctx, keep)
        rc_lost = [_deriv_rc(ctx, w)[0] for w in ws[lost]]
    assert rc_u == 0 and rc_c == 0
    assert all(rc == ENUMERIC for rc in rc_lost), rc_lost
    assert np.array_equal(ivc, ivu) and np.array_equal(ivc, ref_iv[~lost])
    worst = worst_m = 0.0
    for k, w in enumerate(keep):
        spread = np.abs(Mpu[k] - Mpu2[k]).max()
        bar = max(10.0 * spread, TOL * np.abs(Mpu[k]).max())
        err = np.abs(Mpc[k] - Mpu[k]).max()
        worst = max(worst, err / bar)
        # M against the plain cached fill, at the fixture's margin for M
        kk = np.nonzero(fin)[0][np.nonzero(~lost)[0][k]]
        bar_m = max(10.0 * z["spread_max"][kk], TOL * z["maxabs"][kk])
        err_m = np.abs(Mc[k] - Mplain[np.nonzero(~lost)[0][k]]).max()
        worst_m = max(worst_m, err_m / bar_m)
        assert err <= bar, (w, err, bar, spread)
        assert err_m <= bar_m, (w, err_m, bar_m)
    print(f"damped omegas: worst M' error / bar = {worst:.3g}, worst M error / bar = {worst_m:.3g}")


# ---- 6. leaving the cache -------------------------------------------------------------------------------------------------
def _leave_the_cache(ctx, ws, damped=()):
    """The first cached derivative fill of a fresh context (it builds the cache itself) against the uncached one."""
    ctx.profile(True)
    ctx.profile_read(reset=True)
    c = ctx.assemble_derivative(ws, want_intervals=True)
    pr = ctx.profile_read(reset=True)
    assert pr.tile_tasks > 0 and pr.deferred_launches >= 1
    assert ctx.cache_state()[0] >= 0
    ctx.set_options(deriv_cached=0)
    u = ctx.assemble_derivative(ws, want_intervals=True)
    Mu2, Mpu2 = ctx.assemble_derivative(np.asarray(ws) * (1 + 1e-13))
    assert np.array_equal(c[2], u[2])
    for b, w in enumerate(ws):
        bar_m, bar_p = TOL * np.abs(u[0][b]).max(), TOL * np.abs(u[1][b]).max()
        if w in damped:  # the bar of the damped fixture: 10 x the partner's own spread, same floor
            bar_m = max(bar_m, 10.0 * np.abs(u[0][b] - Mu2[b]).max())
            bar_p = max(bar_p, 10.0 * np.abs(u[1][b] - Mpu2[b]).max())
        assert np.abs(c[0][b] - u[0][b]).max() <= bar_m, (w, np.abs(c[0][b] - u[0][b]).max(), bar_m)
        assert np.abs(c[1][b] - u[1][b]).max() <= bar_p, (w, np.abs(c[1][b] - u[1][b]).max(), bar_p)


def test_leaving_the_cache_shallow_cache(emme):
    ws = np.array([-0.8 + 0.25j, -0.6 - 0.21j, 0.5 + 0.1j, 0.153 - 0.316j])
    # (49 tiles x 8 KB per interval: 0.05 GB holds the shallowest shape only, the full tree to depth 3)
    with _ctx(emme, example_tokamak(npoints=40), node_cache_gb=0.05, cache_min_depth=1, wl_min=1, deriv_cached=1) as ctx:
        _leave_the_cache(ctx, ws)
        assert ctx.cache_state()[0] == 3


def test_leaving_the_cache_strongly_damped_omega(emme):
    damped = -0.142 - 1.469j
    ws = np.array([-0.8 + 0.25j, -0.6 - 0.21j, damped, 0.5 + 0.1j])
    with _ctx(emme, example_tokamak(npoints=40), node_cache_gb=8.0, wl_min=1, deriv_cached=1) as ctx:
        _leave_the_cache(ctx, ws, damped=(damped,))


def test_leaving_the_cache_poisoned_tiles(emme, lattice):
    """Re omega > 0 at N = 256: tiles of that contour class hold poisoned blocks, whose integrals go to the list kernel."""
    import bench
    ws = (-lattice.real + 1j * lattice.imag)[::4]
    with _ctx(emme, bench.workload_dict(256), node_cache_gb=24.0, deriv_cached=1) as ctx:
        _leave_the_cache(ctx, ws)


# ---- 8. Newton on the cache ---------------------------------------------------------------------------------------------
def _golden_roots():
    g = np.load(os.path.join(G, "cfg3_chains.npz"))
    r = g["roots"][g["converged"].astype(bool)]
    out = []
    for x in r:
        if all(abs(x - y) > 1e-7 * abs(x) for y in out):
            out.append(x)
    return np.array(out + [MISSED_DAMPED])


def test_newton_converges_to_the_reference_roots(ctx256):
    roots = np.array([x for x in _golden_roots() if abs(x - SPURIOUS) > 1e-6])
    guesses = roots * (1 + 1e-3)
    ctx256.profile_read(reset=True)
    r1, it1, info1 = ctx256.solve_roots_newton(guesses)
    assert ctx256.profile_read(reset=True).tile_tasks > 0  # the fills went through the cache
    assert (info1 == 0).all(), info1
    simple = np.abs(roots - NEAR_DOUBLE) > 1e-6
    assert simple.sum() == len(roots) - 1
    assert (it1[simple] <= 6).all(), it1
    assert (it1[~simple] <= 8).all(), it1
    assert np.abs(r1 - roots).max() <= 1e-9, np.abs(r1 - roots)
    v, vinfo = ctx256.null_vectors(nbatch=len(roots))
    assert (vinfo == 0).all()
    assert np.isfinite(ctx256.final_matrix(0)).all()


def test_newton_on_the_lattice_matches_the_uncached_search(ctx256, lattice):
    """deriv_cached = 0, the same from guess (1 + 1e-13), and deriv_cached = 1.  A chain is compared if it converges in
    both uncached runs to roots within 1e-9 relative (the uncached path's own sensitivity filter); every compared chain
    then has the same iteration count and a root within 1e-9 relative on the cache.  At least 100 chains must be
    compared (123 converge in profiles/r05_newton_vs_secant.txt)."""
    limit = ctx256.params.iteration_step_limit
    try:
        ctx256.set_options(deriv_cached=0)
        ra, ita, ia = ctx256.solve_roots_newton(lattice)
        rb, itb, ib = ctx256.solve_roots_newton(lattice * (1 + 1e-13))
        ctx256.set_options(deriv_cached=1)
        ctx256.profile_read(reset=True)
        rc, itc, ic = ctx256.solve_roots_newton(lattice)
        assert ctx256.profile_read(reset=True).tile_tasks > 0
    finally:
        ctx256.set_options(deriv_cached=1)
    conv_a, conv_b = (ia == 0) & (ita <= limit), (ib == 0) & (itb <= limit)
    with np.errstate(invalid="ignore"):
        cmp_ = conv_a & conv_b & (np.abs(ra - rb) <= 1e-9 * np.abs(ra))
    print(f"lattice Newton: converged {conv_a.sum()} / {conv_b.sum()} uncached, compared {cmp_.sum()}, "
          f"converged on the cache {((ic == 0) & (itc <= limit)).sum()}")
    assert cmp_.sum() >= 100
    assert (ic[cmp_] == 0).all()
    assert np.array_equal(itc[cmp_], ita[cmp_]), np.nonzero(cmp_ & (itc != ita))[0]
    assert (np.abs(rc[cmp_] - ra[cmp_]) <= 1e-9 * np.abs(ra[cmp_])).all()


# ---- 9. fallbacks unchanged ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["es-gk31", "em-gk31"])
def test_other_contexts_keep_the_uncached_kernels_bit_for_bit(emme, case):
    mk, omegas, opt = {
        "es-gk31": (lambda: example_tokamak(npoints=32, integration_start_points=31), OMEGAS_ES, {}),
        "em-gk31": (lambda: example_stellarator(npoints=24), np.array([-1.656 + 2.49j, -0.9 + 0.4j]), {"wl_min": 2}),
    }[case]
    out = []
    for flag in (0, 1):
        with _ctx(emme, mk(), deriv_cached=flag, **opt) as ctx:
            ctx.assemble(omegas)  # (the context has a node cache)
            state = ctx.cache_state()
            out.append(ctx.assemble_derivative(omegas, want_intervals=True))
            assert ctx.cache_state() == state
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(np.ascontiguousarray(a).view(np.float64) if a.dtype == np.complex128 else a,
                              np.ascontiguousarray(b).view(np.float64) if b.dtype == np.complex128 else b)


def test_no_cache_budget_keeps_the_uncached_kernels_bit_for_bit(emme):
    d = example_tokamak(npoints=24)
    out = []
    for flag in (0, 1):
        with _ctx(emme, d, node_cache_gb=0.0, deriv_cached=flag) as ctx:
            out.append(ctx.assemble_derivative(OMEGAS_ES, want_intervals=True))
    assert np.array_equal(out[0][0].view(np.float64), out[1][0].view(np.float64))
    assert np.array_equal(out[0][1].view(np.float64), out[1][1].view(np.float64))
    assert np.array_equal(out[0][2], out[1][2])
