"""Exact dM/domega beside M (emme_assemble_derivative_batch) and the true Newton search (emme_solve_roots_newton),
DESIGN.md §12: M unchanged bit for bit, M' against central differences in both directions of the omega plane, the
argument principle from tr(M^-1 M') against the region search's winding, and Newton onto the reference's roots."""
import os

import numpy as np
import pytest

from oracle.binding import example_stellarator, example_tokamak

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_CFG3 = os.path.join(ROOT, "tests", "golden", "cfg3_chains.npz")
MISSED_DAMPED = -0.6497855437578175 - 0.2619896194079743j

OMEGAS_ES = np.array([-0.8 + 0.25j, -0.792 + 0.2475j, 0.6 + 0.1j, -0.3 - 0.05j])
CASES = {
    "es-gk15": (lambda: example_tokamak(npoints=24), OMEGAS_ES, {}),
    "es-gk31": (lambda: example_tokamak(npoints=32, integration_start_points=31), OMEGAS_ES, {}),
    # (wl_min = 2: a batch of two goes through the omega-lane kernel)
    "em-gk31": (lambda: example_stellarator(npoints=24), np.array([-1.656 + 2.49j, -0.9 + 0.4j]), {"wl_min": 2}),
}


def _ctx(emme, d, **options):
    return emme.Context(emme.params_from_dict(d), **options)


@pytest.mark.parametrize("case", sorted(CASES))
def test_m_is_bit_identical_to_the_plain_fill(emme, case):
    mk, omegas, opt = CASES[case]
    d = mk()
    with _ctx(emme, d, node_cache_gb=0.0, **opt) as ctx:
        for batch in (omegas, omegas[:1]):  # omega-lane kernel, then lanes-are-nodes
            M, iv = ctx.assemble(batch, want_intervals=True)
            Md, Mp, ivd = ctx.assemble_derivative(batch, want_intervals=True)
            assert np.array_equal(M.view(np.float64), Md.view(np.float64)), (case, len(batch))
            assert np.array_equal(iv, ivd)
            assert np.isfinite(Mp).all() and np.abs(Mp).max() > 0
    with _ctx(emme, d, **opt) as ctx:  # a cached context: the derivative fill neither reads nor grows the cache
        M, iv = ctx.assemble(omegas, want_intervals=True)
        state = ctx.cache_state()
        Md, Mp, ivd = ctx.assemble_derivative(omegas, want_intervals=True)
        assert ctx.cache_state() == state
        assert np.array_equal(iv, ivd)
        for b in range(len(omegas)):
            assert np.abs(Md[b] - M[b]).max() <= 1e-10 * np.abs(M[b]).max()


@pytest.mark.parametrize("case", sorted(CASES))
def test_m_matches_the_oracle(emme, oracle, case):
    mk, omegas, opt = CASES[case]
    d = mk()
    with _ctx(emme, d, node_cache_gb=0.0, **opt) as ctx:
        M, _, iv = ctx.assemble_derivative(omegas, want_intervals=True)
    po = oracle.params(d)
    for b, w in enumerate(omegas):
        Mo, tot = oracle.assemble(po, complex(w))
        assert np.abs(M[b] - Mo).max() <= 1e-10 * np.abs(Mo).max(), (case, b)
        assert iv[b] == tot


@pytest.mark.parametrize("case", sorted(CASES))
def test_mp_is_the_complex_derivative(emme, case):
    mk, omegas, opt = CASES[case]
    with _ctx(emme, mk(), node_cache_gb=0.0, **opt) as ctx:
        _, Mp, iv = ctx.assemble_derivative(omegas, want_intervals=True)
        for b, w in enumerate(omegas):
            h = 1e-6 * abs(w)
            scale = np.abs(Mp[b]).max()
            for step in (h, 1j * h):  # along Re omega and along Im omega: M is analytic, both give M'
                M2, iv2 = ctx.assemble(np.array([w + step, w - step]), want_intervals=True)
                assert (iv2 == iv[b]).all(), (case, b, step, iv2, iv[b])  # same trees: the difference is M'
                fd = (M2[0] - M2[1]) / (2 * step)
                err = np.abs(fd - Mp[b]).max()
                assert err <= 1e-6 * scale, (case, b, step, err / scale)


ELLIPSES = [(-0.80 + 0.25j, 0.25, 0.20), (-0.641 - 0.232j, 0.085, 0.05)]


@pytest.fixture(scope="module")
def ctx256(emme):
    import bench
    ctx = emme.Context(emme.params_from_dict(bench.workload_dict(256)), device=0)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("ell", range(len(ELLIPSES)))
def test_argument_principle_from_mp_matches_the_winding(ctx256, ell):
    c, a, b = ELLIPSES[ell]
    res = ctx256.find_roots_in_contour(c, (a, b))
    assert res["winding"] >= 0
    N = 64
    t = 2 * np.pi * np.arange(N) / N
    z = c + a * np.cos(t) + 1j * b * np.sin(t)
    dz = -a * np.sin(t) + 1j * b * np.cos(t)
    M, Mp = ctx256.assemble_derivative(z)
    tr, info = ctx256.trace_solve(M, Mp)
    assert (info == 0).all()
    count = np.sum(tr * dz) / (1j * N)  # (1 / 2 pi i) closed integral of tr(M^-1 M') d omega, trapezoid rule
    assert abs(count - res["winding"]) < 0.02, (count, res["winding"])


def _golden_roots():
    g = np.load(GOLDEN_CFG3)
    r = g["roots"][g["converged"].astype(bool)]
    out = []
    for x in r:
        if all(abs(x - y) > 1e-7 * abs(x) for y in out):
            out.append(x)
    return np.array(out + [MISSED_DAMPED])


# Two golden chains are left out of the 6-step rule: the one that ended at 0.0468 + 0.0036i, next to
# Re omega = 0 where M is not analytic, stopped on its step size away from any root (the secant from the same guess
# stops 4.7e-5 from it, Newton does not settle), and -0.4561 - 0.1966i is a near-double root: Newton and the secant
# both converge linearly there, in 7 steps each.
SPURIOUS = 0.04680305249320635 + 0.0035554167215062246j
NEAR_DOUBLE = -0.4561423236079871 - 0.1966192121085958j


def test_newton_converges_to_the_reference_roots(emme, ctx256):
    roots = np.array([x for x in _golden_roots() if abs(x - SPURIOUS) > 1e-6])
    guesses = roots * (1 + 1e-3)
    state = ctx256.cache_state()
    r1, it1, info1 = ctx256.solve_roots_newton(guesses)
    assert ctx256.cache_state() == state
    assert (info1 == 0).all(), info1
    simple = np.abs(roots - NEAR_DOUBLE) > 1e-6
    assert simple.sum() == len(roots) - 1
    assert (it1[simple] <= 6).all(), it1
    assert (it1[~simple] <= 8).all(), it1
    assert np.abs(r1 - roots).max() <= 1e-9, np.abs(r1 - roots)
    r2, it2, info2, its = ctx256.solve_roots_newton(guesses, want_iterates=True)
    assert np.array_equal(r1.view(np.float64), r2.view(np.float64))
    assert np.array_equal(it1, it2) and np.array_equal(info1, info2)
    assert np.isnan(its[0, it2[0]:]).all() and np.isfinite(its[0, :it2[0]]).all()
    # the last fill's M per chain stays available, as after solve_roots
    v, vinfo = ctx256.null_vectors(nbatch=len(roots))
    assert (vinfo == 0).all()
    Mf = ctx256.final_matrix(0)
    assert np.isfinite(Mf).all()


def test_newton_does_not_confirm_the_spurious_golden_chain_end(ctx256):
    """What Newton does from the chain end next to Re omega = 0 that the 6-step rule above leaves out: it does not
    arrive at it (the secant from the same guess stops 4.7e-5 away from it, on its step size)."""
    params = ctx256.params
    r, it, info = ctx256.solve_roots_newton(np.array([SPURIOUS * (1 + 1e-3)]))
    rs, its, infos = ctx256.solve_roots(np.array([SPURIOUS * (1 + 1e-3)]))
    assert not (info[0] == 0 and it[0] <= params.iteration_step_limit and abs(r[0] - SPURIOUS) <= 1e-9), (r, it, info)
    assert abs(rs[0] - SPURIOUS) > 1e-6


def test_newton_qr_form(emme):
    import bench
    root = _golden_roots()[0]
    d = bench.workload_dict(256, iteration_method="QRSecant")
    with _ctx(emme, d) as ctx:
        r, it, info = ctx.solve_roots_newton(np.array([root * (1 + 1e-3)]))
    assert info[0] == 0 and it[0] <= 6
    assert abs(r[0] - root) <= 1e-9
