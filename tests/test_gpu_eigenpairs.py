"""Newton on the eigenpair (omega, v): the step kernel k_eigpair_step on constructed matrices against
numpy, emme_solve_eigenpairs against an independent restatement of the iteration (numpy's solve on M and M' from
ctx.assemble_derivative: the fills are older code, the iteration is not the code under test), and the null vectors of
emme_null_vectors_batch frozen bit for bit across the move of its triangular solves into tri_solve.hpp."""
import hashlib
import os

import numpy as np
import pytest

from oracle.binding import example_stellarator, example_tokamak

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FROZEN = os.path.join(ROOT, "tests", "golden", "null_vectors_frozen.npz")
EPS = np.finfo(np.float64).eps
EMME_EINVAL, EMME_ECONFIG = -1, -5
TOL, STEPS = 1e-10, 20


def _ctx(emme, d, **options):
    return emme.Context(emme.params_from_dict(d), **options)


def _overlap(a, b):
    return abs(np.vdot(a, b)) / (np.linalg.norm(a) * np.linalg.norm(b))


def _start_vector(n):
    """s of include/emme_hip.h: what a step without a caller vector starts from."""
    i = np.arange(n, dtype=np.float64)
    return (1.0 + 0.37 * np.sin(1.0 + i)) + 1j * 0.21 * np.cos(2.0 * i)


@pytest.fixture(scope="module")
def small_ctx(emme):
    ctx = _ctx(emme, example_tokamak(npoints=16))
    yield ctx
    ctx.close()


# ---- 1. the step kernel on constructed matrices -----------------------------------------------------------------
# 5: one partial block; 16 / 17: the edge of the 16-row blocks of the solves; 24, 64: whole and partial blocks in one
# workgroup pass; 300: one-workgroup factorisation; 600: strided loops past 512 threads, chunked two-workgroup
# factorisation; 1040 / 1100: the unblocked branch, with and without a partial last block.
STEP_ORDERS = [5, 16, 17, 24, 64, 300, 600, 1040, 1100]


def _constructed(n):
    rng = np.random.default_rng(1000 + n)
    cplx = lambda *shape: rng.normal(size=shape) + 1j * rng.normal(size=shape)
    sig = np.logspace(0.0, -3.0, n)
    M = np.array([(np.linalg.qr(cplx(n, n))[0] * sig) @ np.linalg.qr(cplx(n, n))[0].conj().T for _ in range(2)])
    Mp = cplx(2, n, n)
    v = cplx(2, n)
    v /= np.linalg.norm(v, axis=1)[:, None]
    return M, Mp, v


@pytest.mark.parametrize("n", STEP_ORDERS)
def test_step_matches_numpy(small_ctx, n):
    M, Mp, v = _constructed(n)
    kappa = [np.linalg.cond(M[b], 2) for b in range(2)]
    s = _start_vector(n)
    for have_v in (1, 0):
        vd, tau, resid, info = small_ctx.eigenpair_step(M, Mp, v if have_v else None)
        assert (info == 0).all(), (n, have_v, info)
        for b in range(2):
            vin = v[b] if have_v else np.linalg.solve(M[b], s)
            vin = vin / np.linalg.norm(vin)
            u = np.linalg.solve(M[b], Mp[b] @ vin)
            t = np.vdot(vin, u)
            bound = 100.0 * n * EPS * kappa[b]  # forward bound of a pivoted LU solve, x 100 for its constant and growth
            e_dir = 1.0 - _overlap(vd[b], u)
            e_tau = abs(tau[b] - t) / abs(t)
            e_nrm = abs(np.linalg.norm(vd[b]) - 1.0)
            e_res = abs(resid[b] - np.linalg.norm(M[b] @ vin) / np.linalg.norm(M[b]))
            print(f"n={n} have_v={have_v} b={b}: dir {e_dir:.1e} tau {e_tau:.1e} norm {e_nrm:.1e} (bound {bound:.1e}) resid {e_res:.1e}")
            assert e_dir <= bound and e_tau <= bound and e_nrm <= bound, (n, have_v, b, e_dir, e_tau, e_nrm, bound)
            assert e_res <= 1e-12, (n, have_v, b, e_res)  # n eps of an n-term sum; 2048 eps = 4.5e-13
    again = small_ctx.eigenpair_step(M, Mp, v)
    first = small_ctx.eigenpair_step(M, Mp, v)
    for a, b in zip(again, first):
        assert a.tobytes() == b.tobytes(), n  # no atomics, fixed reduction order


def test_step_reports_an_exactly_zero_column(small_ctx):
    n = 64
    M, Mp, v = _constructed(n)
    M[1][:, 10] = 0.0
    vd, tau, resid, info = small_ctx.eigenpair_step(M, Mp, v)
    assert info[0] == 0 and info[1] == 11
    assert np.isnan(vd[1]).all() and np.isnan(tau[1]) and np.isnan(resid[1])
    alone = small_ctx.eigenpair_step(M[:1], Mp[:1], v[:1])
    assert vd[0].tobytes() == alone[0][0].tobytes() and tau[0] == alone[1][0] and resid[0] == alone[2][0]


def test_step_refuses_orders_above_2048(emme, small_ctx):
    n = 2049
    M = np.zeros((1, n, n), dtype=np.complex128)
    with pytest.raises(emme.EmmeError) as e:
        small_ctx.eigenpair_step(M, M, None)
    assert e.value.code == EMME_ECONFIG


# ---- 2. the triangular solves moved into tri_solve.hpp: emme_null_vectors_batch frozen bit for bit ----------------
def _frozen_matrix(n, k):
    """Caller matrix k of order n, by integer arithmetic alone (the same bits on every machine); its last row nearly a
    combination of the first two, so that the sweeps have a direction to find."""
    i = np.arange(n, dtype=np.uint64)[:, None]
    j = np.arange(n, dtype=np.uint64)[None, :]
    mask = np.uint64(0xFFFFFFFF)

    def h(salt):
        x = (i * np.uint64(2654435761) + j * np.uint64(40503) + np.uint64(salt)) & mask
        x = x ^ (x >> np.uint64(15))
        x = (x * np.uint64(2246822519)) & mask
        x = x ^ (x >> np.uint64(13))
        x = (x * np.uint64(3266489917)) & mask
        x = x ^ (x >> np.uint64(16))
        return x.astype(np.float64) / 4294967296.0 - 0.5

    M = h(2 * k + 1) + 1j * h(2 * k + 2)
    if n >= 3:
        M[n - 1] = 0.5 * (M[0] + M[1]) + 1e-8 * M[n - 1]
    return np.ascontiguousarray(M)


@pytest.mark.parametrize("n", [5, 17, 64, 300, 1100])
def test_null_vectors_are_the_recorded_ones_bit_for_bit(small_ctx, n):
    """tests/golden/null_vectors_frozen.npz holds what emme_null_vectors_batch returned for these matrices at the commit
    before its solves were hoisted out of k_null_iterate's lambdas (and the sha256 of the matrices themselves)."""
    g = np.load(FROZEN)
    M = np.array([_frozen_matrix(n, 0), _frozen_matrix(n, 1)])
    assert hashlib.sha256(M.tobytes()).digest() == g[f"sha{n}"].tobytes(), "the test's matrices are not the recorded ones"
    v, info = small_ctx.null_vectors(M)
    assert (info == 0).all()
    assert v.tobytes() == g[f"v{n}"].tobytes(), (n, np.abs(v - g[f"v{n}"]).max())


# ---- 3. the search against an independent restatement ----------------------------------------------------------
LAT_ES = (np.linspace(-1.0, -0.4, 4)[None, :] + 1j * np.linspace(-0.3, 0.3, 4)[:, None]).ravel()
# The stellarator lattice stays around the modes of the upper half plane near -0.4 + 0.5i.  Chains started further left
# (Re omega <= -0.77) wander to the neighbourhood of -1.1232 + 0.0674i next to the real axis, where a search stops on its
# step size without M being singular (a "chain that stops without a root" of DESIGN.md §11): on the oracle's matrix
# sigma_min / sigma_max is 1.8e-7 there and the same 1.3e-8 to the side, the reference's own secant search uses all its
# 101 steps, and trace-form Newton chains from two lattices stop 7.9e-5 apart.  The sigma rule's 1e-6 lets those points
# through, and none of them is a root to compare at.
LAT_EM = (np.linspace(-0.55, -0.25, 4)[None, :] + 1j * np.linspace(0.2, 0.8, 3)[:, None]).ravel()
CASES = {
    "es-gk15": (lambda **o: example_tokamak(npoints=24, **o), LAT_ES),
    "es-gk31": (lambda **o: example_tokamak(npoints=32, integration_start_points=31, **o), LAT_ES),
    "em-gk31": (lambda **o: example_stellarator(npoints=24, **o), LAT_EM),
}


def _restate(fill, g, v0=None):
    """The iteration of DESIGN.md §14 in numpy: fill(omega) -> (M, M').  Returns omega, v, resid, steps, iterates."""
    w, v, its = complex(g), v0, []
    for j in range(STEPS + 1):
        M, Mp = fill(w)
        if v is None:
            v = np.linalg.solve(M, _start_vector(M.shape[0]))
            v = v / np.linalg.norm(v)
        u = np.linalg.solve(M, Mp @ v)
        d = -1.0 / np.vdot(v, u)
        w = w + d
        v = u / np.linalg.norm(u)
        its.append(w)
        if abs(d) < TOL * abs(w):
            break
    M, _ = fill(w)
    return w, v, np.linalg.norm(M @ v) / np.linalg.norm(M), len(its), np.array(its)


def _simple_roots(ctx, lattice):
    """Newton roots from the lattice that are simple roots of an analytic M: sigma_min < 1e-6 sigma_max
    < 1e2 sigma_n-1."""
    r, _, info = ctx.solve_roots_newton(lattice, tol=TOL, step_limit=STEPS)
    out = []
    for x in r[(info == 0) & np.isfinite(r)]:
        if any(abs(x - y) <= 1e-7 * abs(x) for y in out):
            continue
        sv = np.linalg.svd(ctx.assemble(np.array([x]))[0], compute_uv=False)
        if sv[-1] < 1e-6 * sv[0] < 1e2 * sv[-2]:
            out.append(x)
    return np.array(out)


class _Case:
    def __init__(self, emme, name):
        mk, lattice = CASES[name]
        self.ctx = _ctx(emme, mk())
        self.roots = _simple_roots(self.ctx, lattice)
        self.guesses = self.roots * (1 + 1e-3)
        self.out = self.ctx.solve_eigenpairs(self.guesses, tol=TOL, step_limit=STEPS, want_iterates=True)
        self.final = [self.ctx.final_matrix(b) for b in range(len(self.guesses))]


@pytest.fixture(scope="module")
def cases(emme):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Case(emme, name)
        return made[name]

    yield get
    for c in made.values():
        c.ctx.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_search_matches_the_restatement(cases, name):
    c = cases(name)
    assert len(c.roots) >= 2, (name, c.roots)  # (the test cannot pass empty)
    roots, vecs, resid, iters, info, its = c.out
    fill = lambda w: tuple(a[0] for a in c.ctx.assemble_derivative(np.array([w])))
    for b, g in enumerate(c.guesses):
        wr, vr, rr, nr, itr = _restate(fill, g)
        bar = 1e-9 * abs(wr)
        print(f"{name} chain {b}: root {roots[b]:.12g} restatement {wr:.12g} newton {c.roots[b]:.12g} info {info[b]} resid {resid[b]:.1e}")
        assert info[b] == 0, (name, b, info)
        assert abs(roots[b] - wr) <= bar and abs(roots[b] - c.roots[b]) <= bar, (name, b, roots[b], wr, c.roots[b])
        assert abs(int(iters[b]) - nr) <= 1, (name, b, iters[b], nr)
        k = min(int(iters[b]), nr)
        assert np.abs(its[b, :k] - itr[:k]).max() <= bar, (name, b, its[b, :k], itr[:k])
        assert np.isnan(its[b, iters[b]:]).all()
        Mf = c.final[b]
        sv = np.linalg.svd(Mf)
        r_np = np.linalg.norm(Mf @ vecs[b]) / np.linalg.norm(Mf)
        e_svd = 1.0 - _overlap(vecs[b], sv[2][-1].conj())
        print(f"{name} chain {b}: {iters[b]} steps (restatement {nr}), resid {resid[b]:.1e} (restatement {rr:.1e}, "
              f"numpy on the final matrix {r_np:.1e}), 1 - overlap with the SVD {e_svd:.1e}, "
              f"sigma_min/sigma_max {sv[1][-1] / sv[1][0]:.1e}")
        assert abs(np.linalg.norm(vecs[b]) - 1.0) <= 1e-12
        assert abs(resid[b] - r_np) <= 1e-12, (name, b, resid[b], r_np)
        assert resid[b] <= 10.0 * rr + 1e-12, (name, b, resid[b], rr)
        assert e_svd <= 100.0 * resid[b] * sv[1][0] / sv[1][-2], (name, b, e_svd, resid[b], sv[1][0] / sv[1][-2])


def test_restart_from_the_vectors_takes_no_more_steps(cases):
    c = cases("es-gk15")
    roots, vecs, _, iters, info, _ = c.out
    r2, v2, resid2, it2, info2 = c.ctx.solve_eigenpairs(c.guesses, v0=3.0 * vecs, tol=TOL, step_limit=STEPS)  # (rows are normalised on entry)
    assert (info2 == 0).all() and (it2 <= iters).all(), (iters, it2)
    assert (np.abs(r2 - roots) <= 1e-9 * np.abs(roots)).all()
    assert (resid2 <= 1e-12).all()


def test_repeated_call_is_bit_identical_and_iterates_do_not_matter(cases):
    c = cases("es-gk15")
    again = c.ctx.solve_eigenpairs(c.guesses, tol=TOL, step_limit=STEPS, want_iterates=True)
    for a, b in zip(c.out, again):
        assert a.tobytes() == b.tobytes()
    plain = c.ctx.solve_eigenpairs(c.guesses, tol=TOL, step_limit=STEPS)
    assert len(plain) == 5
    for a, b in zip(c.out[:5], plain):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("options", [dict(node_cache_gb=0.0, tile_uncached=1, deriv_cached=1), dict(deriv_cached=1)],
                         ids=["tile-uncached", "cached"])
def test_routed_fills_reach_the_same_roots(emme, cases, options):
    c = cases("es-gk15")
    with _ctx(emme, CASES["es-gk15"][0](), **options) as ctx:
        roots, vecs, resid, iters, info = ctx.solve_eigenpairs(c.guesses, tol=TOL, step_limit=STEPS)
    assert (info == 0).all()
    assert (np.abs(roots - c.out[0]) <= 1e-9 * np.abs(roots)).all(), (roots, c.out[0])
    assert (resid <= 1e-12).all(), resid


def test_chains_on_three_parameter_sets(emme):
    dicts = [example_tokamak(npoints=24, k_rho=0.3182 * f) for f in (1.0, 1.15, 1.3)]
    with _ctx(emme, dicts[0]) as ctx:
        ctx.bind_param_sets([emme.params_from_dict(d) for d in dicts])
        sets = np.array([0, 1, 2, 2, 1, 0], dtype=np.int32)
        g0 = np.array([-0.57 + 0.24j, -0.57 + 0.24j, -0.57 + 0.24j, -0.72 - 0.22j, -0.72 - 0.22j, -0.72 - 0.22j])
        r0, _, info0 = ctx.solve_roots_sets(sets, g0, exact=True, tol=TOL, step_limit=STEPS)
        assert (info0 == 0).all()
        g = r0 * (1 + 1e-3)
        roots, vecs, resid, iters, info, its = ctx.solve_eigenpairs(g, set=sets, tol=TOL, step_limit=STEPS, want_iterates=True)
        assert (info == 0).all()
        assert len({complex(np.round(x, 6)) for x in roots}) >= 4  # (the sets do move the roots)
        for b in range(len(g)):
            fill = lambda w: tuple(a[0] for a in ctx.assemble_sets(sets[b:b + 1], np.array([w]), want_derivative=True))
            wr, vr, rr, nr, itr = _restate(fill, g[b])
            bar = 1e-9 * abs(wr)
            assert abs(roots[b] - wr) <= bar and abs(roots[b] - r0[b]) <= bar, (b, roots[b], wr, r0[b])
            assert abs(int(iters[b]) - nr) <= 1
            k = min(int(iters[b]), nr)
            assert np.abs(its[b, :k] - itr[:k]).max() <= bar
            assert resid[b] <= 10.0 * rr + 1e-12 and 1.0 - _overlap(vecs[b], vr) <= 1e-9
        with pytest.raises(emme.EmmeError) as e:
            ctx.solve_eigenpairs(g, set=np.array([0, 1, 2, 3, 1, 0]), tol=TOL, step_limit=STEPS)
        assert e.value.code == EMME_EINVAL
        ctx.bind_param_sets([])
        with pytest.raises(emme.EmmeError) as e:
            ctx.solve_eigenpairs(g, set=sets, tol=TOL, step_limit=STEPS)
        assert e.value.code == EMME_EINVAL


def test_the_iteration_method_is_not_consulted(emme, cases):
    c = cases("es-gk15")
    with _ctx(emme, CASES["es-gk15"][0](iteration_method="QRSecant")) as ctx:
        out = ctx.solve_eigenpairs(c.guesses, tol=TOL, step_limit=STEPS, want_iterates=True)
    for a, b in zip(c.out, out):
        assert a.tobytes() == b.tobytes()


def test_null_vectors_and_final_matrix_work_afterwards(cases):
    c = cases("es-gk15")
    roots, vecs, resid, iters, info, _ = c.ctx.solve_eigenpairs(c.guesses, tol=TOL, step_limit=STEPS, want_iterates=True)
    v, vinfo = c.ctx.null_vectors(nbatch=len(roots))
    assert (vinfo == 0).all()
    for b in range(len(roots)):
        Mf = c.ctx.final_matrix(b)
        assert Mf.tobytes() == c.final[b].tobytes()
        assert 1.0 - _overlap(v[b], vecs[b]) <= 1e-10  # the same null vector, by two routes


def test_bad_start_vectors_and_a_chain_out_of_steps(emme, cases):
    c = cases("es-gk15")
    v0 = c.out[1].copy()
    v0[1] = 0.0
    with pytest.raises(emme.EmmeError) as e:
        c.ctx.solve_eigenpairs(c.guesses, v0=v0, tol=TOL, step_limit=STEPS)
    assert e.value.code == EMME_EINVAL
    v0[1, 3] = np.nan
    with pytest.raises(emme.EmmeError) as e:
        c.ctx.solve_eigenpairs(c.guesses, v0=v0, tol=TOL, step_limit=STEPS)
    assert e.value.code == EMME_EINVAL
    # one step from 5 % off: info stays 0 as in the other searches, and resid says that this is no root
    roots, vecs, resid, iters, info = c.ctx.solve_eigenpairs(c.roots * 1.05, tol=TOL, step_limit=0)
    assert (info == 0).all() and (iters == 1).all()
    assert (resid > 1e-6).all() and np.isfinite(vecs).all(), resid
