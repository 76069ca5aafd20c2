"""The secant eigenpair step and search, and the region searches that return eigenpairs, on the
device: k_eigpair_secant_step on constructed matrices against numpy, emme_solve_eigenpairs_secant against a numpy
restatement of the same iteration on ctx.assemble matrices, the routing of its fills (plain fills only: a default
context keeps its mirrored cache and its options), and emme_find_eigenpairs_in_contour /
emme_find_eigenpairs_in_contours_sets against the root forms of the same searches and the SVD's null vectors.

As tests/test_gpu_contour_sets.py says, a failing node fill cannot be provoked through a legal contour: the path that
takes an item out of a call is the shared driver's, covered by the host self-test of the round plan."""
import numpy as np
import pytest

from oracle.binding import example_stellarator, example_tokamak

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
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


# ---- 1. the secant step kernel on constructed matrices ---------------------------------------------------------------
# 5: one partial block; 16 / 17: the edge of the 16-row blocks of the solves; 24, 64: a ragged and a whole 64-lane row;
# 300: one-workgroup factorisation, strided rows; 1040: beyond the 48 KiB dynamic-LDS default, the unblocked branch
STEP_ORDERS = [5, 16, 17, 24, 64, 300, 1040]
DOMEGA = [1e-2 * np.exp(0.7j), 1e-7 * np.exp(-2.1j)]


def _constructed(n):
    rng = np.random.default_rng(2000 + n)
    cplx = lambda *shape: rng.normal(size=shape) + 1j * rng.normal(size=shape)
    sig = np.logspace(0.0, -3.0, n)
    M = np.array([(np.linalg.qr(cplx(n, n))[0] * sig) @ np.linalg.qr(cplx(n, n))[0].conj().T for _ in range(2)])
    D = cplx(2, n, n)
    v = cplx(2, n)
    v /= np.linalg.norm(v, axis=1)[:, None]
    return M, D, v


@pytest.mark.parametrize("n", STEP_ORDERS)
def test_secant_step_matches_numpy(small_ctx, n):
    M, D, v = _constructed(n)
    kappa = [np.linalg.cond(M[b], 2) for b in range(2)]
    s = _start_vector(n)
    dw = np.array(DOMEGA)
    Mold = M - dw[:, None, None] * D
    for have_v in (1, 0):
        vd, tau, resid, info = small_ctx.eigenpair_secant_step(M, Mold, dw, v if have_v else None)
        assert (info == 0).all(), (n, have_v, info)
        for b in range(2):
            vin = v[b] if have_v else np.linalg.solve(M[b], s)
            vin = vin / np.linalg.norm(vin)
            # the same secant in numpy: the difference of the two matrices as they are held, over domega
            u = np.linalg.solve(M[b], ((M[b] - Mold[b]) @ vin) / dw[b])
            t = np.vdot(vin, u)
            # forward bound of a pivoted LU solve, x 100 for its constant and growth (tests/test_gpu_eigenpairs.py).  tau
            # is linear in D, so the relative error below is the bound "scaled by |D|": it does not change with |D|
            bound = 100.0 * n * EPS * kappa[b]
            e_dir = 1.0 - _overlap(vd[b], u)
            e_tau = abs(tau[b] - t) / abs(t)
            e_nrm = abs(np.linalg.norm(vd[b]) - 1.0)
            e_res = abs(resid[b] - np.linalg.norm(M[b] @ vin) / np.linalg.norm(M[b]))
            print(f"n={n} |dw|={abs(dw[b]):.0e} have_v={have_v}: dir {e_dir:.1e} tau {e_tau:.1e} norm {e_nrm:.1e} "
                  f"(bound {bound:.1e}) resid {e_res:.1e}")
            assert e_dir <= bound and e_tau <= bound and e_nrm <= bound, (n, have_v, b, e_dir, e_tau, e_nrm, bound)
            assert e_res <= 1e-12, (n, have_v, b, e_res)  # n eps of an n-term sum; 2048 eps = 4.5e-13
    again = small_ctx.eigenpair_secant_step(M, Mold, dw, v)
    first = small_ctx.eigenpair_secant_step(M, Mold, dw, v)
    for a, b in zip(again, first):
        assert a.tobytes() == b.tobytes(), n  # no atomics, fixed reduction order


def test_secant_step_reports_a_zero_column_and_a_zero_domega(emme, small_ctx):
    n = 64
    M, D, v = _constructed(n)
    dw = np.array(DOMEGA)
    Mold = M - dw[:, None, None] * D
    M[1][:, 10] = 0.0
    vd, tau, resid, info = small_ctx.eigenpair_secant_step(M, Mold, dw, v)
    assert info[0] == 0 and info[1] == 11
    assert np.isnan(vd[1]).all() and np.isnan(tau[1]) and np.isnan(resid[1])
    alone = small_ctx.eigenpair_secant_step(M[:1], Mold[:1], dw[:1], v[:1])
    assert vd[0].tobytes() == alone[0][0].tobytes() and tau[0] == alone[1][0] and resid[0] == alone[2][0]
    vd, tau, resid, info = small_ctx.eigenpair_secant_step(M[:1], Mold[:1], [0.0], v[:1])
    assert info[0] == -6  # EMME_ENUMERIC: a zero domega has no reciprocal
    big = np.zeros((1, 2049, 2049), dtype=np.complex128)
    with pytest.raises(emme.EmmeError) as e:
        small_ctx.eigenpair_secant_step(big, big, [1e-3], None)
    assert e.value.code == -5


# ---- 2. the search against a numpy restatement ------------------------------------------------------------------------
LAT_ES = (np.linspace(-1.0, -0.4, 4)[None, :] + 1j * np.linspace(-0.3, 0.3, 4)[:, None]).ravel()
LAT_EM = (np.linspace(-0.55, -0.25, 4)[None, :] + 1j * np.linspace(0.2, 0.8, 3)[:, None]).ravel()  # (tests/test_gpu_eigenpairs.py)
CASES = {
    "es-gk15": (lambda **o: example_tokamak(npoints=24, **o), LAT_ES),
    "es-gk31": (lambda **o: example_tokamak(npoints=32, integration_start_points=31, **o), LAT_ES),
    "em-gk31": (lambda **o: example_stellarator(npoints=24, **o), LAT_EM),
}


def _restate(fill, g, v0=None):
    """The iteration of emme_solve_eigenpairs_secant in numpy: fill(omega) -> M.  Returns omega, v, resid, steps,
    iterates."""
    g = complex(g)
    w0 = 0.99 * g
    dw = 0.01 * g
    w = w0 + dw
    Mold, M = fill(w0), fill(w)
    v, its = v0, []
    for j in range(STEPS + 1):
        if v is None:
            v = np.linalg.solve(M, _start_vector(M.shape[0]))
            v = v / np.linalg.norm(v)
        u = np.linalg.solve(M, ((M - Mold) @ v) / dw)
        d = -1.0 / np.vdot(v, u)
        w, dw = w + d, d
        v = u / np.linalg.norm(u)
        its.append(w)
        Mold, M = M, fill(w)
        if abs(d) < TOL * abs(w):
            break
    return w, v, np.linalg.norm(M @ v) / np.linalg.norm(M), len(its), np.array(its)


def _simple_roots(ctx, lattice):
    """Newton roots from the lattice that are simple roots of an analytic M (tests/test_gpu_eigenpairs.py)."""
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
        self.out = self.ctx.solve_eigenpairs(self.guesses, tol=TOL, step_limit=STEPS, want_iterates=True, secant=True)
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
def test_secant_search_matches_the_restatement(cases, name):
    c = cases(name)
    assert len(c.roots) >= 2, (name, c.roots)  # (the test cannot pass empty)
    roots, vecs, resid, iters, info, its = c.out
    fill = lambda w: c.ctx.assemble(np.array([w]))[0]
    for b, g in enumerate(c.guesses):
        wr, vr, rr, nr, itr = _restate(fill, g)
        bar = 1e-9 * abs(wr)
        print(f"{name} chain {b}: root {roots[b]:.12g} restatement {wr:.12g} newton {c.roots[b]:.12g} info {info[b]} "
              f"steps {iters[b]} / {nr} resid {resid[b]:.1e} / {rr:.1e}")
        assert info[b] == 0, (name, b, info)
        assert int(iters[b]) == nr, (name, b, iters[b], nr)
        assert np.abs(its[b, :nr] - itr).max() <= bar, (name, b, its[b, :nr], itr)
        assert abs(roots[b] - wr) <= bar and abs(roots[b] - c.roots[b]) <= bar, (name, b, roots[b], wr, c.roots[b])
        assert np.isnan(its[b, iters[b]:]).all()
        assert resid[b] < 1e-12, (name, b, resid[b])
        Mf = c.final[b]
        sv = np.linalg.svd(Mf)
        r_np = np.linalg.norm(Mf @ vecs[b]) / np.linalg.norm(Mf)
        e_svd = 1.0 - _overlap(vecs[b], sv[2][-1].conj())
        print(f"{name} chain {b}: numpy resid on the final matrix {r_np:.1e}, 1 - overlap with the SVD {e_svd:.1e}")
        assert abs(np.linalg.norm(vecs[b]) - 1.0) <= 1e-12
        assert abs(resid[b] - r_np) <= 1e-12, (name, b, resid[b], r_np)
        assert e_svd <= 100.0 * resid[b] * sv[1][0] / sv[1][-2], (name, b, e_svd, resid[b], sv[1][0] / sv[1][-2])


def test_secant_search_twice_and_from_its_own_vectors(cases):
    c = cases("es-gk15")
    # (two calls on the settled context: the fixture's call may have grown the node cache)
    again = c.ctx.solve_eigenpairs(c.guesses, tol=TOL, step_limit=STEPS, want_iterates=True, secant=True)
    third = c.ctx.solve_eigenpairs(c.guesses, tol=TOL, step_limit=STEPS, want_iterates=True, secant=True)
    for a, b in zip(again, third):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(c.out[:1] + c.out[3:5], again[:1] + again[3:5]):  # roots, iters, info
        assert np.allclose(a, b, rtol=1e-12, atol=0, equal_nan=True)
    roots, vecs, _, iters, info, _ = c.out
    r2, v2, resid2, it2, info2 = c.ctx.solve_eigenpairs(c.guesses, v0=3.0 * vecs, tol=TOL, step_limit=STEPS, secant=True)
    assert (info2 == 0).all() and (it2 <= iters).all(), (iters, it2)
    assert (np.abs(r2 - roots) <= 1e-9 * np.abs(roots)).all() and (resid2 <= 1e-12).all()
    v, vinfo = c.ctx.null_vectors(nbatch=len(roots))  # (the last fill's matrices: the polish's)
    assert (vinfo == 0).all()
    for b in range(len(roots)):
        assert 1.0 - _overlap(v[b], v2[b]) <= 1e-10


# ---- 3. routing: plain fills only ------------------------------------------------------------------------------------
def test_secant_search_leaves_a_default_context_as_it_was(emme, cases):
    c = cases("es-gk15")
    d = CASES["es-gk15"][0]
    w = np.array([-0.8 + 0.25j, -0.6 + 0.1j])
    with _ctx(emme, d()) as ctx, _ctx(emme, d()) as fresh:
        assert ctx.mirror_pairs() == 1
        before = bytes(ctx.options())
        out = ctx.solve_eigenpairs(c.guesses, tol=TOL, step_limit=STEPS, want_iterates=True, secant=True)
        assert ctx.mirror_pairs() == 1 and bytes(ctx.options()) == before
        assert ctx.assemble(w).tobytes() == fresh.assemble(w).tobytes()
    assert (out[4] == 0).all() and (out[2] < 1e-12).all()
    assert (np.abs(out[0] - c.out[0]) <= 1e-9 * np.abs(out[0])).all()
    # iteration_method is not consulted: a QR-secant context with the same history gives the same bits
    with _ctx(emme, d(iteration_method="QRSecant")) as qr:
        out_qr = qr.solve_eigenpairs(c.guesses, tol=TOL, step_limit=STEPS, want_iterates=True, secant=True)
    for a, b in zip(out, out_qr):
        assert a.tobytes() == b.tobytes()


def test_secant_chains_on_three_parameter_sets(emme):
    dicts = [example_tokamak(npoints=24, k_rho=0.3182 * f) for f in (1.0, 1.15, 1.3)]
    sets = np.array([0, 1, 2, 2, 1, 0], dtype=np.int32)
    g0 = np.array([-0.57 + 0.24j, -0.57 + 0.24j, -0.57 + 0.24j, -0.72 - 0.22j, -0.72 - 0.22j, -0.72 - 0.22j])
    with _ctx(emme, dicts[0]) as ctx:
        ctx.bind_param_sets([emme.params_from_dict(d) for d in dicts])
        r0, _, info0 = ctx.solve_roots_sets(sets, g0, exact=True, tol=TOL, step_limit=STEPS)
        assert (info0 == 0).all()
        g = r0 * (1 + 1e-3)
        roots, vecs, resid, iters, info = ctx.solve_eigenpairs(g, set=sets, tol=TOL, step_limit=STEPS, secant=True)
    assert (info == 0).all() and (resid < 1e-12).all(), (info, resid)
    assert len({complex(np.round(x, 6)) for x in roots}) >= 4  # (the sets do move the roots)
    for s in range(3):
        with _ctx(emme, dicts[s], node_cache_gb=0) as one:
            sel = np.flatnonzero(sets == s)
            r1, v1, resid1, it1, info1 = one.solve_eigenpairs(g[sel], tol=TOL, step_limit=STEPS, secant=True)
        assert (info1 == 0).all()
        for q, b in enumerate(sel):
            assert abs(roots[b] - r1[q]) <= 1e-9 * abs(r1[q]) and abs(roots[b] - r0[b]) <= 1e-9 * abs(r0[b]), (s, b)
            assert 1.0 - _overlap(vecs[b], v1[q]) <= 1e-9, (s, b)


# ---- 4. region searches that return eigenpairs ------------------------------------------------------------------------
def _lattice_roots(ctx, re, im):
    """Distinct converged roots of the lattice search that are simple roots (tests/test_gpu_contour.py)."""
    g = (re[None, :] + 1j * im[:, None]).reshape(-1)
    roots, iters, info = ctx.solve_roots(g)
    out = []
    for x in roots[info == 0]:
        if np.isfinite(x) and x.real < 0 and all(abs(x - y) > 1e-6 * abs(x) for y in out):
            s = np.linalg.svd(ctx.assemble([x])[0], compute_uv=False)
            if s[-1] < 1e-6 * s[0] and s[-2] > 1e-4 * s[0]:
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
    circ = _pair_circle(lat)
    if circ is None:  # one lattice root: a circle of half the distance to its nearest neighbour
        near = [np.sort(np.abs(lat - x))[1] if len(lat) > 1 else np.inf for x in lat]
        k = int(np.argmax(near))
        circ = (lat[k], min(0.5 * near[k], 0.9 * abs(lat[k].real), 0.3))
    return circ


def _check_pairs(ctx, res, fill):
    """info, residuals and every vector against the numpy SVD null vector of the matrix at its root"""
    assert np.all(res["info"] == 0)
    assert res["vecs"].shape == (len(res["roots"]), ctx.dim)
    for q, x in enumerate(res["roots"]):
        assert res["resid"][q] <= 1e-12, (q, res["resid"])
        assert abs(np.linalg.norm(res["vecs"][q]) - 1.0) <= 1e-12
        sv = np.linalg.svd(fill(x))
        e_svd = 1.0 - _overlap(res["vecs"][q], sv[2][-1].conj())
        print(f"root {x:.10g}: resid {res['resid'][q]:.1e}, 1 - overlap with the SVD {e_svd:.1e}, iters {res['iters'][q]}")
        assert e_svd <= 100.0 * max(res["resid"][q], EPS) * sv[1][0] / sv[1][-2], (q, e_svd, res["resid"][q])
    for q in range(len(res["roots"])):
        for p in range(q):
            assert _overlap(res["vecs"][p], res["vecs"][q]) < 1.0 - 1e-6, (p, q)


@pytest.mark.parametrize("model", ["tokamak_es", "stellarator_em"])
def test_find_eigenpairs_in_contour_small(emme, model):
    if model == "tokamak_es":
        d = example_tokamak(npoints=32)
        re, im = np.linspace(-1.2, -0.4, 8), np.linspace(-0.3, 0.4, 8)
    else:
        d = example_stellarator(npoints=32)
        re, im = np.linspace(-2.2, -1.1, 8), np.linspace(1.9, 3.1, 8)
    with emme.Context(emme.params_from_dict(d), device=0) as ctx:
        # tol: the searches stop on their step, and from a Beyn seed the first step is already below the context's own
        # iteration_precision -- the pair is then one step old (residuals 1e-11 measured).  The residual bar below is
        # that of a converged pair, so both searches run to the tolerance of the tests above
        tol = TOL
        lat = _lattice_roots(ctx, re, im)
        assert len(lat) >= 1, "the lattice found no root"
        if model == "tokamak_es":
            assert _pair_circle(lat) is not None, lat
        c, r = _circle(lat)
        ref = ctx.find_roots_in_contour(c, (r, r), tol=tol, step_limit=STEPS)
        assert ref["complete"], ref
        if model == "tokamak_es":
            assert ref["n_roots"] >= 2
        for exact in (False, True):
            res = ctx.find_eigenpairs_in_contour(c, (r, r), exact=exact, tol=tol, step_limit=STEPS)
            assert (res["winding"], res["n_roots"], res["complete"], res["points_used"]) == \
                   (ref["winding"], ref["n_roots"], ref["complete"], ref["points_used"]), (exact, res, ref)
            for x, y in zip(res["roots"], ref["roots"]):  # (both sorted by Im omega descending)
                assert abs(x - y) <= 1e3 * tol * abs(y), (exact, res["roots"], ref["roots"])
            _check_pairs(ctx, res, lambda x: ctx.assemble([x])[0])
            # two calls on the settled context (the first may have grown the node cache)
            again = ctx.find_eigenpairs_in_contour(c, (r, r), exact=exact, tol=tol, step_limit=STEPS)
            third = ctx.find_eigenpairs_in_contour(c, (r, r), exact=exact, tol=tol, step_limit=STEPS)
            for key in ("roots", "vecs", "resid", "iters", "info"):
                assert again[key].tobytes() == third[key].tobytes(), (exact, key)
            v, vinfo = ctx.null_vectors(nbatch=1)  # (the polish's matrices are the context's last)
            assert vinfo[0] == 0


def test_find_eigenpairs_in_contours_sets(emme):
    dicts = [example_tokamak(npoints=24, k_rho=0.3182 * f) for f in (1.0, 1.15, 1.3)]
    g0 = np.array([-0.57 + 0.24j] * 3)
    with _ctx(emme, dicts[0]) as ctx:
        ctx.bind_param_sets([emme.params_from_dict(d) for d in dicts])
        r0, _, info0 = ctx.solve_roots_sets([0, 1, 2], g0, exact=True, tol=TOL, step_limit=STEPS)
        assert (info0 == 0).all()
        rad = [0.25 * abs(x.real) for x in r0]
        kw = dict(tol=TOL, step_limit=STEPS)  # (a converged pair: see test_find_eigenpairs_in_contour_small)
        got = {ex: ctx.find_eigenpairs_in_contours_sets([0, 1, 2], r0, [(r, r) for r in rad], exact=ex, **kw)
               for ex in (False, True)}
        plain = ctx.find_roots_in_contours_sets([0, 1, 2], r0, [(r, r) for r in rad], **kw)
        for ex in (False, True):
            for k in range(3):
                g, p = got[ex][k], plain[k]
                assert g["status"] == 0
                assert (g["winding"], g["n_roots"], g["points_used"]) == (p["winding"], p["n_roots"], p["points_used"])
                assert g["n_roots"] >= 1
                _check_pairs(ctx, g, lambda x, k=k: ctx.assemble_sets([k], [x])[0])
    for k in range(3):
        with _ctx(emme, dicts[k], node_cache_gb=0) as one:
            single = one.find_eigenpairs_in_contour(r0[k], (rad[k], rad[k]), **kw)
        g = got[False][k]
        assert single["n_roots"] == g["n_roots"] and single["winding"] == g["winding"]
        for q in range(len(g["roots"])):
            assert abs(g["roots"][q] - single["roots"][q]) <= 1e-9 * abs(single["roots"][q]), (k, q)
            assert 1.0 - _overlap(g["vecs"][q], single["vecs"][q]) <= 1e-9, (k, q)
