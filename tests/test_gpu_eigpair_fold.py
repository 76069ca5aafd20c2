"""The folded secant eigenpair step: the step alone on matrices of the promised structure
(emme_eigenpair_secant_folded_step_batch), on the device's own mirrored fills, inside the secant eigenpair search
(option eigpair_fold), the routing rule, the region search's polish, and mode parity.

Orders of the step alone: those of test_gpu_fold.py -- 2 and 4 (half order 1 and 2), 16, 30 (half order odd), 34, and
126 / 128 / 130 / 256 / 258, half orders ragged against the panel width 16 on both sides of a multiple.  The bar per
item and figure: the largest of ten times the error of emme_eigenpair_secant_step_batch (the unfolded kernel) on the same
inputs against the same numpy answer, ten times the error of the numpy restatement of the folded formulas
(eigpair_fold_reference.py), and 1e-13 -- the factor ten is test_gpu_fold.py's allowance for the other pivot order and
the extra roundings.  Near a root tau carries eps * cond(M) whichever way the step is taken: the searches are compared by
omega, the vector up to phase and the residual, never by tau."""
import numpy as np
import pytest

from device_buffers import GuardedBuffer
from eigpair_fold_reference import direct_step, folded_step
from fold_reference import structured, structured_pair
from oracle.binding import example_stellarator, example_tokamak

pytestmark = pytest.mark.gpu

# the 16-guess secant search and the shallow cache of test_gpu_fold.py
GUESSES = np.array([-0.7249 + 0.1803j, -0.5617 + 0.3641j, -0.6346 + 0.2529j, -0.9649 + 0.3541j, -0.9199 + 0.2919j,
                    -0.5759 + 0.3225j, -1.0968 + 0.1274j, -0.6073 + 0.2623j, -0.6218 + 0.2523j, -0.8192 + 0.3614j,
                    -0.9182 + 0.2084j, -0.9329 + 0.2795j, -0.9471 + 0.1178j, -0.833 + 0.2163j, -0.7973 + 0.1969j,
                    -0.7679 + 0.1451j])
TINY = dict(node_cache_gb=0.05, cache_min_depth=1)

ORDERS = [2, 4, 16, 30, 34, 126, 128, 130, 256, 258]
FLOOR = 1e-13
EINVAL, ENUMERIC = -1, -6

_INPUTS = {}


def _overlap(a, b):
    return abs(np.vdot(a, b)) / (np.linalg.norm(a) * np.linalg.norm(b))


def _figures(v, tau, resid, ref):
    """(relative error of tau, 1 - |overlap|, | |v| - 1 |, absolute error of resid) per item against numpy's step."""
    return np.array([[abs(tau[b] - ref[b][1]) / abs(ref[b][1]), abs(1.0 - _overlap(v[b], ref[b][0])),
                      abs(np.linalg.norm(v[b]) - 1.0), abs(resid[b] - ref[b][2])] for b in range(len(ref))])


def _inputs(n, nb):
    """(M, M_old, domega, v, numpy's step, the restatement's figures) of nb items of order n, computed once."""
    key = (n, nb)
    if key not in _INPUTS:
        rng = np.random.default_rng(7000 * n + nb)
        pairs = [structured_pair(rng, n) for _ in range(nb)]
        M, Mo = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
        dw = (0.2 + 0.3 * rng.random(nb)) * np.exp(2j * np.pi * rng.random(nb))
        v = rng.standard_normal((nb, n)) + 1j * rng.standard_normal((nb, n))
        v /= np.linalg.norm(v, axis=1)[:, None]
        ref = [direct_step(M[b], Mo[b], dw[b], v[b])[:3] for b in range(nb)]
        re = [folded_step(M[b], Mo[b], dw[b], v[b])[:3] for b in range(nb)]
        err_r = _figures([r[0] for r in re], [r[1] for r in re], [r[2] for r in re], ref)
        _INPUTS[key] = (M, Mo, dw, v, ref, err_r)
    return _INPUTS[key]


@pytest.fixture(scope="module")
def ctx(emme):
    with emme.Context(emme.params_from_dict(example_tokamak(npoints=24))) as c:
        yield c


# ---- 1. the step alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 5])
@pytest.mark.parametrize("n", ORDERS)
def test_step_against_numpy(ctx, n, nb):
    M, Mo, dw, v, ref, err_r = _inputs(n, nb)
    vf, tau, resid, info = ctx.eigenpair_secant_folded_step(M, Mo, dw, v)
    assert (info == 0).all(), info
    assert ctx.linstep_kernel_symbol() == "k_lu_inplace"
    err = _figures(vf, tau, resid, ref)
    vu, tau_u, resid_u, info_u = ctx.eigenpair_secant_step(M, Mo, dw, v)
    assert (info_u == 0).all()
    err_u = _figures(vu, tau_u, resid_u, ref)
    bar = np.maximum(np.maximum(10.0 * err_u, 10.0 * err_r), FLOOR)
    print(f"folded eigenpair step n={n} nb={nb}: tau / 1 - overlap / | |v| - 1 | / resid  folded {err.max(axis=0)}, "
          f"unfolded {err_u.max(axis=0)}, restatement {err_r.max(axis=0)}")
    assert (err <= bar).all(), (n, nb, err, bar)
    again = ctx.eigenpair_secant_folded_step(M, Mo, dw, v)
    for a, b in zip((vf, tau, resid, info), again):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n", [30, 130, 256])
def test_item_alone_and_in_a_batch(ctx, n):
    M, Mo, dw, v, _, _ = _inputs(n, 5)
    out5 = ctx.eigenpair_secant_folded_step(M, Mo, dw, v)
    out1 = ctx.eigenpair_secant_folded_step(M[2:3], Mo[2:3], dw[2:3], v[2:3])
    for a, b in zip(out5, out1):
        assert a[2].tobytes() == b[0].tobytes()


@pytest.mark.parametrize("n", [16, 130])
def test_singular_half(ctx, n):
    """A11 = A12 J: the odd block is exactly zero.  That item fails; its neighbours keep their bits."""
    M, Mo, dw, v, _, _ = _inputs(n, 5)
    M, Mo, v = M[:3].copy(), Mo[:3].copy(), v[:3]
    m = n // 2
    rng = np.random.default_rng(n)
    A = structured(rng, m, 4.0)
    A = np.triu(A) + np.triu(A, 1).T
    S = np.block([[A, A[:, ::-1]], [A[::-1, :], A[::-1, ::-1]]])
    u = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    u[0] = 0.0
    S[:, n - 1] += u
    S[n - 1, :] += u
    M[1] = S
    vf, tau, resid, info = ctx.eigenpair_secant_folded_step(M, Mo, dw[:3], v)
    assert m < info[1] <= n, info  # a column of the odd block
    assert np.isnan(vf[1]).all() and np.isnan(tau[1]) and np.isnan(resid[1])
    assert info[0] == 0 and info[2] == 0
    for b in (0, 2):
        alone = ctx.eigenpair_secant_folded_step(M[b:b + 1], Mo[b:b + 1], dw[b:b + 1], v[b:b + 1])
        for x, y in zip((vf, tau, resid), alone):
            assert x[b].tobytes() == y[0].tobytes(), b


def test_zero_domega(ctx):
    M, Mo, dw, v, _, _ = _inputs(30, 5)
    dw = dw.copy()
    dw[3] = 0.0
    vf, tau, resid, info = ctx.eigenpair_secant_folded_step(M, Mo, dw, v)
    assert info.tolist() == [0, 0, 0, ENUMERIC, 0], info
    assert np.isnan(vf[3]).all() and np.isnan(tau[3]) and np.isnan(resid[3])
    assert np.isfinite(vf[[0, 1, 2, 4]]).all()


def test_refusals(emme, ctx):
    M, Mo, dw, v, _, _ = _inputs(4, 1)
    with pytest.raises(emme.EmmeError) as e:
        ctx.eigenpair_secant_folded_step(np.eye(3, dtype=complex)[None], np.eye(3, dtype=complex)[None], dw, np.ones((1, 3)))
    assert e.value.code == EINVAL
    # mixed sides: M on the device, M_old on the host
    with GuardedBuffer(M.shape).upload(M) as dM:
        with pytest.raises(emme.EmmeError) as e:
            ctx.eigenpair_secant_folded_step((1, 4), None, dw, v, device_ptrs=(dM.ptr, Mo.ctypes.data))
        assert e.value.code == EINVAL
        dM.assert_unchanged(M)
        dM.assert_guards_intact()


@pytest.mark.parametrize("n", [30, 258])
def test_device_form(ctx, n):
    """Device operands: the inputs are unchanged, nothing beside them is written, the bits are the host form's."""
    nb = 5
    M, Mo, dw, v, _, _ = _inputs(n, nb)
    host = ctx.eigenpair_secant_folded_step(M, Mo, dw, v)
    with GuardedBuffer(M.shape).upload(M) as dM, GuardedBuffer(Mo.shape).upload(Mo) as dO:
        dev = ctx.eigenpair_secant_folded_step((nb, n), None, dw, v, device_ptrs=(dM.ptr, dO.ptr))
        for buf, a in ((dM, M), (dO, Mo)):
            buf.assert_unchanged(a)
            buf.assert_guards_intact()
    for a, b in zip(host, dev):
        assert a.tobytes() == b.tobytes()


def _start_vector(n):
    """s of include/emme_hip.h: what a step without a caller vector starts from."""
    i = np.arange(n, dtype=np.float64)
    return (1.0 + 0.37 * np.sin(1.0 + i)) + 1j * 0.21 * np.cos(2.0 * i)


def test_step_on_the_fills(ctx):
    """N = 24, mirrored fills at two omegas, v = M^-1 s / |M^-1 s|: the folded step on the device's own M, M_old against
    the unfolded one, by the omega each of them steps to."""
    w0 = np.array([-0.8 + 0.25j, -0.6 + 0.3j])
    dw = 0.01 * w0
    Mo = ctx.assemble(w0)
    M = ctx.assemble(w0 + dw)
    assert ctx.mirror_pairs() == 1 and ctx.fill_kernel_symbol().startswith("k_assemble_dense")
    v = np.array([np.linalg.solve(M[b], _start_vector(24)) for b in range(2)])
    v /= np.linalg.norm(v, axis=1)[:, None]
    vf, tau, resid, info = ctx.eigenpair_secant_folded_step(M, Mo, dw, v)
    vu, tau_u, resid_u, info_u = ctx.eigenpair_secant_step(M, Mo, dw, v)
    assert (info == 0).all() and (info_u == 0).all()
    w = w0 + dw
    e_w = np.abs((w - 1.0 / tau) - (w - 1.0 / tau_u)) / np.abs(w)
    e_v = np.array([1.0 - _overlap(vf[b], vu[b]) for b in range(2)])
    print(f"folded eigenpair step on the fills N=24: new omega {e_w}, 1 - overlap {e_v}, resid {np.abs(resid - resid_u)}")
    assert (e_w <= 1e-12).all() and (e_v <= 1e-12).all(), (e_w, e_v)


# ---- 2. in the search -------------------------------------------------------------------------------------------------
_STARTS = {}


def _starts(emme, n):
    """The distinct converged roots of the 16-guess root search at N = n, moved by 1e-3."""
    if n not in _STARTS:
        with emme.Context(emme.params_from_dict(example_tokamak(npoints=n)), **TINY) as c:
            roots, _, info = c.solve_roots(GUESSES)
        out = []
        for x in roots[info == 0]:
            if np.isfinite(x) and all(abs(x - y) > 1e-6 * abs(x) for y in out):
                out.append(x)
        assert len(out) >= 1, roots
        _STARTS[n] = np.array(out) * (1 + 1e-3)
    return _STARTS[n]


def _search(emme, d, g, fold, v0=None, set=None, bind=None, prepare=None, step_limit=None, **options):
    with emme.Context(emme.params_from_dict(d), **options) as c:
        if prepare:
            prepare(c)
        if bind:
            c.bind_param_sets([emme.params_from_dict(x) for x in bind])
        if fold is not None:
            c.set_eigpair_fold(fold)
            assert c.eigpair_fold() == fold
        out = c.solve_eigenpairs(g, set=set, v0=v0, secant=True, step_limit=step_limit)
        return out, c.last_folded_eigpair_steps()


@pytest.mark.parametrize("n", [24, 32])
def test_search_folded_against_unfolded(emme, n):
    d = example_tokamak(npoints=n)
    g = _starts(emme, n)
    (r1, v1, res1, it1, in1), steps1 = _search(emme, d, g, 1, **TINY)
    (r0, v0, res0, it0, in0), steps0 = _search(emme, d, g, 0, **TINY)
    assert steps1 > 0 and steps0 == 0, (steps1, steps0)
    assert np.array_equal(in1, in0) and (in0 == 0).all(), (in1, in0)
    rel = np.abs(r1 - r0) / np.abs(r0)
    ov = np.array([1.0 - _overlap(v1[b], v0[b]) for b in range(len(g))])
    par = emme.vector_parity(v1)
    print(f"eigenpair search N={n}: {steps1} folded steps, roots folded against unfolded {rel.max():.3g}, "
          f"1 - overlap {ov.max():.3g}, resid folded {res1} unfolded {res0}, iterations {it1} / {it0}")
    for x, p in zip(r1, par):
        print(f"  N={n} root {x:.8f}: even share {p:.12f} (1 - p = {1.0 - p:.3g})")
    assert (rel <= 1e-9).all(), rel
    assert (ov <= 1e-10).all(), ov
    assert (res1 <= np.maximum(10.0 * res0, 1e-14)).all(), (res1, res0)
    diff = np.abs(it1.astype(int) - it0.astype(int))
    assert diff.max() <= 1 and np.count_nonzero(diff) <= 1, (it1, it0)
    # the option off is the context that never saw the setter, bit for bit
    never, steps_n = _search(emme, d, g, None, **TINY)
    assert steps_n == 0
    for a, b in zip((r0, v0, res0, it0, in0), never):
        assert a.tobytes() == b.tobytes()
    # with start vectors the first step is folded too: a search of one step
    (_, _, _, _, in_v), steps_v = _search(emme, d, g, 1, v0=v1, step_limit=0, **TINY)
    (_, _, _, _, _), steps_s = _search(emme, d, g, 1, step_limit=0, **TINY)
    assert (in_v == 0).all() and steps_v == 1 and steps_s == 0, (steps_v, steps_s)


def test_parity_of_a_root(emme):
    """The N = 24 root near -0.5667 + 0.2401i is an even mode (the CPU check: 1.6e-10 from even)."""
    want = -0.56672 + 0.24013j
    (r, v, res, it, info), steps = _search(emme, example_tokamak(npoints=24), np.array([want * (1 + 1e-3)]), 1)
    assert info[0] == 0 and abs(r[0] - want) <= 1e-4 * abs(want), (r, info)
    p = emme.vector_parity(v)[0]
    print(f"parity of the N=24 root {r[0]:.8f}: even share {p:.12f} (1 - p = {1.0 - p:.3g}), {steps} folded steps")
    assert min(p, 1.0 - p) <= 1e-6, p


# ---- 3. routing -------------------------------------------------------------------------------------------------------
ROUTING = {
    "odd": (example_tokamak(npoints=25), {}),
    "theta": (example_tokamak(npoints=24, theta=0.3), {}),
    "gk31": (example_tokamak(npoints=24, integration_start_points=31), {}),
    "stellarator": (example_stellarator(npoints=10), {}),
    "mirror_off": (example_tokamak(npoints=24), dict(prepare=lambda c: c.set_mirror_pairs(False))),
    "sets": (example_tokamak(npoints=24),
             dict(bind=[example_tokamak(npoints=24, k_rho=0.3182 * f) for f in (1.0, 1.15, 1.3)],
                  set=np.array([0, 1, 2, 2], dtype=np.int32))),
}


@pytest.mark.parametrize("case", sorted(ROUTING))
def test_routing_unfolded_cases(emme, case):
    d, kw = ROUTING[case]
    g = GUESSES[:4] if case != "stellarator" else np.array([-1.656 + 2.490j, -1.5 + 2.3j])  # (its initial_guess)
    out1, steps1 = _search(emme, d, g, 1, **kw)
    out0, steps0 = _search(emme, d, g, 0, **kw)
    assert steps1 == 0 and steps0 == 0, (case, steps1)
    for a, b in zip(out1, out0):
        assert a.tobytes() == b.tobytes(), case


def test_folded_search_leaves_a_default_context_as_it_was(emme):
    d = example_tokamak(npoints=24)
    w = np.array([-0.8 + 0.25j, -0.6 + 0.1j])
    with emme.Context(emme.params_from_dict(d)) as c, emme.Context(emme.params_from_dict(d)) as fresh:
        before = bytes(c.options())
        c.set_eigpair_fold(1)
        c.solve_eigenpairs(GUESSES[:8], secant=True)
        assert c.last_folded_eigpair_steps() > 0
        assert c.mirror_pairs() == 1 and bytes(c.options()) == before
        fresh.solve_eigenpairs(GUESSES[:8], secant=True)
        assert fresh.last_folded_eigpair_steps() == 0
        assert c.assemble(w).tobytes() == fresh.assemble(w).tobytes()


def test_env_override_and_setter_range(emme, monkeypatch):
    p = emme.params_from_dict(example_tokamak(npoints=24))
    monkeypatch.setenv("EMME_EIGPAIR_FOLD", "1")
    with emme.Context(p) as c:
        assert c.eigpair_fold() == 1
    monkeypatch.delenv("EMME_EIGPAIR_FOLD")
    with emme.Context(p) as c:
        assert c.eigpair_fold() == 0
        with pytest.raises(emme.EmmeError):
            c.set_eigpair_fold(2)
        assert c.eigpair_fold() == 0


# ---- 4. several chains that converge on different steps; the region search's polish -----------------------------------
TOL, STEPS = 1e-10, 20  # (tests/test_gpu_contour_eigenpairs.py)
_LATTICE = {}


def _lattice(emme):
    """The small tokamak case of tests/test_gpu_contour_eigenpairs.py: N = 32, the 8 x 8 lattice search and its distinct
    converged simple roots (_lattice_roots there).  Returns (the 64 guesses, the roots)."""
    if not _LATTICE:
        re, im = np.linspace(-1.2, -0.4, 8), np.linspace(-0.3, 0.4, 8)
        g = (re[None, :] + 1j * im[:, None]).reshape(-1)
        with emme.Context(emme.params_from_dict(example_tokamak(npoints=32))) as c:
            roots, _, info = c.solve_roots(g)
            out = []
            for x in roots[info == 0]:
                if np.isfinite(x) and x.real < 0 and all(abs(x - y) > 1e-6 * abs(x) for y in out):
                    sv = np.linalg.svd(c.assemble([x])[0], compute_uv=False)
                    if sv[-1] < 1e-6 * sv[0] and sv[-2] > 1e-4 * sv[0]:
                        out.append(x)
        _LATTICE["g"], _LATTICE["roots"] = g, np.array(out)
    return _LATTICE["g"], _LATTICE["roots"]


def _pair_circle(roots):
    """The smallest circle around the midpoint of two lattice roots that holds both at normalised radius < 0.8, has no
    other lattice root below 1.25 and stays inside Re omega < 0 (tests/test_gpu_contour_eigenpairs.py)."""
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


def test_search_of_several_chains_folded_against_unfolded(emme):
    """Every lattice root of the N = 32 case from three distances (1e-6, 1e-3, 3e-2 relative): chains of one call that
    converge on different steps, so the folded step's list of live half problems becomes a proper subset of the batch.
    The same assertions as for the single root above."""
    _, lat = _lattice(emme)
    assert len(lat) >= 2, lat
    g = np.concatenate([lat * (1 + 1e-6), lat * (1 + 1e-3), lat * (1 + 3e-2)])
    d = example_tokamak(npoints=32)
    (r1, v1, res1, it1, in1), steps1 = _search(emme, d, g, 1)
    (r0, v0, res0, it0, in0), steps0 = _search(emme, d, g, 0)
    ok = in0 == 0
    rel = np.abs(r1[ok] - r0[ok]) / np.abs(r0[ok])
    ov = np.array([1.0 - _overlap(v1[b], v0[b]) for b in np.flatnonzero(ok)])
    print(f"eigenpair search of {len(g)} chains N=32: {steps1} folded steps, info {in1} / {in0}, iterations {it1} / {it0}, "
          f"roots folded against unfolded {rel.max():.3g}, 1 - overlap {ov.max():.3g}, resid folded {res1} unfolded {res0}")
    for x, p in zip(r1[:len(lat)], emme.vector_parity(v1[:len(lat)])):
        print(f"  N=32 root {x:.8f}: even share {p:.12f} (1 - p = {1.0 - p:.3g})")
    assert steps1 > 0 and steps0 == 0, (steps1, steps0)
    assert np.array_equal(in1, in0) and ok.sum() >= len(lat), (in1, in0)
    assert len(set(it0[ok].tolist())) >= 2, it0  # (chains leave the list on different steps)
    assert (rel <= 1e-9).all(), rel
    assert (ov <= 1e-10).all(), ov
    assert (res1[ok] <= np.maximum(10.0 * res0[ok], 1e-14)).all(), (res1, res0)
    diff = np.abs(it1.astype(int) - it0.astype(int))
    assert diff.max() <= 1 and np.count_nonzero(diff) <= 1, (it1, it0)


def test_region_search_with_the_option_on(emme):
    """find_eigenpairs_in_contour(exact=False) on the small tokamak case of tests/test_gpu_contour_eigenpairs.py: N = 32,
    the pair circle around two roots of the 8 x 8 lattice search, which both contexts run first (it lays the cache out
    mirrored; on a fresh context the region search would lay it out over the full pair list, DESIGN.md 5.0c, and its
    polish would take no folded step).  Option on against option off."""
    g, lat = _lattice(emme)
    circ = _pair_circle(lat)
    assert circ is not None, lat
    c0, r = circ
    res = {}
    for fold in (0, 1):
        with emme.Context(emme.params_from_dict(example_tokamak(npoints=32)), eigpair_fold=fold) as c:
            c.solve_roots(g)
            assert c.mirror_pairs() == 1
            res[fold] = c.find_eigenpairs_in_contour(c0, (r, r), exact=False, tol=TOL, step_limit=STEPS)
            res[fold]["folded"] = c.last_folded_eigpair_steps()
    a, b = res[1], res[0]
    print(f"region search N=32: circle {c0:.6f} r {r:.4f}, {a['n_roots']} roots, {a['folded']} folded steps, "
          f"iterations {a['iters']} / {b['iters']}; roots {a['roots']}; even shares {emme.vector_parity(a['vecs'])}")
    assert b["folded"] == 0 and a["folded"] > 0, (a["folded"], b["folded"])
    assert (a["winding"], a["n_roots"], a["complete"], a["points_used"]) == \
           (b["winding"], b["n_roots"], b["complete"], b["points_used"]), (a, b)
    assert a["n_roots"] >= 2 and a["complete"]
    assert np.array_equal(a["info"], b["info"]) and (a["info"] == 0).all()
    assert (np.abs(a["roots"] - b["roots"]) <= 1e-9 * np.abs(b["roots"])).all()
    for x, y in zip(a["vecs"], b["vecs"]):
        assert 1.0 - _overlap(x, y) <= 1e-10
    assert (a["resid"] <= np.maximum(10.0 * b["resid"], 1e-14)).all(), (a["resid"], b["resid"])
