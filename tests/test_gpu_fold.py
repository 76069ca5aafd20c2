"""The folded trace-secant step: the step alone on matrices of the promised structure
(emme_trace_secant_folded_batch), on the device's own mirrored fills, inside the secant search, and the routing rule.

Orders of the step alone: 2 and 4 (half order 1 and 2), 16, 30 (half order odd), 34, and 126 / 128 / 130 / 256 / 258 --
half orders ragged against the panel width 16 on both sides of a multiple.  The bar: ten times the error of
emme_trace_solve_batch on the same inputs against the same numpy reference, but not below 1e-13 relative (the factor ten
covers the other pivot order and the few extra roundings of the rank-2 terms)."""
import numpy as np
import pytest

from device_buffers import GuardedBuffer
from fold_reference import structured, structured_pair
from oracle.binding import example_stellarator, example_tokamak

pytestmark = pytest.mark.gpu

# the 16-guess secant search and the shallow cache of test_gpu_mirror_pairs.py
GUESSES = np.array([-0.7249 + 0.1803j, -0.5617 + 0.3641j, -0.6346 + 0.2529j, -0.9649 + 0.3541j, -0.9199 + 0.2919j,
                    -0.5759 + 0.3225j, -1.0968 + 0.1274j, -0.6073 + 0.2623j, -0.6218 + 0.2523j, -0.8192 + 0.3614j,
                    -0.9182 + 0.2084j, -0.9329 + 0.2795j, -0.9471 + 0.1178j, -0.833 + 0.2163j, -0.7973 + 0.1969j,
                    -0.7679 + 0.1451j])
TINY = dict(node_cache_gb=0.05, cache_min_depth=1)

ORDERS = [2, 4, 16, 30, 34, 126, 128, 130, 256, 258]
FLOOR = 1e-13
EINVAL = -1

_INPUTS = {}


def _inputs(n, nb):
    """(M, M_old, domega, numpy's tr(M^-1 (M - M_old) / domega)) of nb items of order n, computed once."""
    key = (n, nb)
    if key not in _INPUTS:
        rng = np.random.default_rng(1000 * n + nb)
        pairs = [structured_pair(rng, n) for _ in range(nb)]
        M, Mo = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
        dw = (0.2 + 0.3 * rng.random(nb)) * np.exp(2j * np.pi * rng.random(nb))
        ref = np.array([np.trace(np.linalg.solve(M[b], (M[b] - Mo[b]) / dw[b])) for b in range(nb)])
        _INPUTS[key] = (M, Mo, dw, ref)
    return _INPUTS[key]


@pytest.fixture(scope="module")
def ctx(emme):
    with emme.Context(emme.params_from_dict(example_tokamak(npoints=24))) as c:
        yield c


def _bar(ctx, M, Mo, dw, ref):
    """max(10 x the unfolded step's relative error, 1e-13) per item, and that error."""
    tr_u, info_u = ctx.trace_solve(M, (M - Mo) / dw[:, None, None])
    assert (info_u == 0).all()
    err_u = np.abs(tr_u - ref) / np.abs(ref)
    return np.maximum(10.0 * err_u, FLOOR), err_u


@pytest.mark.parametrize("nb", [1, 5])
@pytest.mark.parametrize("n", ORDERS)
def test_step_against_numpy(ctx, n, nb):
    M, Mo, dw, ref = _inputs(n, nb)
    tr, info = ctx.trace_secant_folded(M, Mo, dw)
    assert (info == 0).all(), info
    err = np.abs(tr - ref) / np.abs(ref)
    bar, err_u = _bar(ctx, M, Mo, dw, ref)
    print(f"folded step n={n} nb={nb}: err {err.max():.3g}, unfolded {err_u.max():.3g}, "
          f"ratio {(err / np.maximum(err_u, 1e-17)).max():.3g}")
    assert (err <= bar).all(), (n, nb, err, bar)


@pytest.mark.parametrize("n", [30, 130, 256])
def test_item_alone_and_in_a_batch(ctx, n):
    M, Mo, dw, _ = _inputs(n, 5)
    tr5, _ = ctx.trace_secant_folded(M, Mo, dw)
    tr1, _ = ctx.trace_secant_folded(M[2:3], Mo[2:3], dw[2:3])
    assert tr5[2].tobytes() == tr1[0].tobytes()


@pytest.mark.parametrize("n", [34, 256, 258])
def test_same_bits_under_lu_split(ctx, n):
    M, Mo, dw, _ = _inputs(n, 5)
    out = {}
    try:
        for k in (1, 2, 4):
            ctx.set_options(lu_split=k)
            out[k] = ctx.trace_secant_folded(M, Mo, dw)
    finally:
        ctx.set_options(lu_split=0)
    for k in (2, 4):
        assert out[k][0].tobytes() == out[1][0].tobytes() and np.array_equal(out[k][1], out[1][1]), k


@pytest.mark.parametrize("n", [16, 130])
def test_singular_half(ctx, n):
    """A11 = A12 J: the odd block is exactly zero.  That item fails; its neighbours keep their bits."""
    M, Mo, dw, _ = _inputs(n, 5)
    M, Mo = M[:3].copy(), Mo[:3].copy()
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
    tr, info = ctx.trace_secant_folded(M, Mo, dw[:3])
    assert info[1] != 0 and np.isnan(tr[1].real) and np.isnan(tr[1].imag), (info, tr)
    assert info[0] == 0 and info[2] == 0
    for b in (0, 2):
        alone, _ = ctx.trace_secant_folded(M[b:b + 1], Mo[b:b + 1], dw[b:b + 1])
        assert tr[b].tobytes() == alone[0].tobytes(), b


def test_refusals(emme, ctx):
    M, Mo, dw, _ = _inputs(4, 1)
    with pytest.raises(emme.EmmeError) as e:
        ctx.trace_secant_folded(np.eye(3, dtype=complex)[None], np.eye(3, dtype=complex)[None], dw)
    assert e.value.code == EINVAL
    # mixed sides: M on the device, everything else on the host
    tr, info = np.zeros(1, complex), np.zeros(1, np.int32)
    with GuardedBuffer(M.shape).upload(M) as dM:
        with pytest.raises(emme.EmmeError):
            ctx.trace_secant_folded((1, 4), None, None,
                                    device_ptrs=(dM.ptr, Mo.ctypes.data, dw.ctypes.data, tr.ctypes.data, info.ctypes.data))
        dM.assert_unchanged(M)
        dM.assert_guards_intact()


@pytest.mark.parametrize("n", [30, 258])
def test_device_form(ctx, n):
    """Device operands: the inputs are unchanged, nothing beside the outputs is written, the bits are the host form's."""
    nb = 5
    M, Mo, dw, _ = _inputs(n, nb)
    tr_h, info_h = ctx.trace_secant_folded(M, Mo, dw)
    with GuardedBuffer(M.shape).upload(M) as dM, GuardedBuffer(Mo.shape).upload(Mo) as dO, \
            GuardedBuffer((nb,), matrix_bytes=16).upload(dw) as dD, GuardedBuffer((nb,), matrix_bytes=16) as dT, \
            GuardedBuffer((nb,), np.int32, matrix_bytes=4) as dI:
        ctx.trace_secant_folded((nb, n), None, None, device_ptrs=(dM.ptr, dO.ptr, dD.ptr, dT.ptr, dI.ptr))
        for buf, a in ((dM, M), (dO, Mo), (dD, dw)):
            buf.assert_unchanged(a)
        for buf in (dM, dO, dD, dT, dI):
            buf.assert_guards_intact()
        dT.assert_fully_written()
        dI.assert_fully_written()
        assert dT.read().tobytes() == tr_h.tobytes() and np.array_equal(dI.read(), info_h)


def test_step_on_the_fills(emme, ctx):
    """N = 24, mirrored fills at two omegas: the folded step on the device's own M, M_old against numpy."""
    w0 = np.array([-0.8 + 0.25j, -0.6 + 0.3j])
    dw = 0.01 * w0
    Mo = ctx.assemble(w0)
    M = ctx.assemble(w0 + dw)
    assert ctx.mirror_pairs() == 1 and ctx.fill_kernel_symbol().startswith("k_assemble_dense")
    ref = np.array([np.trace(np.linalg.solve(M[b], (M[b] - Mo[b]) / dw[b])) for b in range(2)])
    tr, info = ctx.trace_secant_folded(M, Mo, dw)
    assert (info == 0).all()
    err = np.abs(tr - ref) / np.abs(ref)
    bar, err_u = _bar(ctx, M, Mo, dw, ref)
    print(f"folded step on the fills N=24: err {err}, unfolded {err_u}")
    assert (err <= bar).all(), (err, bar)


_ORACLE_ROOTS = {}


def _oracle_roots(oracle, n):
    if n not in _ORACLE_ROOTS:
        d = example_tokamak(npoints=n)
        po = oracle.params(d)
        out = [oracle.solve_root(po, complex(g)) for g in GUESSES]
        conv = np.array([len(its) <= d["iteration_step_limit"] and np.isfinite(r) for r, its, _, _ in out])
        _ORACLE_ROOTS[n] = (np.array([r for r, _, _, _ in out]), conv)
    return _ORACLE_ROOTS[n]


def _search(emme, d, guesses, fold, **options):
    with emme.Context(emme.params_from_dict(d), lu_fold=fold, **options) as c:
        assert c.lu_fold() == fold
        roots, iters, info = c.solve_roots(guesses)
        return roots, iters, info, c.last_folded_steps()


@pytest.mark.parametrize("n", [24, 32])
def test_search_folded_against_unfolded(emme, oracle, n):
    d = example_tokamak(npoints=n)
    r1, it1, in1, steps1 = _search(emme, d, GUESSES, 1)
    r0, it0, in0, steps0 = _search(emme, d, GUESSES, 0)
    assert steps1 > 0 and steps0 == 0, (steps1, steps0)
    assert np.array_equal(in1, in0), (in1, in0)
    assert np.array_equal(it1, it0), (it1, it0)
    rel = np.abs(r1 - r0) / np.abs(r0)
    print(f"search N={n}: {steps1} folded steps, roots folded against unfolded {rel.max():.3g}")
    assert (rel <= 1e-9).all(), rel
    ro, conv = _oracle_roots(oracle, n)
    assert conv.any()
    ok = conv & (in1 == 0)
    assert np.array_equal(ok, conv), (conv, in1)
    assert (np.abs(r1[ok] - ro[ok]) <= 1e-9 * np.abs(ro[ok])).all(), np.abs(r1 - ro)


ROUTING = {
    "odd": (example_tokamak(npoints=25), {}),
    "theta": (example_tokamak(npoints=24, theta=0.3), {}),
    "stellarator": (example_stellarator(npoints=10), {}),
    "gk31": (example_tokamak(npoints=24, integration_start_points=31), {}),
    "mirror_off": (example_tokamak(npoints=24), {"EMME_MIRROR": "0"}),
    "qr": (example_tokamak(npoints=24, iteration_method="QRSecant"), {}),
}


@pytest.mark.parametrize("case", sorted(ROUTING))
def test_routing_unfolded_cases(emme, monkeypatch, case):
    d, env = ROUTING[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = GUESSES[:4] if case != "stellarator" else np.array([-1.656 + 2.490j, -1.5 + 2.3j])  # (its initial_guess)
    r1, it1, in1, steps1 = _search(emme, d, g, 1)
    r0, it0, in0, steps0 = _search(emme, d, g, 0)
    assert steps1 == 0 and steps0 == 0, (case, steps1)
    assert r1.tobytes() == r0.tobytes() and np.array_equal(it1, it0) and np.array_equal(in1, in0), case


def test_env_override(emme, monkeypatch):
    monkeypatch.setenv("EMME_LU_FOLD", "0")
    with emme.Context(emme.params_from_dict(example_tokamak(npoints=24))) as c:
        assert c.lu_fold() == 0
        c.solve_roots(GUESSES[:4])
        assert c.last_folded_steps() == 0
    monkeypatch.delenv("EMME_LU_FOLD")
    with emme.Context(emme.params_from_dict(example_tokamak(npoints=24))) as c:
        assert c.lu_fold() == 1
        with pytest.raises(emme.EmmeError):
            c.set_lu_fold(2)


@pytest.mark.parametrize("case", ["damped", "minority"])
def test_search_with_unmirrored_fills(emme, case):
    """damped: a depth-4 cache and one damped guess, whose integrals leave the dense fill for the deferred pass.
    minority: one guess of sixteen on the Re omega > 0 side -- a contour class too small to earn a cache, which goes
    through the omega-lane kernel on the full pair list: the steps whose fills include it are not folded.  Either way
    the search ends as the unfolded one does."""
    if case == "damped":
        g, options = np.concatenate([GUESSES[:7], [-0.6 - 0.21j]]), TINY
    else:
        g, options = np.concatenate([GUESSES[:15], [0.6 + 0.25j]]), {}
    d = example_tokamak(npoints=24)
    r1, it1, in1, steps1 = _search(emme, d, g, 1, **options)
    r0, it0, in0, steps0 = _search(emme, d, g, 0, **options)
    print(f"search with unmirrored fills ({case}): {steps1} folded steps, iterations {it1}")
    assert steps0 == 0
    assert np.array_equal(in1, in0), (in1, in0)
    assert np.array_equal(it1, it0), (it1, it0)
    if case == "minority":
        assert steps1 < it1.max(), (steps1, it1)  # the steps the minority chain lived through ran unfolded
