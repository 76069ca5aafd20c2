"""The dense linear-algebra kernels at their dispatch edges.  Every test asserts the kernel it ran through
Context.linstep_kernel_symbol() (what the launcher launched, not what was asked for), on the shared inputs of
linalg_cases.py, against numpy and under the project's existing bars:

  trace_solve      1e-10 max(1, |want|) up to n = 1100, times n / 1100 above
  null_vectors     1 - overlap <= 1e-10
  eigenpair steps  100 n eps kappa (direction, tau, norm), 1e-12 on the residual
  contour_moments  1e-11 relative in norm, 1e-10 on the log-determinant
  qr_secant        1e-9 against oracle.qr_secant
  folded step      max(10 x the unfolded step's error on the same inputs, 1e-13)

The edge between the one-workgroup kernels and the chunked build is where trace_solve_blocked_lds(n) passes 150 KB:
n = 525 | 526 (linalg_cases.lds_edge()); the scans below find it on the device and compare.  Every test prints its worst
error / bar ratio (pytest -s)."""
import numpy as np
import pytest

import linalg_cases as lc
from device_buffers import GuardedBuffer
from linalg_cases import EPS

pytestmark = pytest.mark.gpu

EDGE = lc.lds_edge()
EDGE_ORDERS = [EDGE, EDGE + 1, 1023, 1024, 1025]
BLOCK_EDGES = [15, 16, 17, 31, 32, 33, 47, 48, 49]
EINVAL, EDEVICE, ECONFIG = -1, -3, -5
DOMEGA = [1e-2 * np.exp(0.7j), 1e-7 * np.exp(-2.1j)]  # (test_gpu_contour_eigenpairs.py)
# the 16-guess secant search of test_gpu_fold.py
GUESSES = np.array([-0.7249 + 0.1803j, -0.5617 + 0.3641j, -0.6346 + 0.2529j, -0.9649 + 0.3541j, -0.9199 + 0.2919j,
                    -0.5759 + 0.3225j, -1.0968 + 0.1274j, -0.6073 + 0.2623j, -0.6218 + 0.2523j, -0.8192 + 0.3614j,
                    -0.9182 + 0.2084j, -0.9329 + 0.2795j, -0.9471 + 0.1178j, -0.833 + 0.2163j, -0.7973 + 0.1969j,
                    -0.7679 + 0.1451j])


@pytest.fixture(scope="module")
def ctx(emme):
    from oracle.binding import example_tokamak
    with emme.Context(emme.params_from_dict(example_tokamak(npoints=16))) as c:
        yield c


@pytest.fixture(scope="module")
def n_cu(ctx):
    """Compute units of the context's device, as the library read them from the device properties."""
    n = ctx.compute_units()
    assert n >= 16, n
    return n


@pytest.fixture
def split(ctx):
    """Sets lu_split for a call and puts the default back afterwards."""
    def use(k):
        ctx.set_options(lu_split=k)
    yield use
    ctx.set_options(lu_split=0)


def _say(what, route, ratio):
    print(f"[linalg routes] {what}: {route}: worst error / bar {ratio:.3g}")


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _trace_ratio(n, tr, want):
    return (np.abs(tr - want) / lc.trace_bar(n, want)).max()


# ---- a. the edge, found on the device ---------------------------------------------------------------------------------
def _scan_matrix():
    rng = np.random.default_rng(560)
    A = rng.normal(size=(560, 560)) + 1j * rng.normal(size=(560, 560))
    return A + A.T + 0.5 * 560 ** 0.5 * np.eye(560), rng.normal(size=(560, 560)) + 1j * rng.normal(size=(560, 560))


def test_trace_solve_route_flips_once_at_the_lds_edge(ctx):
    """Leading blocks of one matrix, orders 500 .. 560, lu_split at its default: blocked up to the order the LDS formula
    gives, chunked from the next one on."""
    A, B = _scan_matrix()
    routes = []
    for n in range(500, 561):
        tr, info = ctx.trace_solve(A[:n, :n], B[:n, :n])
        assert info[0] == 0, (n, info)
        routes.append(ctx.linstep_kernel_symbol())
    blocked = [r in (lc.ONE_WG, lc.SPLIT, lc.GROUPED) for r in routes]
    flips = [500 + i for i in range(60) if routes[i] != routes[i + 1]]
    print(f"[linalg routes] trace_solve scan 500..560: {routes[0]} -> {routes[-1]}, flips after {flips}")
    assert flips == [EDGE], (flips, EDGE)
    assert all(blocked[:EDGE - 500 + 1]) and all(r == lc.CHUNKED for r in routes[EDGE - 500 + 1:]), routes
    assert routes[0] == lc.SPLIT  # (one matrix of order >= 384: eight workgroups, look-ahead)


def test_null_vectors_route_flips_once_at_the_lds_edge(ctx):
    A, _ = _scan_matrix()
    routes = []
    for n in range(500, 561):
        v, info = ctx.null_vectors(A[:n, :n])
        assert info[0] == 0, (n, info)
        routes.append(ctx.linstep_kernel_symbol())
        assert ctx.last_lu_slices() == 1
    flips = [500 + i for i in range(60) if routes[i] != routes[i + 1]]
    print(f"[linalg routes] null_vectors scan 500..560: {routes[0]} -> {routes[-1]}, flips after {flips}")
    assert flips == [EDGE], (flips, EDGE)
    assert routes[0] == lc.LU_INPLACE and routes[-1] == lc.CHUNKED


# ---- b. both sides of every edge ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGE_ORDERS)
def test_trace_solve_both_sides(ctx, split, n_cu, n):
    """lu_split 1, 2 and 8 on three matrices: the route of each, the project's bar, and the same bits wherever the
    existing tests promise them -- across every split at a blocked order, across the workgroup counts of the chunked
    build (one workgroup per matrix is the unblocked kernel there: same numbers, other rounding)."""
    A, B, want = lc.shifted_symmetric(n)
    gmin = ctx.options().lu_group_min_n
    out = {}
    for k in (1, 2, 8):
        split(k)
        tr, info = ctx.trace_solve(A, B)
        route = ctx.linstep_kernel_symbol()
        assert route == lc.expected_trace_route(n, lc.lu_workgroups(n, 3, n_cu, k), gmin), (n, k, route)
        assert ctx.last_lu_workgroups() == (1 if route in (lc.ONE_WG, lc.UNBLOCKED) else k), (n, k)
        assert (info == 0).all(), (n, k, info)
        ratio = _trace_ratio(n, tr, want)
        _say(f"trace_solve n={n} lu_split={k}", route, ratio)
        assert ratio <= 1.0, (n, k, tr, want)
        out[k] = (tr, route)
    if n <= EDGE:
        assert {out[k][1] for k in out} == {lc.ONE_WG, lc.GROUPED if 0 < gmin <= n else lc.SPLIT, lc.SPLIT}
        assert _bits(out[1][0]) == _bits(out[2][0]) == _bits(out[8][0])
    elif n <= 1024:
        assert _bits(out[2][0]) == _bits(out[8][0])
    else:
        assert _bits(out[1][0]) == _bits(out[2][0]) == _bits(out[8][0])  # one kernel whatever the option says


@pytest.mark.parametrize("n", [2047, 2048])
def test_trace_solve_at_the_largest_order(ctx, n):
    """One matrix through the unblocked kernel at the order where its two pivot rows take all 64 KB of LDS."""
    A, B, want = lc.shifted_symmetric(n, nb=1)
    tr, info = ctx.trace_solve(A, B)
    assert ctx.linstep_kernel_symbol() == lc.UNBLOCKED and ctx.last_lu_workgroups() == 1
    assert info[0] == 0
    ratio = _trace_ratio(n, tr, want)
    _say(f"trace_solve n={n}", lc.UNBLOCKED, ratio)
    assert ratio <= 1.0, (n, tr, want)


@pytest.mark.parametrize("n", EDGE_ORDERS + BLOCK_EDGES)
def test_null_vectors_both_sides(ctx, n):
    M, want = lc.null_family(n)
    v, info = ctx.null_vectors(M)
    route = ctx.linstep_kernel_symbol()
    assert route == lc.expected_lu_route(n) and ctx.last_lu_slices() == 1, (n, route)
    assert (info == 0).all(), (n, info)
    err = np.array([1.0 - lc.overlap(v[b], want[b]) for b in range(len(M))])
    _say(f"null_vectors n={n}", route, err.max() / 1e-10)
    assert np.abs(np.linalg.norm(v, axis=1) - 1.0).max() <= 1e-12
    assert (err <= 1e-10).all(), (n, err)


def _check_eigpair(n, M, Bm, vin_of, out, kappa, items):
    vd, tau, resid, info = out
    worst = 0.0
    for b in items:
        vin = vin_of(b)
        vin = vin / np.linalg.norm(vin)
        u = np.linalg.solve(M[b], Bm(b) @ vin)
        e_dir, e_tau, e_nrm, e_res = lc.eigpair_errors(M[b], Bm(b), vin, u, vd[b], tau[b], resid[b])
        bound = 100.0 * n * EPS * kappa[b]
        assert e_dir <= bound and e_tau <= bound and e_nrm <= bound, (n, b, e_dir, e_tau, e_nrm, bound)
        assert e_res <= 1e-12, (n, b, e_res)
        worst = max(worst, e_dir / bound, e_tau / bound, e_nrm / bound, e_res / 1e-12)
    return worst


@pytest.mark.parametrize("secant", [False, True])
@pytest.mark.parametrize("n", EDGE_ORDERS)
def test_eigenpair_steps_both_sides(ctx, n, secant):
    M, Mp, v, kappa = lc.constructed(n)
    s = lc.start_vector(n)
    dw = np.array(DOMEGA)
    Mold = M - dw[:, None, None] * Mp if secant else None
    # (the secant in numpy: the difference of the two matrices as they are held, over domega)
    Bm = (lambda b: (M[b] - Mold[b]) / dw[b]) if secant else (lambda b: Mp[b])
    worst = 0.0
    for have_v in (1, 0):
        vv = v if have_v else None
        out = ctx.eigenpair_secant_step(M, Mold, dw, vv) if secant else ctx.eigenpair_step(M, Mp, vv)
        route = ctx.linstep_kernel_symbol()
        assert route == lc.expected_lu_route(n) and ctx.last_lu_slices() == 1, (n, route)
        assert (out[3] == 0).all(), (n, have_v, out[3])
        vin_of = (lambda b: v[b]) if have_v else (lambda b: np.linalg.solve(M[b], s))
        worst = max(worst, _check_eigpair(n, M, Bm, vin_of, out, kappa, range(2)))
    _say(f"eigenpair_{'secant_' if secant else ''}step n={n}", route, worst)


def _check_contour(ctx, n, M, z, w, V, route):
    L = V.shape[1]
    A0, A1, ld, info = ctx.contour_moments(M, z, w, L, V=V)
    got = ctx.linstep_kernel_symbol()
    assert got == route and ctx.last_lu_slices() == 1, (n, got)
    assert (info == 0).all(), (n, info)
    R0, R1 = lc.moments_of(np.linalg.solve(M, np.broadcast_to(V, (len(M), n, L))), z, w)
    sgn, lab = np.linalg.slogdet(M)
    errs = lc.contour_errors(A0, A1, ld, R0, R1, sgn, lab)
    _say(f"contour_moments n={n} L={L}", got, max(errs))
    assert max(errs) <= 1.0, (n, errs)


@pytest.mark.parametrize("n", EDGE_ORDERS + BLOCK_EDGES)
def test_contour_moments_both_sides(ctx, n):
    M, z, w, V = lc.contour_inputs(n)
    _check_contour(ctx, n, M, z, w, V, lc.expected_lu_route(n))


@pytest.mark.parametrize("n", [255, 256, 257, 511, 512, 513, 1023, 1024])
def test_qr_secant_register_width_edges(ctx, oracle, n):
    """The three register-width variants of k_qr_secant on both sides of 256 | 257 and 512 | 513, and the widest with
    every per-thread slot in use (1024): generic and nearly singular, against the same LAPACK sequence on the host."""
    A, B = lc.qr_inputs(n)
    q, info = ctx.qr_secant(A, B)
    assert (info == 0).all(), (n, info)
    worst = 0.0
    for b in range(2):
        dw, i_or = oracle.qr_secant(A[b], B[b])
        assert i_or == 0
        err = abs(-1.0 / q[b] - dw) / abs(dw)
        worst = max(worst, err / 1e-9)
        assert err <= 1e-9, (n, b, -1.0 / q[b], dw)
    _say(f"qr_secant n={n}", "k_qr_secant", worst)


# ---- c. the chunked build falls back to the unblocked kernel when its grid cannot be resident ------------------------
def test_chunked_falls_back_to_unblocked(ctx, split, n_cu):
    """n = edge + 1, sixteen workgroups per matrix and one matrix more than the device holds that way: the launcher
    must see that the grid cannot be resident and the step must run unblocked -- no time-out codes, numpy's traces, the
    singular matrix reported at its own column on both routes and its neighbours untouched by it."""
    n, nb = EDGE + 1, n_cu // 16 + 1
    A, B, want = lc.shifted_symmetric(n, nb=nb)
    sing, col = nb // 2, n // 3
    As = A.copy()
    As[sing, :, col] = 0.0
    ok = np.arange(nb) != sing
    infos = {}
    for k, route in ((16, lc.UNBLOCKED), (2, lc.CHUNKED)):
        split(k)
        tr, info = ctx.trace_solve(A, B)
        got = ctx.linstep_kernel_symbol()
        assert got == route, (k, got)
        assert ctx.last_lu_workgroups() == (1 if k == 16 else 2)
        assert not (info == EDEVICE).any() and (info == 0).all(), (k, info)
        ratio = _trace_ratio(n, tr, want)
        _say(f"trace_solve n={n} x {nb} lu_split={k}", got, ratio)
        assert ratio <= 1.0, (k, tr, want)
        trs, infos[k] = ctx.trace_solve(As, B)
        assert ctx.linstep_kernel_symbol() == route
        assert infos[k][sing] == col + 1 and (infos[k][ok] == 0).all(), (k, infos[k])
        assert np.isnan(trs[sing].real) and np.isnan(trs[sing].imag)
        assert _bits(trs[ok]) == _bits(tr[ok]), k
    assert np.array_equal(infos[16], infos[2])


# ---- d. slices of lu_factor_batch --------------------------------------------------------------------------------------
class _Slices:
    """n = edge + 1 and two matrices more than one slice of the chunked factorisation holds (half the compute units):
    the P D M_0 batch, the same batch reversed, and the reversed batch with an exactly singular matrix in its second
    slice (position nb - 1 holds item 0: column `col` zero)."""

    def __init__(self, n_cu):
        self.n, self.nb = EDGE + 1, n_cu // 2 + 2
        self.first = n_cu // 2  # items per slice
        self.F = lc.pdm_family(self.n, self.nb)
        self.M = self.F.M
        self.Mrev = np.ascontiguousarray(self.M[::-1])
        self.col = self.n // 2
        self.check = sorted({0, 1, self.first - 2, self.first - 1} | set(range(self.first, self.nb)))

    def make_singular(self):
        """Position nb - 1 of the reversed batch (item 0) gets a zero column; returns the position."""
        self.Mrev[self.nb - 1][:, self.col] = 0.0
        return self.nb - 1

    def restore(self):
        self.Mrev[self.nb - 1] = self.M[0]


@pytest.fixture(scope="module")
def slices(n_cu):
    return _Slices(n_cu)


def _two_chunked_slices(ctx):
    assert ctx.linstep_kernel_symbol() == lc.CHUNKED and ctx.last_lu_workgroups() == 2
    assert ctx.last_lu_slices() == 2


def test_null_vectors_second_slice(ctx, slices):
    """Every item against its base matrix's null vector (neighbours have different ones), the same bits per item with
    the batch reversed -- k_trace_solve_blocked<true, true> and k_null_iterate give a matrix its own workgroups, fixed
    reduction orders and no atomics, so an item's result does not depend on its position or its slice -- and a singular
    matrix in the second slice reported at its own column with its neighbours' bits unchanged."""
    S, F = slices, slices.F
    v, info = ctx.null_vectors(S.M)
    _two_chunked_slices(ctx)
    assert (info == 0).all(), info
    err = np.array([1.0 - lc.overlap(v[b], F.want[b % 2]) for b in range(S.nb)])
    _say(f"null_vectors n={S.n} x {S.nb} (2 slices)", lc.CHUNKED, err.max() / 1e-10)
    assert (err <= 1e-10).all(), (np.flatnonzero(err > 1e-10), err.max())
    vr, infor = ctx.null_vectors(S.Mrev)
    _two_chunked_slices(ctx)
    assert (infor == 0).all()
    for b in range(S.nb):
        assert _bits(vr[S.nb - 1 - b]) == _bits(v[b]), b
    try:
        p = S.make_singular()
        vs, infos = ctx.null_vectors(S.Mrev)
    finally:
        S.restore()
    _two_chunked_slices(ctx)
    assert infos[p] == S.col + 1 and (np.delete(infos, p) == 0).all(), infos
    assert np.isnan(vs[p]).all()
    assert _bits(np.delete(vs, p, axis=0)) == _bits(np.delete(vr, p, axis=0))


@pytest.mark.parametrize("secant", [False, True])
def test_eigenpair_step_second_slice(ctx, slices, secant):
    """Item b steps on (M_b, M' = M_{nb-1-b}) (secant: M_old = M_{nb-1-b}), so the second operand of the forward call
    is the reversed batch and the other way round.  Checked against numpy: items 0 and 1, the last two of the first
    slice and the whole second slice; kappa is the base matrix's."""
    S, F = slices, slices.F
    n, nb = S.n, S.nb
    rng = np.random.default_rng(n)
    v = rng.normal(size=(nb, n)) + 1j * rng.normal(size=(nb, n))
    v /= np.linalg.norm(v, axis=1)[:, None]
    dw = np.resize(np.array(DOMEGA), nb)
    step = (lambda A, B, d, x: ctx.eigenpair_secant_step(A, B, d, x)) if secant else (lambda A, B, d, x: ctx.eigenpair_step(A, B, x))
    out = step(S.M, S.Mrev, dw, v)
    _two_chunked_slices(ctx)
    assert (out[3] == 0).all(), out[3]
    Bm = (lambda b: (S.M[b] - S.Mrev[b]) / dw[b]) if secant else (lambda b: S.Mrev[b])
    worst = 0.0
    for b in S.check:
        u = F.solve(b, Bm(b) @ v[b])
        errs = lc.eigpair_errors(S.M[b], Bm(b), v[b], u, out[0][b], out[1][b], out[2][b])
        bound = 100.0 * n * EPS * F.kappa[b % 2]
        assert max(errs[:3]) <= bound and errs[3] <= 1e-12, (b, errs, bound)
        worst = max(worst, max(errs[:3]) / bound, errs[3] / 1e-12)
    _say(f"eigenpair_{'secant_' if secant else ''}step n={n} x {nb} (2 slices)", lc.CHUNKED, worst)
    rev = step(S.Mrev, S.M, dw[::-1].copy(), v[::-1].copy())
    _two_chunked_slices(ctx)
    for a, r in zip(out, rev):
        assert _bits(r[::-1]) == _bits(a)
    try:
        p = S.make_singular()
        sing = step(S.Mrev, S.M, dw[::-1].copy(), v[::-1].copy())
    finally:
        S.restore()
    _two_chunked_slices(ctx)
    assert sing[3][p] == S.col + 1 and (np.delete(sing[3], p) == 0).all(), sing[3]
    assert np.isnan(sing[0][p]).all() and np.isnan(sing[1][p]) and np.isnan(sing[2][p])
    for r, s in zip(rev[:3], sing[:3]):
        assert _bits(np.delete(s, p, axis=0)) == _bits(np.delete(r, p, axis=0))


def test_contour_moments_second_slice(ctx, slices):
    """The moments are sums over every node, so one wrong item anywhere breaks the 1e-11 bar; the log-determinants are
    per item: numpy's for the checked items, the same bits with the batch reversed (the moments are summed in node
    order, so theirs differ), and with a singular node in the second slice that node alone drops out."""
    S, F = slices, slices.F
    n, nb, L = S.n, S.nb, 8
    rng = np.random.default_rng(n + 1)
    cplx = lambda *s: rng.normal(size=s) + 1j * rng.normal(size=s)
    z, w, V = cplx(nb), cplx(nb), cplx(n, L)
    R0, R1 = F.moments(V, z, w)
    sgn, lab = np.linalg.slogdet(S.M[S.check])
    A0, A1, ld, info = ctx.contour_moments(S.M, z, w, L, V=V)
    _two_chunked_slices(ctx)
    assert (info == 0).all(), info
    errs = lc.contour_errors(A0, A1, ld[S.check], R0, R1, sgn, lab)
    _say(f"contour_moments n={n} x {nb} (2 slices)", lc.CHUNKED, max(errs))
    assert max(errs) <= 1.0, errs
    zr, wr = z[::-1].copy(), w[::-1].copy()
    B0, B1, ldr, infor = ctx.contour_moments(S.Mrev, zr, wr, L, V=V)
    _two_chunked_slices(ctx)
    assert (infor == 0).all() and _bits(ldr[::-1]) == _bits(ld)
    errs = lc.contour_errors(B0, B1, ldr[::-1][S.check], R0, R1, sgn, lab)
    _say(f"contour_moments n={n} x {nb} (2 slices, reversed)", lc.CHUNKED, max(errs))
    assert max(errs) <= 1.0, errs
    try:
        p = S.make_singular()
        C0, C1, lds, infos = ctx.contour_moments(S.Mrev, zr, wr, L, V=V)
    finally:
        S.restore()
    _two_chunked_slices(ctx)
    assert infos[p] == S.col + 1 and (np.delete(infos, p) == 0).all(), infos
    assert np.isneginf(lds[p].real) and _bits(np.delete(lds, p)) == _bits(np.delete(ldr, p))
    Q0, Q1 = F.moments(V, z, w, items=range(1, nb))  # (position p of the reversed batch is item 0)
    errs = lc.contour_errors(C0, C1, ld[S.check][1:], Q0, Q1, sgn[1:], lab[1:])
    _say(f"contour_moments n={n} x {nb} (2 slices, one singular)", lc.CHUNKED, max(errs))
    assert max(errs) <= 1.0, errs


# ---- e. the folded step over its whole range ---------------------------------------------------------------------------
FLOOR = 1e-13


def _fold_bar(ctx, n, M, Mo, dw, ref):
    """max(10 x the unfolded step's relative error on the same inputs, 1e-13) per item (test_gpu_fold.py)."""
    tr_u, info_u = ctx.trace_solve(M, (M - Mo) / dw[:, None, None])
    assert (info_u == 0).all()
    err_u = np.abs(tr_u - ref) / np.abs(ref)
    return np.maximum(10.0 * err_u, FLOOR), err_u


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("n", [316, 512, 766, 768, 770, 1048, 1050] + [2 * h for h in BLOCK_EDGES])
def test_folded_step_whole_range(ctx, n_cu, n, nb):
    M, Mo, dw, ref = lc.fold_inputs(n, nb)
    tr, info = ctx.trace_secant_folded(M, Mo, dw)
    route = ctx.linstep_kernel_symbol()  # (of the half problems: order n / 2, two per chain)
    m = n // 2
    assert route == lc.expected_trace_route(m, lc.lu_workgroups(m, 2 * nb, n_cu), ctx.options().lu_group_min_n), (n, route)
    assert (info == 0).all(), info
    err = np.abs(tr - ref) / np.abs(ref)
    bar, err_u = _fold_bar(ctx, n, M, Mo, dw, ref)
    unfolded = ctx.linstep_kernel_symbol()
    assert unfolded == lc.expected_trace_route(n, lc.lu_workgroups(n, nb, n_cu), ctx.options().lu_group_min_n), (n, unfolded)
    _say(f"folded step n={n} nb={nb} (err {err.max():.2g}, unfolded {err_u.max():.2g} by {unfolded})", route, (err / bar).max())
    assert (err <= bar).all(), (n, nb, err, bar)


@pytest.mark.parametrize("n", [768, 1050])
def test_folded_step_same_bits_under_lu_split(ctx, split, n):
    M, Mo, dw, _ = lc.fold_inputs(n, 3)
    out, routes = {}, {}
    for k in (0, 1, 4):
        split(k)
        out[k] = ctx.trace_secant_folded(M, Mo, dw)
        routes[k] = ctx.linstep_kernel_symbol()
    assert routes[1] == lc.ONE_WG and routes[4] == lc.SPLIT and routes[0] == lc.SPLIT, routes
    for k in (1, 4):
        assert _bits(out[k][0]) == _bits(out[0][0]) and np.array_equal(out[k][1], out[0][1]), k


def test_folded_step_refuses_orders_above_1050(emme, ctx):
    z = np.zeros((1, 2 * EDGE + 2, 2 * EDGE + 2), dtype=np.complex128)
    with pytest.raises(emme.EmmeError) as e:
        ctx.trace_secant_folded(z, z, [0.1])
    assert e.value.code == ECONFIG


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("n,k", [(16, 5), (130, 16), (130, 40)])
def test_folded_step_reports_the_singular_half_and_column(ctx, n, k, odd):
    """Item 1 has an exactly zero row and column k in its even (odd) half: info is that column, counted from 1, plus
    the half order for the odd half; the neighbours keep their bits."""
    M, Mo, dw, _ = lc.fold_inputs(n, 3)
    clean = ctx.trace_secant_folded(M, Mo, dw)
    Ms = M.copy()
    Ms[1] = lc.with_singular_half(M[1], k, odd)
    tr, info = ctx.trace_secant_folded(Ms, Mo, dw)
    assert info[1] == k + 1 + (n // 2 if odd else 0), (info, k, odd)
    assert np.isnan(tr[1].real) and np.isnan(tr[1].imag)
    assert info[0] == 0 and info[2] == 0
    assert _bits(tr[[0, 2]]) == _bits(clean[0][[0, 2]])


@pytest.mark.parametrize("n", [16, 130])
def test_folded_step_reports_a_singular_rank2_system(ctx, n):
    """Both halves regular and det K = 0 bit for bit (linalg_cases.singular_k_matrix): info = n + 1.  The unfolded step
    on the same matrix stops at its last column."""
    M, Mo, dw, _ = lc.fold_inputs(n, 3)
    Ms, Mos = M.copy(), Mo.copy()
    Ms[1], Mos[1] = lc.singular_k_matrix(n)
    tr, info = ctx.trace_secant_folded(Ms, Mos, dw)
    assert info[1] == n + 1, info
    assert np.isnan(tr[1].real) and np.isnan(tr[1].imag)
    assert info[0] == 0 and info[2] == 0
    clean = ctx.trace_secant_folded(M, Mo, dw)
    assert _bits(tr[[0, 2]]) == _bits(clean[0][[0, 2]])
    _, info_u = ctx.trace_solve(Ms, (Ms - Mos) / dw[:, None, None])
    assert info_u[1] == n and info_u[0] == 0 and info_u[2] == 0, info_u


# At N = 528 chains 6 and 12 of the sixteen use every step without reaching a root (chain 12 walks on in steps of 1e-5
# |omega|), so where they stop follows the rounding of the route and is no root to compare: that search starts from the
# other fourteen guesses, and every one of its chains has to converge.
SEARCHES = {256: GUESSES, 528: np.delete(GUESSES, [6, 12])}


def _search(emme, d, guesses, fold):
    with emme.Context(emme.params_from_dict(d), lu_fold=fold) as c:
        roots, iters, info = c.solve_roots(guesses)
        return roots, iters, info, c.last_folded_steps(), c.linstep_kernel_symbol()


@pytest.mark.parametrize("npoints", sorted(SEARCHES))
def test_search_folded_against_unfolded_at_size(emme, npoints):
    """The headline geometry at N = 256 (its 16 guesses), and N = 528, where the half order 264 is blocked and the full
    order chunked: the folded search against the unfolded one on the same build (lu_fold = 0: the unfolded step bit for
    bit), as test_search_folded_against_unfolded asserts it -- same info, same iteration counts, every root within
    1e-9.  At N = 528 every chain must also have converged.  (The oracle's search is not the reference at these sizes:
    a chain of it takes seconds of every host core at N = 256, a minute and a half for the sixteen.)"""
    import bench
    d, guesses = bench.workload_dict(npoints), SEARCHES[npoints]
    r1, it1, in1, steps1, route1 = _search(emme, d, guesses, 1)
    r0, it0, in0, steps0, route0 = _search(emme, d, guesses, 0)
    assert steps1 > 0 and steps0 == 0, (steps1, steps0)
    assert np.array_equal(in1, in0), (in1, in0)
    assert np.array_equal(it1, it0), (it1, it0)
    assert not (in1 == EDEVICE).any()
    rel = np.abs(r1 - r0) / np.abs(r0)
    _say(f"search N={npoints}: {len(guesses)} chains, {steps1} folded steps, unfolded by {route0}", route1, rel.max() / 1e-9)
    assert (rel <= 1e-9).all(), rel
    if npoints > EDGE:
        assert (in1 == 0).all() and (it1 <= d["iteration_step_limit"]).all(), (in1, it1)
        assert route0 == lc.CHUNKED and route1 in (lc.ONE_WG, lc.SPLIT, lc.GROUPED), (route0, route1)


# ---- f. refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call,n,code", [("trace_solve", 2049, EINVAL), ("qr_secant", 1025, ECONFIG)])
def test_refusals_launch_nothing(emme, ctx, call, n, code):
    with GuardedBuffer((1, n, n), matrix_bytes=16 * n) as dA, GuardedBuffer((1, n, n), matrix_bytes=16 * n) as dB:
        with pytest.raises(emme.EmmeError) as e:
            getattr(ctx, call)((1, n), None, a_device_ptr=dA.ptr, b_device_ptr=dB.ptr)
        assert e.value.code == code, e.value
        dA.assert_untouched()
        dB.assert_untouched()
