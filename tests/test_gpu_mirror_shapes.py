"""Mirror-image pairs for electromagnetic and GK31 contexts (emme_ctx_set_mirror_shapes): with
MIRROR_SHAPES_ALL the tiled cache of such a context on a symmetric grid is laid out over one pair of every couple
(i, j) / (N-1-j, N-1-i) and k_assemble_dense<1, PTS, NM> and the deferred kernels write both entries in the block of
the integral's moment.  Routing, entries and interval counts against the oracle and against the unmirrored fill, the
deferred pass, the cache size, the secant search, which steps fold, and the hand-over to cached derivative fills --
the checks of test_gpu_mirror_pairs.py for the three shapes it pins as unmirrored by default.

N = 24 and 25: both parities of N (self-mirror pairs on alternate diagonals) and a ragged last tile (144 and 156 =
9 x 16 + 12 half pairs).  At every omega below the oracle's mirror couples have equal interval counts (checked on the
CPU: assemble(..., want_counts=True), 0 mismatches of 276 / 300) and kappa's that differ by <= 3.2e-14 of the block's
largest."""
import numpy as np
import pytest

from oracle.binding import example_stellarator, example_tokamak

pytestmark = pytest.mark.gpu

TOL_M = 1e-10  # test_gpu_parity.py
WS_TOK = np.array([-0.8 + 0.25j, -1.2 + 0.05j, -0.5 + 0.4j, -0.6 - 0.21j])
WS_STELL = np.array([-1.656 + 2.49j, -1 + 1j, -0.8 + 0.25j, -0.5 - 0.2j])
# name -> (input of npoints and overrides, omegas; the last one is the damped omega of the deferred pass)
SHAPES = {
    "em15": (lambda n, **kw: example_tokamak(npoints=n, beta_e=0.02, **kw), WS_TOK),
    "gk31": (lambda n, **kw: example_tokamak(npoints=n, integration_start_points=31, **kw), WS_TOK),
    "stellarator": (lambda n, **kw: example_stellarator(npoints=n, **kw), WS_STELL),
}
ASYMMETRIC = {"em15": dict(theta=0.3), "gk31": dict(theta=0.3), "stellarator": dict(alpha_0=0.3)}
# The shallowest caches (test_gpu_mirror_pairs.py).  This budget holds the full tree to depth 4 and the subtree to depth
# 7 for the 8-KB blocks of GK15 and to depth 3 / 5 for the 16-KB blocks of GK31; the reference's trees at the damped
# omegas reach depth 8 (tokamak, electromagnetic GK15), 7 (tokamak GK31) and 6 (stellarator): oracle_depth_hist.
TINY = dict(node_cache_gb=0.05, cache_min_depth=1)
# test_gpu_mirror_pairs.py: the oracle's solve_root converges from each of these at npoints = 24 -- electrostatic GK31:
# the first eight, 5 .. 10 iterates to -0.56672+0.24013i; electromagnetic GK15: the second to the eighth, 7 .. 9 iterates
# to -0.63179+0.58488i (the first wanders for 21 steps)
GUESSES = np.array([-0.7249 + 0.1803j, -0.5617 + 0.3641j, -0.6346 + 0.2529j, -0.9649 + 0.3541j, -0.9199 + 0.2919j,
                    -0.5759 + 0.3225j, -1.0968 + 0.1274j, -0.6073 + 0.2623j])
# stellarator, npoints = 24, iteration_step_limit = 20: 16 .. 18 iterates to -0.46297+0.57078i
GUESSES_STELL = np.array([-1.656 + 2.49j, -1.5 + 2.3j, -1.6 + 2j, -1.2 + 2.4j])
SEARCHES = {
    "gk31": (lambda: example_tokamak(npoints=24, integration_start_points=31), GUESSES),
    "em15": (lambda: example_tokamak(npoints=24, beta_e=0.02), GUESSES[1:]),
    "stellarator": (lambda: example_stellarator(npoints=24, iteration_step_limit=20), GUESSES_STELL),
}


def _ctx(emme, d, shapes_all, mirror=None, **options):
    ctx = emme.Context(emme.params_from_dict(d), **options)
    if shapes_all:
        ctx.set_mirror_shapes(emme.MIRROR_SHAPES_ALL)
    if mirror is not None:
        ctx.set_mirror_pairs(mirror)
    return ctx


def _half_pairs(n):
    return (n * (n - 1) // 2 + n // 2) // 2


_ORACLE = {}


def _oracle_at(oracle, shape, n):
    """(matrices, interval totals, W dx, dx) of the oracle, computed once per (shape, n)."""
    key = (shape, n)
    if key not in _ORACLE:
        make, ws = SHAPES[shape]
        d = make(n)
        po = oracle.params(d)
        out = [oracle.assemble(po, complex(w)) for w in ws]
        _, dx = oracle.grid(d["length"], n)
        _ORACLE[key] = (np.array([m for m, _ in out]), np.array([t for _, t in out]), oracle.weights(n) * dx, dx)
    return _ORACLE[key]


def _kappas(M, n, wdx, dx):
    """kappa of every pair i < j per block, recovered from the strict upper triangles: A = -kappa_0 W dx, and on
    electromagnetic matrices B = kappa_1 dx, D = kappa_2 dx (include/solver.h:448-453, 472-509)."""
    iu = np.triu_indices(n, 1)
    out = {"A": M[:n, :n][iu] / (-wdx[iu])}
    if M.shape[-1] == 2 * n:
        out["B"] = M[:n, n:][iu] / dx
        out["D"] = M[n:, n:][iu] / dx
    return out, iu


def _mirror_discrepancy(M, n, wdx, dx):
    """per block, max |kappa_ij - kappa_mirror| / max |kappa|: what the reference's own arithmetic leaves between the
    two integrals of a couple."""
    ks, iu = _kappas(M, n, wdx, dx)
    out = {}
    for name, k in ks.items():
        full = np.zeros((n, n), complex)
        full[iu] = k
        out[name] = np.abs(k - full[n - 1 - iu[1], n - 1 - iu[0]]).max() / np.abs(k).max()
    return out


def _unwritten(M, n):
    """the entries no pair writes: the diagonals of A and D (and of B and its transpose)"""
    i = np.arange(n)
    if M.shape[-1] == n:
        return M[..., i, i]
    return np.stack([M[..., i, i], M[..., i + n, i + n], M[..., i, i + n], M[..., i + n, i]], axis=-1)


def _compare(emme, oracle, shape, n, label, **options):
    make, ws = SHAPES[shape]
    d = make(n)
    Mo, tot, wdx, dx = _oracle_at(oracle, shape, n)
    out = {}
    for on in (True, False):
        with _ctx(emme, d, on, **options) as ctx:
            ctx.profile(True)
            assert ctx.mirror_pairs() == int(on)
            M, iv = ctx.assemble(ws, want_intervals=True)
            assert ctx.fill_kernel_symbol().startswith("k_assemble_dense") and ctx.mirror_pairs() == int(on)
            out[on] = (M, iv, ctx.last_deferred(), ctx.profile_read())
    for on, (M, iv, _, _) in out.items():
        # counts: the reference algorithm's, mirrored or not
        assert np.array_equal(iv, tot), (label, on, iv, tot)
        for b in range(len(ws)):
            err = np.abs(M[b] - Mo[b]).max() / np.abs(Mo[b]).max()
            assert err <= TOL_M, (label, on, ws[b], err)
            assert np.array_equal(M[b], M[b].T), (label, on, ws[b])
    assert _unwritten(out[True][0], n).tobytes() == _unwritten(out[False][0], n).tobytes(), label
    # on against off, per block: within 100 x what the oracle's own mirror pairs differ by in that block (the device's
    # exp / sincos are not the host's)
    for b in range(len(ws)):
        ref = _mirror_discrepancy(Mo[b], n, wdx, dx)
        k_on, _ = _kappas(out[True][0][b], n, wdx, dx)
        k_off, _ = _kappas(out[False][0][b], n, wdx, dx)
        for name in k_on:
            diff = np.abs(k_on[name] - k_off[name]).max() / np.abs(k_off[name]).max()
            ratio = diff / ref[name] if ref[name] > 0 else (0.0 if diff == 0 else np.inf)
            print(f"mirror shapes {shape} {label} N={n} omega={ws[b]} block {name}: on/off {diff:.3g}, "
                  f"oracle mirror discrepancy {ref[name]:.3g}, ratio {ratio:.3g}")
            assert diff <= 100.0 * ref[name], (shape, label, ws[b], name, diff, ref[name])
    return out


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_routing(emme, monkeypatch, shape):
    make, ws = SHAPES[shape]
    d = make(24)
    with _ctx(emme, d, False, mirror=False) as off:
        assert off.mirror_pairs() == 0 and off.mirror_shapes() == emme.MIRROR_SHAPES_ES15
        M_off = off.assemble(ws)
    # without the setter: the unmirrored fill, bit for bit
    with _ctx(emme, d, False) as ctx:
        assert ctx.mirror_shapes() == emme.MIRROR_SHAPES_ES15 and ctx.mirror_pairs() == 0
        assert np.array_equal(ctx.assemble(ws), M_off)
        assert ctx.mirror_pairs() == 0
    with _ctx(emme, d, True) as ctx:
        assert ctx.mirror_shapes() == emme.MIRROR_SHAPES_ALL and ctx.mirror_pairs() == 1
        with pytest.raises(emme.EmmeError):
            ctx.set_mirror_shapes(2)
        M_on = ctx.assemble(ws)
        assert ctx.mirror_pairs() == 1 and ctx.fill_kernel_symbol().startswith("k_assemble_dense")
        with pytest.raises(emme.EmmeError):  # a layout setting: the cache exists
            ctx.set_mirror_shapes(emme.MIRROR_SHAPES_ES15)
        assert ctx.mirror_shapes() == emme.MIRROR_SHAPES_ALL and ctx.mirror_pairs() == 1
    assert np.abs(M_on - M_off).max() <= TOL_M * np.abs(M_off).max()
    # the keyword of Context
    with emme.Context(emme.params_from_dict(d), mirror_shapes=emme.MIRROR_SHAPES_ALL) as ctx:
        assert ctx.mirror_shapes() == emme.MIRROR_SHAPES_ALL and ctx.mirror_pairs() == 1
    # an asymmetric grid never mirrors: theta = 0.3 in the tokamak's tables (g and b lose their symmetry by 4e-2 and
    # 6e-2 of their largest value).  The stellarator's tables do not read theta -- its grid stays symmetric and the
    # context mirrors; alpha_0 = 0.3 is what skews its g (3e-2).
    with _ctx(emme, make(24, **ASYMMETRIC[shape]), True) as ctx:
        assert ctx.mirror_pairs() == 0
    if shape == "stellarator":
        with _ctx(emme, make(24, theta=0.3), True) as ctx:
            assert ctx.mirror_pairs() == 1
    # set_mirror_pairs(False) still switches it off
    with _ctx(emme, d, True, mirror=False) as ctx:
        assert ctx.mirror_pairs() == 0
        assert np.array_equal(ctx.assemble(ws), M_off)
    # a context created for cached derivative fills never mirrors
    with _ctx(emme, d, True, deriv_cached=1) as ctx:
        assert ctx.mirror_pairs() == 0
    # the environment override, read at creation
    monkeypatch.setenv("EMME_MIRROR_SHAPES", "1")
    with _ctx(emme, d, False) as ctx:
        assert ctx.mirror_shapes() == emme.MIRROR_SHAPES_ALL and ctx.mirror_pairs() == 1
        assert np.array_equal(ctx.assemble(ws), M_on)
    monkeypatch.setenv("EMME_MIRROR", "0")
    with _ctx(emme, d, False) as ctx:
        assert ctx.mirror_shapes() == emme.MIRROR_SHAPES_ALL and ctx.mirror_pairs() == 0
        assert np.array_equal(ctx.assemble(ws), M_off)
    monkeypatch.delenv("EMME_MIRROR")
    monkeypatch.delenv("EMME_MIRROR_SHAPES")
    with _ctx(emme, d, False) as ctx:
        assert ctx.mirror_shapes() == emme.MIRROR_SHAPES_ES15 and ctx.mirror_pairs() == 0


@pytest.mark.parametrize("n", [24, 25])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_entries_and_counts(emme, oracle, shape, n):
    _compare(emme, oracle, shape, n, "default", node_cache_gb=8.0)


@pytest.mark.parametrize("shape,n,wide", [("em15", 24, 0), ("em15", 25, 0), ("gk31", 24, 0), ("gk31", 25, 0),
                                          ("gk31", 25, 1), ("stellarator", 24, 0), ("stellarator", 25, 0)])
def test_deferred_pass(emme, oracle, shape, n, wide):
    """A shallow cache: the damped omega's integrals leave it for the list / cooperative kernels, which scatter the
    mirror entries of the integral's moment and count its intervals as the dense fill does; once with dense_wide."""
    out = _compare(emme, oracle, shape, n, f"tiny wide={wide}", dense_wide=wide, **TINY)
    for on, (_, _, deferred, prof) in out.items():
        assert prof.deferred_launches >= 1 and deferred > 0, (on, deferred)
    # undoubled: the mirrored fill defers one integral per couple and moment
    assert out[True][2] < out[False][2]


@pytest.mark.parametrize("n", [24, 25])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_cache_size(emme, shape, n):
    """The cache holds ceil(pairs / 16) tiles of the same intervals: bytes on / off = tiles on / off, exactly."""
    make, ws = SHAPES[shape]
    bytes_ = {}
    for on in (True, False):
        with _ctx(emme, make(n), on, **TINY) as ctx:
            ctx.assemble(ws)  # (one fill: the main part alone -- what grows later depends on the room left)
            bytes_[on] = round(ctx.node_cache_gib() * 2 ** 30)
            geom = ctx.cache_state()[:2]
        bytes_[on, "geom"] = geom
    assert bytes_[True, "geom"] == bytes_[False, "geom"]
    t_on, t_off = (_half_pairs(n) + 15) // 16, (n * (n - 1) // 2 + 15) // 16
    assert bytes_[True] > 0 and bytes_[True] * t_off == bytes_[False] * t_on, (bytes_, t_on, t_off)


@pytest.mark.parametrize("shape", sorted(SEARCHES))
def test_secant_search(emme, shape):
    make, guesses = SEARCHES[shape]
    res = {}
    for on in (True, False):
        with _ctx(emme, make(), on) as ctx:
            res[on] = ctx.solve_roots(guesses)
            assert ctx.mirror_pairs() == int(on)
    (r_on, it_on, info_on), (r_off, it_off, info_off) = res[True], res[False]
    print(f"secant search {shape}: iterations {it_on}, roots on against off "
          f"{(np.abs(r_on - r_off) / np.abs(r_off)).max():.3g}")
    assert (info_on == 0).all() and (info_off == 0).all(), (info_on, info_off)
    assert np.array_equal(it_on, it_off), (it_on, it_off)
    assert (np.abs(r_on - r_off) <= 1e-9 * np.abs(r_off)).all(), np.abs(r_on - r_off).max()


def _search(emme, d, guesses, fold, **options):
    with _ctx(emme, d, True, lu_fold=fold, **options) as c:
        assert c.lu_fold() == fold and c.mirror_pairs() == 1
        roots, iters, info = c.solve_roots(guesses)
        assert c.mirror_pairs() == 1
        return roots, iters, info, c.last_folded_steps()


@pytest.mark.parametrize("shape", ["em15", "stellarator"])
def test_mirrored_electromagnetic_contexts_never_fold(emme, shape):
    """dim = 2 N is even, but the matrix is a 2 x 2 block matrix of centrosymmetric blocks, not centrosymmetric."""
    make, guesses = SEARCHES[shape]
    r1, it1, in1, steps1 = _search(emme, make(), guesses, 1)
    r0, it0, in0, steps0 = _search(emme, make(), guesses, 0)
    assert steps1 == 0 and steps0 == 0, (steps1, steps0)
    assert r1.tobytes() == r0.tobytes() and np.array_equal(it1, it0) and np.array_equal(in1, in0)
    res = {}
    for fold in (1, 0):
        with _ctx(emme, make(), True, eigpair_fold=fold) as c:
            assert c.mirror_pairs() == 1
            res[fold] = c.solve_eigenpairs(guesses[:2], secant=True)
            assert c.mirror_pairs() == 1
            assert c.last_folded_eigpair_steps() == 0 and c.last_folded_steps() == 0
    for a, b in zip(res[1], res[0]):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_mirrored_gk31_folds(emme, oracle):
    """Electrostatic GK31, mirrored: the matrix structure of DESIGN.md §5.4c -- the folded trace-secant step under its
    existing rule (even order), to the bar of test_gpu_fold.py."""
    make, guesses = SEARCHES["gk31"]
    d = make()
    r1, it1, in1, steps1 = _search(emme, d, guesses, 1)
    r0, it0, in0, steps0 = _search(emme, d, guesses, 0)
    assert steps1 > 0 and steps0 == 0, (steps1, steps0)
    assert np.array_equal(in1, in0) and (in1 == 0).all(), (in1, in0)
    assert np.array_equal(it1, it0), (it1, it0)
    rel = np.abs(r1 - r0) / np.abs(r0)
    po = oracle.params(d)
    ro = np.array([oracle.solve_root(po, complex(g))[0] for g in guesses])
    print(f"gk31 search N=24: {steps1} folded steps, roots folded against unfolded {rel.max():.3g}, "
          f"against the oracle {(np.abs(r1 - ro) / np.abs(ro)).max():.3g}")
    assert (rel <= 1e-9).all(), rel
    assert (np.abs(r1 - ro) <= 1e-9 * np.abs(ro)).all(), np.abs(r1 - ro)
    # odd order: no folded step
    d25 = example_tokamak(npoints=25, integration_start_points=31)
    assert _search(emme, d25, guesses[:4], 1)[3] == 0


def test_cached_derivative_request_ends_mirroring(emme):
    make, ws = SHAPES["em15"]
    d = make(25)
    with _ctx(emme, d, False, deriv_cached=1) as fresh:
        fresh.set_deriv_cache_shapes(emme.DERIV_CACHE_SHAPES_ALL)
        M0, Mp0, iv0 = fresh.assemble_derivative(ws, want_intervals=True)
    with _ctx(emme, d, True) as ctx:
        ctx.assemble(ws)
        assert ctx.mirror_pairs() == 1 and ctx.node_cache_gib() > 0
        ctx.set_deriv_cache_shapes(emme.DERIV_CACHE_SHAPES_ALL)
        ctx.set_options(deriv_cached=1)
        assert ctx.mirror_pairs() == 1  # (the cache stays as it is until a derivative request needs it)
        ctx.profile_read(reset=True)
        M, Mp, iv = ctx.assemble_derivative(ws, want_intervals=True)
        assert ctx.profile_read().tile_tasks > 0 and ctx.mirror_pairs() == 0
        assert np.array_equal(M, M0) and np.array_equal(Mp, Mp0) and np.array_equal(iv, iv0)
        assert ctx.mirror_shapes() == emme.MIRROR_SHAPES_ALL
