"""Mirror-image pairs: on a grid symmetric under i -> N-1-i the tiled cache and the dense fill behind
it take one pair of every couple (i, j) / (N-1-j, N-1-i) and write both entries.  Routing, entries against the oracle
and against the unmirrored fill, interval counts, the deferred pass, the secant search, the cache size, and the
hand-over to cached derivative fills.

N = 24 and 25: both parities of N (self-mirror pairs on alternate diagonals) and a ragged last tile (144 + 0 and 156 =
9 x 16 + 12 half pairs).  The omegas are tame ones at which the oracle's mirror pairs have equal interval counts
(checked on the CPU: assemble(..., want_counts=True), c[i, j] against c[N-1-j, N-1-i], 0 mismatches at both sizes for
all four) and differ by 1e-15 .. 5e-15 of max |kappa|."""
import numpy as np
import pytest

from oracle.binding import example_tokamak

pytestmark = pytest.mark.gpu

TOL_M = 1e-10  # test_gpu_parity.py
WS = np.array([-0.8 + 0.25j, -1.2 + 0.05j, -0.5 + 0.4j])
WS_DEEP = np.array([-0.8 + 0.25j, -1.2 + 0.05j, -0.5 + 0.4j, -0.6 - 0.21j])  # the last one leaves a depth-4 cache
TINY = dict(node_cache_gb=0.05, cache_min_depth=1)  # test_gpu_derivative_cached.py: the shallowest shapes only
# 16 guesses for which the oracle's solve_root converges at npoints = 24 (5 .. 10 iterates, all to -0.56672+0.24013i)
GUESSES = np.array([-0.7249 + 0.1803j, -0.5617 + 0.3641j, -0.6346 + 0.2529j, -0.9649 + 0.3541j, -0.9199 + 0.2919j,
                    -0.5759 + 0.3225j, -1.0968 + 0.1274j, -0.6073 + 0.2623j, -0.6218 + 0.2523j, -0.8192 + 0.3614j,
                    -0.9182 + 0.2084j, -0.9329 + 0.2795j, -0.9471 + 0.1178j, -0.833 + 0.2163j, -0.7973 + 0.1969j,
                    -0.7679 + 0.1451j])


def _ctx(emme, d, mirror=None, **options):
    ctx = emme.Context(emme.params_from_dict(d), **options)
    if mirror is not None:
        ctx.set_mirror_pairs(mirror)
    return ctx


def _half_pairs(n):
    return (n * (n - 1) // 2 + n // 2) // 2


_ORACLE = {}


def _oracle_at(oracle, n, ws):
    """(matrices, interval totals, W dx of the upper triangle) of the oracle, computed once per (n, omegas)."""
    key = (n, tuple(ws))
    if key not in _ORACLE:
        d = example_tokamak(npoints=n)
        po = oracle.params(d)
        out = [oracle.assemble(po, complex(w)) for w in ws]
        _, dx = oracle.grid(d["length"], n)
        _ORACLE[key] = (np.array([m for m, _ in out]), np.array([t for _, t in out]), oracle.weights(n) * dx)
    return _ORACLE[key]


def _kappa(M, wdx):
    iu = np.triu_indices(M.shape[-1], 1)
    return M[..., iu[0], iu[1]] / (-wdx[iu]), iu


def _mirror_discrepancy(M, wdx):
    """max |kappa_ij - kappa_mirror| / max |kappa| of one matrix: what the reference's own arithmetic leaves between
    the two integrals of a couple."""
    n = M.shape[-1]
    kap = np.zeros((n, n), complex)
    k, iu = _kappa(M, wdx)
    kap[iu] = k
    return np.abs(kap[iu] - kap[n - 1 - iu[1], n - 1 - iu[0]]).max() / np.abs(k).max()


def _compare(emme, oracle, n, ws, label, **options):
    d = example_tokamak(npoints=n)
    Mo, tot, wdx = _oracle_at(oracle, n, ws)
    out = {}
    for mirror in (True, False):
        with _ctx(emme, d, mirror=mirror, **options) as ctx:
            ctx.profile(True)
            assert ctx.mirror_pairs() == int(mirror)
            M, iv = ctx.assemble(ws, want_intervals=True)
            assert ctx.fill_kernel_symbol().startswith("k_assemble_dense") and ctx.mirror_pairs() == int(mirror)
            out[mirror] = (M, iv, ctx.last_deferred(), ctx.profile_read())
    for mirror, (M, iv, _, _) in out.items():
        # 3. counts: the reference algorithm's, mirrored or not
        assert np.array_equal(iv, tot), (label, mirror, iv, tot)
        for b in range(len(ws)):
            err = np.abs(M[b] - Mo[b]).max() / np.abs(Mo[b]).max()
            assert err <= TOL_M, (label, mirror, ws[b], err)
            assert np.array_equal(M[b], M[b].T)
    # 2. on against off: within 100 x what the oracle's own mirror pairs differ by (the device's exp / sincos are not
    # the host's)
    for b in range(len(ws)):
        ref = _mirror_discrepancy(Mo[b], wdx)
        k_on, _ = _kappa(out[True][0][b], wdx)
        k_off, _ = _kappa(out[False][0][b], wdx)
        diff = np.abs(k_on - k_off).max() / np.abs(k_off).max()
        print(f"mirror {label} N={n} omega={ws[b]}: on/off {diff:.3g}, oracle mirror discrepancy {ref:.3g}, "
              f"ratio {diff / ref:.3g}")
        assert diff <= 100.0 * ref, (label, ws[b], diff, ref)
    return out


def test_routing(emme, monkeypatch):
    off_cases = {"theta": example_tokamak(npoints=24, theta=0.3), "em": example_tokamak(npoints=24, beta_e=0.02),
                 "gk31": example_tokamak(npoints=24, integration_start_points=31)}
    with _ctx(emme, example_tokamak(npoints=24)) as ctx:
        assert ctx.mirror_pairs() == 1
        M_on = ctx.assemble(WS)
        assert ctx.mirror_pairs() == 1 and ctx.fill_kernel_symbol().startswith("k_assemble_dense")
        with pytest.raises(emme.EmmeError):  # a layout setting: the cache exists
            ctx.set_mirror_pairs(False)
        assert ctx.mirror_pairs() == 1
    for name, d in off_cases.items():
        with _ctx(emme, d) as ctx, _ctx(emme, d, mirror=False) as off:
            assert ctx.mirror_pairs() == 0 and off.mirror_pairs() == 0, name
            assert np.array_equal(ctx.assemble(WS), off.assemble(WS)), name
            assert ctx.mirror_pairs() == 0, name
    with _ctx(emme, example_tokamak(npoints=24), mirror=False) as off:
        assert off.mirror_pairs() == 0
        M_off = off.assemble(WS)
        assert off.mirror_pairs() == 0
    monkeypatch.setenv("EMME_MIRROR", "0")
    with _ctx(emme, example_tokamak(npoints=24)) as ctx:
        assert ctx.mirror_pairs() == 0
        assert np.array_equal(ctx.assemble(WS), M_off)
    monkeypatch.delenv("EMME_MIRROR")
    # (mirrored against unmirrored entries: test_entries_and_counts)
    assert np.abs(M_on - M_off).max() <= TOL_M * np.abs(M_off).max()
    # a context created for cached derivative fills never mirrors
    with _ctx(emme, example_tokamak(npoints=24), deriv_cached=1) as ctx:
        assert ctx.mirror_pairs() == 0
        assert np.array_equal(ctx.assemble(WS), M_off)


@pytest.mark.parametrize("n", [24, 25])
def test_entries_and_counts(emme, oracle, n):
    _compare(emme, oracle, n, WS, "default", node_cache_gb=8.0)


@pytest.mark.parametrize("n,wide", [(24, 0), (25, 0), (25, 1)])
def test_deferred_pass(emme, oracle, n, wide):
    """A cache of depth 4: the damped omega's integrals leave it for the list / cooperative kernels, which scatter the
    mirror entry and count its intervals as the dense fill does; once through the 128-entry build."""
    out = _compare(emme, oracle, n, WS_DEEP, f"tiny wide={wide}", dense_wide=wide, **TINY)
    for mirror, (_, _, deferred, prof) in out.items():
        assert prof.deferred_launches >= 1 and deferred > 0, (mirror, deferred)
    # undoubled: the mirrored fill defers one integral per couple
    assert out[True][2] < out[False][2]


def test_secant_search(emme):
    d = example_tokamak(npoints=24)
    res = {}
    for mirror in (True, False):
        with _ctx(emme, d, mirror=mirror) as ctx:
            res[mirror] = ctx.solve_roots(GUESSES)
            assert ctx.mirror_pairs() == int(mirror)
    (r_on, it_on, info_on), (r_off, it_off, info_off) = res[True], res[False]
    assert (info_on == 0).all() and (info_off == 0).all(), (info_on, info_off)
    assert np.array_equal(it_on, it_off), (it_on, it_off)
    assert (np.abs(r_on - r_off) <= 1e-9 * np.abs(r_off)).all(), np.abs(r_on - r_off).max()


@pytest.mark.parametrize("n", [24, 25])
def test_cache_size(emme, n):
    """The cache holds ceil(pairs / 16) tiles of the same intervals: bytes on / off = tiles on / off, exactly."""
    d = example_tokamak(npoints=n)
    bytes_ = {}
    for mirror in (True, False):
        with _ctx(emme, d, mirror=mirror, **TINY) as ctx:
            ctx.assemble(WS_DEEP)  # (one fill: the main part alone -- what grows later depends on the room left)
            bytes_[mirror] = round(ctx.node_cache_gib() * 2 ** 30)
            geom = ctx.cache_state()[:2]
        bytes_[mirror, "geom"] = geom
    assert bytes_[True, "geom"] == bytes_[False, "geom"]
    t_on, t_off = (_half_pairs(n) + 15) // 16, (n * (n - 1) // 2 + 15) // 16
    assert bytes_[True] > 0 and bytes_[True] * t_off == bytes_[False] * t_on, (bytes_, t_on, t_off)


def test_cached_derivative_request_ends_mirroring(emme):
    d = example_tokamak(npoints=25)
    with _ctx(emme, d, deriv_cached=1) as fresh:
        M0, Mp0, iv0 = fresh.assemble_derivative(WS, want_intervals=True)
    with _ctx(emme, d) as ctx:
        ctx.assemble(WS)
        assert ctx.mirror_pairs() == 1 and ctx.node_cache_gib() > 0
        ctx.set_options(deriv_cached=1)
        assert ctx.mirror_pairs() == 1  # (the cache stays as it is until a derivative request needs it)
        ctx.profile_read(reset=True)
        M, Mp, iv = ctx.assemble_derivative(WS, want_intervals=True)
        assert ctx.profile_read().tile_tasks > 0 and ctx.mirror_pairs() == 0
        assert np.array_equal(M, M0) and np.array_equal(Mp, Mp0) and np.array_equal(iv, iv0)
        # plain fills go on, unmirrored, on the rebuilt cache (to the 1e-13 between two fills of one omega in
        # test_every_fill_kernel_matches_oracle: the two caches need not have grown alike)
        with _ctx(emme, d, mirror=False) as off:
            Ma, Mb = ctx.assemble(WS), off.assemble(WS)
            assert np.abs(Ma - Mb).max() <= 1e-13 * np.abs(Mb).max()
        assert ctx.mirror_pairs() == 0
