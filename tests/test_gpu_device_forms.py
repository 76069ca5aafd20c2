"""The device-pointer forms of the C ABI (include/emme_hip.h: "host or device") held to the bits of the host forms.

Every output lives in a guarded buffer (tests/device_buffers.py): a front guard, the payload and a back guard in one
allocation, all pre-filled with a sentinel no kernel produces.  After every call the guards of every buffer must be
intact, every output must be written completely -- no fill zeroes M, so an entry a kernel skipped shows here and
nowhere else -- and every input the header calls "not modified" must be byte for byte what was uploaded.

A "twin" is a second fresh context with the same parameters and options that makes the same single call through the
host form: the two calls have no cache history to differ in (test_gpu_dense_stage.py relies on two such contexts
giving the same bytes).  "Same bits" is tobytes() equality, NaNs included.  No new tolerance: the only other bars are
TOL_M = 1e-10 max|M| against the oracle with identical interval totals (test_gpu_parity.py).

The library names no kernel for a derivative fill (emme_ctx_fill_mode keeps naming the last plain fill), so the cases
that ask "an uncached kernel ran" read the profile's counters, as test_gpu_derivative_cached.py does."""
import ctypes as C

import numpy as np
import pytest

import device_buffers as db
from device_buffers import GuardedBuffer
from oracle.binding import example_stellarator, example_tokamak

pytestmark = pytest.mark.gpu

TOL_M = 1e-10  # test_gpu_parity.py
EMME_EINVAL = -1
W_FILL = np.array([-0.8 + 0.25j, -0.6 - 0.21j, 0.5 + 0.1j, 0.153 - 0.316j])  # both contour classes
WS_DEEP = np.array([-0.8 + 0.25j, -1.2 + 0.05j, -0.5 + 0.4j, -0.6 - 0.21j])  # test_gpu_mirror_pairs.py
TINY = dict(node_cache_gb=0.05, cache_min_depth=1)                            # test_gpu_mirror_pairs.py
OMEGAS_ES = np.array([-0.8 + 0.25j, -0.792 + 0.2475j, 0.6 + 0.1j, -0.3 - 0.05j])  # test_gpu_derivative.py
OMEGAS_EM = np.array([-1.656 + 2.49j, -0.85 - 0.32j, 0.4 - 0.2j])                  # test_gpu_parity.py


def _ctx(emme, d, mirror=None, tile_shapes=None, deriv_shapes=None, stream=None, **options):
    ctx = emme.Context(emme.params_from_dict(d), **options)
    if mirror is not None:
        ctx.set_mirror_pairs(mirror)
    if tile_shapes is not None:
        ctx.set_tile_shapes(tile_shapes)
    if deriv_shapes is not None:
        ctx.set_deriv_cache_shapes(deriv_shapes)
    if stream is not None:
        ctx.set_stream(stream.value)
    return ctx


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _after_call(outputs=(), inputs=(), others=()):
    """The three checks every call is followed by.  inputs: (buffer, what was uploaded) pairs."""
    for buf in list(outputs) + [b for b, _ in inputs] + list(others):
        buf.assert_guards_intact()
    for buf in outputs:
        buf.assert_fully_written()
    for buf, original in inputs:
        buf.assert_unchanged(original)


def _mats(shape_or_array, n, stream=None):
    """A guarded buffer for [nbatch, n, n] complex matrices (an array: uploaded)."""
    if isinstance(shape_or_array, np.ndarray):
        return GuardedBuffer(shape_or_array.shape, matrix_bytes=16 * n * n, stream=stream).upload(shape_or_array)
    return GuardedBuffer(shape_or_array, matrix_bytes=16 * n * n, stream=stream)


def _vec(count, dtype, n, stream=None, data=None):
    buf = GuardedBuffer((count,), dtype=dtype, matrix_bytes=16 * n * n, stream=stream)
    return buf if data is None else buf.upload(data)


_ORACLE = {}


def _oracle_fill(oracle, d, ws):
    """(matrices, interval totals) of the oracle: computed once per (parameters, omegas), shared, never modified."""
    key = (repr(sorted(d.items())), tuple(complex(w) for w in ws))
    if key not in _ORACLE:
        po = oracle.params(d)
        out = [oracle.assemble(po, complex(w)) for w in ws]
        M, tot = np.array([m for m, _ in out]), np.array([t for _, t in out])
        M.setflags(write=False), tot.setflags(write=False)
        _ORACLE[key] = (M, tot)
    return _ORACLE[key]


# ---- A. plain fill into caller memory, route by route --------------------------------------------------------------
TOK25, TOK24, STEL10 = dict(npoints=25), dict(npoints=24), dict(npoints=10)
ROUTES = {
    # 25: odd N, a ragged last tile of the half pair list (test_gpu_mirror_pairs.py)
    "dense-mirrored": dict(d=example_tokamak(**TOK25), mirror_is=1, symbol="k_assemble_dense<1, 15, 1>"),
    "dense-unmirrored": dict(d=example_tokamak(**TOK25), ctx=dict(mirror=False), mirror_is=0,
                             symbol="k_assemble_dense<1, 15, 1>"),
    # a depth-4 cache: the deferred list and cooperative kernels write into caller memory
    "dense-deferred": dict(d=example_tokamak(**TOK25), ctx=TINY, ws=WS_DEEP, deferred=True,
                           symbol="k_assemble_dense<1, 15, 1>"),
    "omega-lane": dict(d=example_tokamak(**TOK24), ctx=dict(node_cache_gb=0.0, wl_min=1), symbol="k_assemble_wl<15>"),
    "wl-min-100000": dict(d=example_tokamak(**TOK24), ctx=dict(wl_min=100000)),
    # (with the cache budget the tests' default options leave, wl_min alone does not reach the lanes-are-nodes kernel:
    # the "nodes" options of test_gpu_parity.py beside it)
    "nodes": dict(d=example_tokamak(**TOK24), ctx=dict(node_cache_gb=0.0, wl_min=100000), symbol="k_assemble<15, false>"),
    # (EMME_FILL_UNION: the 48-byte records; a launch of few chunks may take the independent lanes on them)
    "union": dict(d=example_tokamak(**TOK24), ctx=dict(fill=1), symbol=("k_assemble_union<15", "k_assemble_cached<15")),
    "tile": dict(d=example_tokamak(**TOK24), ctx=dict(tile_uncached=1, node_cache_gb=0.0), symbol="k_assemble_tile"),
    "stellarator": dict(d=example_stellarator(**STEL10)),
    "stellarator-tile-shapes": dict(d=example_stellarator(**STEL10),
                                    ctx=dict(tile_uncached=1, node_cache_gb=0.0, tile_shapes=1),
                                    symbol="k_assemble_tile_shape<"),
    "gk31": dict(d=example_tokamak(npoints=24, integration_start_points=31)),
}
SMALLEST_ROUTE = "stellarator"  # (dim 20)


def _fill_device_form(emme, route, stream=None):
    """One plain fill of the route's omegas into a guarded buffer on a fresh context."""
    r = ROUTES[route]
    ws = r.get("ws", W_FILL)
    with _ctx(emme, r["d"], stream=stream, **r.get("ctx", {})) as ctx:
        if "mirror_is" in r:
            assert ctx.mirror_pairs() == r["mirror_is"]
        with _mats((len(ws), ctx.dim, ctx.dim), ctx.dim, stream) as buf:
            try:
                iv = ctx.assemble(ws, out_device_ptr=buf.ptr)
                _after_call(outputs=[buf])
                out = dict(M=buf.read(), iv=iv, symbol=ctx.fill_kernel_symbol(), deferred=ctx.last_deferred())
            finally:
                ctx.set_stream(0)
        if "mirror_is" in r:
            assert ctx.mirror_pairs() == r["mirror_is"]
    return out


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_plain_fill_into_caller_memory(emme, oracle, route):
    r = ROUTES[route]
    ws = r.get("ws", W_FILL)
    got = _fill_device_form(emme, route)
    with _ctx(emme, r["d"], **r.get("ctx", {})) as twin:
        Mh, ivh = twin.assemble(ws, want_intervals=True)
        assert twin.fill_kernel_symbol() == got["symbol"], (route, twin.fill_kernel_symbol(), got["symbol"])
        assert twin.last_deferred() == got["deferred"]
    if "symbol" in r:
        assert got["symbol"].startswith(r["symbol"]), (route, got["symbol"])
    if r.get("deferred"):
        assert got["deferred"] > 0
    Mo, tot = _oracle_fill(oracle, r["d"], ws)
    for b in range(len(ws)):
        err = np.abs(got["M"][b] - Mo[b]).max() / np.abs(Mo[b]).max()
        print(f"{route} omega {ws[b]}: device form vs oracle {err:.3g}, intervals {got['iv'][b]} / {tot[b]}, "
              f"vs host form {np.abs(got['M'][b] - Mh[b]).max() / np.abs(Mh[b]).max():.3g}")
        assert err <= TOL_M, (route, ws[b], err)
    assert np.array_equal(got["iv"], tot), (route, got["iv"], tot)
    assert np.array_equal(got["iv"], ivh), (route, got["iv"], ivh)
    assert _same(got["M"], Mh), (route, np.abs(got["M"] - Mh).max())


# ---- B. derivative fill --------------------------------------------------------------------------------------------
DERIV = {
    "tokamak": dict(d=example_tokamak(**TOK25), ws=OMEGAS_ES),
    "tokamak-cached": dict(d=example_tokamak(**TOK25), ws=OMEGAS_ES, ctx=dict(deriv_cached=1)),
    "tokamak-cached-tile": dict(d=example_tokamak(**TOK25), ws=OMEGAS_ES,
                                ctx=dict(deriv_cached=1, tile_uncached=1, node_cache_gb=0.0),
                                plain=dict(tile_uncached=1, node_cache_gb=0.0)),
    "stellarator": dict(d=example_stellarator(**STEL10), ws=OMEGAS_EM),
    "stellarator-cached-shapes": dict(d=example_stellarator(**STEL10), ws=OMEGAS_EM,
                                      ctx=dict(deriv_cached=1, deriv_shapes=1)),
}
SMALLEST_DERIV = "stellarator"


def _deriv_device_form(emme, case, device_omega, stream=None, profile=False):
    """One derivative fill with M and Mp (and, device_omega, the omegas) in guarded buffers on a fresh context."""
    k = DERIV[case]
    ws = k["ws"]
    with _ctx(emme, k["d"], stream=stream, **k.get("ctx", {})) as ctx:
        n, nb = ctx.dim, len(ws)
        if profile:
            ctx.profile(True)
        state = ctx.cache_state()
        with _mats((nb, n, n), n, stream) as bM, _mats((nb, n, n), n, stream) as bMp, \
                _vec(nb, np.complex128, n, stream, ws) as bw:
            try:
                if device_omega:
                    _, _, iv = ctx.assemble_derivative(nb, want_intervals=True, omega_device_ptr=bw.ptr,
                                                       out_device_ptr=bM.ptr, mp_device_ptr=bMp.ptr)
                else:
                    _, _, iv = ctx.assemble_derivative(ws, want_intervals=True, out_device_ptr=bM.ptr,
                                                       mp_device_ptr=bMp.ptr)
                _after_call(outputs=[bM, bMp], inputs=[(bw, ws)])
                out = dict(M=bM.read(), Mp=bMp.read(), iv=iv, state=state, state_after=ctx.cache_state(),
                           deferred=ctx.last_deferred(), profile=ctx.profile_read() if profile else None)
            finally:
                ctx.set_stream(0)
    return out


@pytest.mark.parametrize("case", sorted(DERIV))
def test_derivative_fill_into_caller_memory(emme, case):
    k = DERIV[case]
    got = _deriv_device_form(emme, case, device_omega=False)
    with _ctx(emme, k["d"], **k.get("ctx", {})) as twin:
        M, Mp, iv = twin.assemble_derivative(k["ws"], want_intervals=True)
    assert np.array_equal(got["iv"], iv), (case, got["iv"], iv)
    assert _same(got["M"], M), (case, np.abs(got["M"] - M).max())
    assert _same(got["Mp"], Mp), (case, np.abs(got["Mp"] - Mp).max())
    if "plain" in k:  # the header: M of the tile derivative fill is the plain tile fill's bit for bit
        with _ctx(emme, k["d"], **k["plain"]) as plain:
            Mplain, ivp = plain.assemble(k["ws"], want_intervals=True)
            assert plain.fill_kernel_symbol() == "k_assemble_tile"
        assert _same(got["M"], Mplain) and np.array_equal(got["iv"], ivp), case


@pytest.mark.parametrize("case", sorted(DERIV))
def test_derivative_fill_with_device_omegas_keeps_the_uncached_kernels(emme, case):
    """Device omegas: no cache and no tile fill, whatever the options say."""
    k = DERIV[case]
    got = _deriv_device_form(emme, case, device_omega=True, profile=True)
    pr = got["profile"]
    # no dense or tile task, no work list behind one, no cache built or grown (the omega-lane kernel counts its rounds
    # in the first round counter: test_gpu_derivative_cached.py)
    assert pr.tile_tasks == 0 and pr.sparse_rounds == 0 and pr.deferred_launches == 0 and pr.cache_build_launches == 0
    assert pr.matrices == len(k["ws"]) and got["deferred"] == 0
    assert got["state_after"] == got["state"], (case, got["state"], got["state_after"])
    with _ctx(emme, k["d"]) as twin:  # default options, host omegas
        M, Mp, iv = twin.assemble_derivative(k["ws"], want_intervals=True)
    assert np.array_equal(got["iv"], iv), (case, got["iv"], iv)
    assert _same(got["M"], M), (case, np.abs(got["M"] - M).max())
    assert _same(got["Mp"], Mp), (case, np.abs(got["Mp"] - Mp).max())
    # the header: M is that of the plain fill of the same (uncached) kernel, bit for bit
    with _ctx(emme, k["d"], node_cache_gb=0.0) as plain:
        Mplain, ivp = plain.assemble(k["ws"], want_intervals=True)
        assert plain.fill_kernel_symbol().startswith(("k_assemble_wl<", "k_assemble<"))
    assert _same(got["M"], Mplain) and np.array_equal(got["iv"], ivp), (case, np.abs(got["M"] - Mplain).max())


# ---- C. fill over parameter sets -----------------------------------------------------------------------------------
def _sets_cases():
    import test_gpu_param_sets as ps
    return ps.CASES


SETS_ROUTES = {"nodes": {}, "tile": dict(tile_uncached=1)}
# beside what the issue of this test asks for: the options under which the tile fill over sets does run
# (test_gpu_tile_sets.py), so that k_assemble_tile_sets and its list kernel write into caller memory too; host omegas
SETS_TILE_TAKEN = dict(node_cache_gb=0.0, wl_min=1, tile_uncached=1, dense_min_tasks=0, deriv_cached=1)


def _bound(emme, dicts, stream=None, **options):
    ctx = _ctx(emme, dicts[0], stream=stream, **options)
    ctx.bind_param_sets([emme.params_from_dict(d) for d in dicts])
    return ctx


def _sets_device_form(emme, case, options, with_mp, device_omega, stream=None):
    dicts, st, w = _sets_cases()[case]
    w = np.asarray(w, dtype=np.complex128)
    with _bound(emme, dicts, stream=stream, **options) as ctx:
        n, nb = ctx.dim, len(w)
        with _mats((nb, n, n), n, stream) as bM, _mats((nb, n, n), n, stream) as bMp, \
                _vec(nb, np.complex128, n, stream, w) as bw:
            try:
                res = ctx.assemble_sets(st, w, want_intervals=True, out_device_ptr=bM.ptr,
                                        omega_device_ptr=bw.ptr if device_omega else None,
                                        mp_device_ptr=bMp.ptr if with_mp else None)
                _after_call(outputs=[bM, bMp] if with_mp else [bM], inputs=[(bw, w)], others=[bMp])
                if not with_mp:
                    bMp.assert_untouched()
                out = dict(M=bM.read(), Mp=bMp.read() if with_mp else None, iv=res[-1],
                           mode=ctx.lib.emme_ctx_fill_mode(ctx.h))
            finally:
                ctx.set_stream(0)
    return out


def _sets_host_form(emme, case, options, with_mp):
    dicts, st, w = _sets_cases()[case]
    with _bound(emme, dicts, **options) as twin:
        res = twin.assemble_sets(st, w, want_derivative=with_mp, want_intervals=True)
        return dict(M=res[0], Mp=res[1] if with_mp else None, iv=res[-1], mode=twin.lib.emme_ctx_fill_mode(twin.h))


@pytest.mark.parametrize("device_omega", [False, True], ids=["host-omega", "device-omega"])
@pytest.mark.parametrize("with_mp", [False, True], ids=["M", "M-Mp"])
@pytest.mark.parametrize("route", sorted(SETS_ROUTES))
@pytest.mark.parametrize("case", ["es15", "es31", "em"])
def test_fill_over_sets_into_caller_memory(emme, case, route, with_mp, device_omega):
    got = _sets_device_form(emme, case, SETS_ROUTES[route], with_mp, device_omega)
    if device_omega:
        assert got["mode"] == 6  # k_assemble_sets: the tile fill over sets needs the omegas on the host
    want = _sets_host_form(emme, case, SETS_ROUTES[route], with_mp)
    assert np.array_equal(got["iv"], want["iv"]), (got["iv"], want["iv"], want["mode"])
    assert _same(got["M"], want["M"]), (np.abs(got["M"] - want["M"]).max(), want["mode"])
    if with_mp:
        assert _same(got["Mp"], want["Mp"]), (np.abs(got["Mp"] - want["Mp"]).max(), want["mode"])


@pytest.mark.parametrize("with_mp", [False, True], ids=["M", "M-Mp"])
def test_tile_fill_over_sets_into_caller_memory(emme, with_mp):
    got = _sets_device_form(emme, "es15", SETS_TILE_TAKEN, with_mp, device_omega=False)
    want = _sets_host_form(emme, "es15", SETS_TILE_TAKEN, with_mp)
    assert got["mode"] == 7 and want["mode"] == 7
    assert np.array_equal(got["iv"], want["iv"]) and _same(got["M"], want["M"])
    if with_mp:
        assert _same(got["Mp"], want["Mp"])


# ---- D. the Newton step with all five arrays on the device ---------------------------------------------------------
NEWTON = {
    "tokamak-trace": dict(d=example_tokamak(**TOK24), method=0, g=[-0.8 + 0.25j, -0.7 + 0.3j]),
    "tokamak-trace-uncached": dict(d=example_tokamak(**TOK24), method=0, g=[-0.8 + 0.25j, -0.7 + 0.3j],
                                   ctx=dict(node_cache_gb=0.0)),
    "stellarator-qr": dict(d=example_stellarator(**STEL10), method=1, g=[-1.656 + 2.49j, -1.6 + 2.4j]),
}
SMALLEST_NEWTON = "stellarator-qr"
_NEWTON_IN = {}


def _newton_inputs(oracle, case):
    """omega, M(omega) and the secant M' there, built as test_newton_step_matches_oracle builds them; once per case."""
    if case not in _NEWTON_IN:
        k = NEWTON[case]
        po = oracle.params(k["d"])
        w, M, Mp = [], [], []
        for g in k["g"]:
            w0, dw = 0.99 * g, 0.01 * g
            M0, _ = oracle.assemble(po, w0)
            M1, _ = oracle.assemble(po, w0 + dw)
            w.append(w0 + dw), M.append(M1), Mp.append((M1 - M0) / dw)
        out = tuple(np.ascontiguousarray(a, dtype=np.complex128) for a in (w, M, Mp))
        for a in out:
            a.setflags(write=False)
        _NEWTON_IN[case] = out
    return _NEWTON_IN[case]


def _newton_device_form(emme, oracle, case, stream=None):
    k = NEWTON[case]
    w, M, Mp = _newton_inputs(oracle, case)
    with _ctx(emme, k["d"], stream=stream, **k.get("ctx", {})) as ctx:
        n, nb = ctx.dim, len(w)
        with _vec(nb, np.complex128, n, stream, w) as bw, _vec(nb, np.complex128, n, stream) as bdw, \
                _mats(M, n, stream) as bM, _mats(Mp, n, stream) as bMp, _vec(nb, np.int32, n, stream) as binfo:
            try:
                ctx.newton_step(nb, None, None, method=k["method"], omega_device_ptr=bw.ptr, domega_device_ptr=bdw.ptr,
                                m_device_ptr=bM.ptr, mp_device_ptr=bMp.ptr, info_device_ptr=binfo.ptr)
                _after_call(outputs=[bw, bdw, bM, bMp, binfo])
                out = (bw.read(), bdw.read(), bM.read(), bMp.read(), binfo.read())
            finally:
                ctx.set_stream(0)
    return out


@pytest.mark.parametrize("case", sorted(NEWTON))
def test_newton_step_on_device_arrays(emme, oracle, case):
    k = NEWTON[case]
    got = _newton_device_form(emme, oracle, case)
    w, M, Mp = _newton_inputs(oracle, case)
    with _ctx(emme, k["d"], **k.get("ctx", {})) as twin:
        want = twin.newton_step(w, M, Mp, method=k["method"])
    assert (want[4] == 0).all(), want[4]
    assert not _same(want[0], w)  # (the step moved)
    for name, a, b in zip(("omega", "domega", "M", "Mp", "info"), got, want):
        assert _same(a, b), (case, name, np.abs(a - b).max())


# ---- E. linear algebra on caller matrices --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_ctx(emme):
    ctx = _ctx(emme, example_tokamak(npoints=16))
    yield ctx
    ctx.close()


_LINALG = {}


def _symmetric_batch(n):
    """Three matrices A + A^T + 0.5 sqrt(n) I with random B (test_gpu_parity.py), the middle A exactly singular."""
    if ("sym", n) not in _LINALG:
        rng = np.random.default_rng(n)
        A = rng.normal(size=(3, n, n)) + 1j * rng.normal(size=(3, n, n))
        A = A + np.transpose(A, (0, 2, 1)) + 0.5 * n ** 0.5 * np.eye(n)
        B = rng.normal(size=(3, n, n)) + 1j * rng.normal(size=(3, n, n))
        A[1, :, n // 2] = 0.0  # column n/2 + 1 of the factorisation is exactly zero
        A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
        A.setflags(write=False), B.setflags(write=False)
        _LINALG["sym", n] = (A, B)
    return _LINALG["sym", n]


def _constructed_batch(n):
    """_constructed(n) of test_gpu_eigenpairs.py as a batch of three: its two matrices around a copy of the second
    with an exactly zero column."""
    if ("con", n) not in _LINALG:
        import test_gpu_eigenpairs as ep
        M, Mp, v = ep._constructed(n)
        sing = M[1].copy()
        sing[:, n // 2] = 0.0
        out = (np.ascontiguousarray(np.array([M[0], sing, M[1]])), np.ascontiguousarray(np.array([Mp[0], Mp[1], Mp[1]])),
               np.ascontiguousarray(np.array([v[0], v[1], v[1]])))
        for a in out:
            a.setflags(write=False)
        _LINALG["con", n] = out
    return _LINALG["con", n]


def _trace_solve_device(ctx, n, stream=None):
    A, B = _symmetric_batch(n)
    with _mats(A, n, stream) as bA, _mats(B, n, stream) as bB:
        tr, info = ctx.trace_solve((3, n), None, a_device_ptr=bA.ptr, b_device_ptr=bB.ptr)
        _after_call(others=[bA, bB])  # (destroyed by the call: only the guards apply)
    return tr, info


@pytest.mark.parametrize("n", [5, 37, 300, 600, 1100])
def test_trace_solve_on_device_operands(small_ctx, n):
    A, B = _symmetric_batch(n)
    tr, info = _trace_solve_device(small_ctx, n)
    tr_h, info_h = small_ctx.trace_solve(A, B)
    assert info_h[0] == 0 and info_h[1] == n // 2 + 1 and info_h[2] == 0 and np.isnan(tr_h[1])
    assert _same(tr, tr_h) and _same(info, info_h), (n, tr, tr_h, info, info_h)


def _qr_secant_device(ctx, n, stream=None):
    A, B = _symmetric_batch(n)
    with _mats(A, n, stream) as bA, _mats(B, n, stream) as bB:
        q, info = ctx.qr_secant((3, n), None, a_device_ptr=bA.ptr, b_device_ptr=bB.ptr)
        _after_call(inputs=[(bA, A), (bB, B)])
    return q, info


@pytest.mark.parametrize("n", [17, 300, 640])
def test_qr_secant_on_device_operands(small_ctx, n):
    A, B = _symmetric_batch(n)
    q, info = _qr_secant_device(small_ctx, n)
    q_h, info_h = small_ctx.qr_secant(A, B)
    assert info_h[0] == 0 and info_h[2] == 0
    assert _same(q, q_h) and _same(info, info_h), (n, q, q_h, info, info_h)


def _null_vectors_device(ctx, n, stream=None):
    A, _ = _symmetric_batch(n)
    with _mats(A, n, stream) as bA:
        v, info = ctx.null_vectors((3, n), device_ptr=bA.ptr)
        _after_call(inputs=[(bA, A)])
    return v, info


@pytest.mark.parametrize("n", [37, 600, 1100])
def test_null_vectors_on_device_matrices(small_ctx, n):
    A, _ = _symmetric_batch(n)
    v, info = _null_vectors_device(small_ctx, n)
    v_h, info_h = small_ctx.null_vectors(A)
    assert info_h[0] == 0 and info_h[1] == n // 2 + 1 and info_h[2] == 0 and np.isnan(v_h[1]).all()
    assert _same(v, v_h) and _same(info, info_h), (n, info, info_h)


def _eigenpair_device(ctx, n, secant, have_v, stream=None):
    M, Mp, v = _constructed_batch(n)
    dw = np.array([0.01 - 0.002j, -0.003 + 0.004j, 0.002 + 0.001j])
    with _mats(M, n, stream) as bM, _mats(Mp, n, stream) as bMp:
        if secant:
            out = ctx.eigenpair_secant_step((3, n), None, dw, v if have_v else None, m_device_ptr=bM.ptr,
                                            m_old_device_ptr=bMp.ptr)
        else:
            out = ctx.eigenpair_step((3, n), None, v if have_v else None, m_device_ptr=bM.ptr, mp_device_ptr=bMp.ptr)
        _after_call(inputs=[(bM, M), (bMp, Mp)])
    return out, dw


@pytest.mark.parametrize("have_v", [0, 1])
@pytest.mark.parametrize("secant", [False, True], ids=["exact", "secant"])
@pytest.mark.parametrize("n", [17, 600, 1100])
def test_eigenpair_steps_on_device_matrices(small_ctx, n, secant, have_v):
    M, Mp, v = _constructed_batch(n)
    got, dw = _eigenpair_device(small_ctx, n, secant, have_v)
    if secant:
        want = small_ctx.eigenpair_secant_step(M, Mp, dw, v if have_v else None)
    else:
        want = small_ctx.eigenpair_step(M, Mp, v if have_v else None)
    assert want[3][0] == 0 and want[3][1] == n // 2 + 1 and want[3][2] == 0, want[3]
    for name, a, b in zip(("v", "tau", "resid", "info"), got, want):
        assert _same(a, b), (n, secant, have_v, name)


def _moments_inputs():
    if "moments" not in _LINALG:
        rng = np.random.default_rng(5)
        n, nq, L = 64, 8, 8
        M = (rng.standard_normal((nq, n, n)) + 1j * rng.standard_normal((nq, n, n))) / np.sqrt(n) + np.eye(n)[None]
        M[3, :, 0] = 0.0  # exactly singular: left out of its group's sums
        V = rng.standard_normal((n, L)) + 1j * rng.standard_normal((n, L))
        z = rng.standard_normal(nq) + 1j * rng.standard_normal(nq)
        w = rng.standard_normal(nq) + 1j * rng.standard_normal(nq)
        group = np.array([0, 1, 2, 0, 1, 2, 0, 1], dtype=np.int32)  # three interleaved groups
        _LINALG["moments"] = (np.ascontiguousarray(M), np.ascontiguousarray(V), z, w, group)
    return _LINALG["moments"]


def _moments_device(ctx, stream=None, groups=True):
    M, V, z, w, group = _moments_inputs()
    nq, n, L = M.shape[0], M.shape[1], V.shape[1]
    with _mats(M, n, stream) as bM, GuardedBuffer(V.shape, matrix_bytes=16 * n * n, stream=stream).upload(V) as bV:
        if groups:
            out = ctx.contour_moments_groups((nq, n), group, 3, z, w, L, device_ptr=bM.ptr, v_device_ptr=bV.ptr)
        else:
            out = ctx.contour_moments((nq, n), z, w, L, device_ptr=bM.ptr, v_device_ptr=bV.ptr)
        _after_call(inputs=[(bM, M), (bV, V)])
    return out


@pytest.mark.parametrize("groups", [True, False], ids=["groups", "batch"])
def test_contour_moments_on_device_operands(small_ctx, groups):
    M, V, z, w, group = _moments_inputs()
    got = _moments_device(small_ctx, groups=groups)
    if groups:
        want = small_ctx.contour_moments_groups(M, group, 3, z, w, V.shape[1], V=V)
    else:
        want = small_ctx.contour_moments(M, z, w, V.shape[1], V=V)
    assert want[3][3] > 0 and (np.delete(want[3], 3) == 0).all()
    for name, a, b in zip(("A0", "A1", "logdet", "info"), got, want):
        assert _same(a, b), name


# ---- F. on a non-blocking stream -----------------------------------------------------------------------------------
def test_device_forms_on_a_non_blocking_stream(emme, oracle):
    """One case of each of A-E, at its smallest size, with the sentinel fill, the uploads and the library's work queued
    on a hipStreamNonBlocking stream; the buffers synchronise that stream before they read back.  The bits are those
    of the null-stream run."""
    st = db.create_non_blocking_stream()
    try:
        a0, a1 = _fill_device_form(emme, SMALLEST_ROUTE), _fill_device_form(emme, SMALLEST_ROUTE, stream=st)
        assert _same(a0["M"], a1["M"]) and np.array_equal(a0["iv"], a1["iv"]) and a0["symbol"] == a1["symbol"]
        for device_omega in (False, True):
            b0 = _deriv_device_form(emme, SMALLEST_DERIV, device_omega)
            b1 = _deriv_device_form(emme, SMALLEST_DERIV, device_omega, stream=st)
            assert _same(b0["M"], b1["M"]) and _same(b0["Mp"], b1["Mp"]) and np.array_equal(b0["iv"], b1["iv"])
        c0 = _sets_device_form(emme, "es15", {}, True, True)
        c1 = _sets_device_form(emme, "es15", {}, True, True, stream=st)
        assert _same(c0["M"], c1["M"]) and _same(c0["Mp"], c1["Mp"]) and np.array_equal(c0["iv"], c1["iv"])
        d0 = _newton_device_form(emme, oracle, SMALLEST_NEWTON)
        d1 = _newton_device_form(emme, oracle, SMALLEST_NEWTON, stream=st)
        for a, b in zip(d0, d1):
            assert _same(a, b)
        with _ctx(emme, example_tokamak(npoints=16)) as ctx:
            runs = []
            for stream in (None, st):
                try:
                    ctx.set_stream(stream.value if stream is not None else 0)
                    runs.append([_trace_solve_device(ctx, 5, stream), _qr_secant_device(ctx, 17, stream),
                                 _null_vectors_device(ctx, 37, stream), _eigenpair_device(ctx, 17, False, 1, stream)[0],
                                 _eigenpair_device(ctx, 17, True, 0, stream)[0], _moments_device(ctx, stream)])
                finally:
                    ctx.set_stream(0)
            for r0, r1 in zip(*runs):
                for a, b in zip(r0, r1):
                    assert _same(a, b)
    finally:
        db.destroy_stream(st)


# ---- G. pointer rules ----------------------------------------------------------------------------------------------
def _refused(emme, call, *words):
    with pytest.raises(emme.EmmeError) as e:
        call()
    assert e.value.code == EMME_EINVAL, (e.value.code, e.value.reason)
    for word in words:
        assert word in e.value.reason, e.value.reason


def test_mixed_sides_are_refused_by_the_fills(emme):
    dicts, st, w = _sets_cases()["es15"]
    w = np.asarray(w, dtype=np.complex128)

    def good(ctx):
        return (ctx.assemble(W_FILL, want_intervals=True), ctx.assemble_derivative(W_FILL, want_intervals=True),
                ctx.assemble_sets(st, w, want_derivative=True, want_intervals=True))

    with _bound(emme, dicts) as ctx:
        n, nb = ctx.dim, len(w)
        with _mats((nb, n, n), n) as buf, _vec(nb, np.complex128, n, data=w) as bw:
            _refused(emme, lambda: ctx.assemble_derivative(w, out_device_ptr=buf.ptr), "M and Mp")
            _refused(emme, lambda: ctx.assemble_derivative(w, mp_device_ptr=buf.ptr), "M and Mp")
            _refused(emme, lambda: ctx.assemble_sets(st, w, want_derivative=True, out_device_ptr=buf.ptr), "M and Mp")
            _refused(emme, lambda: ctx.assemble_sets(st, w, mp_device_ptr=buf.ptr), "M and Mp")
            buf.assert_untouched()
            # emme_assemble_batch: the header has always said that omega is a host array
            M = np.zeros((nb, n, n), dtype=np.complex128)
            for out in (M.ctypes.data, C.c_void_p(buf.ptr)):
                assert ctx.lib.emme_assemble_batch(ctx.h, C.c_void_p(bw.ptr), nb, out, None) == EMME_EINVAL
                assert "emme_assemble_batch" in emme.last_error() and "omega" in emme.last_error()
            assert not M.any()
            buf.assert_untouched()
            _after_call(inputs=[(bw, w)])
        after = good(ctx)
    with _bound(emme, dicts) as fresh:
        want = good(fresh)
    for a, b in zip(after, want):
        for x, y in zip(a, b):
            assert _same(x, y)


def test_mixed_sides_are_refused_by_the_linear_algebra(emme):
    n = 17
    A, B = _symmetric_batch(n)
    M, Mp, v = _constructed_batch(n)
    dw = np.array([0.01 - 0.002j, -0.003 + 0.004j, 0.002 + 0.001j])

    def good(ctx):
        return ctx.trace_solve(A, B) + ctx.qr_secant(A, B) + ctx.eigenpair_step(M, Mp, v) + \
            ctx.eigenpair_secant_step(M, Mp, dw, v)

    with _ctx(emme, example_tokamak(npoints=16)) as ctx:
        with _mats(A, n) as bA:
            for kw in (dict(a_device_ptr=bA.ptr), dict(b_device_ptr=bA.ptr)):
                _refused(emme, lambda: ctx.trace_solve(A, B, **kw), "A and B")
                _refused(emme, lambda: ctx.qr_secant(A, B, **kw), "A and B")
            for kw in (dict(m_device_ptr=bA.ptr), dict(mp_device_ptr=bA.ptr)):
                _refused(emme, lambda: ctx.eigenpair_step(M, Mp, v, **kw), "A and B")
            for kw in (dict(m_device_ptr=bA.ptr), dict(m_old_device_ptr=bA.ptr)):
                _refused(emme, lambda: ctx.eigenpair_secant_step(M, Mp, dw, v, **kw), "A and B")
            _after_call(inputs=[(bA, A)])
        after = good(ctx)
    with _ctx(emme, example_tokamak(npoints=16)) as fresh:
        want = good(fresh)
    for a, b in zip(after, want):
        assert _same(a, b)


NEWTON_ARRAYS = ("omega", "domega", "m", "mp", "info")


def test_mixed_sides_are_refused_by_the_newton_step(emme, oracle):
    """Each of the five arrays on the other side in turn: one device array among host ones, one host array among
    device ones."""
    case = "tokamak-trace"
    k = NEWTON[case]
    w, M, Mp = _newton_inputs(oracle, case)
    with _ctx(emme, k["d"]) as ctx:
        n, nb = ctx.dim, len(w)
        with _vec(nb, np.complex128, n, data=w) as bw, _vec(nb, np.complex128, n) as bdw, _mats(M, n) as bM, \
                _mats(Mp, n) as bMp, _vec(nb, np.int32, n) as binfo:
            ptrs = dict(omega=bw.ptr, domega=bdw.ptr, m=bM.ptr, mp=bMp.ptr, info=binfo.ptr)
            for odd in NEWTON_ARRAYS:
                for device_base in (False, True):
                    on_device = [a for a in NEWTON_ARRAYS if (a == odd) != device_base]
                    kw = {a + "_device_ptr": ptrs[a] for a in on_device}
                    _refused(emme, lambda: ctx.newton_step(nb if "omega" in on_device else w, M, Mp, **kw),
                             "emme_newton_step_batch", "omega, domega, M, Mp and info")
            bdw.assert_untouched(), binfo.assert_untouched()
            _after_call(inputs=[(bw, w), (bM, M), (bMp, Mp)])
        after = ctx.newton_step(w, M, Mp)
    with _ctx(emme, k["d"]) as fresh:
        want = fresh.newton_step(w, M, Mp)
    for a, b in zip(after, want):
        assert _same(a, b)


# ---- H. the checks bite --------------------------------------------------------------------------------------------
def test_the_checks_bite(emme):
    nbatch = len(W_FILL)
    with _ctx(emme, example_tokamak(npoints=16)) as ctx:
        n = ctx.dim
        with _mats((nbatch, n, n), n) as buf:
            ctx.assemble(W_FILL[:nbatch - 1], out_device_ptr=buf.ptr)
            buf.assert_guards_intact()
            with pytest.raises(AssertionError, match=rf"\(item, row, column\) = \({nbatch - 1}, 0, 0\)"):
                buf.assert_fully_written()
            ctx.assemble(W_FILL, out_device_ptr=buf.ptr)
            buf.assert_fully_written()
            buf.poke(-8, [0])  # the word in front of the payload
            with pytest.raises(AssertionError, match="front guard"):
                buf.assert_guards_intact()
            buf.poke(-8, [db.SENTINEL])
            buf.assert_guards_intact()
            buf.poke(buf.nbytes, [db.CANONICAL_NAN])  # one matrix entry too far
            with pytest.raises(AssertionError, match="back guard"):
                buf.assert_guards_intact()
