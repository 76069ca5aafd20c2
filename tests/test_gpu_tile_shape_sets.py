"""The table-free tile fill over parameter sets on electromagnetic and GK31 contexts (k_assemble_tile_shape_sets<PTS, NM>
/ k_assemble_tile_shape_sets_deriv<PTS, NM>): with the tile shapes at TILE_SHAPES_ALL a (parameter set,
contour class) group of a sets call goes through the matrix-core tile fill, a set per omega chunk -- 5 omegas x 3 moments
on an electromagnetic context, 16 omegas on an electrostatic GK31 one.

Every bound context uses node_cache_gb = 0, wl_min = 1, tile_uncached = 1, dense_min_tasks = 0: a chunk is then cut from
exactly one (set, class) group in the given order, in the sets call and in a per-set context alike, so the two can be
compared bit for bit.

Bars (tests/test_gpu_tile_sets.py's): bits against per-set tile-shape contexts; against the oracle entries
1e-10 * max|M|, interval counts equal item by item, roots 1e-9; 1e-13 * max|M| with equal counts where only the company of
a column differs; for strongly damped or handed-over wide omegas max(1e-10 * max|M|, 10 x the reference's own
sensitivity to omega (1 + 1e-13)), computed from the reference, never from the code under test."""
import numpy as np
import pytest

from oracle.binding import example_stellarator, example_tokamak

pytestmark = pytest.mark.gpu

# ---- the inputs of tests/test_gpu_tile_shapes.py (the one-set shape kernels' tests) ----
W_DAMPED = -0.142 - 1.469j
WS_EM = [-1.656 + 2.49j, -0.85 - 0.32j, 0.4 - 0.2j, W_DAMPED]
WS_ES = [-0.8 + 0.25j, -0.6 - 0.21j, 0.5 + 0.1j, W_DAMPED]
# trees with more than 64 intervals on one bisection level: (parameters, the wide omega, two ordinary omegas)
W_WIDE15 = -0.00552674 - 0.73419159j
W_WIDE31 = -0.005 - 2j
HAND_OVER = {
    "em15-stellarator": (lambda: example_stellarator(npoints=4, integration_start_points=15), W_WIDE15, WS_EM[:2]),
    "em31-stellarator": (lambda: example_stellarator(npoints=3, integration_precision=1e-9), W_WIDE31, WS_EM[:2]),
    "es31-tokamak": (lambda: example_tokamak(npoints=3, integration_start_points=31, integration_accuracy=1e-9,
                                             integration_precision=1e-9), W_WIDE31, WS_ES[:2]),
}


def _check_blocks(d, M):
    """include/solver.h:461-511: A and D symmetric, B antisymmetric, C = -B (electromagnetic); M symmetric (electrostatic)"""
    N = d["npoints"]
    for Mk in M:
        if d["beta_e"] == 0.0:
            assert np.array_equal(Mk, Mk.T)
            continue
        A, B, C, D = Mk[:N, :N], Mk[:N, N:], Mk[N:, :N], Mk[N:, N:]
        assert np.array_equal(A, A.T) and np.array_equal(D, D.T)
        assert np.array_equal(C, -B) and np.array_equal(B, -B.T)


TOL_M = 1e-10
TOL_W = 1e-9
TS = dict(node_cache_gb=0.0, wl_min=1, tile_uncached=1, dense_min_tasks=0)
K_ST, K_TK = 0.247487, 0.3182  # k_rho of the two shipped inputs

EM_SETS = [{}, dict(beta_e=0.03, eta_k=0.2), dict(k_rho=K_ST * 1.3)]
ES_SETS = [{}, dict(k_rho=K_TK * 1.7), dict(shat=1.35)]
# twelve items over three sets in shuffled set order; both contour classes inside sets 1 and 2; six omegas of Re omega < 0
# on set 1, so that an electromagnetic group spans two chunks (5 + 1).  The omegas: WS_EM / WS_ES and neighbours.
SET = [1, 0, 2, 1, 0, 1, 2, 1, 1, 0, 1, 1]
W_EM = [WS_EM[0], WS_EM[1], WS_EM[2], WS_EM[2], WS_EM[0], WS_EM[1], -1.6 + 2.4j, -1.6 + 2.4j, -1.7 + 2.55j, W_DAMPED,
        -1.64 + 2.465j, -0.9 + 0.4j]
W_ES = [WS_ES[0], WS_ES[1], WS_ES[2], WS_ES[2], WS_ES[0], WS_ES[1], -0.7 + 0.15j, -0.7 + 0.15j, -0.5 + 0.1j, W_DAMPED,
        -0.792 + 0.2475j, -0.9 + 0.2j]


def _em31(npoints=10, **over):
    return example_stellarator(npoints=npoints, **over)


def _em15(npoints=10, **over):
    return example_stellarator(npoints=npoints, integration_start_points=15, **over)


def _es31(npoints=12, **over):
    return example_tokamak(npoints=npoints, integration_start_points=31, **over)


SHAPES = {"em31": (_em31, EM_SETS, W_EM), "em15": (_em15, EM_SETS, W_EM), "es31": (_es31, ES_SETS, W_ES)}


def _dicts(shape, npoints=None):
    make, overs, _ = SHAPES[shape]
    return [make(**over) if npoints is None else make(npoints=npoints, **over) for over in overs]


def _symbol(d, deriv=False, sets=True):
    return "k_assemble_tile_shape%s%s<%d, %d>" % ("_sets" if sets else "", "_deriv" if deriv else "",
                                                  d["integration_start_points"], 3 if d["beta_e"] != 0.0 else 1)


def _ctx(emme, d, shapes=None, **options):
    ctx = emme.Context(emme.params_from_dict(d), **options)
    if shapes is not None:
        ctx.set_tile_shapes(shapes)
    return ctx


def _bound(emme, dicts, shapes=None, **options):
    ctx = _ctx(emme, dicts[0], shapes, **options)
    ctx.bind_param_sets([emme.params_from_dict(d) for d in dicts])
    return ctx


def _bits(a):
    return np.ascontiguousarray(a).view(np.float64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b), equal_nan=True)


def _mode(ctx):
    return ctx.lib.emme_ctx_fill_mode(ctx.h)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _bar(scale, ref, ref_shifted):
    """TOL_M of the scale, or 10 x the reference's own sensitivity to the last bits of omega where that is larger"""
    return max(TOL_M * scale, 10 * np.abs(ref - ref_shifted).max())


_ORACLE = {}


def _oracle_items(oracle, shape):
    """The oracle's matrix, interval total and matrix at omega (1 + 1e-13) of the twelve items: computed once per shape"""
    if shape not in _ORACLE:
        po = [oracle.params(d) for d in _dicts(shape)]
        out = []
        for s, w in zip(SET, SHAPES[shape][2]):
            Mo, tot = oracle.assemble(po[s], complex(w))
            Mo2, _ = oracle.assemble(po[s], complex(w) * (1 + 1e-13))
            _freeze(Mo, Mo2)
            out.append((Mo, tot, Mo2))
        _ORACLE[shape] = out
    return _ORACLE[shape]


_SETS_TILE = {}


def _sets_tile(emme, shape):
    """The twelve items through the tile fill over sets, plain and (deriv_cached = 1) with the derivative: computed
    once per shape, shared, never modified"""
    if shape not in _SETS_TILE:
        dicts, ws = _dicts(shape), SHAPES[shape][2]
        with _bound(emme, dicts, emme.TILE_SHAPES_ALL, **TS) as ctx:
            ctx.profile(True)
            M, iv = ctx.assemble_sets(SET, ws, want_intervals=True)
            mode, symbol, name = _mode(ctx), ctx.fill_kernel_symbol(), ctx.fill_kernel()
            tasks = ctx.profile_read(reset=True).tile_tasks
        with _bound(emme, dicts, emme.TILE_SHAPES_ALL, deriv_cached=1, **TS) as ctx:
            ctx.profile(True)
            M2, Mp, iv2 = ctx.assemble_sets(SET, ws, want_derivative=True, want_intervals=True)
            mode2 = _mode(ctx)
            tasks2 = ctx.profile_read(reset=True).tile_tasks
        _freeze(M, iv, M2, Mp, iv2)
        _SETS_TILE[shape] = dict(M=M, iv=iv, mode=mode, symbol=symbol, name=name, tasks=tasks, M2=M2, Mp=Mp, iv2=iv2,
                                 mode2=mode2, tasks2=tasks2)
    return _SETS_TILE[shape]


# ---- 1. bit for bit against per-set tile-shape contexts ---------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fill_matches_per_set_tile_shape_contexts_bit_for_bit(emme, oracle, shape):
    dicts, ws = _dicts(shape), SHAPES[shape][2]
    groups = {}
    for s, w in zip(SET, ws):
        groups[(s, w.real < 0)] = groups.get((s, w.real < 0), 0) + 1
    assert len(set(SET)) == 3 and any((s, True) in groups and (s, False) in groups for s in set(SET))
    assert max(groups.values()) > 5  # an electromagnetic group of two chunks
    # every (set, omega) has a finite matrix (CPU)
    for b, (Mo, tot, _) in enumerate(_oracle_items(oracle, shape)):
        assert np.isfinite(Mo).all() and tot > 0, (shape, b)
    got = _sets_tile(emme, shape)
    print(f"{shape}: mode {got['mode']}, symbol {got['symbol']}, tile tasks {got['tasks']} / {got['tasks2']}")
    assert got["mode"] == 7 and got["mode2"] == 7
    assert got["symbol"] == _symbol(dicts[0])
    assert got["tasks"] > 0 and got["tasks2"] > 0
    # the derivative call's M and counts are the plain call's: K and G decide as in the plain kernel
    assert _same_bits(got["M2"], got["M"]) and np.array_equal(got["iv2"], got["iv"])
    for s in sorted(set(SET)):
        items = [b for b in range(len(SET)) if SET[b] == s]
        with _ctx(emme, dicts[s], emme.TILE_SHAPES_ALL, deriv_cached=1, **TS) as ctx:
            ctx.profile(True)
            M, iv = ctx.assemble([ws[b] for b in items], want_intervals=True)
            assert ctx.fill_kernel_symbol() == _symbol(dicts[s], sets=False)
            assert ctx.profile_read(reset=True).tile_tasks > 0
            Md, Mp, ivd = ctx.assemble_derivative([ws[b] for b in items], want_intervals=True)
            assert ctx.profile_read(reset=True).tile_tasks > 0  # the derivative went through the tile fill too
        for q, b in enumerate(items):
            diff = np.abs(M[q] - got["M"][b]).max() / np.abs(M[q]).max()
            diffp = np.abs(Mp[q] - got["Mp"][b]).max() / np.abs(Mp[q]).max()
            print(f"set {s} item {b}: intervals {got['iv'][b]} / {iv[q]}, max|dM|/max|M| = {diff:.2e}, "
                  f"max|dM'|/max|M'| = {diffp:.2e}")
            assert got["iv"][b] == iv[q] and got["iv2"][b] == ivd[q], (s, b)
            assert _same_bits(M[q], got["M"][b]), (s, b, diff)
            assert _same_bits(Md[q], got["M2"][b]), (s, b)
            assert _same_bits(Mp[q], got["Mp"][b]), (s, b, diffp)


# ---- 2. against the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fill_matches_the_oracle(emme, oracle, shape):
    """Set 1 of the electromagnetic shapes has another beta_e than the context's own set: diag_d and the b table of the
    diagonal block, and the kappa_e terms, must be the item's set's."""
    dicts, ws = _dicts(shape), SHAPES[shape][2]
    if dicts[0]["beta_e"] != 0.0:
        assert dicts[1]["beta_e"] != dicts[0]["beta_e"]
    got = _sets_tile(emme, shape)
    for b, ((Mo, tot, Mo2), s, w) in enumerate(zip(_oracle_items(oracle, shape), SET, ws)):
        scale = np.abs(Mo).max()
        # (the strongly damped omega: entries are remainders of integrand values many orders larger, and the bar is the
        # one tests/test_gpu_tile_shapes.py gives the same omega on the one-set kernels, sensitive=(W_DAMPED,) -- the
        # larger of the entry bar and 10 x the ORACLE's own change under omega (1 + 1e-13).  Every other item: TOL_M.)
        bar = _bar(scale, Mo, Mo2) if complex(w) == W_DAMPED else TOL_M * scale
        err = np.abs(got["M"][b] - Mo).max()
        print(f"item {b} set {s} omega {complex(w)}: error {err / scale:.3e} of max|M|, bar {bar / scale:.3e}, "
              f"intervals {got['iv'][b]} / {tot}")
        assert got["iv"][b] == tot, (b, s)
        assert err <= bar, (b, s, err / scale, bar / scale)
        _check_blocks(dicts[s], got["M"][b:b + 1])
        if dicts[s]["beta_e"] != 0.0:
            # the diagonal blocks as the oracle has them, entry for entry on the diagonals
            N = dicts[s]["npoints"]
            for blk in (np.s_[:N, :N], np.s_[:N, N:], np.s_[N:, :N], np.s_[N:, N:]):
                assert np.abs(np.diag(got["M"][b][blk]) - np.diag(Mo[blk])).max() <= bar, (b, s)


# ---- 3. items do not leak ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_items_do_not_leak(emme, shape):
    dicts, ws = _dicts(shape), SHAPES[shape][2]
    ref = _sets_tile(emme, shape)
    # a permutation that keeps each set's internal order: set 2's items first, then set 0's, then set 1's
    keep = [b for s in (2, 0, 1) for b in range(len(SET)) if SET[b] == s]
    # ... and an arbitrary one: the columns of a chunk in another order and in other company
    anyp = [7, 3, 10, 1, 9, 5, 0, 11, 2, 8, 6, 4]
    assert sorted(keep) == sorted(anyp) == list(range(len(SET))) and keep != list(range(len(SET)))
    with _bound(emme, dicts, emme.TILE_SHAPES_ALL, **TS) as ctx:
        M, iv = ctx.assemble_sets([SET[k] for k in keep], [ws[k] for k in keep], want_intervals=True)
        assert _mode(ctx) == 7
        Ma, iva = ctx.assemble_sets([SET[k] for k in anyp], [ws[k] for k in anyp], want_intervals=True)
        assert _mode(ctx) == 7
    for q, k in enumerate(keep):
        assert iv[q] == ref["iv"][k] and _same_bits(M[q], ref["M"][k]), (q, k)
    for q, k in enumerate(anyp):
        diff = np.abs(Ma[q] - ref["M"][k]).max() / np.abs(ref["M"][k]).max()
        print(f"position {q} item {k}: max|dM|/max|M| = {diff:.2e}")
        assert iva[q] == ref["iv"][k], (q, k)
        assert diff <= 1e-13, (q, k, diff)


# ---- 4. small and odd grids -------------------------------------------------------------------------------------
GRIDS = [("em31", n) for n in (2, 3, 7)] + [("em15", n) for n in (2, 3, 7)] + [("es31", n) for n in (2, 5)]


@pytest.mark.parametrize("shape,n", GRIDS, ids=[f"{s}-{n}" for s, n in GRIDS])
def test_small_and_odd_grids(emme, oracle, shape, n):
    """One pair, three, ten and 21 pairs: partial tiles, and fewer tiles than a workgroup has waves.  Two sets, four
    items each, both contour classes."""
    dicts = _dicts(shape, npoints=n)[:2]
    w3 = (WS_EM if dicts[0]["beta_e"] != 0.0 else WS_ES)[:3]
    st = [1, 0, 0, 1, 1, 0, 1, 0]
    ws = [w3[0], w3[0], w3[1], w3[1], w3[2], w3[2], w3[0] * 0.97, w3[1] * 1.05]
    with _bound(emme, dicts, emme.TILE_SHAPES_ALL, **TS) as ctx:
        M, iv = ctx.assemble_sets(st, ws, want_intervals=True)
        assert _mode(ctx) == 7 and ctx.fill_kernel_symbol() == _symbol(dicts[0])
    po = [oracle.params(d) for d in dicts]
    for b, (s, w) in enumerate(zip(st, ws)):
        Mo, tot = oracle.assemble(po[s], complex(w))
        err = np.abs(M[b] - Mo).max() / np.abs(Mo).max()
        print(f"item {b} set {s}: max|dM|/max|M| = {err:.2e}, intervals {iv[b]} / {tot}")
        assert err <= TOL_M and iv[b] == tot, (b, s, err, iv[b], tot)
        _check_blocks(dicts[s], M[b:b + 1])


# ---- 5. hand-over with several segments -------------------------------------------------------------------------
HAND_CASES = ["em15-stellarator", "em31-stellarator", "es31-tokamak"]
HAND_SET = [0, 1, 2, 0, 2, 1]


def _hand_inputs(case):
    make, wide, ordinary = HAND_OVER[case]
    base = make()
    other = dict(base, k_rho=base["k_rho"] * (1.3 if base["beta_e"] != 0.0 else 1.7))
    assert wide in (W_WIDE15, W_WIDE31)
    return [other, base, dict(base)], [ordinary[0], wide, ordinary[1], ordinary[1], wide, ordinary[0]], wide


@pytest.mark.parametrize("case", HAND_CASES)
def test_hand_over_with_several_segments(emme, oracle, case):
    """Sets 1 and 2 are the same parameters and both hold the wide omega: their segments receive the integrals a
    per-set tile-shape context hands over for the same items; the sets call hands over the sum over the sets."""
    dicts, ws, wide = _hand_inputs(case)
    one = []
    for s in range(3):
        with _ctx(emme, dicts[s], emme.TILE_SHAPES_ALL, **TS) as ctx:
            ctx.assemble([ws[b] for b in range(len(ws)) if HAND_SET[b] == s])
            assert ctx.fill_kernel_symbol() == _symbol(dicts[s], sets=False)
            one.append(ctx.last_deferred())
    with _bound(emme, dicts, emme.TILE_SHAPES_ALL, **TS) as ctx:
        ctx.profile(True)
        M, iv = ctx.assemble_sets(HAND_SET, ws, want_intervals=True)
        assert _mode(ctx) == 7 and ctx.fill_kernel_symbol() == _symbol(dicts[0])
        handed = ctx.last_deferred()
        pr = ctx.profile_read(reset=True)
    with _bound(emme, dicts, emme.TILE_SHAPES_ALL, deriv_cached=1, **TS) as ctx:
        ctx.profile(True)
        M2, Mp, iv2 = ctx.assemble_sets(HAND_SET, ws, want_derivative=True, want_intervals=True)
        assert _mode(ctx) == 7
        handed2 = ctx.last_deferred()
        pr2 = ctx.profile_read(reset=True)
    print(f"handed over: {handed} integrals, with the derivative {handed2} (per-set contexts: {one}); deferred launches "
          f"{pr.deferred_launches} / {pr2.deferred_launches}")
    assert sum(1 for v in one if v > 0) >= 2
    assert handed == sum(one) and pr.deferred_launches > 0
    assert handed2 == sum(one) and pr2.deferred_launches > 0
    po = [oracle.params(d) for d in dicts]
    for b, (s, w) in enumerate(zip(HAND_SET, ws)):
        Mo, tot = oracle.assemble(po[s], complex(w))
        scale = np.abs(Mo).max()
        bar = TOL_M * scale
        if complex(w) == wide:
            bar = _bar(scale, Mo, oracle.assemble(po[s], complex(w) * (1 + 1e-13))[0])
        for which, Mg, ivg in (("plain", M, iv), ("derivative", M2, iv2)):
            err = np.abs(Mg[b] - Mo).max()
            print(f"{which} item {b} set {s} omega {complex(w)}: error {err / scale:.3e} of max|M|, bar {bar / scale:.3e}")
            assert ivg[b] == tot, (which, b, s, ivg[b], tot)
            assert err <= bar, (which, b, s, err / scale, bar / scale)
        if complex(w) != wide:
            continue
        # M' of the handed-over items: a per-set context's lanes-are-nodes derivative kernel, and its own M' spread
        with _ctx(emme, dicts[s], node_cache_gb=0) as ctx:
            _, Mpr = ctx.assemble_derivative([w])
            _, Mpr2 = ctx.assemble_derivative([complex(w) * (1 + 1e-13)])
        scale = np.abs(Mpr[0]).max()
        bar = _bar(scale, Mpr[0], Mpr2[0])
        err = np.abs(Mp[b] - Mpr[0]).max()
        print(f"item {b} set {s} M': error {err / scale:.3e} of max|M'|, bar {bar / scale:.3e}")
        assert err <= bar, (b, s, err / scale, bar / scale)


# ---- 6. routing -------------------------------------------------------------------------------------------------
R_SET = [1, 1, 0, 1, 1, 1]
R_W = [WS_EM[0], WS_EM[1], -0.9 + 0.4j, -1.6 + 2.4j, -1.7 + 2.55j, -1.64 + 2.465j]


def test_routing_mixed_call(emme):
    """wl_min = 4: a group of 5 (set 1, Re omega < 0) through the tile fill, a group of 1 (set 0) through k_assemble_sets
    in the second pass of the same call."""
    dicts = _dicts("em31")
    with _bound(emme, dicts, emme.TILE_SHAPES_ALL, **dict(TS, wl_min=4)) as ctx:
        ctx.profile(True)
        M, iv = ctx.assemble_sets(R_SET, R_W, want_intervals=True)
        assert _mode(ctx) == 7 and ctx.fill_kernel_symbol() == _symbol(dicts[0])
        pr = ctx.profile_read(reset=True)
        assert pr.tile_tasks == 3 and pr.matrices == 6  # one chunk of 5 on the 3 tiles of 45 pairs
        # a call whose groups are all below wl_min: the nodes kernel alone
        Ms, ivs = ctx.assemble_sets(R_SET[1:4], R_W[1:4], want_intervals=True)
        assert _mode(ctx) == 6
        assert ctx.profile_read(reset=True).tile_tasks == 0
    with _bound(emme, dicts, emme.TILE_SHAPES_ALL, node_cache_gb=0.0) as ctx:  # the all-nodes call
        Mn, ivn = ctx.assemble_sets(R_SET, R_W, want_intervals=True)
        assert _mode(ctx) == 6
    with _bound(emme, dicts, emme.TILE_SHAPES_ALL, **TS) as ctx:  # the all-tile call
        Mt, ivt = ctx.assemble_sets(R_SET, R_W, want_intervals=True)
        assert _mode(ctx) == 7
    assert np.array_equal(iv, ivn) and np.array_equal(iv, ivt)
    assert _same_bits(M[2], Mn[2])
    for b in (0, 1, 3, 4, 5):
        assert _same_bits(M[b], Mt[b]), b
        assert np.abs(M[b] - Mn[b]).max() <= TOL_M * np.abs(Mn[b]).max()
    for q, b in enumerate((1, 2, 3)):
        assert _same_bits(Ms[q], Mn[b]) and ivs[q] == ivn[b], b


def _sets_fill(emme, dicts, shapes, deriv, **options):
    with _bound(emme, dicts, shapes, **options) as ctx:
        ctx.profile(True)
        out = ctx.assemble_sets(R_SET, R_W, want_derivative=deriv, want_intervals=True)
        return out, _mode(ctx), ctx.fill_kernel_symbol(), ctx.profile_read(reset=True).tile_tasks


@pytest.mark.parametrize("case", ["tight-accuracy", "deriv-not-cached"])
def test_routing_keeps_the_nodes_kernel(emme, case):
    dicts, deriv = _dicts("em31"), False
    if case == "tight-accuracy":  # (no item on the tight set: the rule asks every BOUND set)
        dicts = dicts + [_em31(integration_accuracy=1e-12)]
    else:
        deriv = True
    got, mode, symbol, tasks = _sets_fill(emme, dicts, emme.TILE_SHAPES_ALL, deriv, **TS)
    assert mode == 6 and symbol.startswith("k_assemble_sets<") and tasks == 0, (case, mode, symbol, tasks)
    # the same call without the option
    ref, rmode, _, _ = _sets_fill(emme, dicts, emme.TILE_SHAPES_ALL, deriv, node_cache_gb=0.0)
    assert rmode == 6
    for a, b in zip(got, ref):
        assert _same_bits(a, b), case
    if case == "deriv-not-cached":  # (with deriv_cached the same call does take the tile fill)
        _, mode7, _, tasks7 = _sets_fill(emme, dicts, emme.TILE_SHAPES_ALL, True, deriv_cached=1, **TS)
        assert mode7 == 7 and tasks7 > 0


def test_routing_follows_the_tile_shapes_of_a_live_context(emme):
    dicts = _dicts("em31")
    with _bound(emme, dicts, emme.TILE_SHAPES_ALL, **TS) as ctx:
        ctx.profile(True)
        M7, iv7 = ctx.assemble_sets(R_SET, R_W, want_intervals=True)
        assert _mode(ctx) == 7 and ctx.profile_read(reset=True).tile_tasks > 0
        ctx.set_tile_shapes(emme.TILE_SHAPES_ES15)
        M6, iv6 = ctx.assemble_sets(R_SET, R_W, want_intervals=True)
        assert _mode(ctx) == 6 and ctx.fill_kernel_symbol().startswith("k_assemble_sets<")
        assert ctx.profile_read(reset=True).tile_tasks == 0
        ctx.set_tile_shapes(emme.TILE_SHAPES_ALL)
        M7b, iv7b = ctx.assemble_sets(R_SET, R_W, want_intervals=True)
        assert _mode(ctx) == 7
    assert np.array_equal(iv7, iv6) and np.array_equal(iv7, iv7b) and _same_bits(M7, M7b)
    for b in range(len(R_SET)):
        assert np.abs(M7[b] - M6[b]).max() <= TOL_M * np.abs(M6[b]).max(), b


# ---- 7. root searches -------------------------------------------------------------------------------------------
# (guess, set, the CPU oracle's secant iteration count with tol = 1e-6: every chain converges inside the step limit, its
# last relative step <= 8.4e-8 after a step >= 1.0e-5 -- a factor >= 10 away from tol on either side, so equal iteration
# counts is a fair demand.  The em31 chains of a set end at two different roots.)
SEARCHES = {
    "em31": ([_em31(npoints=16), _em31(npoints=16, beta_e=0.03, eta_k=0.2)],
             [(0, -0.4 + 0.55j, 5), (0, -0.36 + 0.5j, 6), (0, -0.3 + 0.6j, 5), (1, -0.4 + 0.55j, 10),
              (1, -0.12 + 0.57j, 4), (1, -0.3 + 0.6j, 8)]),
    "es31": ([_es31(npoints=16), _es31(npoints=16, k_rho=K_TK * 1.7)],
             [(0, -0.853 - 0.078j, 9), (0, -0.806 - 0.042j, 7), (1, -0.806 - 0.042j, 4), (1, -0.82 - 0.07j, 4)]),
}


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("shape", sorted(SEARCHES))
def test_root_searches(emme, oracle, shape, exact):
    dicts, chains = SEARCHES[shape]
    st, g = [c[0] for c in chains], [c[1] for c in chains]
    options = dict(TS, deriv_cached=1) if exact else TS
    with _bound(emme, dicts, emme.TILE_SHAPES_ALL, **options) as ctx:
        ctx.profile(True)
        roots, iters, info = ctx.solve_roots_sets(st, g, exact=bool(exact), tol=1e-6)
        assert _mode(ctx) == 7 and ctx.fill_kernel_symbol() == _symbol(dicts[0]), ctx.fill_kernel()
        assert ctx.profile_read(reset=True).tile_tasks > 0
        mats = [ctx.final_matrix(b) for b in range(len(st))]
    po = [oracle.params(d) for d in dicts]
    if not exact:
        for b, (s, gb, want) in enumerate(chains):
            r_or, its_or, _, _ = oracle.solve_root(po[s], complex(gb))
            print(f"chain {b} set {s}: root {roots[b]:.12f} info {info[b]}, iters {iters[b]} (oracle's secant search "
                  f"{len(its_or)}), |w - w_oracle| = {abs(roots[b] - r_or):.2e}")
            assert np.isfinite(r_or) and len(its_or) == want, (b, len(its_or), want)
            assert info[b] == 0, b
            assert abs(roots[b] - r_or) <= TOL_W, b
            assert iters[b] == len(its_or), b
        for s in set(st) if shape == "em31" else ():  # (em31: the chains of a set end at two different roots)
            assert max(abs(roots[b] - roots[c]) for b in range(len(st)) for c in range(len(st))
                       if st[b] == st[c] == s) > 1e-3, s
        return
    for s in sorted(set(st)):
        mine = [b for b in range(len(st)) if st[b] == s]
        with _ctx(emme, dicts[s], emme.TILE_SHAPES_ALL, **options) as ctx:
            ctx.profile(True)
            r1, i1, f1 = ctx.solve_roots_newton([g[b] for b in mine], tol=1e-6)
            assert ctx.profile_read(reset=True).tile_tasks > 0
        for q, b in enumerate(mine):
            Mw, _ = oracle.assemble(po[s], complex(roots[b]))
            err = np.abs(mats[b] - Mw).max() / np.abs(Mw).max()
            print(f"chain {b} set {s}: root {roots[b]:.12f} info {info[b]} / {f1[q]}, iters {iters[b]} / {i1[q]}, "
                  f"|w - w_ctx|/|w| = {abs(roots[b] - r1[q]) / abs(r1[q]):.2e}, final matrix {err:.2e} of max|M|")
            assert info[b] == f1[q] and iters[b] == i1[q], b
            assert abs(roots[b] - r1[q]) <= 1e-9 * abs(r1[q]), b
            assert err <= 1e-8, (b, err)
