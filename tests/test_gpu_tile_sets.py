"""The table-free tile fill over parameter sets (k_assemble_tile_sets / k_assemble_tile_sets_deriv):
a (parameter set, contour class) group of a sets call goes through the matrix-core tile fill, a set per omega chunk.

Every bound context uses node_cache_gb = 0, wl_min = 1, tile_uncached = 1, dense_min_tasks = 0: a chunk is then exactly
one (set, class) group of <= 16 omegas in the given order, in the sets call and in a per-set context alike, so the two
can be compared bit for bit.

Bars: bits against per-set tile contexts; against the oracle the project's own -- entries 1e-10 * max|M|, interval
counts equal item by item, roots 1e-9; 1e-13 * max|M| with equal counts where only the company of a column differs
(test_tile_fill_matches_oracle's batch-versus-single bar)."""
import numpy as np
import pytest

from oracle.binding import example_stellarator, example_tokamak

pytestmark = pytest.mark.gpu

TOL_M = 1e-10
TOL_W = 1e-9
TS = dict(node_cache_gb=0.0, wl_min=1, tile_uncached=1, dense_min_tasks=0)
W_WIDE = -0.00552674 - 0.73419159j  # test_gpu_tile_fill.py: more than 64 intervals on one bisection level

# the five ES15 sets of test_gpu_param_sets.py (npoints 16: 120 pairs, 8 tiles, the last partial)
ES15 = [example_tokamak(npoints=16), example_tokamak(npoints=16, k_rho=0.3182 * 1.7),
        example_tokamak(npoints=16, eta_i=3.13 * 0.6), example_tokamak(npoints=16, shat=1.35),
        example_tokamak(npoints=16, conf="cylinder")]
# twelve items over three sets in shuffled set order; both contour classes inside set 3; |Im omega| <= 0.5
SET = [3, 0, 4, 3, 0, 3, 4, 0, 3, 4, 3, 0]
W = [-0.8 + 0.25j, -0.5 + 0.1j, -0.3 - 0.05j, 0.4 + 0.2j, -0.6 + 0.3j, -0.2 + 0.15j, -0.7 + 0.15j, -0.9 + 0.2j,
     0.6 + 0.1j, -0.4 - 0.1j, -0.792 + 0.2475j, -0.35 + 0.05j]


def _ctx(emme, d, **options):
    return emme.Context(emme.params_from_dict(d), **options)


def _bound(emme, dicts, **options):
    ctx = _ctx(emme, dicts[0], **options)
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


@pytest.fixture(scope="module")
def sets_tile(emme):
    """The twelve items through the tile fill over sets, plain and (deriv_cached = 1) with the derivative: computed
    once, shared, never modified"""
    with _bound(emme, ES15, **TS) as ctx:
        M, iv = ctx.assemble_sets(SET, W, want_intervals=True)
        mode, symbol, name = _mode(ctx), ctx.fill_kernel_symbol(), ctx.fill_kernel()
    with _bound(emme, ES15, deriv_cached=1, **TS) as ctx:
        M2, Mp, iv2 = ctx.assemble_sets(SET, W, want_derivative=True, want_intervals=True)
        mode2 = _mode(ctx)
    _freeze(M, iv, M2, Mp, iv2)
    return dict(M=M, iv=iv, mode=mode, symbol=symbol, name=name, M2=M2, Mp=Mp, iv2=iv2, mode2=mode2)


@pytest.fixture(scope="module")
def per_set_tile(emme):
    """Per set, a per-set context with the same options fills that set's omegas in the same order: k_assemble_tile and
    (deriv_cached = 1) k_assemble_tile_deriv"""
    out = {}
    for s in sorted(set(SET)):
        items = [b for b in range(len(SET)) if SET[b] == s]
        with _ctx(emme, ES15[s], deriv_cached=1, **TS) as ctx:
            ctx.profile(True)
            M, iv = ctx.assemble([W[b] for b in items], want_intervals=True)
            assert ctx.fill_kernel_symbol() == "k_assemble_tile"
            assert ctx.profile_read(reset=True).tile_tasks > 0
            Md, Mp, ivd = ctx.assemble_derivative([W[b] for b in items], want_intervals=True)
            assert ctx.profile_read(reset=True).tile_tasks > 0  # the derivative went through the tile fill too
        _freeze(M, iv, Md, Mp, ivd)
        out[s] = dict(items=items, M=M, iv=iv, Md=Md, Mp=Mp, ivd=ivd)
    return out


# ---- 1. bit for bit against per-set tile contexts ---------------------------------------------------------------
def test_fill_matches_per_set_tile_contexts_bit_for_bit(sets_tile, per_set_tile):
    assert len(set(SET)) >= 3 and any(
        len({W[b].real < 0 for b in range(len(SET)) if SET[b] == s}) == 2 for s in set(SET))
    assert sets_tile["symbol"] == "k_assemble_tile_sets" and sets_tile["mode"] == 7
    assert sets_tile["name"].startswith("k_assemble_tile_sets (")
    for s, ref in per_set_tile.items():
        for q, b in enumerate(ref["items"]):
            diff = np.abs(ref["M"][q] - sets_tile["M"][b]).max() / np.abs(ref["M"][q]).max()
            print(f"set {s} item {b}: intervals {sets_tile['iv'][b]} / {ref['iv'][q]}, max|dM|/max|M| = {diff:.2e}")
            assert sets_tile["iv"][b] == ref["iv"][q], (s, b)
            assert _same_bits(ref["M"][q], sets_tile["M"][b]), (s, b, diff)


# ---- 2. against the oracle --------------------------------------------------------------------------------------
def test_fill_matches_the_oracle(oracle, sets_tile):
    assert all(abs(w.imag) <= 0.5 for w in W)
    po = [oracle.params(d) for d in ES15]
    for b, (s, om) in enumerate(zip(SET, W)):
        Mo, tot = oracle.assemble(po[s], complex(om))
        err = np.abs(sets_tile["M"][b] - Mo).max() / np.abs(Mo).max()
        print(f"item {b} set {s}: max|dM|/max|M| = {err:.2e}, intervals {sets_tile['iv'][b]} / {tot}")
        assert err <= TOL_M, (b, s, err)
        assert sets_tile["iv"][b] == tot, (b, s)


# ---- 3. the derivative ------------------------------------------------------------------------------------------
def test_derivative_fill(sets_tile, per_set_tile):
    assert sets_tile["mode2"] == 7
    # K and G decide as in the plain kernel: its M and counts, bit for bit
    assert _same_bits(sets_tile["M2"], sets_tile["M"]) and np.array_equal(sets_tile["iv2"], sets_tile["iv"])
    for s, ref in per_set_tile.items():
        for q, b in enumerate(ref["items"]):
            diff = np.abs(ref["Mp"][q] - sets_tile["Mp"][b]).max() / np.abs(ref["Mp"][q]).max()
            print(f"set {s} item {b}: max|dM'|/max|M'| = {diff:.2e}")
            assert sets_tile["iv2"][b] == ref["ivd"][q], (s, b)
            assert _same_bits(ref["Md"][q], sets_tile["M2"][b]), (s, b)
            assert _same_bits(ref["Mp"][q], sets_tile["Mp"][b]), (s, b, diff)


# ---- 4. more than one chunk per group ---------------------------------------------------------------------------
def test_several_chunks_per_group(emme, oracle):
    """npoints 24 (18 tiles), two sets: 20 omegas of one class on set 1 (chunks of 16 and 4), 3 on set 0, one of them
    of the other class (chunks of 2 and 1)."""
    dicts = [example_tokamak(npoints=24), example_tokamak(npoints=24, k_rho=0.3182 * 1.3)]
    rng = np.random.default_rng(5)
    w1 = rng.uniform(-1.2, -0.4, 20) + 1j * rng.uniform(0.05, 0.4, 20)
    w0 = [-0.8 + 0.25j, 0.5 + 0.1j, -0.6 - 0.21j]
    st = [1] * 7 + [0] + [1] * 6 + [0] + [1] * 7 + [0]
    it1, it0 = iter(w1), iter(w0)
    ws = [next(it1) if s == 1 else next(it0) for s in st]
    with _bound(emme, dicts, **TS) as ctx:
        ctx.profile(True)
        M, iv = ctx.assemble_sets(st, ws, want_intervals=True)
        assert _mode(ctx) == 7
        pr = ctx.profile_read(reset=True)
        M2, iv2 = ctx.assemble_sets(st, ws, want_intervals=True)
    ntiles = (24 * 23 // 2 + 15) // 16
    assert ntiles == 18
    print(f"tile tasks {pr.tile_tasks}")
    assert pr.tile_tasks % ntiles == 0 and pr.tile_tasks > 3 * ntiles and pr.matrices == len(st)
    po = [oracle.params(d) for d in dicts]
    for b, (s, om) in enumerate(zip(st, ws)):
        Mo, tot = oracle.assemble(po[s], complex(om))
        err = np.abs(M[b] - Mo).max() / np.abs(Mo).max()
        print(f"item {b} set {s}: max|dM|/max|M| = {err:.2e}, intervals {iv[b]} / {tot}")
        assert err <= TOL_M and iv[b] == tot, (b, s, err, iv[b], tot)
    # two calls give the same bits
    assert np.array_equal(iv, iv2) and _same_bits(M, M2)


# ---- 5. items do not leak ---------------------------------------------------------------------------------------
def test_items_do_not_leak(emme, sets_tile):
    # a permutation that keeps each set's internal order: set 4's items first, then set 0's, then set 3's
    keep = [b for s in (4, 0, 3) for b in range(len(SET)) if SET[b] == s]
    # ... and an arbitrary one: the columns of a chunk in another order
    anyp = [7, 3, 10, 1, 9, 5, 0, 11, 2, 8, 6, 4]
    assert sorted(keep) == sorted(anyp) == list(range(len(SET))) and keep != list(range(len(SET)))
    with _bound(emme, ES15, **TS) as ctx:
        M, iv = ctx.assemble_sets([SET[k] for k in keep], [W[k] for k in keep], want_intervals=True)
        assert _mode(ctx) == 7
        Ma, iva = ctx.assemble_sets([SET[k] for k in anyp], [W[k] for k in anyp], want_intervals=True)
    for q, k in enumerate(keep):
        assert iv[q] == sets_tile["iv"][k] and _same_bits(M[q], sets_tile["M"][k]), (q, k)
    for q, k in enumerate(anyp):
        ref = sets_tile["M"][k]
        diff = np.abs(Ma[q] - ref).max() / np.abs(ref).max()
        print(f"position {q} item {k}: max|dM|/max|M| = {diff:.2e}")
        assert iva[q] == sets_tile["iv"][k], (q, k)
        assert diff <= 1e-13, (q, k, diff)


# ---- 6. hand-over with two non-empty segments -------------------------------------------------------------------
HAND = [example_tokamak(npoints=5, k_rho=0.3182 * 1.7), example_tokamak(npoints=5), example_tokamak(npoints=5)]
HAND_SET = [0, 1, 2, 0, 2, 1]
HAND_W = [-0.8 + 0.25j, W_WIDE, -0.6 - 0.21j, -0.5 + 0.1j, W_WIDE, -0.7 + 0.15j]


def _bar(scale, ref, ref_shifted):
    """TOL_M of the scale, or 10 x the reference's own sensitivity to the last bits of omega where that is larger
    (test_tile_fill_hands_over_full_level_lists)"""
    return max(TOL_M * scale, 10 * np.abs(ref - ref_shifted).max())


def _check_hand_over(oracle, M, iv):
    po = [oracle.params(d) for d in HAND]
    for b, (s, w) in enumerate(zip(HAND_SET, HAND_W)):
        Mo, tot = oracle.assemble(po[s], complex(w))
        assert iv[b] == tot, (b, s, iv[b], tot)
        scale = np.abs(Mo).max()
        bar = TOL_M * scale
        if complex(w) == W_WIDE:
            bar = _bar(scale, Mo, oracle.assemble(po[s], complex(w) * (1 + 1e-13))[0])
        err = np.abs(M[b] - Mo).max()
        print(f"item {b} set {s} omega {complex(w)}: error {err / scale:.3e} of max|M|, bar {bar / scale:.3e}")
        assert err <= bar, (b, s, err / scale, bar / scale)


def test_hand_over_with_two_segments(emme, oracle):
    """npoints 5 (10 pairs, one tile): every integral of W_WIDE outgrows the 64-entry level list.  Sets 1 and 2 are the
    same parameters, so their segments receive the same integrals: twice what a per-set context hands over."""
    with _ctx(emme, HAND[1], **TS) as ctx:
        ctx.assemble([W_WIDE, -0.7 + 0.15j])
        assert ctx.fill_kernel_symbol() == "k_assemble_tile"
        one = ctx.last_deferred()
    with _bound(emme, HAND, **TS) as ctx:
        ctx.profile(True)
        M, iv = ctx.assemble_sets(HAND_SET, HAND_W, want_intervals=True)
        assert _mode(ctx) == 7
        handed = ctx.last_deferred()
        pr = ctx.profile_read(reset=True)
    print(f"handed over: {handed} integrals (a per-set context: {one}); deferred launches {pr.deferred_launches}")
    assert pr.deferred_launches > 0
    assert 0 < one <= 10 and handed == 2 * one
    _check_hand_over(oracle, M, iv)


def test_hand_over_with_the_derivative(emme, oracle):
    with _bound(emme, HAND, deriv_cached=1, **TS) as ctx:
        ctx.profile(True)
        M, Mp, iv = ctx.assemble_sets(HAND_SET, HAND_W, want_derivative=True, want_intervals=True)
        assert _mode(ctx) == 7
        handed = ctx.last_deferred()
        pr = ctx.profile_read(reset=True)
    print(f"handed over: {handed} integrals; deferred launches {pr.deferred_launches}")
    assert pr.deferred_launches > 0 and handed > 0 and handed % 2 == 0
    _check_hand_over(oracle, M, iv)
    for b, (s, w) in enumerate(zip(HAND_SET, HAND_W)):
        if complex(w) != W_WIDE:
            continue
        # M' of the handed-over items: a per-set context's lanes-are-nodes derivative kernel, and its own M' spread
        with _ctx(emme, HAND[s], node_cache_gb=0) as one:
            _, Mpr = one.assemble_derivative([w])
            _, Mpr2 = one.assemble_derivative([complex(w) * (1 + 1e-13)])
        scale = np.abs(Mpr[0]).max()
        bar = _bar(scale, Mpr[0], Mpr2[0])
        err = np.abs(Mp[b] - Mpr[0]).max()
        print(f"item {b} set {s} M': error {err / scale:.3e} of max|M'|, bar {bar / scale:.3e}")
        assert err <= bar, (b, s, err / scale, bar / scale)


# ---- 7. routing: what stays on k_assemble_sets ------------------------------------------------------------------
def _nodes_fill(emme, dicts, st, w, deriv, **options):
    with _bound(emme, dicts, **options) as ctx:
        out = ctx.assemble_sets(st, w, want_derivative=deriv, want_intervals=True)
        return out, _mode(ctx), ctx.fill_kernel_symbol()


@pytest.mark.parametrize("case", ["default-options", "gk31", "electromagnetic", "tight-accuracy", "deriv-not-cached"])
def test_routing_keeps_the_nodes_kernel(emme, case):
    st, w, deriv, options = SET[:5], W[:5], False, TS
    if case == "default-options":
        dicts, options = ES15, {}
    elif case == "gk31":
        dicts = [example_tokamak(npoints=16, integration_start_points=31),
                 example_tokamak(npoints=16, integration_start_points=31, k_rho=0.3182 * 1.7)]
        st = [1, 0, 1, 1, 0]
    elif case == "electromagnetic":
        dicts = [example_stellarator(npoints=8), example_stellarator(npoints=8, beta_e=0.03, eta_k=0.2)]
        st, w = [1, 0, 0, 1, 0], [-1.656 + 2.49j, -0.9 + 0.4j, 0.7 + 0.5j, -0.8 + 0.3j, -0.7 + 0.6j]
    elif case == "tight-accuracy":
        dicts = ES15[:4] + [example_tokamak(npoints=16, conf="cylinder", integration_accuracy=1e-12)]
        st = [3, 0, 1, 3, 0]  # (no item on the tight set: the rule asks every BOUND set)
    else:
        dicts, deriv = ES15, True
    got, mode, symbol = _nodes_fill(emme, dicts, st, w, deriv, **options)
    assert mode == 6 and symbol.startswith("k_assemble_sets<"), (case, mode, symbol)
    # today's result: the same call without the option (k_assemble_sets whatever the other options are)
    ref, rmode, _ = _nodes_fill(emme, dicts, st, w, deriv, node_cache_gb=0.0)
    assert rmode == 6
    for a, b in zip(got, ref):
        assert _same_bits(a, b), case
    if case == "default-options":
        # ... which is what per-set contexts give (test_gpu_param_sets.py)
        for b in range(len(st)):
            with _ctx(emme, dicts[st[b]], node_cache_gb=0) as one:
                M1, iv1 = one.assemble([w[b]], want_intervals=True)
                assert _mode(one) == 0
            assert _same_bits(M1[0], got[0][b]) and iv1[0] == got[1][b], b
    if case == "deriv-not-cached":  # (with deriv_cached the same call does take the tile fill)
        _, mode7, _ = _nodes_fill(emme, dicts, st, w, True, deriv_cached=1, **TS)
        assert mode7 == 7


# ---- 8. routing: a mixed call -----------------------------------------------------------------------------------
def test_routing_mixed_call(emme, sets_tile):
    """wl_min = 4: a group of 5 (set 3, Re omega < 0) through the tile fill, a group of 1 (set 0) through k_assemble_sets
    in the second pass of the same call."""
    st = [3, 3, 0, 3, 3, 3]
    w = [-0.8 + 0.25j, -0.2 + 0.15j, -0.5 + 0.1j, -0.792 + 0.2475j, -0.6 + 0.2j, -0.45 + 0.3j]
    mixed = dict(TS, wl_min=4)
    with _bound(emme, ES15, **mixed) as ctx:
        ctx.profile(True)
        M, iv = ctx.assemble_sets(st, w, want_intervals=True)
        assert _mode(ctx) == 7 and ctx.fill_kernel_symbol() == "k_assemble_tile_sets"
        pr = ctx.profile_read(reset=True)
        assert pr.tile_tasks == 8 and pr.matrices == 6  # one chunk of 5 on 8 tiles
        # a call whose groups are all below wl_min: the nodes kernel alone
        Ms, ivs = ctx.assemble_sets(st[1:4], w[1:4], want_intervals=True)
        assert _mode(ctx) == 6
    with _bound(emme, ES15, node_cache_gb=0.0) as ctx:  # the all-nodes call
        Mn, ivn = ctx.assemble_sets(st, w, want_intervals=True)
        assert _mode(ctx) == 6
    with _bound(emme, ES15, **TS) as ctx:  # the all-tile call
        Mt, ivt = ctx.assemble_sets(st, w, want_intervals=True)
        assert _mode(ctx) == 7
    assert np.array_equal(iv, ivn) and np.array_equal(iv, ivt)
    assert _same_bits(M[2], Mn[2])
    for b in (0, 1, 3, 4, 5):
        assert _same_bits(M[b], Mt[b]), b
        assert np.abs(M[b] - Mn[b]).max() <= TOL_M * np.abs(Mn[b]).max()
    for q, b in enumerate((1, 2, 3)):
        assert _same_bits(Ms[q], Mn[b]) and ivs[q] == ivn[b], b


# ---- 9. root searches -------------------------------------------------------------------------------------------
# (guesses within a few per cent of a root of their set, so that the secant search and Newton on the exact derivative
# end in the same root; the CPU oracle's secant search ends every chain with |domega| / |omega| <= 2.3e-7 after a step
# of >= 4.0e-6 -- away from tol = 1e-6 on either side, so equal iteration counts is a fair demand)
SEARCH = [ES15[0], ES15[1]]
SEARCH_SET = [0, 1, 0, 1, 1, 0]
SEARCH_G = [-0.725 - 0.215j, -0.853 - 0.078j, -0.69 - 0.175j, -0.806 - 0.042j, -0.82 - 0.07j, -0.879 - 0.302j]


@pytest.mark.parametrize("exact", [0, 1])
def test_root_searches(emme, oracle, exact):
    options = dict(TS, deriv_cached=1) if exact else TS
    with _bound(emme, SEARCH, **options) as ctx:
        roots, iters, info = ctx.solve_roots_sets(SEARCH_SET, SEARCH_G, exact=bool(exact))
        assert _mode(ctx) == 7, ctx.fill_kernel()
    checked = 0
    for b, (s, g) in enumerate(zip(SEARCH_SET, SEARCH_G)):
        r_or, its_or, _, _ = oracle.solve_root(oracle.params(SEARCH[s]), complex(g))
        print(f"exact={exact} chain {b} set {s}: root {roots[b]:.12f} info {info[b]}, iters {iters[b]} (oracle's secant "
              f"search {len(its_or)}), |w - w_oracle| = {abs(roots[b] - r_or):.2e}")
        if not np.isfinite(r_or) or len(its_or) > SEARCH[s]["iteration_step_limit"]:
            continue  # (the oracle did not converge)
        checked += 1
        assert info[b] == 0, b
        assert abs(roots[b] - r_or) <= TOL_W, b
        if not exact:
            assert iters[b] == len(its_or), b
    assert checked == len(SEARCH_SET)
