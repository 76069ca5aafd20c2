"""Root sensitivities from eigenpairs on the device: the forms kernel k_sym_forms / k_sym_forms_finish
against numpy with derived bars, bit-reproducibility across launch composition and the device-pointer form; then
emme_root_sensitivities_sets against numpy on the library's own fills, against re-solved roots (bar measured on the
CPU oracle, not on the code under test), across chunk caps, on a scan line's own neighbours, under failures, and fed
straight from the region search."""
import numpy as np
import pytest

import device_buffers as db
from oracle.binding import Oracle, example_stellarator, example_tokamak

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
EMME_EINVAL, EMME_ECONFIG, EMME_ENUMERIC = -1, -5, -6
REL_STEP = 1e-4
CASES = {
    "tokamak": (lambda: example_tokamak(npoints=16), ["eta_i", "k_rho", "shat", "q", "tau", "epsilon_n"]),
    "stellarator": (lambda: example_stellarator(npoints=8), ["eta_i", "k_rho", "beta_e"]),
}


def _ctx(emme, d, **options):
    return emme.Context(emme.params_from_dict(d), **options)


@pytest.fixture(scope="module")
def small_ctx(emme):
    ctx = _ctx(emme, example_tokamak(npoints=16))
    yield ctx
    ctx.close()


# ---- 1. the forms kernel on random matrices ------------------------------------------------------------------------
# 5: one partial row block, a row shorter than a wave; 16 / 17; 64 / 65: the edge of the 64-row block and one row past
# it; 128: two whole blocks; 300, 600, 1040: columns past one pass of the lanes, partial last blocks; 2048: the limit
FORM_ORDERS = [5, 16, 17, 64, 65, 128, 300, 600, 1040, 2048]
# (a, b, x, y): b none | a != b | the same matrices with another vector | x != y | B close to A | none, x != y | a = b index
ITEMS = np.array([(0, -1, 0, 0), (0, 1, 1, 1), (0, 1, 2, 2), (1, 0, 0, 1), (2, 2, 1, 1), (2, -1, 1, 2), (1, 1, 2, 0)],
                 dtype=np.int32)
CLOSE = 4  # the item whose B is A - 1e-7 D
_forms_cache = {}


def _forms_data(n):
    """Matrices, vectors and the numpy reference of order n, made once and left unchanged."""
    if n in _forms_cache:
        return _forms_cache[n]
    rng = np.random.default_rng(7000 + n)
    cplx = lambda *shape: rng.normal(size=shape) + 1j * rng.normal(size=shape)
    A, B, v = cplx(3, n, n), cplx(3, n, n), cplx(3, n)
    D0 = cplx(n, n)
    B[2] = A[2] - 1e-7 * D0
    ref_f, ref_s, bar_f, bar_s, naive = [], [], [], [], []
    for a, b, x, y in ITEMS:
        # the difference the pair of stored matrices represents: a correctly rounded subtraction per entry (exact where
        # the entries agree to a factor of two), which for the close item IS its D -- 1e-7 D0 up to the rounding of B
        D = A[a] - B[b] if b >= 0 else A[a]
        ref_f.append(v[x] @ (D @ v[y]))
        ref_s.append(float(np.sum(D.real ** 2 + D.imag ** 2)))
        # 2n rounding steps of a fixed-order sum times the constant of a complex product
        bar_f.append(8 * n * EPS * float(np.abs(v[x]) @ (np.abs(D) @ np.abs(v[y]))))
        bar_s.append(4 * n * EPS * ref_s[-1])
        naive.append(v[x] @ (A[a] @ v[y]) - (v[x] @ (B[b] @ v[y]) if b >= 0 else 0.0))
    assert np.abs(A[2] - B[2] - 1e-7 * D0).max() <= 2 * EPS * np.abs(A[2]).max()
    out = {"A": A, "B": B, "v": v, "f": np.array(ref_f), "s": np.array(ref_s), "bar_f": np.array(bar_f),
           "bar_s": np.array(bar_s), "naive": np.array(naive)}
    if len(_forms_cache) >= 2:  # (the large orders hold hundreds of MB)
        _forms_cache.pop(next(iter(_forms_cache)))
    _forms_cache[n] = out
    return out


def _call(ctx, d, items=ITEMS, y=True, **kw):
    items = np.asarray(items)
    return ctx.sym_forms(d["A"], d["B"], d["v"], items[:, 0], items[:, 1], items[:, 2], items[:, 3] if y else None, **kw)


@pytest.mark.parametrize("n", FORM_ORDERS)
def test_forms_match_numpy_and_do_not_depend_on_the_launch(small_ctx, n):
    d = _forms_data(n)
    f, s = _call(small_ctx, d)
    for t in range(len(ITEMS)):
        ef, es = abs(f[t] - d["f"][t]), abs(s[t] - d["s"][t])
        print(f"n={n} item {t} {tuple(ITEMS[t])}: |f - numpy| {ef:.2e} (bar {d['bar_f'][t]:.2e})  "
              f"|s - numpy| {es:.2e} (bar {d['bar_s'][t]:.2e})")
        assert ef <= d["bar_f"][t], (n, t, ef, d["bar_f"][t])
        assert es <= d["bar_s"][t], (n, t, es, d["bar_s"][t])
    # the close item: two separately rounded products, as numpy forms them, miss the bar the per-entry difference holds
    e_naive = abs(d["naive"][CLOSE] - d["f"][CLOSE])
    print(f"n={n} close item: two products and a subtraction are off by {e_naive:.2e}, bar {d['bar_f'][CLOSE]:.2e}")
    assert e_naive > d["bar_f"][CLOSE]
    # two calls: the same bytes
    f2, s2 = _call(small_ctx, d)
    assert f.tobytes() == f2.tobytes() and s.tobytes() == s2.tobytes()
    # y omitted: y = x
    same = ITEMS[:, 2] == ITEMS[:, 3]
    fy, sy = _call(small_ctx, d, y=False)
    assert fy[same].tobytes() == f[same].tobytes() and sy.tobytes() == s.tobytes()
    # device-pointer form: guarded, sentinel-filled buffers; the same bits, inputs untouched, guards intact
    with db.GuardedBuffer(d["A"].shape) as ga, db.GuardedBuffer(d["B"].shape) as gb:
        ga.upload(d["A"]), gb.upload(d["B"])
        ga.synchronize(), gb.synchronize()
        dev = dict(a_device_ptr=ga.ptr, b_device_ptr=gb.ptr)
        shape = {"A": (3, n), "B": None, "v": d["v"]}
        fd, sd = _call(small_ctx, shape, **dev)
        assert fd.tobytes() == f.tobytes() and sd.tobytes() == s.tobytes()
        # every item alone, the items in reversed order, and among 200 others: the same bytes per item
        for t in range(len(ITEMS)):
            f1, s1 = _call(small_ctx, shape, items=ITEMS[t:t + 1], **dev)
            assert f1[0].tobytes() == f[t].tobytes() and s1[0].tobytes() == s[t].tobytes(), (n, t)
        fr, sr = _call(small_ctx, shape, items=ITEMS[::-1], **dev)
        assert fr[::-1].tobytes() == f.tobytes() and sr[::-1].tobytes() == s.tobytes()
        rng = np.random.default_rng(n)
        others = np.stack([rng.integers(0, 3, 200), rng.integers(-1, 3, 200), rng.integers(0, 3, 200),
                           rng.integers(0, 3, 200)], axis=1).astype(np.int32)
        pos = np.sort(rng.choice(207, size=7, replace=False))
        mixed = np.zeros((207, 4), dtype=np.int32)
        mask = np.zeros(207, dtype=bool)
        mask[pos] = True
        mixed[mask], mixed[~mask] = ITEMS, others
        fm, sm = _call(small_ctx, shape, items=mixed, **dev)
        assert fm[mask].tobytes() == f.tobytes() and sm[mask].tobytes() == s.tobytes()
        ga.assert_unchanged(d["A"]), gb.assert_unchanged(d["B"])
        ga.assert_guards_intact(), gb.assert_guards_intact()


def test_forms_refuse_orders_above_2048_and_mixed_sides(emme, small_ctx):
    n = 2049
    M = np.zeros((1, n, n), dtype=np.complex128)
    with pytest.raises(emme.EmmeError) as e:
        small_ctx.sym_forms(M, None, np.ones((1, n)), [0])
    assert e.value.code == EMME_ECONFIG
    zero = np.zeros(1, dtype=np.int32)
    with db.GuardedBuffer((1, 4, 4)) as g:
        rc = small_ctx.lib.emme_sym_forms_batch(small_ctx.h, 4, 1, db.C.c_void_p(g.ptr), M.ctypes.data, 1, M.ctypes.data, 1,
                                                zero.ctypes.data, None, zero.ctypes.data, None, M.ctypes.data, None)
        assert rc == EMME_EINVAL and "both be host or both be device" in emme.last_error()
        g.assert_untouched()


def test_a_skew_derivative_puts_the_form_at_its_rounding_level(small_ctx):
    """info = 1 on caller terms: with M' skew, v^T M' v is exactly 0, and what the kernel returns for it is within the
    finish rule's 64 n eps |M'|_F |v|^2 -- while a generic M' is far above it."""
    for n in (16, 65, 300):
        rng = np.random.default_rng(n)
        R = rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))
        v = rng.normal(size=(1, n)) + 1j * rng.normal(size=(1, n))
        vn2 = float(np.vdot(v, v).real)
        f, s = small_ctx.sym_forms(np.array([R - R.T, R]), None, v, [0, 1], x=[0, 0])
        level = 64 * n * EPS * np.sqrt(s) * vn2
        print(f"n={n}: skew |f| {abs(f[0]):.2e} <= {level[0]:.2e};  generic |f| {abs(f[1]):.2e} > {level[1]:.2e}")
        assert abs(f[0]) <= level[0] and abs(f[1]) > level[1]


# ---- 2. the entry point -------------------------------------------------------------------------------------------
def _bases(case):
    mk, names = CASES[case]
    d = mk()
    return [d, dict(d, k_rho=d["k_rho"] * 1.05)], names


def _neighbour_dicts(base, name):
    p = base[name]
    h = abs(p) * REL_STEP
    return dict(base, **{name: p + h}), dict(base, **{name: p - h})


_oracle_cache = {}


def oracle_disagreement(case):
    """What separates the formula from the root difference, measured on the CPU oracle and not on the code under test:
    per base and parameter, |formula - (w(p+) - w(p-)) / dp| / |formula| with the formula in numpy on Oracle.assemble
    matrices (null vector by SVD, M' by a central omega-difference) and the roots from Oracle.solve_root at p+-, all
    with iteration_precision 1e-12.  Returns (disagreement [nbases, ndir], formula [nbases, ndir], roots [nbases])."""
    if case in _oracle_cache:
        return _oracle_cache[case]
    orc = Oracle()
    bases, names = _bases(case)
    dis, val, roots = np.zeros((len(bases), len(names))), np.zeros((len(bases), len(names)), dtype=complex), []
    for ib, base in enumerate(bases):
        tight = lambda d: orc.params(dict(d, iteration_precision=1e-12))
        pb = tight(base)
        w = orc.solve_root(pb, complex(*base["initial_guess"]))[0]
        roots.append(w)
        M = orc.assemble(pb, w)[0]
        v = np.linalg.svd(M)[2][-1].conj()
        h = 1e-5 * abs(w)
        Mp = (orc.assemble(pb, w + h)[0] - orc.assemble(pb, w - h)[0]) / (2 * h)
        den = v @ Mp @ v
        for k, name in enumerate(names):
            dplus, dminus = _neighbour_dicts(base, name)
            dp = dplus[name] - dminus[name]
            Mdiff = orc.assemble(tight(dplus), w)[0] - orc.assemble(tight(dminus), w)[0]
            val[ib, k] = -(v @ Mdiff @ v) / (dp * den)
            fd = (orc.solve_root(tight(dplus), w)[0] - orc.solve_root(tight(dminus), w)[0]) / dp
            dis[ib, k] = abs(val[ib, k] - fd) / abs(val[ib, k])
    _oracle_cache[case] = (dis, val, np.array(roots))
    return _oracle_cache[case]


class Case:
    """One context with the sets of neighbour_sets over two bases bound, the two polished eigenpairs, the call under
    test on them."""

    def __init__(self, emme, case):
        self.name = case
        self.bases, self.names = _bases(case)
        self.ctx = _ctx(emme, self.bases[0])
        self.params, self.set, self.sp, self.sm, self.dp = emme.neighbour_sets(self.bases, self.names, rel_step=REL_STEP)
        self.ctx.bind_param_sets(self.params)
        guess = complex(*self.bases[0]["initial_guess"])
        r0, _, info = self.ctx.solve_roots_sets(self.set, [guess, guess])
        assert (info == 0).all()
        self.w, self.v, self.resid, _, info = self.ctx.solve_eigenpairs(r0, set=self.set, tol=1e-13)
        assert (info == 0).all() and (self.resid <= 1e-13).all(), (info, self.resid)  # the precondition
        self.out = self.ctx.root_sensitivities(self.set, self.w, self.v, self.sp, self.sm, self.dp)


_cases = {}


@pytest.fixture(scope="module")
def cases(emme):
    def get(name):
        if name not in _cases:
            _cases[name] = Case(emme, name)
        return _cases[name]
    yield get
    for c in _cases.values():
        c.ctx.close()
    _cases.clear()


def _form(x, D, y):
    """x^T D y in numpy with the bar of the forms kernel."""
    return x @ (D @ y), 8 * D.shape[0] * EPS * float(np.abs(x) @ (np.abs(D) @ np.abs(y)))


def _check_against_numpy(c, label, base, w, v, resid, dwdp, denom, corr, cond):
    """One root's outputs against numpy's evaluation of the formulas on the library's own fills: with default options
    assemble_sets at the same (set, omega) items gives the very matrices.  Bars: the forms' bars, propagated (a quotient
    a / b moves by da / |b| + |a / b| db / |b|, plus its own few roundings), times 2."""
    n, nd = c.ctx.dim, len(c.names)
    M, Mp = c.ctx.assemble_sets([c.set[base]], [w], want_derivative=True)
    Mplus = c.ctx.assemble_sets(c.sp[base], np.full(nd, w))
    Mminus = c.ctx.assemble_sets(c.sm[base], np.full(nd, w))
    f0, b0 = _form(v, M[0], v)
    f1, b1 = _form(v, Mp[0], v)
    cond_np = np.linalg.norm(M[0]) * np.vdot(v, v).real / abs(f1)
    corr_np = -f0 / f1
    assert abs(denom - f1) <= 2 * b1
    assert abs(corr - corr_np) <= 2 * (b0 / abs(f1) + abs(corr_np) * (b1 / abs(f1) + 4 * EPS))
    assert abs(cond - cond_np) <= 2 * cond_np * (2 * n * EPS + b1 / abs(f1) + 4 * EPS)
    sane = 100 * resid * cond_np * abs(w)
    print(f"{label}: omega {w:.8f} resid {resid:.1e} |v^T v| {abs(v @ v):.3f} denom {denom:.6f} cond {cond:.3f} "
          f"|corr| {abs(corr):.2e} (sanity bound {sane:.2e})")
    assert abs(corr) <= sane
    for k, name in enumerate(c.names):
        fd, bd = _form(v, Mplus[k] - Mminus[k], v)
        q = -fd / (c.dp[base, k] * f1)
        bar = 2 * (bd / abs(c.dp[base, k] * f1) + abs(q) * (b1 / abs(f1) + 6 * EPS))
        print(f"{label} d omega / d {name} = {dwdp[k]:.8f}: |gpu - numpy| {abs(dwdp[k] - q):.2e} (bar {bar:.2e})")
        assert abs(dwdp[k] - q) <= bar, (label, name)


@pytest.mark.parametrize("case", list(CASES))
def test_sensitivities_match_numpy_on_the_librarys_own_fills(cases, case):
    c = cases(case)
    dwdp, denom, corr, cond, info = c.out
    assert (info == 0).all()
    if case == "tokamak":
        assert abs(c.w[0] - (-0.56975 - 0.28050j)) < 1e-4  # where the CPU oracle's search from this guess ends
    for r in range(2):
        _check_against_numpy(c, f"{case} root {r}", r, c.w[r], c.v[r], c.resid[r], dwdp[r], denom[r], corr[r], cond[r])


@pytest.mark.parametrize("case", list(CASES))
def test_sensitivities_match_resolved_roots(cases, case):
    """The independent check.  Measured on one MI355X (gpu: |dwdp - (w+ - w-) / dp| / |dwdp| from emme_solve_eigenpairs at
    p+-; oracle: the same comparison on the CPU oracle): see the table of DESIGN.md §15.5."""
    c = cases(case)
    dwdp = c.out[0]
    nd = len(c.names)
    o_dis, o_val, o_roots = oracle_disagreement(case)
    assert (o_dis <= 1e-4).all(), o_dis  # the condition on the inputs: a case that breaks it is replaced, not loosened
    both = np.concatenate([c.sp.ravel(), c.sm.ravel()])
    w_pm, _, resid, _, info = c.ctx.solve_eigenpairs(np.tile(np.repeat(c.w, nd), 2), set=both,
                                                     v0=np.tile(np.repeat(c.v, nd, axis=0), (2, 1)), tol=1e-13)
    assert (info == 0).all() and (resid <= 1e-13).all()
    fd = ((w_pm[:2 * nd] - w_pm[2 * nd:]) / c.dp.ravel()).reshape(2, nd)
    for r in range(2):
        for k, name in enumerate(c.names):
            dis = abs(dwdp[r, k] - fd[r, k]) / abs(dwdp[r, k])
            bar = max(10 * o_dis[r, k], 1e-9)
            print(f"{case} base {r} {name}: gpu formula {dwdp[r, k]:.8f} vs re-solved roots {dis:.2e};  oracle formula "
                  f"{o_val[r, k]:.8f} vs its roots {o_dis[r, k]:.2e};  bar {bar:.2e};  |gpu - oracle formula| "
                  f"{abs(dwdp[r, k] - o_val[r, k]) / abs(o_val[r, k]):.2e}")
            assert dis <= bar, (case, r, name, dis, bar)


def test_chunk_caps_give_the_same_bytes(cases):
    c = cases("tokamak")  # ndir = 6 on two roots: 24 neighbour matrices
    for cap in (2, 3, 0):
        out = c.ctx.root_sensitivities(c.set, c.w, c.v, c.sp, c.sm, c.dp, max_items=cap)
        for a, b in zip(out, c.out):
            assert a.tobytes() == b.tobytes(), cap


def test_a_scan_lines_own_neighbours(emme, cases):
    c = cases("tokamak")
    base = c.bases[0]
    spacing = 1e-3
    line = [dict(base, k_rho=base["k_rho"] * (1 + spacing * j)) for j in range(-2, 3)]
    params, st, sp, sm, dp = emme.neighbour_sets(line[1:4], ["k_rho"], rel_step=REL_STEP)
    nl = len(line)
    ctx = _ctx(emme, base)
    try:
        ctx.bind_param_sets([emme.params_from_dict(d) for d in line] + params)
        # the root of every point by continuation from the middle one
        w, v = np.zeros(nl, dtype=complex), np.zeros((nl, ctx.dim), dtype=complex)
        w[2], v[2] = c.w[0], c.v[0]
        for i, src in ((2, 2), (1, 2), (3, 2), (0, 1), (4, 3)):
            wi, vi, resid, _, info = ctx.solve_eigenpairs([w[src]], set=[i], v0=v[src][None], tol=1e-13)
            assert info[0] == 0 and resid[0] <= 1e-13
            w[i], v[i] = wi[0], vi[0]
        inner = np.array([1, 2, 3], dtype=np.int32)
        kr = np.array([d["k_rho"] for d in line])
        own = ctx.root_sensitivities(inner, w[inner], v[inner], inner[:, None] + 1, inner[:, None] - 1,
                                     (kr[inner + 1] - kr[inner - 1])[:, None])
        ded = ctx.root_sensitivities(nl + st, w[inner], v[inner], nl + sp, nl + sm, dp)
        assert (own[4] == 0).all() and (ded[4] == 0).all()
        o_dis = oracle_disagreement("tokamak")[0][0, c.names.index("k_rho")]
        bar = max(10 * o_dis, 1e-9) * (spacing / REL_STEP) ** 2
        for j in range(3):
            dis = abs(own[0][j, 0] - ded[0][j, 0]) / abs(ded[0][j, 0])
            print(f"scan point {inner[j]}: own neighbours {own[0][j, 0]:.8f}, dedicated {ded[0][j, 0]:.8f}: {dis:.2e} (bar {bar:.2e})")
            assert dis <= bar
        # another item order: the same bytes per item
        perm = np.array([2, 0, 1])
        again = ctx.root_sensitivities(inner[perm], w[inner][perm], v[inner][perm], inner[perm][:, None] + 1,
                                       inner[perm][:, None] - 1, (kr[inner + 1] - kr[inner - 1])[perm][:, None])
        for a, b in zip(again, own):
            assert a.tobytes() == b[perm].tobytes()
    finally:
        ctx.close()


def test_failures_stay_with_their_root(emme, cases):
    c = cases("tokamak")
    three = np.array([0, 1, 0])
    st, w, v, sp, sm, dp = c.set[three], c.w[three], c.v[three].copy(), c.sp[three], c.sm[three], c.dp[three]
    good = c.ctx.root_sensitivities(st[[0, 2]], w[[0, 2]], v[[0, 2]], sp[[0, 2]], sm[[0, 2]], dp[[0, 2]])
    for blank_root in (False, True):  # a failed chain leaves its vector row NaN (the search) or root and row (the region search)
        wb, vb = w.copy(), v.copy()
        vb[1] = np.nan
        if blank_root:
            wb[1] = np.nan
        out = c.ctx.root_sensitivities(st, wb, vb, sp, sm, dp)
        assert out[4].tolist() == [0, EMME_ENUMERIC, 0]
        for a, b in zip(out[:4], good[:4]):
            assert a[[0, 2]].tobytes() == b.tobytes()
            assert np.isnan(a[1]).all()
    # all roots bad: nothing but NaN, no error
    out = c.ctx.root_sensitivities(st[:1], [np.nan], v[:1], sp[:1], sm[:1], dp[:1])
    assert out[4].tolist() == [EMME_ENUMERIC] and np.isnan(out[0]).all()
    # a zero vector row is a caller's mistake
    vz = v.copy()
    vz[2] = 0.0
    with pytest.raises(emme.EmmeError) as e:
        c.ctx.root_sensitivities(st, w, vz, sp, sm, dp)
    assert e.value.code == EMME_EINVAL and "row 2" in e.value.reason
    # an index beyond the binding
    with pytest.raises(emme.EmmeError) as e:
        c.ctx.root_sensitivities(st, w, v, sp + len(c.params), sm, dp)
    assert e.value.code == EMME_EINVAL
    # no binding
    ctx = _ctx(emme, c.bases[0])
    try:
        with pytest.raises(emme.EmmeError) as e:
            ctx.root_sensitivities(st, w, v, sp, sm, dp)
        assert e.value.code == EMME_EINVAL and "bound" in e.value.reason
    finally:
        ctx.close()
    # ndir = 0: denom, corr and cond alone, the same bytes
    out = c.ctx.root_sensitivities(c.set, c.w, c.v, np.zeros((2, 0)), np.zeros((2, 0)), np.zeros((2, 0)))
    assert out[0].shape == (2, 0)
    for a, b in zip(out[1:], c.out[1:]):
        assert a.tobytes() == b.tobytes()
    # a vector that is not an eigenvector is caught by corr, not by info
    rng = np.random.default_rng(5)
    vr = rng.normal(size=c.v.shape) + 1j * rng.normal(size=c.v.shape)
    out = c.ctx.root_sensitivities(c.set, c.w, vr, c.sp, c.sm, c.dp)
    print(f"random vectors: info {out[4]}, |corr| {np.abs(out[2])} against {np.abs(c.out[2])} for the eigenvectors")
    assert (out[4] == 0).all() and (np.abs(out[2]) > 1e6 * np.abs(c.out[2])).all()


def test_nothing_else_moved(emme):
    d = example_tokamak(npoints=16)
    ctx = _ctx(emme, d)
    try:
        params, st, sp, sm, dp = emme.neighbour_sets(d, ["eta_i", "k_rho"], rel_step=REL_STEP)
        ctx.bind_param_sets(params)
        w0 = np.array([-0.8 + 0.25j, -0.5 - 0.3j])
        before = ctx.assemble(w0)
        w, v, resid, _, info = ctx.solve_eigenpairs([complex(*d["initial_guess"])], set=[0], tol=1e-13)
        state = (ctx.mirror_pairs(), bytes(ctx.options()), ctx.param_sets())
        out = ctx.root_sensitivities(st, w, v, sp, sm, dp)
        assert (out[4] == 0).all()
        assert (ctx.mirror_pairs(), bytes(ctx.options()), ctx.param_sets()) == state
        assert ctx.assemble(w0).tobytes() == before.tobytes()
    finally:
        ctx.close()


def test_region_search_outputs_pass_straight_through(cases):
    c = cases("tokamak")
    found = c.ctx.find_eigenpairs_in_contours_sets([0], [c.w[0]], [(0.05, 0.05)], exact=True, tol=1e-13, max_roots=4)[0]
    assert found["status"] == 0 and found["n_roots"] >= 1
    # what the C call returns: max_roots rows per item, the rows behind the kept roots empty; as a failed chain is
    # blanked, an empty row goes in as NaN
    nrow = 4
    w = np.full(nrow, np.nan, dtype=complex)
    v = np.full((nrow, c.ctx.dim), np.nan, dtype=complex)
    k = len(found["roots"])
    w[:k], v[:k] = found["roots"], found["vecs"]
    rows = np.zeros(nrow, dtype=int)
    out = c.ctx.root_sensitivities(c.set[rows], w, v, c.sp[rows], c.sm[rows], c.dp[rows])
    hit = int(np.argmin(np.abs(w[:k] - c.w[0])))
    assert abs(w[hit] - c.w[0]) < 1e-9 * abs(c.w[0]) and found["resid"][hit] <= 1e-13
    assert out[4][hit] == 0 and (out[4][k:] == EMME_ENUMERIC).all() and np.isnan(out[0][k:]).all()
    # the item whose root matches: the check against numpy on the library's own fills, within its bar
    _check_against_numpy(c, "region search root", 0, w[hit], v[hit], found["resid"][hit], out[0][hit], out[1][hit],
                         out[2][hit], out[3][hit])
    alone = c.ctx.root_sensitivities(c.set[:1], w[hit:hit + 1], v[hit:hit + 1], c.sp[:1], c.sm[:1], c.dp[:1])
    for a, b in zip(alone, out):
        assert a[0].tobytes() == b[hit].tobytes()
