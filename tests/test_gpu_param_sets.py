"""Parameter sets on one context: k_assemble_sets / k_assemble_sets_deriv against per-set contexts bit
for bit and against the CPU oracle, items that do not leak into each other, the errors, both root searches over
(set, guess) items, and the lock-step scan driver against the sequential one.

The `emme` fixture sets cache_min_batch = 1, so the per-set comparison contexts are created with node_cache_gb = 0 and
the tests assert that they ran the lanes-are-nodes kernel (fill mode 0)."""

import numpy as np
import pytest

from oracle.binding import example_stellarator, example_tokamak

pytestmark = pytest.mark.gpu

TOL_M = 1e-10  # test_gpu_parity.py
TOL_W = 1e-9
EMME_EINVAL, EMME_ENUMERIC = -1, -6

# ---- the fill cases -------------------------------------------------------------------------------------------
ES15 = [example_tokamak(npoints=16), example_tokamak(npoints=16, k_rho=0.3182 * 1.7),
        example_tokamak(npoints=16, eta_i=3.13 * 0.6), example_tokamak(npoints=16, shat=1.35),
        example_tokamak(npoints=16, conf="cylinder")]
# seven items in shuffled set order, set 2 twice; omegas on both sides of Re omega = 0 and one damped
ES15_SET = [3, 0, 2, 4, 1, 2, 0]
ES15_W = [-0.8 + 0.25j, 0.6 + 0.1j, -0.3 - 0.05j, -0.792 + 0.2475j, 0.45 + 0.2j, -0.6 + 0.3j, -0.7 + 0.15j]
ES31 = [example_tokamak(npoints=16, integration_start_points=31),
        example_tokamak(npoints=16, integration_start_points=31, k_rho=0.3182 * 1.7)]
EM = [example_stellarator(npoints=16), example_stellarator(npoints=16, beta_e=0.03, eta_k=0.2)]
CASES = {"es15": (ES15, ES15_SET, ES15_W),
         "es31": (ES31, [1, 0, 1], [-0.8 + 0.25j, 0.6 + 0.1j, -0.3 - 0.05j]),
         "em": (EM, [1, 0, 0], [-1.656 + 2.49j, -0.9 + 0.4j, 0.7 + 0.5j])}


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


@pytest.fixture(scope="module")
def sets_fill(emme):
    """assemble_sets of every case, with the derivative: computed once, shared, never modified"""
    out = {}
    for name, (dicts, st, w) in CASES.items():
        with _bound(emme, dicts) as ctx:
            assert ctx.param_sets() == len(dicts)
            M, iv = ctx.assemble_sets(st, w, want_intervals=True)
            mode = ctx.lib.emme_ctx_fill_mode(ctx.h)
            M2, Mp, iv2 = ctx.assemble_sets(st, w, want_derivative=True, want_intervals=True)
        for a in (M, iv, M2, Mp, iv2):
            a.setflags(write=False)
        out[name] = dict(M=M, iv=iv, M2=M2, Mp=Mp, iv2=iv2, mode=mode)
    return out


# ---- 1. against per-set contexts, bit for bit -------------------------------------------------------------------
def test_fill_matches_per_set_contexts_bit_for_bit(emme, sets_fill):
    dicts, st, w = CASES["es15"]
    got = sets_fill["es15"]
    for b, (s, om) in enumerate(zip(st, w)):
        with _ctx(emme, dicts[s], node_cache_gb=0) as ctx:
            M, iv = ctx.assemble([om], want_intervals=True)
            assert ctx.lib.emme_ctx_fill_mode(ctx.h) == 0
            Md, Mpd, ivd = ctx.assemble_derivative([om], want_intervals=True)
        assert iv[0] == got["iv"][b] and ivd[0] == got["iv2"][b], (b, s)
        assert _same_bits(M[0], got["M"][b]), (b, s, np.abs(M[0] - got["M"][b]).max())
        assert _same_bits(Md[0], got["M2"][b]), (b, s)
        assert _same_bits(Mpd[0], got["Mp"][b]), (b, s, np.abs(Mpd[0] - got["Mp"][b]).max())
    # the derivative kernel decides on K and G alone: its M is the plain kernel's
    assert _same_bits(got["M"], got["M2"]) and np.array_equal(got["iv"], got["iv2"])


# ---- 2. against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["es15", "es31", "em"])
def test_fill_matches_the_oracle(emme, oracle, sets_fill, case):
    dicts, st, w = CASES[case]
    got = sets_fill[case]
    po = [oracle.params(d) for d in dicts]
    if case == "em":
        assert got["M"].shape[1:] == (32, 32)
    for b, (s, om) in enumerate(zip(st, w)):
        Mo, tot = oracle.assemble(po[s], complex(om))
        err = np.abs(got["M"][b] - Mo).max() / np.abs(Mo).max()
        print(f"{case} item {b} set {s}: max|dM|/max|M| = {err:.2e}, intervals {got['iv'][b]} / {tot}")
        assert err <= TOL_M
        assert got["iv"][b] == tot and got["iv2"][b] == tot
        assert np.abs(got["M2"][b] - Mo).max() <= TOL_M * np.abs(Mo).max()


# ---- 3. items do not leak -------------------------------------------------------------------------------------
def test_items_do_not_leak(emme, sets_fill):
    dicts, st, w = CASES["es15"]
    got = sets_fill["es15"]
    assert got["mode"] == 6
    perm = [4, 2, 6, 0, 5, 1, 3]
    with _bound(emme, dicts) as ctx:
        M, iv = ctx.assemble_sets([st[k] for k in perm], [w[k] for k in perm], want_intervals=True)
        for q, k in enumerate(perm):
            assert _same_bits(M[q], got["M"][k]) and iv[q] == got["iv"][k], (q, k)
        for k in range(len(st)):
            M1, Mp1, iv1 = ctx.assemble_sets([st[k]], [w[k]], want_derivative=True, want_intervals=True)
            assert _same_bits(M1[0], got["M"][k]) and _same_bits(Mp1[0], got["Mp"][k]) and iv1[0] == got["iv"][k], k
        assert ctx.fill_kernel().startswith("k_assemble_sets")
        # the context's own entry points do not see the binding
        Mb = ctx.assemble(w[:3])
        rb = ctx.solve_roots([-0.8 + 0.25j])
    with _ctx(emme, dicts[0]) as ctx:
        Mu = ctx.assemble(w[:3])
        ru = ctx.solve_roots([-0.8 + 0.25j])
    assert _same_bits(Mb, Mu)
    assert _same_bits(rb[0], ru[0]) and np.array_equal(rb[1], ru[1]) and np.array_equal(rb[2], ru[2])


# ---- 4. errors ------------------------------------------------------------------------------------------------
def test_errors(emme):
    dicts, st, w = CASES["es15"]
    with _ctx(emme, dicts[0], node_cache_gb=0) as ctx:
        # no binding
        with pytest.raises(emme.EmmeError) as e:
            ctx.assemble_sets([0], [w[0]])
        assert e.value.code == EMME_EINVAL
        with pytest.raises(emme.EmmeError) as e:
            ctx.solve_roots_sets([0], [w[0]])
        assert e.value.code == EMME_EINVAL
        # another npoints; an electromagnetic set on an electrostatic context
        for other in (example_tokamak(npoints=18), example_tokamak(npoints=16, beta_e=0.01)):
            with pytest.raises(emme.EmmeError) as e:
                ctx.bind_param_sets([emme.params_from_dict(dicts[1]), emme.params_from_dict(other)])
            assert e.value.code == EMME_EINVAL
            assert ctx.param_sets() == 0
        ctx.bind_param_sets([emme.params_from_dict(d) for d in dicts[:2]])
        assert ctx.param_sets() == 2
        for bad in (2, -1):
            with pytest.raises(emme.EmmeError) as e:
                ctx.assemble_sets([0, bad], w[:2])
            assert e.value.code == EMME_EINVAL
            with pytest.raises(emme.EmmeError) as e:
                ctx.solve_roots_sets([bad], [w[0]], exact=True)
            assert e.value.code == EMME_EINVAL
        # omega = 0 (test_run_json_marks_enumeric_failures_as_nan_records): the secant step is 0/0.  The chain is
        # marked like a plain search's, the other chain of the batch is not touched
        roots, iters, info = ctx.solve_roots_sets([1, 0], [0.0, -0.8 + 0.25j])
        plain = ctx.solve_roots([0.0, -0.8 + 0.25j])
        assert info[0] == plain[2][0] == EMME_ENUMERIC
        assert info[1] == 0 and plain[2][1] == 0 and abs(roots[1] - plain[0][1]) <= 1e-9 * abs(plain[0][1])
        # ... and the fill at that omega answers as the plain fill does
        rc_plain = ctx.assemble_rc([0.0])
        M = np.zeros((2, ctx.dim, ctx.dim), dtype=np.complex128)
        st2, w2 = np.array([0, 1], dtype=np.int32), np.array([0.0, w[0]], dtype=np.complex128)
        rc = ctx.lib.emme_assemble_sets_batch(ctx.h, st2.ctypes.data, w2.ctypes.data, 2, M.ctypes.data, None, None)
        assert rc == rc_plain and rc in (0, EMME_ENUMERIC)
        ctx.bind_param_sets([])
        assert ctx.param_sets() == 0
        with pytest.raises(emme.EmmeError):
            ctx.assemble_sets([0], [w[0]])


# ---- 5. searches ----------------------------------------------------------------------------------------------
# (guesses: the last |domega| / |omega| of every chain is more than a factor 10 away from tol = 1e-6 on either side
# -- CPU oracle, secant search: 1.2e-8 after 1.4e-5, 1.2e-8 after 1.3e-5, 8.2e-9 after 1.1e-5, 1.7e-8 after 1.4e-5 --
# so equal iteration counts is a fair demand; -0.8+0.25j itself ends sets 0 and 1 at 2.4e-7 and 3.1e-7)
SEARCH = [example_tokamak(npoints=24, omega_d_coeff=1.01), example_tokamak(npoints=24, omega_d_coeff=0.91),
          example_tokamak(npoints=24, omega_d_coeff=0.81), example_tokamak(npoints=24, k_rho=0.3182 * 1.3)]
SEARCH_SET = [2, 0, 3, 1]
SEARCH_G = [-0.8 + 0.25j, -0.75 + 0.25j, -0.8 + 0.25j, -0.75 + 0.25j]


def _overlap(a, b):
    return abs(np.vdot(a, b)) / (np.linalg.norm(a) * np.linalg.norm(b))


@pytest.mark.parametrize("exact", [0, 1])
def test_searches_over_sets(emme, oracle, exact):
    with _bound(emme, SEARCH) as ctx:
        roots, iters, info = ctx.solve_roots_sets(SEARCH_SET, SEARCH_G, exact=bool(exact))
        assert ctx.lib.emme_ctx_fill_mode(ctx.h) == 6
        mats = [ctx.final_matrix(b) for b in range(len(SEARCH_SET))]
        vecs, vinfo = ctx.null_vectors(None, nbatch=len(SEARCH_SET))
    assert (info == 0).all() and (vinfo == 0).all()
    for b, (s, g) in enumerate(zip(SEARCH_SET, SEARCH_G)):
        po = oracle.params(SEARCH[s])
        r_or, its_or, Mo, _ = oracle.solve_root(po, complex(g), want_matrix=True)
        with _ctx(emme, SEARCH[s], node_cache_gb=0) as one:
            r1, i1, f1 = (one.solve_roots_newton if exact else one.solve_roots)([g])
        print(f"exact={exact} chain {b} set {s}: root {roots[b]:.12f}, iters {iters[b]} / {i1[0]}, "
              f"|w - w_oracle| = {abs(roots[b] - r_or):.2e}, |w - w_ctx|/|w| = {abs(roots[b] - r1[0]) / abs(r1[0]):.2e}")
        assert f1[0] == 0
        assert abs(roots[b] - r1[0]) <= 1e-9 * abs(r1[0])
        assert iters[b] == i1[0]
        if not exact:
            assert abs(roots[b] - r_or) <= TOL_W
            assert iters[b] == len(its_or)
            assert np.abs(mats[b] - Mo).max() <= 1e-8 * np.abs(Mo).max()
        else:
            Mw, _ = oracle.assemble(po, complex(roots[b]))
            assert np.abs(mats[b] - Mw).max() <= 1e-8 * np.abs(Mw).max()
        want = np.linalg.svd(mats[b])[2][-1].conj()
        assert 1.0 - _overlap(vecs[b], want) <= 1e-8


# ---- 6. the lock-step driver ------------------------------------------------------------------------------------
def _compare_runs(seq, lock, n, dir_seq, dir_lock):
    assert list(seq["result"].keys()) == list(lock["result"].keys())
    for key, us in seq["result"].items():
        ul = lock["result"][key]
        assert ul["scan_key"] == us["scan_key"] == key
        assert ul["scan_values"] == us["scan_values"]
        assert len(ul["scan_result"]) == len(us["scan_result"])
        for k, (rs, rl) in enumerate(zip(us["scan_result"], ul["scan_result"])):
            assert (rs["eigenvalue"] == "NaN") == (rl["eigenvalue"] == "NaN"), (key, k)
            if rs["eigenvalue"] == "NaN":
                assert rl["reason"] == rs["reason"]
                continue
            ws, wl = complex(*rs["eigenvalue"]), complex(*rl["eigenvalue"])
            assert abs(wl - ws) <= 2e-6 * abs(ws), (key, k)  # the text carries six digits
            assert rl["iterations"] == rs["iterations"], (key, k)
            assert rl["scan_value"] == rs["scan_value"]
            if dir_seq is not None:
                assert rl["eigenMatrix"].replace(dir_lock, "") == rs["eigenMatrix"].replace(dir_seq, "")
                Ms = np.fromfile(rs["eigenMatrix"], dtype=np.complex128).reshape(n, n)
                Ml = np.fromfile(rl["eigenMatrix"], dtype=np.complex128).reshape(n, n)
                assert np.abs(Ml - Ms).max() <= 1e-8 * np.abs(Ms).max(), (key, k)
            vs = np.array([complex(*z) for z in rs["eigenvector"]])
            vl = np.array([complex(*z) for z in rl["eigenvector"]])
            assert abs(_overlap(vs, vl) - 1.0) < 1e-4, (key, k)


def test_lockstep_driver_matches_the_sequential_one(emme, tmp_path):
    d = example_tokamak(npoints=24, omega_d_coeff={"head": 1.01, "step": 0.1, "tail": [0.81, 1.11]},
                        eta_i={"head": 3.13, "step": 0.2, "tail": 3.53})
    text = emme.json_text(d)
    ds, dl = tmp_path / "seq", tmp_path / "lock"
    ds.mkdir(), dl.mkdir()
    seq = emme.run_json(text, str(ds))
    lock = emme.run_json_lockstep(text, str(dl))
    assert np.allclose(seq["result"]["omega_d_coeff"]["scan_values"], [1.01, 0.91, 0.81, 1.11])
    assert len(seq["result"]["eta_i"]["scan_values"]) == 3
    assert lock["input"] == seq["input"] and "run_time" in lock
    _compare_runs(seq, lock, 24, str(ds), str(dl))
    assert all(r["eigenvalue"] != "NaN" for u in lock["result"].values() for r in u["scan_result"])


def test_lockstep_driver_failing_point(emme):
    """initial_guess 0 (test_run_json_marks_enumeric_failures_as_nan_records): the head of every axis fails, and so
    does what continues from initial_guess; NaN records at the sequential driver's places, with its reasons."""
    d = example_tokamak(npoints=16, initial_guess=[0.0, 0.0],
                        omega_d_coeff={"head": 1.01, "step": 0.1, "tail": [0.91, 1.11]})
    text = emme.json_text(d)
    seq, lock = emme.run_json(text, None), emme.run_json_lockstep(text, None)
    _compare_runs(seq, lock, 16, None, None)
    recs = lock["result"]["omega_d_coeff"]["scan_result"]
    assert len(recs) == 3 and all(r["eigenvalue"] == "NaN" and "EMME_ENUMERIC" in r["reason"] for r in recs)
    # an axis the rounds cannot carry goes through the sequential driver, inside the same output
    d2 = example_tokamak(npoints=16, iteration_step_limit={"head": 20, "step": 5, "tail": 25},
                         eta_i={"head": 3.13, "step": 0.2, "tail": 3.33})
    t2 = emme.json_text(d2)
    _compare_runs(emme.run_json(t2, None), emme.run_json_lockstep(t2, None), 16, None, None)
