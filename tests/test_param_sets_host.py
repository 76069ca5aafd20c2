"""Parameter sets on one context, host side: the new symbols and wrappers, the shape rule, argument
errors that must be found before any device is looked for, and the round plan of the lock-step scan driver.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from oracle.binding import example_stellarator, example_tokamak

EMME_OK, EMME_EINVAL = 0, -1


def test_symbols_and_wrappers_exist(emme):
    lib = emme.load()
    for name in ("emme_params_same_shape", "emme_ctx_bind_param_sets", "emme_ctx_param_sets", "emme_assemble_sets_batch",
                 "emme_solve_roots_sets", "emme_run_json_lockstep", "emme_scan_plan"):
        assert hasattr(lib, name), name
    assert lib.emme_version() == 4
    for name in ("bind_param_sets", "assemble_sets", "solve_roots_sets"):
        assert callable(getattr(emme.Context, name))
    assert callable(emme.params_same_shape) and callable(emme.run_json_lockstep) and callable(emme.scan_plan)
    assert emme.Context.SETS_FILL_KERNEL.startswith("k_assemble_sets")


def test_params_same_shape(emme):
    base = emme.params_from_dict(example_tokamak(npoints=16))
    for over in (dict(k_rho=0.5), dict(eta_i=2.0), dict(shat=1.1), dict(tau=1.3), dict(conf="cylinder"),
                 dict(length=14.0)):
        assert emme.params_same_shape(base, emme.params_from_dict(example_tokamak(npoints=16, **over))), over
    for over, name in ((dict(npoints=18), "npoints"), (dict(beta_e=0.01), "beta_e"),
                       (dict(integration_start_points=31), "integration_start_points"),
                       (dict(iteration_method="QRSecant"), "iteration_method")):
        other = emme.params_from_dict(example_tokamak(**dict(dict(npoints=16), **over)))
        assert emme.load().emme_params_same_shape(C.byref(base), C.byref(other)) == EMME_EINVAL
        assert name in emme.last_error(), (name, emme.last_error())
        assert not emme.params_same_shape(base, other)
    # two electromagnetic sets of different beta_e share a shape
    a = emme.params_from_dict(example_stellarator(npoints=16))
    b = emme.params_from_dict(example_stellarator(npoints=16, beta_e=0.03, eta_k=0.2))
    assert emme.params_same_shape(a, b)
    assert emme.load().emme_params_same_shape(None, C.byref(base)) == EMME_EINVAL


def test_argument_errors_come_before_the_device(emme):
    lib = emme.load()
    one = np.zeros(4)
    i1 = np.zeros(2, dtype=np.int32)
    p = one.ctypes.data
    fake = C.c_void_p(1)  # (never dereferenced: every call below fails on another argument first)
    assert lib.emme_assemble_sets_batch(None, i1.ctypes.data, p, 1, p, None, None) == EMME_EINVAL
    assert lib.emme_assemble_sets_batch(fake, None, p, 1, p, None, None) == EMME_EINVAL
    assert lib.emme_assemble_sets_batch(fake, i1.ctypes.data, None, 1, p, None, None) == EMME_EINVAL
    assert lib.emme_assemble_sets_batch(fake, i1.ctypes.data, p, 1, None, None, None) == EMME_EINVAL
    assert lib.emme_assemble_sets_batch(fake, i1.ctypes.data, p, 0, p, None, None) == EMME_EINVAL
    args = (1e-6, 5, p, i1.ctypes.data, i1.ctypes.data, None)
    assert lib.emme_solve_roots_sets(None, i1.ctypes.data, p, 1, 0, *args) == EMME_EINVAL
    assert lib.emme_solve_roots_sets(fake, None, p, 1, 0, *args) == EMME_EINVAL
    assert lib.emme_solve_roots_sets(fake, i1.ctypes.data, None, 1, 1, *args) == EMME_EINVAL
    assert lib.emme_solve_roots_sets(fake, i1.ctypes.data, p, 0, 0, *args) == EMME_EINVAL
    assert lib.emme_solve_roots_sets(fake, i1.ctypes.data, p, 1, 0, 1e-6, 5, None, i1.ctypes.data, i1.ctypes.data,
                                     None) == EMME_EINVAL
    assert lib.emme_ctx_bind_param_sets(None, None, 0) == EMME_EINVAL
    assert lib.emme_ctx_bind_param_sets(fake, None, 2) == EMME_EINVAL
    assert lib.emme_ctx_bind_param_sets(fake, None, -1) == EMME_EINVAL
    assert lib.emme_ctx_param_sets(None) == EMME_EINVAL
    out = C.c_void_p()
    assert lib.emme_run_json_lockstep(None, None, C.byref(out)) == EMME_EINVAL


def test_round_plan_two_axes(emme):
    """Two axes, one with a two-sided tail: every point of emme_scan_values once per axis, each continuing from the
    previous point of its line, the second direction from the head, rounds = the longest line + 1."""
    d = example_tokamak(npoints=24, omega_d_coeff={"head": 1.01, "step": 0.1, "tail": [0.81, 1.21]},
                        eta_i={"head": 3.13, "step": 0.2, "tail": 3.53})
    plan = emme.scan_plan(emme.json_text(d))
    assert list(plan["sequential"]) == [False, False]
    longest = 0
    keys = [k for k, v in d.items() if isinstance(v, dict)]  # axes come in input order
    assert sorted(keys) == ["eta_i", "omega_d_coeff"]
    for a, key in enumerate(keys):
        vals, turn = emme.scan_values(d[key]["head"], d[key]["step"], d[key]["tail"])
        sel = plan["axis"] == a
        assert list(plan["index"][sel]) == list(range(len(vals)))  # every point exactly once, in order
        pred, rnd = plan["pred"][sel], plan["round"][sel]
        assert pred[0] == -1 and rnd[0] == 0
        in_line = 0
        for k in range(1, len(vals)):
            if turn[k]:
                in_line = 0
            assert pred[k] == (0 if in_line == 0 else k - 1), (key, k)  # the head, or the previous point of the line
            in_line += 1
            assert rnd[k] == in_line and rnd[pred[k]] < rnd[k]
            longest = max(longest, in_line)
    assert list(emme.scan_values(1.01, 0.1, [0.81, 1.21])[1]) == [0, 0, 0, 1, 0]  # (the axis does turn)
    assert plan["n_rounds"] == longest + 1 == 3


@pytest.mark.parametrize("key, axis", [("npoints", {"head": 24, "step": 8, "tail": 40}),
                                       ("iteration_precision", {"head": 1.0e-6, "step": 1.0e-6, "tail": 3.0e-6}),
                                       ("iteration_step_limit", {"head": 20, "step": 5, "tail": 30}),
                                       ("integration_start_points", {"head": 15, "step": 16, "tail": 31}),
                                       ("beta_e", {"head": 0.0, "step": 0.01, "tail": 0.02})])
def test_round_plan_marks_sequential_axes(emme, key, axis):
    d = example_tokamak(npoints=24, eta_i={"head": 3.13, "step": 0.2, "tail": 3.53})
    d[key] = axis
    plan = emme.scan_plan(emme.json_text(d))
    keys = [k for k, v in d.items() if isinstance(v, dict)]
    for a, k in enumerate(keys):
        assert bool(plan["sequential"][a]) == (k == key)
        assert ((plan["round"][plan["axis"] == a] == -1).all()) == (k == key)
    assert plan["n_rounds"] == 3  # eta_i alone rides along: head + two points
    # beta_e that stays away from zero rides along
    if key == "beta_e":
        d[key] = {"head": 0.01, "step": 0.01, "tail": 0.03}
        assert not emme.scan_plan(emme.json_text(d))["sequential"].any()
