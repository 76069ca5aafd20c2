"""Host side of the pointwise tests (no GPU): the two probe entry points exist and check their arguments before they
look for a device; the case generator of tests/pointwise_cases.py is sound (finite oracle values, at most 1 % of the
items inside the clamp band); and the oracle's exported integrand is the one its golden-checked kappa integrates.
"""
import ctypes

import numpy as np
import pytest

from oracle.binding import example_stellarator, example_tokamak

import pointwise_cases as pc

EINVAL, EDEVICE = -1, -3


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_probe_symbols_exist(emme):
    lib = emme.load()
    assert hasattr(lib, "emme_elementary_batch") and hasattr(lib, "emme_integrand_batch")


def _elementary_rc(emme, fn, x, n, out):
    return emme.load().emme_elementary_batch(fn, x, n, out)


def test_elementary_batch_rejects_bad_arguments_without_a_device(emme):
    x, out = np.ones(4), np.zeros(8)
    px, po = x.ctypes.data, out.ctypes.data
    assert _elementary_rc(emme, 0, None, 4, po) == EINVAL
    assert _elementary_rc(emme, 0, px, 4, None) == EINVAL
    assert _elementary_rc(emme, 0, px, 0, po) == EINVAL
    assert _elementary_rc(emme, 0, px, -3, po) == EINVAL
    assert _elementary_rc(emme, -1, px, 4, po) == EINVAL
    assert _elementary_rc(emme, 9, px, 4, po) == EINVAL
    for fn in range(9):  # every known primitive gets past the argument check
        assert _elementary_rc(emme, fn, px, 2, po) != EINVAL


def _integrand_rc(emme, p, form, i, j, m, x, w, null=None):
    """emme_integrand_batch's return code; `null` names one argument to pass as NULL (or "n": n = 0)"""
    i, j, m = (np.asarray(a, dtype=np.int32) for a in (i, j, m))
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.complex128)
    out = np.zeros(10 * len(x))
    a = {"p": ctypes.byref(p) if p is not None else None, "i": i.ctypes.data, "j": j.ctypes.data, "m": m.ctypes.data,
         "x": x.ctypes.data, "w": w.ctypes.data, "out": out.ctypes.data, "n": len(x)}
    if null is not None:
        a[null] = 0 if null == "n" else None
    return emme.load().emme_integrand_batch(a["p"], form, a["n"], a["i"], a["j"], a["m"], a["x"], a["w"], a["out"])


def test_integrand_batch_rejects_bad_arguments_without_a_device(emme):
    es = emme.params_from_dict(example_tokamak(npoints=16))
    em = emme.params_from_dict(example_stellarator(npoints=16))
    ok = dict(i=[0, 3], j=[1, 15], m=[0, 0], x=[0.3, 1.2], w=[-0.8 + 0.25j, 0.4 - 0.1j])
    for null in ("p", "i", "j", "m", "x", "w", "out", "n"):
        assert _integrand_rc(emme, es if null != "p" else None, 0, null=null, **ok) == EINVAL, null
    for form in (-1, 4):
        assert _integrand_rc(emme, es, form, **ok) == EINVAL
    bad = [dict(i=[0, 5], j=[1, 5]), dict(i=[0, 6], j=[1, 5]), dict(i=[0, -1], j=[1, 5]), dict(i=[0, 3], j=[1, 16]),
           dict(m=[0, 1]), dict(m=[0, -1]), dict(x=[0.3, 0.0]), dict(x=[0.3, np.pi / 2]), dict(x=[0.3, -0.1]),
           dict(x=[0.3, 1.6]), dict(x=[0.3, np.nan])]
    for b in bad:
        assert _integrand_rc(emme, es, 0, **{**ok, **b}) == EINVAL, b
    # moments 1 and 2 exist on an electromagnetic context, 3 on none
    assert _integrand_rc(emme, em, 0, **{**ok, "m": [1, 2]}) != EINVAL
    assert _integrand_rc(emme, em, 0, **{**ok, "m": [0, 3]}) == EINVAL
    for form in range(4):
        assert _integrand_rc(emme, es, form, **ok) != EINVAL
    for name in ("arc_coeff", "vt", "tau"):  # scalars the kernels divide by
        for v in (0.0, np.inf, np.nan):
            broken = emme.params_from_dict(example_tokamak(npoints=16))
            setattr(broken, name, v)
            assert _integrand_rc(emme, broken, 0, **ok) == EINVAL, (name, v)


@pytest.mark.skipif(_has_gpu(), reason="checks the answer of a machine without a GPU")
def test_probes_report_no_device_without_a_gpu(emme):
    x, out = np.ones(4), np.zeros(8)
    assert _elementary_rc(emme, 2, x.ctypes.data, 4, out.ctypes.data) == EDEVICE
    es = emme.params_from_dict(example_tokamak(npoints=16))
    assert _integrand_rc(emme, es, 0, i=[0], j=[1], m=[0], x=[0.3], w=[-0.8 + 0.25j]) == EDEVICE
    with pytest.raises(emme.EmmeError) as e:
        emme.elementary("exp", [1.0])
    assert e.value.code == EDEVICE


def test_case_set_is_small_finite_and_mostly_outside_the_clamp_band(oracle):
    sets = pc.case_sets(oracle)
    assert set(sets) == {"tokamak_es", "stellarator_em", "taylor"}
    total = excluded = live = 0
    for name, cs in sets.items():
        f, arg = pc.oracle_values(oracle, name)
        assert np.isfinite(f.view(np.float64)).all() and np.isfinite(arg).all(), name
        assert ((cs.x > 0) & (cs.x < np.pi / 2)).all() and (cs.i < cs.j).all()
        # the clamp as the oracle applies it: exact zeros below -40, and only there (a live value may underflow,
        # but not in this set)
        assert ((f == 0) == (arg < pc.CLAMP)).all(), name
        total += cs.n
        excluded += int((np.abs(arg - pc.CLAMP) < pc.CLAMP_BAND).sum())
        live += int((arg >= pc.CLAMP).sum())
        # both sides of the clamp, within CLAMP_NEAR of it, in every group that has a live node (the two nodes found
        # with PairNodes.a0_t); a group clamped altogether is rare
        has_live = np.zeros(cs.ngroups, dtype=bool)
        has_live[cs.group[arg >= pc.CLAMP]] = True
        assert (~has_live).sum() <= 3, name
        for side in (arg < pc.CLAMP, arg >= pc.CLAMP):
            near = np.full(cs.ngroups, np.inf)
            np.minimum.at(near, cs.group[side], np.abs(arg[side] - pc.CLAMP))
            assert near[has_live].max() < 2 * pc.CLAMP_NEAR, (name, near[has_live].max())
    assert 1.5e4 <= total <= 3e4
    assert excluded <= 0.01 * total
    assert live >= 5000  # enough nodes that are not exact zeros
    assert sets["stellarator_em"].m.max() == 2 and sets["tokamak_es"].m.max() == 0
    assert (pc.OMEGAS.real < 0).any() and (pc.OMEGAS.real > 0).any() and (pc.OMEGAS.imag == -1.5).any()
    x = pc.fixed_abscissae()
    assert np.tan(x.min()) < 1e-6 and np.tan(x.max()) > 1e6


def test_no_item_sits_where_the_miller_start_index_is_ambiguous(oracle):
    """n0 = floor|z| + 1, and the fill takes |z| = s * rsqrt(|lambda|^2), a few ulp from the oracle's cabs(s / lambda):
    an item whose |z| lies within 8 ulp of an integer could start the recurrence one index from the oracle and differ by
    the algorithm's own error (6e-10 of the ratio, DESIGN.md appendix "pointwise accuracy"), far above the node bar.
    The value tests stand on no item being there."""
    for name, cs in pc.case_sets(oracle).items():
        za = pc.node_zabs(oracle, cs)
        assert np.isfinite(za).all() and (za > 0).all()
        big = za >= 0.5  # (below, the nearest integer 0 is never reached: |z| > 0)
        gap = np.abs(za[big] - np.rint(za[big]))
        assert (gap > 8 * np.spacing(za[big])).all(), (name, gap.min())


def test_case_set_is_deterministic(oracle):
    a = pc.case_sets(oracle)
    b = pc.case_sets.__wrapped__(oracle)
    for name in a:
        for k in ("i", "j", "m", "x", "w", "group"):
            assert np.array_equal(getattr(a[name], k), getattr(b[name], k))


def test_bessel_arguments_cover_the_switches():
    z = pc.bessel_arguments()
    r = np.array([abs(complex(v)) for v in z])  # the C library's hypot, as the oracle's cabs
    assert r.min() <= 1e-6 and r.max() >= 300
    on_re = z[(z.imag == 0) & (z.real > 0)].real
    for k in range(1, 65):  # every integer |z| and its two neighbouring doubles, exactly, on the real axis
        assert {np.nextafter(float(k), 0.0), float(k), np.nextafter(float(k), np.inf)} <= set(on_re)
    imag_axis = z[z.real == 0]
    assert (np.signbit(imag_axis.real)).any() and (~np.signbit(imag_axis.real)).any()
    assert (imag_axis.imag > 0).any() and (imag_axis.imag < 0).any()
    assert np.array_equal(r, np.array([pc._rounded_abs(v.real, v.imag) for v in z]))  # |z| is unambiguous
    radii = set(np.geomspace(1e-6, 300.0, 60))
    for k in range(1, 65):
        radii |= {np.nextafter(float(k), 0.0), float(k), np.nextafter(float(k), np.inf)}
    assert set(r) == radii
    r0 = np.geomspace(1e-6, 300.0, 60)[30]
    assert len(np.unique(np.round(np.angle(z[np.isclose(r, r0, rtol=1e-12, atol=0)]), 9))) >= 33


@pytest.mark.parametrize("name", ["tokamak_es", "stellarator_em"])
def test_exported_integrand_is_the_one_kappa_integrates(oracle, name):
    """oracle.kappa on an input whose tree cannot split (integration_iteration_limit = 0) is the GK15 rule on the one
    interval (0, pi/2), times -i qR / (vt sqrt(2 pi)); the same rule, summed in the same order, on the exported
    integrand reproduces it to the rounding of a 15-term sum: 16 * 2^-52 of sum w |f| (the complex products of the two
    sides are not the same instructions)."""
    d, moments = pc.contexts()[name]
    WK = np.array([2.09482141084727828e-01, 2.04432940075298892e-01, 1.90350578064785410e-01, 1.69004726639267903e-01,
                   1.40653259715525919e-01, 1.04790010322250184e-01, 6.30920926299785533e-02, 2.29353220105292250e-02])
    po = oracle.params(dict(d, integration_start_points=15, integration_iteration_limit=0))
    eta, _ = oracle.grid(po.length, po.npoints)
    pref = -1j * po.q * po.R / (po.vt * np.sqrt(2 * np.pi))
    xs = pc.kronrod_nodes(0, 0)  # centre, +x_1..+x_7, -x_1..-x_7
    scale = np.pi / 4
    for (i, j) in ((0, 1), (3, 9), (0, po.npoints - 1)):
        for m in moments:
            for w in (-0.8 + 0.25j, 0.4 - 0.05j, -0.5 - 1.5j):
                want, nint = oracle.kappa(po, m, eta[i], eta[j], w)
                assert nint == 1
                fa = [oracle.kappa_integrand(po, m, eta[i], eta[j], w, float(x), want_clamp_arg=True) for x in xs]
                f = np.array([v[0] for v in fa])
                assert all((v[0] == 0) == (v[1] < pc.CLAMP) for v in fa)
                K = WK[0] * f[0]
                for q in range(1, 8):
                    K += (f[q] + f[q + 7]) * WK[q]
                got = pref * (K * scale)
                size = abs(pref) * scale * (np.concatenate([WK, WK[1:]]) * np.abs(f)).sum()
                assert size > 0 and abs(got - want) <= 16 * 2.0 ** -52 * size, (i, j, m, w, got, want)
