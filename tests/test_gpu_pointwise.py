"""GPU tests, node by node (pytest -m gpu): the math primitives of the fill alone against mpmath, the Bessel helper
at its switches against the oracle (and both against mpmath), and the pointwise integrand in its four device
formulations against the oracle's integrand and against each other.  Every check prints its measured worst case
(`POINTWISE <name> <value>`, visible with -s) before it asserts: DESIGN.md's appendix "pointwise accuracy" is that list.

Bounds.  ULP = 2^-52.  fexp and fsincos: the CPU measurements of a plain-C copy against long double (DESIGN.md
appendix) with headroom for an unsampled worst case only.  frcp / frsqrt / rcp: 0.5 ulp of the correctly rounded
result + 1.5 ulp for the last, uncorrected Newton step.  Bessel: the bars of test_gpu_round2.py.  Integrand: 1e-12 of
the largest oracle value of the item's (context, pair, m, omega) group -- the matrix bar 1e-10, a hundred times
tighter because nothing is summed.
"""
import functools
import os
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointwise_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52
DPS = 40
SEED = 7
NAMES = ("tokamak_es", "stellarator_em", "taylor")


def report(name, value):
    print(f"\nPOINTWISE {name} {value:.4g}")


def hilo(values):
    """mpmath numbers as unevaluated sums hi + lo of two doubles (hi = the correctly rounded value)"""
    hi = np.array([float(v) for v in values])
    lo = np.array([float(v - mp.mpf(h)) for v, h in zip(values, hi)])
    return hi, lo


def err_abs(got, ref):
    hi, lo = ref
    return np.abs((got - hi) - lo)


def err_rel(got, ref):
    return err_abs(got, ref) / np.abs(ref[0])


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ---- fexp ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exp_cases():
    rng = np.random.default_rng(SEED)
    ln2 = np.log(2.0)
    edge = [c for k in range(-57, 1023) for c in (np.nextafter(k * ln2, -np.inf), k * ln2, np.nextafter(k * ln2, np.inf))]
    x = np.concatenate([rng.uniform(-40.0, 709.0, 100000), [-40.0, 709.0], edge])
    x = x[(x >= -40.0) & (x <= 709.0)]
    with mp.workdps(DPS):
        ref = hilo([mp.exp(mp.mpf(float(v))) for v in x])
    return x, ref


def test_fexp_every_copy_against_mpmath(emme):
    x, ref = exp_cases()
    got = {fn: emme.elementary(fn, x) for fn in ("exp", "exp_s", "exp_v")}
    for fn, g in got.items():
        e = err_rel(g, ref) / ULP
        report(f"fexp[{fn}]_rel_ulp", e.max())
    for fn, g in got.items():
        e = err_rel(g, ref) / ULP
        assert e.max() <= 1.0, (fn, e.max(), x[e.argmax()])
    assert same_bits(got["exp"], got["exp_s"]) and same_bits(got["exp"], got["exp_v"])


# ---- fsincos -------------------------------------------------------------------------------------------------
SCALES = (1.0, 1e2, 1e4, 1e6, 1e9, 1e12)
N_PER_SCALE = 3000


def _sincos_args(scale, rng):
    x = rng.uniform(-scale, scale, N_PER_SCALE)
    with mp.workdps(DPS):  # a third of them: the double nearest to a multiple of pi / 2
        hp = mp.pi / 2
        for k in range(0, N_PER_SCALE, 3):
            x[k] = float(mp.nint(mp.mpf(float(x[k])) / hp) * hp)
    return x


@functools.lru_cache(maxsize=None)
def sincos_cases():
    """{scale: (x, sin as hi + lo, cos as hi + lo)}; 1e15 is outside the documented range (reported, not asserted)"""
    rng = np.random.default_rng(SEED + 1)
    out = {}
    for scale in SCALES + (1e15,):
        x = _sincos_args(scale, rng)
        with mp.workdps(DPS):
            xm = [mp.mpf(float(v)) for v in x]
            out[scale] = (x, hilo([mp.sin(v) for v in xm]), hilo([mp.cos(v) for v in xm]))
    return out


@pytest.mark.parametrize("fn", ["sincos", "sincos_s", "sincos_v"])
def test_fsincos_against_mpmath(emme, fn):
    """The 1e12 scale is where a quadrant taken from (int)n goes wrong: the conversion saturates from |x| = 3.4e9 on
    (emme_device.hpp::quadrant_bits)."""
    cases = sincos_cases()
    worst_abs, worst_rel, at_abs = 0.0, 0.0, None
    for scale in SCALES:
        x, s_ref, c_ref = cases[scale]
        got = emme.elementary(fn, x)
        ea = np.maximum(err_abs(got[:, 0], s_ref), err_abs(got[:, 1], c_ref)) / ULP
        if ea.max() > worst_abs:
            worst_abs, at_abs = ea.max(), x[ea.argmax()]
        if scale <= 1e9:
            with np.errstate(divide="ignore", invalid="ignore"):
                er = np.maximum(err_rel(got[:, 0], s_ref), err_rel(got[:, 1], c_ref)) / ULP
            worst_rel = max(worst_rel, np.nanmax(er))
    x, s_ref, c_ref = cases[1e15]
    got = emme.elementary(fn, x)
    report(f"fsincos[{fn}]_abs_ulp_1e12", worst_abs)
    report(f"fsincos[{fn}]_rel_ulp_1e9", worst_rel)
    report(f"fsincos[{fn}]_abs_ulp_1e15_unasserted",
           (np.maximum(err_abs(got[:, 0], s_ref), err_abs(got[:, 1], c_ref)) / ULP).max())
    assert worst_abs <= 1.0, (fn, worst_abs, at_abs)
    if fn == "sincos":  # the two-term copies lose relative accuracy near the zeros of sin and cos by design
        assert worst_rel <= 2.0, (fn, worst_rel)


def test_fsincos_register_copies_give_the_same_bits(emme):
    for scale, (x, _, _) in sincos_cases().items():
        assert same_bits(emme.elementary("sincos_s", x), emme.elementary("sincos_v", x)), scale


# ---- frcp, frsqrt, complex rcp ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def positive_arguments():
    """log-uniform in [1e-150, 1e150], and what the integrand really feeds the two functions: sin x cos x at the
    generator's abscissae, 1 + u^2, |lambda|^2, and Miller's |p|^2 up to 1e40"""
    rng = np.random.default_rng(SEED + 2)
    x = np.concatenate([pc.fixed_abscissae(), pc.kronrod_nodes(6, 21), pc.kronrod_nodes(3, 5)])
    t = np.tan(x)
    u = t / 100.0  # arc_coeff of every shipped input
    e = (1 - 1j * u) / np.sqrt(1 + u * u)
    lam2 = [np.abs(1 + 1j * c_lam * t * e) ** 2 for c_lam in (-0.31, 0.012, 2.7)]
    return np.concatenate([10.0 ** rng.uniform(-150, 150, 20000), np.sin(x) * np.cos(x), 1 + u * u, *lam2,
                           10.0 ** rng.uniform(0, 40, 2000)])


def test_frcp_and_frsqrt_against_the_correctly_rounded_result(emme):
    x = positive_arguments()
    with mp.workdps(DPS):
        xm = [mp.mpf(float(v)) for v in x]
        rcp_ref = np.array([float(1 / v) for v in xm])
        rsq_ref = np.array([float(1 / mp.sqrt(v)) for v in xm])
    assert np.array_equal(rcp_ref, 1.0 / x)  # float64 division is the correctly rounded quotient
    e_rcp = np.abs(emme.elementary("rcp", x) - rcp_ref) / np.abs(rcp_ref) / ULP
    e_rsq = np.abs(emme.elementary("rsqrt", x) - rsq_ref) / np.abs(rsq_ref) / ULP
    report("frcp_rel_ulp_vs_rounded", e_rcp.max())
    report("frsqrt_rel_ulp_vs_rounded", e_rsq.max())
    assert e_rcp.max() <= 2.0, (e_rcp.max(), x[e_rcp.argmax()])
    assert e_rsq.max() <= 2.0, (e_rsq.max(), x[e_rsq.argmax()])


def test_complex_rcp_against_the_correctly_rounded_quotient(emme):
    """rcp(a) = conj(a) * frcp(norm2(a)): each component against the correctly rounded a.x / norm2(a), norm2 as the
    device rounds it (one fma on the rounded a.y^2)"""
    # the rounding order below is emme_device.hpp::norm2, fma(a.x, a.x, a.y * a.y): if that definition changes, the
    # reference shifts by up to an ulp and this must follow
    rng = np.random.default_rng(SEED + 3)
    n2 = np.concatenate([10.0 ** rng.uniform(-150, 150, 20000), 10.0 ** rng.uniform(0, 40, 2000)])
    th = rng.uniform(-np.pi, np.pi, len(n2))
    a = np.sqrt(n2) * np.exp(1j * th)
    yy = a.imag * a.imag
    with mp.workdps(DPS):
        d = [mp.mpf(float(mp.mpf(float(re)) ** 2 + mp.mpf(float(y2)))) for re, y2 in zip(a.real, yy)]
        ref_re = np.array([float(mp.mpf(float(re)) / dd) for re, dd in zip(a.real, d)])
        ref_im = np.array([float(-mp.mpf(float(im)) / dd) for im, dd in zip(a.imag, d)])
    got = emme.elementary("crcp", a)
    e = np.maximum(np.abs(got.real - ref_re) / np.abs(ref_re), np.abs(got.imag - ref_im) / np.abs(ref_im)) / ULP
    report("complex_rcp_rel_ulp_vs_rounded", e.max())
    assert e.max() <= 2.0, (e.max(), a[e.argmax()])


# ---- Bessel helper -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bessel_oracle(orc):
    z = pc.bessel_arguments()
    out = np.array([orc.bessel(complex(v)) for v in z])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def bessel_device(emme):
    out = emme.bessel(pc.bessel_arguments())
    out.setflags(write=False)
    return out


def test_bessel_helper_at_its_switches_matches_oracle(emme, oracle):
    z, want, got = pc.bessel_arguments(), bessel_oracle(oracle), bessel_device(emme)
    rel = [np.abs(got[:, c] - want[:, c]) / np.abs(want[:, c]) for c in range(3)]
    r_got, r_want = got[:, :2] / got[:, 2:3], want[:, :2] / want[:, 2:3]
    ratio = np.abs(r_got - r_want).max(axis=1) / np.abs(r_want).max()
    report("bessel_component_rel_vs_oracle", max(r.max() for r in rel))
    report("bessel_ratio_vs_oracle_over_max", ratio.max())
    for c in range(3):
        assert rel[c].max() <= 1e-11, (c, rel[c].max(), z[rel[c].argmax()])
    assert ratio.max() <= 1e-12, (ratio.max(), z[ratio.argmax()])
    assert same_bits(got[:, 3].copy(), want[:, 3].copy())  # -/+ z, the sign of a zero included


N_BESSEL_CHUNKS = 6


@pytest.mark.parametrize("chunk", range(N_BESSEL_CHUNKS))
def test_bessel_ratios_no_worse_than_the_oracle_against_mpmath(emme, oracle, chunk):
    """mpmath documents the ALGORITHM's error (about 1 / threshold = 5e-8 / 10): the device is held to being no worse
    than the oracle, argument by argument, not to mpmath"""
    sel = slice(chunk, None, N_BESSEL_CHUNKS)
    z, want, got = pc.bessel_arguments()[sel], bessel_oracle(oracle)[sel], bessel_device(emme)[sel]
    with mp.workdps(30):
        exact = np.zeros((len(z), 2), dtype=np.complex128)
        for k, v in enumerate(z):
            zz = mp.mpc(float(v.real), float(v.imag))
            ez = mp.exp(zz if v.real < 0 else -zz)
            exact[k] = complex(mp.besseli(0, zz) * ez), complex(mp.besseli(1, zz) * ez)
    size = np.abs(exact).max(axis=1)
    e_dev = np.abs(got[:, :2] / got[:, 2:3] - exact).max(axis=1)
    e_or = np.abs(want[:, :2] / want[:, 2:3] - exact).max(axis=1)
    report(f"bessel_ratio_vs_mpmath_device[{chunk}]", (e_dev / size).max())
    report(f"bessel_ratio_vs_mpmath_oracle[{chunk}]", (e_or / size).max())
    worse = e_dev - (e_or + 1e-12 * size)
    assert (worse <= 0).all(), (z[worse.argmax()], e_dev[worse.argmax()], e_or[worse.argmax()])


# ---- the pointwise integrand ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_forms(emme, orc, name):
    """forms 0, 1, 2 of a case set on the device: F0 [n], (F, F') [n, 2], (A0, T, Q1, Q0, F) [n, 5]"""
    cs = pc.case_sets(orc)[name]
    p = emme.params_from_dict(cs.d)
    out = tuple(emme.integrand(p, form, cs.i, cs.j, cs.m, cs.x, cs.w) for form in (0, 1, 2))
    for o in out:
        o.setflags(write=False)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_integrand_forms_match_oracle_node_by_node(emme, oracle, name):
    cs = pc.case_sets(oracle)[name]
    f_or, arg = pc.oracle_values(oracle, name)
    f0, f1, f2 = device_forms(emme, oracle, name)
    forms = {"integrand": f0[:, 0], "integrand_d": f1[:, 0], "node_eval": f2[:, 4]}
    band = np.abs(arg - pc.CLAMP) < pc.CLAMP_BAND
    clamped = arg < pc.CLAMP
    gmax = pc.group_max(cs, f_or)
    scale = np.where(gmax > 0, gmax, 1.0)
    for k, f in forms.items():
        report(f"integrand[{name}]_{k}_vs_oracle_over_group_max", (np.abs(f - f_or) / scale)[~band].max())
    report(f"integrand[{name}]_forms_apart_over_group_max",
           max((np.abs(a - b) / scale)[~band].max() for a in forms.values() for b in forms.values()))
    assert band.sum() <= 0.01 * cs.n
    for k, f in forms.items():
        assert np.isfinite(f).all(), k
        # the clamp: exact zeros where the oracle clamps and only there
        assert ((f == 0) == clamped)[~band].all(), (k, cs.x[~band][((f == 0) != clamped)[~band]][:4])
        assert (np.abs(f - f_or) <= pc.BAR * gmax)[~band].all(), k
    # inside the band each side returns either exact 0 or the unclamped value: (A0, T, Q1, Q0) of the device carry
    # no clamp, so the unclamped value is their recombination
    for k in np.nonzero(band)[0]:
        a0, t, q1, q0 = f2[k, :4]
        live = np.exp(a0 + t * cs.w[k]) * (cs.w[k] * q1 + q0)
        for f in list(forms.values()) + [f_or]:
            assert f[k] == 0 or abs(f[k] - live) <= pc.BAR * max(gmax[k], abs(live))
    for a in forms.values():
        for b in forms.values():
            assert (np.abs(a - b) <= pc.BAR * gmax)[~band].all()
    assert same_bits(f1[:, 0].copy(), f0[:, 0].copy())  # the derivative fills rely on it


@pytest.mark.parametrize("name", NAMES)
def test_split_and_derivative_recombined_in_mpmath(emme, oracle, name):
    """F = exp(A0 + T w)(w Q1 + Q0) and F' = exp(A0 + T w)(T (w Q1 + Q0) + Q1) from the device's (A0, T, Q1, Q0),
    recombined in mpmath (no device arithmetic shared): F against the oracle, F' against integrand_d's"""
    cs = pc.case_sets(oracle)[name]
    f_or, arg = pc.oracle_values(oracle, name)
    _, f1, f2 = device_forms(emme, oracle, name)
    live = np.nonzero((arg >= pc.CLAMP) & (np.abs(arg - pc.CLAMP) >= pc.CLAMP_BAND))[0]
    F = np.zeros(cs.n, dtype=np.complex128)
    Fd = np.zeros(cs.n, dtype=np.complex128)
    with mp.workdps(DPS):
        for k in live:
            a0, t, q1, q0 = (mp.mpc(float(v.real), float(v.imag)) for v in f2[k, :4])
            w = mp.mpc(float(cs.w[k].real), float(cs.w[k].imag))
            e, s = mp.exp(a0 + t * w), w * q1 + q0
            F[k], Fd[k] = complex(e * s), complex(e * (t * s + q1))
    gmax, gmax_d = pc.group_max(cs, f_or), pc.group_max(cs, Fd)
    e_f = np.abs(F - f_or)[live] / gmax[live]
    e_d = np.abs(Fd - f1[:, 1])[live] / gmax_d[live]
    report(f"split[{name}]_F_recombined_vs_oracle_over_group_max", e_f.max())
    report(f"split[{name}]_dF_recombined_vs_integrand_d_over_group_max", e_d.max())
    assert len(live) >= 1000
    assert np.isfinite(f1).all() and np.isfinite(f2).all()
    assert e_f.max() <= pc.BAR, cs.x[live][e_f.argmax()]
    assert e_d.max() <= pc.BAR, cs.x[live][e_d.argmax()]
    dead = (arg < pc.CLAMP) & (np.abs(arg - pc.CLAMP) >= pc.CLAMP_BAND)
    assert (f1[dead, 1] == 0).all()  # a clamped node is 0 in F' too


def test_moment_factor_recombined_in_mpmath(emme, oracle):
    """F_m = F_0 (c_nv W)^m, W = node_w (electromagnetic contexts with shared records store F_0 and W only)"""
    name = "stellarator_em"
    cs = pc.case_sets(oracle)[name]
    f_or, arg = pc.oracle_values(oracle, name)
    f_m = device_forms(emme, oracle, name)[0][:, 0]
    p = emme.params_from_dict(cs.d)
    sel = np.nonzero((cs.m > 0) & (arg >= pc.CLAMP) & (np.abs(arg - pc.CLAMP) >= pc.CLAMP_BAND))[0]
    assert len(sel) >= 1000 and set(cs.m[sel]) == {1, 2}
    i, j, x, w = cs.i[sel], cs.j[sel], cs.x[sel], cs.w[sel]
    f_0 = emme.integrand(p, emme.FORM_F, i, j, np.zeros_like(i), x, w)[:, 0]
    W = emme.integrand(p, emme.FORM_W, i, j, np.zeros_like(i), x, w)[:, 0]
    po = oracle.params(cs.d)
    eta, _ = oracle.grid(po.length, po.npoints)
    c_nv = po.q * po.R * (eta[i] - eta[j]) / po.vt
    want = np.zeros(len(sel), dtype=np.complex128)
    with mp.workdps(DPS):
        for k in range(len(sel)):
            nv = mp.mpf(float(c_nv[k])) * mp.mpc(float(W[k].real), float(W[k].imag))
            want[k] = complex(mp.mpc(float(f_0[k].real), float(f_0[k].imag)) * nv ** int(cs.m[sel[k]]))
    gmax = pc.group_max(cs, f_or)[sel]
    e = np.abs(f_m[sel] - want) / gmax
    report("moment_factor_F0_W_recombined_vs_F_m_over_group_max", e.max())
    assert e.max() <= pc.BAR, (x[e.argmax()], w[e.argmax()])
