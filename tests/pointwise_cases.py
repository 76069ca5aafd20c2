"""Cases of the pointwise tests (test_pointwise_host.py, test_gpu_pointwise.py): single nodes of the mapped
integrand and single arguments of the Bessel helper.  TEST INFRASTRUCTURE: deterministic (seeded), small, and
built once per process; the oracle values of a case set are computed once and shared (treat them as read-only).

An item is (context, pair i < j, moment m, omega, abscissa x in (0, pi/2)); a GROUP is the items of one
(context, pair, m, omega): the node-level bar of the tests is relative to the largest oracle value of the group.
"""
import functools
import json
import os
import sys

import numpy as np

from oracle.binding import example_stellarator, example_tokamak

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from integrand_np import X15, PairNodes  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 20240607
CLAMP = -40.0          # safe_exp's threshold (src/Parameters.cpp:167-173)
CLAMP_BAND = 1e-9      # |Re arg + 40| below this: device and oracle may disagree on the clamp
CLAMP_NEAR = 1e-3      # the two clamp nodes of a group lie this close to Re arg = -40, one on each side
BAR = 1e-12            # node-level bar, relative to the group's largest |F_oracle|

# both contour senses; growing, weakly damped and strongly damped (Im omega = -1.5) modes
OMEGAS = np.array([-0.8 + 0.25j, 0.6 + 0.3j, -0.55 - 0.12j, 0.4 - 0.05j, -0.5 - 1.5j, 0.7 - 1.5j,
                   -1.656 + 2.49j, 0.3 + 0.02j])
DEPTHS = (0, 4, 10, 20)
CLAMP_SCAN_DEPTH = 6   # the clamp nodes are picked among the Kronrod nodes of every interval of this depth
N_RANDOM_PAIRS = 10
OMEGAS_PER_RANDOM_PAIR = 1


def contexts():
    """name -> (input dict, moments tested)"""
    taylor = json.load(open(os.path.join(G, "inputs.json")))["inputs"]["taylor"]
    return {"tokamak_es": (example_tokamak(npoints=16), (0,)),
            "stellarator_em": (example_stellarator(npoints=16), (0, 1, 2)),
            "taylor": (taylor, (0,))}


def kronrod_nodes(depth, index):
    """the 15 abscissae of interval `index` of bisection depth `depth` of (0, pi/2): scale * X + mid"""
    l, r = np.pi / 2 * index / (1 << depth), np.pi / 2 * (index + 1) / (1 << depth)
    mid, scale = (r + l) / 2, (r - l) / 2
    return np.concatenate([scale * X15 + mid, scale * (-X15[1:]) + mid])


@functools.lru_cache(maxsize=None)
def fixed_abscissae():
    """Kronrod nodes of the first, the last and one inner interval (the one that holds x = pi/6, t = 0.58: where the
    integrand lives) of each depth in DEPTHS; the outer ones reach t ~ 1e-8 and t ~ 1e8"""
    xs = []
    for d in DEPTHS:
        for k in sorted({0, (1 << d) // 3, (1 << d) - 1}):
            xs.append(kronrod_nodes(d, k))
    x = np.concatenate(xs)
    assert ((x > 0) & (x < np.pi / 2)).all()
    return x


@functools.lru_cache(maxsize=None)
def _scan_abscissae():
    return np.concatenate([kronrod_nodes(CLAMP_SCAN_DEPTH, k) for k in range(1 << CLAMP_SCAN_DEPTH)])


def pairs_of(n, rng):
    fixed = [(0, 1), (n - 2, n - 1), (0, n - 1)]
    rnd = []
    while len(rnd) < N_RANDOM_PAIRS:
        i, j = sorted(int(v) for v in rng.integers(0, n, 2))
        if i < j and (i, j) not in fixed and (i, j) not in rnd:
            rnd.append((i, j))
    return fixed, rnd


def _clamp_nodes(pn, w, scan, re_arg):
    """Two abscissae that bracket a crossing of Re(A0 + T w) = -40, both within CLAMP_NEAR of it and, bisection
    halving the distance, far outside CLAMP_BAND.  The crossing is the one between the two adjacent scan nodes that
    lie closest to the threshold, closed in by bisection on PairNodes.a0_t.  A group without a crossing (safe_exp
    zeroes all of it) gets its two scan nodes nearest to the threshold."""
    order = np.argsort(scan)
    xs, g = scan[order], re_arg[order] - CLAMP
    cross = np.nonzero((g[:-1] < 0) != (g[1:] < 0))[0]
    if len(cross) == 0:
        return scan[np.argsort(np.abs(re_arg - CLAMP), kind="stable")[:2]]
    k = cross[np.argmin(np.minimum(np.abs(g[cross]), np.abs(g[cross + 1])))]
    lo, hi, glo, ghi = xs[k], xs[k + 1], g[k], g[k + 1]
    for _ in range(60):
        if max(abs(glo), abs(ghi)) < CLAMP_NEAR:
            break
        mid = 0.5 * (lo + hi)
        a0, t = pn.a0_t(mid)
        gm = (a0 + t * w).real - CLAMP
        if (gm < 0) == (glo < 0):
            lo, glo = mid, gm
        else:
            hi, ghi = mid, gm
    assert max(abs(glo), abs(ghi)) < CLAMP_NEAR and min(abs(glo), abs(ghi)) > 1e3 * CLAMP_BAND
    return np.array([lo, hi])


class CaseSet:
    """items of one context as flat arrays: i, j, m (int32), x (float64), w (complex128), group (int32)"""

    def __init__(self, name, d, i, j, m, x, w, group):
        self.name, self.d = name, d
        self.i, self.j, self.m, self.x, self.w, self.group = i, j, m, x, w, group
        self.n = len(x)
        self.ngroups = int(group.max()) + 1


@functools.lru_cache(maxsize=None)
def case_sets(orc):
    """{context name: CaseSet}.  The three fixed pairs meet every omega, a random pair one of them."""
    rng = np.random.default_rng(SEED)
    out = {}
    for name, (d, moments) in contexts().items():
        po = orc.params(d)
        n = po.npoints
        eta, _ = orc.grid(po.length, n)
        fixed, rnd = pairs_of(n, rng)
        plan = [(p, range(len(OMEGAS))) for p in fixed]
        plan += [(p, sorted(rng.choice(len(OMEGAS), OMEGAS_PER_RANDOM_PAIR, replace=False))) for p in rnd]
        scan = _scan_abscissae()
        I, J, M, X, W, GR = [], [], [], [], [], []
        g = 0
        for (i, j), wsel in plan:
            a0t, pns = {}, {}
            for k in wsel:
                w = complex(OMEGAS[k])
                omi = -np.copysign(1.0, w.real)
                if omi not in a0t:  # (A0, T) of the scan nodes: per pair and contour sense
                    pn = pns[omi] = PairNodes(orc, po, eta[i], eta[j], omi)
                    a0t[omi] = np.array([pn.a0_t(x) for x in scan])
                re_arg = (a0t[omi][:, 0] + a0t[omi][:, 1] * w).real
                near = _clamp_nodes(pns[omi], w, scan, re_arg)
                xs = np.concatenate([fixed_abscissae(), near])
                for m in moments:
                    I.append(np.full(len(xs), i)), J.append(np.full(len(xs), j)), M.append(np.full(len(xs), m))
                    X.append(xs), W.append(np.full(len(xs), w)), GR.append(np.full(len(xs), g))
                    g += 1
        out[name] = CaseSet(name, d, np.concatenate(I).astype(np.int32), np.concatenate(J).astype(np.int32),
                            np.concatenate(M).astype(np.int32), np.concatenate(X), np.concatenate(W),
                            np.concatenate(GR).astype(np.int32))
    return out


@functools.lru_cache(maxsize=None)
def oracle_values(orc, name):
    """(F_oracle [n] complex, Re of safe_exp's argument [n]) of a case set"""
    cs = case_sets(orc)[name]
    po = orc.params(cs.d)
    eta, _ = orc.grid(po.length, po.npoints)
    f = np.zeros(cs.n, dtype=np.complex128)
    arg = np.zeros(cs.n)
    for k in range(cs.n):
        f[k], arg[k] = orc.kappa_integrand(po, int(cs.m[k]), eta[cs.i[k]], eta[cs.j[k]], complex(cs.w[k]),
                                           float(cs.x[k]), want_clamp_arg=True)
    f.setflags(write=False), arg.setflags(write=False)
    return f, arg


def node_zabs(orc, cs):
    """|z| = sqrt(b_i b_j) / |lambda| of every item, the argument of the Bessel helper (as PairNodes builds lambda)"""
    po = orc.params(cs.d)
    eta, _ = orc.grid(po.length, po.npoints)
    out = np.zeros(cs.n)
    for key in sorted({(int(i), int(j), bool(w.real > 0)) for i, j, w in zip(cs.i, cs.j, cs.w)}):
        i, j, pos = key
        pn = PairNodes(orc, po, eta[i], eta[j], -1.0 if pos else 1.0)
        sel = (cs.i == i) & (cs.j == j) & ((cs.w.real > 0) == pos)
        t = np.tan(cs.x[sel])
        u = t * pn.inv_arc
        e = (1 - 1j * pn.omi * u) / np.sqrt(1 + u * u)
        out[sel] = pn.s / np.abs(1 + 1j * pn.c_lam * t * e)
    return out


def group_max(cs, v):
    """per item: the largest |v| of the item's group"""
    gm = np.zeros(cs.ngroups)
    np.maximum.at(gm, cs.group, np.abs(v))
    return gm[cs.group]


# ---- Bessel arguments ------------------------------------------------------------------------------------------------
def _rounded_abs(x, y):
    """|x + i y| correctly rounded (the device probe's |z|)"""
    import mpmath as mp
    with mp.workdps(60):
        return float(mp.sqrt(mp.mpf(x) ** 2 + mp.mpf(y) ** 2))


def _at_radius(r, th):
    """z near r exp(i th) whose modulus is the double r itself: both correctly rounded and as the C library's hypot
    (the oracle's cabs) returns it -- hypot is an ulp off the rounded value in about 1 % of r (cos th, sin th), and the
    Miller start index n0 = floor|z| + 1 is a floor of that number.  The larger component moves by an ulp at a time."""
    x, y = r * np.cos(th), r * np.sin(th)
    for _ in range(16):
        m, h = _rounded_abs(x, y), abs(complex(x, y))
        if m == r and h == r:
            return complex(x, y)
        up = (m < r) or (m == r and h < r)
        if abs(x) >= abs(y):
            x = np.nextafter(x, np.copysign(np.inf, x) if up else 0.0)
        else:
            y = np.nextafter(y, np.copysign(np.inf, y) if up else 0.0)
    raise AssertionError((r, th))


@functools.lru_cache(maxsize=None)
def bessel_arguments():
    """|z|: 60 log-spaced values in [1e-6, 300], every integer 1..64 and its two neighbouring doubles (the Miller
    start index n0 = floor|z| + 1 switches there); 33 angles in [-pi, pi], the axes exact, with both signs of a zero
    real part on the imaginary axis (the Re z < 0 switch) and of a zero imaginary part on the negative real axis.
    Off the axes |z| is the intended double exactly (_at_radius)."""
    radii = list(np.geomspace(1e-6, 300.0, 60))
    for k in range(1, 65):
        radii += [np.nextafter(float(k), 0.0), float(k), np.nextafter(float(k), np.inf)]
    z = []
    for r in radii:
        for k in range(33):
            if k % 8:
                z.append(_at_radius(r, -np.pi + k * np.pi / 16))
        z += [complex(r, 0.0), complex(-r, 0.0), complex(-r, -0.0),
              complex(0.0, r), complex(0.0, -r), complex(-0.0, r), complex(-0.0, -r)]
    z = np.array(z, dtype=np.complex128)
    z.setflags(write=False)
    return z
