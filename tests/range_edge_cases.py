"""Cases of the range-edge tests (test_range_edge_host.py, test_gpu_range_edge.py): omegas whose matrices come within
a few decades of EMME_MAX_ENTRY = 1e150 (assemble_common.hpp), omegas beyond it and omegas whose matrix is lost at once,
for the four shapes of fill kernel.  TEST INFRASTRUCTURE: data, plus the oracle-only measurements both tests share
(computed once per process and read-only).

A ROLE says what an omega is for:
  ordinary_a / ordinary_b   everyday omegas of the shape (W_FILL / OMEGAS_EM of test_gpu_device_forms.py), one of each
                            contour class
  sharp_large / sharp_edge  in range, and the oracle's own matrix moves by <= 1e-9 max|M| under omega (1 + 1e-13):
                            values are compared tightly there
  deep_large / deep_edge    in range, trees of hundreds of intervals per integral; the oracle's spread is 1e-8 .. 2e-3,
                            so values guard finiteness and gross error only -- the interval totals are exact all the same
  beyond                    the oracle is finite, at least one integral is >= 1e152: the device must flag the matrix
  lost                      the oracle's matrix holds a non-finite entry

The premises of every (shape, N, set, omega) are conditions test_range_edge_host.py recomputes from the oracle; RECORDED
holds what they came out as when the cases were chosen (smallest grid of the shape, set 0).
"""
import functools

import numpy as np

from oracle.binding import Oracle, example_stellarator, example_tokamak

MAX_ENTRY = 1e150          # EMME_MAX_ENTRY
IN_RANGE_COMP = 1e148      # an in-range omega keeps every integral's |Re|, |Im| below this
BEYOND_COMP = 1e152        # a beyond omega has at least one integral's |Re| or |Im| above this
SHARP_SPREAD = 1e-9
REL_STEP = 1e-13           # the perturbation of make_golden_cfg3_damped.py

SHAPES = {
    # name: (example, keywords of the smallest grid, the parameter a second bound set changes)
    "es15": (example_tokamak, dict(npoints=12), dict(eta_i=3.0)),
    "es31": (example_tokamak, dict(npoints=12, integration_start_points=31), dict(eta_i=3.0)),
    "em15": (example_tokamak, dict(npoints=8, beta_e=0.02), dict(eta_i=3.0)),
    "em31": (example_stellarator, dict(npoints=8), dict(eta_i=3.13)),
}

OMEGAS = {
    "es15": dict(ordinary_a=-0.8 + 0.25j, ordinary_b=0.153 - 0.316j, sharp_large=0.5 - 4.6j, sharp_edge=0.5 - 5j,
                 deep_large=-0.1 - 3j, deep_edge=-0.1 - 4j, beyond=0.5 - 5.4j, lost=0.5 - 9j),
    "em15": dict(ordinary_a=-1.656 + 2.49j, ordinary_b=0.4 - 0.2j, sharp_large=0.5 - 4.6j, sharp_edge=0.5 - 5j,
                 deep_edge=-0.1 - 4j, beyond=0.5 - 5.4j, lost=0.5 - 9j),
    # GK31 has no sharp point near 1e150: from about 1e130 upwards the oracle's own GK31 matrix moves by 1e-4 .. 1e-2
    # under the 1e-13 perturbation, so 1e115 .. 1e119 is as far as values are compared
    "es31": dict(ordinary_a=-0.8 + 0.25j, ordinary_b=0.153 - 0.316j, sharp_large=1 - 5j, deep_large=2 - 6j,
                 beyond=0.5 - 5.4j, lost=0.5 - 9j),
    "em31": dict(ordinary_a=-1.656 + 2.49j, ordinary_b=0.4 - 0.2j, sharp_large=1 - 5j, deep_large=2 - 6j,
                 beyond=0.5 - 5.4j, lost=0.5 - 9j),
}
IN_RANGE = ("ordinary_a", "ordinary_b", "sharp_large", "sharp_edge", "deep_large", "deep_edge")
SHARP = ("ordinary_a", "ordinary_b", "sharp_large", "sharp_edge")
BAD = ("beyond", "lost")

# (shape, role): max|M|, interval total of the oracle on the smallest grid; None: not finite
RECORDED = {
    ("es15", "sharp_large"): (5.0e131, 202), ("es15", "sharp_edge"): (1.5e148, 202),
    ("es15", "deep_large"): (4.2e100, 35774), ("es15", "deep_edge"): (2.3e141, 64236),
    ("es15", "beyond"): (4.6e164, 202), ("es15", "lost"): (None, 198),
    ("em15", "sharp_large"): (1.5e129, 264), ("em15", "sharp_edge"): (4.6e145, 264),
    ("em15", "deep_edge"): (2.0e143, 79124), ("em15", "beyond"): (1.5e162, 264), ("em15", "lost"): (None, 252),
    ("es31", "sharp_large"): (5.5e117, 198), ("es31", "deep_large"): (9.1e116, 3094),
    ("es31", "beyond"): (3.4e164, 10950), ("es31", "lost"): (None, 198),
    ("em31", "sharp_large"): (6.7e115, 252), ("em31", "deep_large"): (1.8e119, 3784),
    ("em31", "beyond"): (5.2e161, 13062), ("em31", "lost"): (None, 252),
}

# grids beside the smallest one that a route of test_gpu_range_edge.py needs to reach its kernel: shape -> npoints
EXTRA_GRIDS = {"es15": (), "es31": (), "em15": (), "em31": ()}
# the searches of section D: the tokamak at N = 24 with one guess whose first fill is lost
SEARCH_SHAPE, SEARCH_NPOINTS, SEARCH_LOST_GUESS = "es15", 24, 0.5 - 9.2j


def shape_dict(shape, npoints=None, second_set=False):
    make, kw, second = SHAPES[shape]
    kw = dict(kw)
    if npoints is not None:
        kw["npoints"] = npoints
    if second_set:
        kw.update(second)
    return make(**kw)


def grids(shape):
    return (SHAPES[shape][1]["npoints"],) + tuple(EXTRA_GRIDS[shape])


def cases():
    """Every (shape, npoints, second set?, role, omega) a GPU assertion rests on.  The second set serves the ordinary
    omegas only (the sets fills give the large and bad items to set 0)."""
    out = []
    for shape in SHAPES:
        for n in grids(shape):
            for role, w in OMEGAS[shape].items():
                out.append((shape, n, False, role, complex(w)))
                if role.startswith("ordinary"):
                    out.append((shape, n, True, role, complex(w)))
    return out


@functools.lru_cache(maxsize=None)
def _oracle():
    return Oracle()


@functools.lru_cache(maxsize=None)
def oracle_fill(shape, npoints, second_set, omega):
    """(M, interval total) of the oracle; read-only."""
    orc = _oracle()
    M, tot = orc.assemble(orc.params(shape_dict(shape, npoints, second_set)), complex(omega))
    M.setflags(write=False)
    return M, tot


@functools.lru_cache(maxsize=None)
def oracle_spread(shape, npoints, second_set, omega):
    """max|M(omega (1 + 1e-13)) - M(omega)| / max|M(omega)| in the oracle, and whether the interval totals at
    omega (1 +- 1e-13) are that of omega."""
    M, tot = oracle_fill(shape, npoints, second_set, omega)
    Mp, totp = oracle_fill(shape, npoints, second_set, complex(omega) * (1 + REL_STEP))
    _, totm = oracle_fill(shape, npoints, second_set, complex(omega) * (1 - REL_STEP))
    return float(np.abs(Mp - M).max() / np.abs(M).max()), bool(tot == totp == totm)


@functools.lru_cache(maxsize=None)
def oracle_comp(shape, npoints, second_set, omega):
    """|Re| and |Im| of every single integral (pair i < j, moment) of the oracle: the numbers kappa_bad looks at."""
    orc = _oracle()
    po = orc.params(shape_dict(shape, npoints, second_set))
    eta, _ = orc.grid(po.length, po.npoints)
    nm = 1 if po.beta_e == 0.0 else 3
    out = []
    for i in range(po.npoints):
        for j in range(i + 1, po.npoints):
            for m in range(nm):
                k, _ = orc.kappa(po, m, eta[i], eta[j], complex(omega))
                out.append(max(abs(k.real), abs(k.imag)) if np.isfinite(k.real) and np.isfinite(k.imag) else np.inf)
    out = np.array(out)
    out.setflags(write=False)
    return out


RICHARDSON_REL_H = 1e-5


@functools.lru_cache(maxsize=None)
def oracle_derivative(shape, npoints):
    """dM/domega of the oracle at the shape's sharp_large omega: the Richardson-extrapolated central difference
    (4 D(h/2) - D(h)) / 3, h = 1e-5 |omega|, taken along Re omega and along Im omega.  Returns (M' along Re, the largest
    disagreement of the two extrapolations relative to max|M'|, whether every oracle fill used walked the tree of omega
    itself)."""
    w = complex(OMEGAS[shape]["sharp_large"])
    h = RICHARDSON_REL_H * abs(w)
    _, tot = oracle_fill(shape, npoints, False, w)
    same_tree = True

    def D(step):
        nonlocal same_tree
        Mp, tp = oracle_fill(shape, npoints, False, w + step)
        Mm, tm = oracle_fill(shape, npoints, False, w - step)
        same_tree = same_tree and tp == tot == tm
        return (Mp - Mm) / (2.0 * step)

    R = [(4.0 * D(0.5 * h * u) - D(h * u)) / 3.0 for u in (1.0, 1j)]
    R[0].setflags(write=False)
    return R[0], float(np.abs(R[0] - R[1]).max() / np.abs(R[0]).max()), same_tree


def bar(shape, npoints, second_set, omega):
    """The absolute bar on |M - M_oracle|.max(): TOL_M = 1e-10 of max|M|, or 10 x the oracle's own spread (the rule of
    test_damped_omegas_full_size_match_reference_checksums)."""
    M, _ = oracle_fill(shape, npoints, second_set, omega)
    spread, _ = oracle_spread(shape, npoints, second_set, omega)
    return max(1e-10, 10.0 * spread) * float(np.abs(M).max())
