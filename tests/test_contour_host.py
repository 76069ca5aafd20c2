"""The host half of the contour eigensolver (emme_contour_eigs: Beyn's step on given moments) against
numpy, on constructed moments and on moments of small nonlinear eigenvalue problems taken by the trapezoid rule.
No GPU: the moments come from numpy."""
import numpy as np
import pytest

EINVAL = -1


def _unitary(rng, n, k):
    q, _ = np.linalg.qr(rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k)))
    return q


def _match(got, want):
    """Largest distance of a one-to-one pairing (greedy on the sorted distance list)."""
    got, want = list(got), list(want)
    assert len(got) == len(want), (got, want)
    worst = 0.0
    while want:
        d = np.abs(np.subtract.outer(np.array(got), np.array(want)))
        i, j = np.unravel_index(np.argmin(d), d.shape)
        worst = max(worst, d[i, j])
        got.pop(i), want.pop(j)
    return worst


def _spectrum(kind, k, rng):
    if kind == "random":
        return None
    if kind == "clustered":  # three tight clusters
        centres = np.array([0.3 + 0.2j, -0.4 - 0.1j, 0.1 - 0.5j])
        return centres[np.arange(k) % 3] + 1e-4 * (rng.standard_normal(k) + 1j * rng.standard_normal(k))
    if kind == "defective":  # pairs 1e-2 apart coupled by 1: next to a Jordan block, eigenvalue condition ~ 1e2
        base = 0.5 * (rng.standard_normal((k + 1) // 2) + 1j * rng.standard_normal((k + 1) // 2))
        return np.concatenate([base, base + 1e-2])[:k]
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["random", "clustered", "defective"])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 16, 31, 48, 64])
def test_eigs_of_constructed_moments(emme, kind, k):
    rng = np.random.default_rng(1000 * k + len(kind))
    n, L = 120, min(64, k + 3)
    lam = _spectrum(kind, k, rng)
    if lam is None:
        B = (rng.standard_normal((k, k)) + 1j * rng.standard_normal((k, k))) / np.sqrt(k)
    elif kind == "defective":
        # the pairs as 2 x 2 blocks [[l, 1], [0, l + 1e-2]] (a near-Jordan block), similar to B by a unitary
        T = np.diag(lam).astype(complex)
        for j in range(min(len(lam) // 2, k - (k + 1) // 2)):
            i0, i1 = j, (k + 1) // 2 + j
            T[i0, i1] = 1.0
        Q = _unitary(rng, k, k)
        B = Q @ T @ Q.conj().T
    else:
        S = np.eye(k) + 0.3 * (rng.standard_normal((k, k)) + 1j * rng.standard_normal((k, k))) / np.sqrt(k)
        B = S @ np.diag(lam) @ np.linalg.inv(S)
    U, W = _unitary(rng, n, k), _unitary(rng, L, k)
    sig = np.logspace(0, -3, k)
    A0 = U @ np.diag(sig) @ W.conj().T
    A1 = U @ B @ np.diag(sig) @ W.conj().T
    mu, kk, s = emme.contour_eigs(A0, A1, 1e-8)
    assert kk == k
    np.testing.assert_allclose(s[:k], sig, rtol=1e-12)
    assert np.all(s[k:] <= 1e-13)
    ref = np.linalg.eigvals(B)
    scale = np.linalg.norm(B, 2)
    assert _match(mu, ref) <= 1e-10 * scale


def _trapezoid_moments(Minv_apply, c, a, b, N, V):
    """A_k = sum_j w_j z_j^k M(w_j)^-1 V on the ellipse c + a cos t + i b sin t (trapezoid rule)."""
    rho = max(a, b)
    t = 2 * np.pi * np.arange(N) / N
    om = c + a * np.cos(t) + 1j * b * np.sin(t)
    wts = (-a * np.sin(t) + 1j * b * np.cos(t)) / (1j * N)
    z = (om - c) / rho
    A0 = np.zeros(V.shape, complex)
    A1 = np.zeros(V.shape, complex)
    for j in range(N):
        X = Minv_apply(om[j], V)
        A0 += wts[j] * X
        A1 += wts[j] * z[j] * X
    return A0, A1, rho


def _inside(lam, c, a, b):
    return ((lam.real - c.real) / a) ** 2 + ((lam.imag - c.imag) / b) ** 2 < 1.0


def test_linear_pencil_order_40(emme):
    rng = np.random.default_rng(7)
    n = 40
    c, a, b = 0.2 + 0.1j, 0.9, 0.6
    # eigenvalues: 6 inside at normalised radius <= 0.7, the rest at >= 1.4
    t_in = rng.uniform(0, 2 * np.pi, 6)
    r_in = rng.uniform(0.0, 0.7, 6)
    lam_in = c + r_in * (a * np.cos(t_in) + 1j * b * np.sin(t_in))
    t_out = rng.uniform(0, 2 * np.pi, n - 6)
    r_out = rng.uniform(1.4, 3.0, n - 6)
    lam = np.concatenate([lam_in, c + r_out * (a * np.cos(t_out) + 1j * b * np.sin(t_out))])
    S = np.eye(n) + 0.2 * (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) / np.sqrt(n)
    A = S @ np.diag(lam) @ np.linalg.inv(S)
    V = rng.standard_normal((n, 10)) + 1j * rng.standard_normal((n, 10))
    A0, A1, rho = _trapezoid_moments(lambda w, V: np.linalg.solve(A - w * np.eye(n), V), c, a, b, 256, V)
    mu, k, s = emme.contour_eigs(A0, A1, 1e-8)
    assert k == 6, s
    got = c + rho * mu
    assert np.all(_inside(got, c, a, b))
    ref = np.linalg.eigvals(A)
    assert _match(got, ref[_inside(ref, c, a, b)]) < 1e-8


def test_quadratic_problem_order_20(emme):
    rng = np.random.default_rng(11)
    n = 20
    M2, M1, M0 = (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)) for _ in range(3))
    M2 += 4 * np.eye(n)
    # reference eigenvalues: the companion linearisation [[0, I], [-M2^-1 M0, -M2^-1 M1]]
    iM2 = np.linalg.inv(M2)
    Cmp = np.block([[np.zeros((n, n)), np.eye(n)], [-iM2 @ M0, -iM2 @ M1]])
    ref = np.linalg.eigvals(Cmp)
    # a circle around the eigenvalue nearest 0, its radius in the widest gap of the distances to it
    c = complex(ref[np.argmin(np.abs(ref))])
    d = np.sort(np.abs(ref - c))
    j = 2 + int(np.argmax(d[3:8] / d[2:7]))  # radius between d[j] and d[j + 1], at least 3 inside
    r = np.sqrt(d[j] * d[j + 1])
    assert d[j + 1] / d[j] > 1.2
    V = rng.standard_normal((n, 12)) + 1j * rng.standard_normal((n, 12))
    Q = lambda w, V: np.linalg.solve(w * w * M2 + w * M1 + M0, V)
    A0, A1, rho = _trapezoid_moments(Q, c, r, r, 512, V)
    mu, k, s = emme.contour_eigs(A0, A1, 1e-8)
    inside = ref[np.abs(ref - c) < r]
    assert k == len(inside), (k, len(inside), s)
    got = c + rho * mu
    assert np.all(np.abs(got - c) < r)
    assert _match(got, inside) < 1e-8


def test_too_few_probes_report_full_rank(emme):
    rng = np.random.default_rng(3)
    n = 30
    lam = np.concatenate([0.3 * (rng.standard_normal(8) + 1j * rng.standard_normal(8)), 5 + rng.standard_normal(n - 8)])
    A = np.diag(lam) + 0.05 * np.triu(rng.standard_normal((n, n)), 1)
    for L in (2, 4, 7):
        V = rng.standard_normal((n, L)) + 1j * rng.standard_normal((n, L))
        A0, A1, _ = _trapezoid_moments(lambda w, V: np.linalg.solve(A - w * np.eye(n), V), 0j, 1.5, 1.5, 128, V)
        _, k, _ = emme.contour_eigs(A0, A1, 1e-8)
        assert k == L


def test_bad_sizes_are_rejected(emme):
    import ctypes as C
    lib = emme.load()
    A = np.zeros((4, 3), dtype=np.complex128)
    mu = np.zeros(64, dtype=np.complex128)
    k = C.c_int(0)
    args = lambda n, L, tol=1e-8, me=64: (n, L, A.ctypes.data, A.ctypes.data, tol, me, mu.ctypes.data, C.byref(k), None)
    assert lib.emme_contour_eigs(*args(0, 3)) == EINVAL
    assert lib.emme_contour_eigs(*args(4, 0)) == EINVAL
    assert lib.emme_contour_eigs(*args(4, 65)) == EINVAL
    assert lib.emme_contour_eigs(*args(4, 3, tol=0.0)) == EINVAL
    assert lib.emme_contour_eigs(*args(4, 3, tol=1.0)) == EINVAL
    assert lib.emme_contour_eigs(*args(4, 3, me=0)) == EINVAL
    assert lib.emme_contour_eigs(4, 3, None, A.ctypes.data, 1e-8, 64, mu.ctypes.data, C.byref(k), None) == EINVAL
    with pytest.raises(emme.EmmeError) as e:
        emme.contour_eigs(np.zeros((5, 65)), np.zeros((5, 65)))
    assert e.value.code == EINVAL


def test_version_and_contour_defaults(emme):
    lib = emme.load()
    assert lib.emme_version() == 4
    c = emme.contour_default()
    assert c.size == C_sizeof(emme.Contour)
    assert c.points >= 4 and c.points & (c.points - 1) == 0
    assert c.max_points >= c.points and c.max_points & (c.max_points - 1) == 0
    assert 1 <= c.probes <= 64 and 0.0 < c.rank_tol < 1.0


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)
