"""Inputs of the linear-algebra route tests (test_gpu_linalg_routes.py; test_linalg_routes_host.py checks their premises
on the CPU): the project's existing input families, each built once per (family, order) with its numpy reference and
kept unchanged, and what the tests need to know about the launchers' dispatch.

Families (seeds and formulas are those of the tests they come from, so their bars apply):
  shifted_symmetric   test_trace_solve_sizes_against_lapack (test_gpu_parity.py)
  constructed         _constructed of test_gpu_eigenpairs.py (singular values logspace(0, -3): kappa = 1e3)
  null_family         test_null_vectors_batch_general_matrices (test_gpu_round3.py): U diag(s) V^H, s_n = 1e-4 .. 1e-14
  fold_inputs         structured_pair of fold_reference.py, as _inputs of test_gpu_fold.py builds them
  qr_inputs           test_qr_secant_quotient_matches_lapack_sequence (test_gpu_parity.py)
and one cheap family for large batches:
  pdm_family          M_b = P_b D_b M_0: P_b a row permutation, D_b unit-modulus phases, M_0 a null_family member.
                      M_b^H M_b = M_0^H M_0, so every member has M_0's singular values and right singular vectors, and
                      M_b^-1 = M_0^-1 D_b^-1 P_b^T: a batch costs one QR pair and one factorisation per base matrix.
                      Items alternate between two base matrices, so that neighbours have different null vectors.
"""
import numpy as np

from fold_reference import structured, structured_pair

EPS = np.finfo(np.float64).eps

# ---- the launchers' dispatch, restated from the formulas of linstep_blocked.hip -------------------------------------
LDS_LIMIT = 150 * 1024  # bytes of LDS a one-workgroup panel may take
NB = 16                 # rows per panel


def blocked_lds_bytes(n):
    """trace_solve_blocked_lds(n): three int row maps, the 16 x 16 diagonal block and a pivot row, the L21 panel of n
    rows at stride 17 (never less than the operand stage of 2 x 16 waves x 16), in 16-byte complex units."""
    return ((12 * n + 15) // 16 + NB * NB + NB + max(17 * n, 2 * 16 * NB)) * 16


def lds_edge():
    """The largest order whose whole panel fits one workgroup's LDS."""
    n = 1
    while blocked_lds_bytes(n + 1) <= LDS_LIMIT:
        n += 1
    return n


# kernel symbols as Context.linstep_kernel_symbol() reports them
ONE_WG = "k_trace_solve_blocked<false, false>"
SPLIT = "k_trace_solve_blocked<true, false>"
CHUNKED = "k_trace_solve_blocked<true, true>"
GROUPED = "k_trace_solve_grouped"
UNBLOCKED = "k_trace_solve"
LU_INPLACE = "k_lu_inplace"
LU_UNBLOCKED = "k_lu_unblocked_inplace"


def lu_workgroups(n, n_live, n_cu, lu_split=0):
    """Workgroups per matrix that trace_solve asks for (lu_workgroups of linstep_plan.hpp, on a context whose
    hand-overs never timed out)."""
    nwg = 1
    if lu_split > 0:
        nwg = min(lu_split, 16)
    elif n >= 128:
        nwg = max(1, min(16 if n >= 768 else 8 if n >= 384 else 4, n_cu // n_live))
    if n > lds_edge() and nwg < 2 and lu_split != 1:
        nwg = 2
    return nwg


def expected_trace_route(n, nwg, group_min_n, resident=True):
    """What a trace step must launch when it asks for nwg workgroups per matrix; resident: the grid of a launch with
    several workgroups per matrix fits the device at once."""
    if n > 1024:
        return UNBLOCKED
    if n > lds_edge():
        return CHUNKED if nwg >= 2 and resident else UNBLOCKED
    if nwg == 1 or not resident:
        return ONE_WG
    return GROUPED if nwg < 4 and 0 < group_min_n <= n else SPLIT  # (from 4 workgroups on: look-ahead, never grouped)


def expected_lu_route(n):
    edge = lds_edge()
    return LU_INPLACE if n <= edge else CHUNKED if n <= 1024 else LU_UNBLOCKED


# ---- families --------------------------------------------------------------------------------------------------------
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        out = make()
        for a in out if isinstance(out, tuple) else (out,):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def _cplx(rng, *shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def shifted_symmetric(n, nb=3):
    """(A, B, tr(A_b^-1 B_b)): A complex symmetric, its diagonal raised by sqrt(n) / 2."""
    def make():
        rng = np.random.default_rng(n)
        A = _cplx(rng, nb, n, n)
        A = A + np.transpose(A, (0, 2, 1)) + 0.5 * n ** 0.5 * np.eye(n)
        B = _cplx(rng, nb, n, n)
        want = np.array([np.trace(np.linalg.solve(A[b], B[b])) for b in range(nb)])
        return A, B, want
    return _cached(("shifted", n, nb), make)


def trace_bar(n, want):
    """1e-10 max(1, |want|) up to n = 1100, scaled by n / 1100 above (the forward bound of the LU is linear in n)."""
    return 1e-10 * np.maximum(1.0, np.abs(want)) * max(1.0, n / 1100.0)


def constructed(n):
    """(M, Mp, v, kappa): two matrices Q1 diag(logspace(0, -3)) Q2^H, random M' and unit vectors; kappa = cond_2 of
    each M, computed (orders <= 1100) or the construction's 1e3 (above)."""
    def make():
        rng = np.random.default_rng(1000 + n)
        sig = np.logspace(0.0, -3.0, n)
        M = np.array([(np.linalg.qr(_cplx(rng, n, n))[0] * sig) @ np.linalg.qr(_cplx(rng, n, n))[0].conj().T
                      for _ in range(2)])
        Mp = _cplx(rng, 2, n, n)
        v = _cplx(rng, 2, n)
        v /= np.linalg.norm(v, axis=1)[:, None]
        if n <= 1100:
            sv = [np.linalg.svd(M[b], compute_uv=False) for b in range(2)]
            kappa = np.array([s[0] / s[-1] for s in sv])
        else:
            kappa = np.full(2, 1e3)
        return M, Mp, v, kappa
    return _cached(("constructed", n), make)


def start_vector(n):
    """s of include/emme_hip.h: what an eigenpair step without a caller vector starts from."""
    i = np.arange(n, dtype=np.float64)
    return (1.0 + 0.37 * np.sin(1.0 + i)) + 1j * 0.21 * np.cos(2.0 * i)


def overlap(a, b):
    return abs(np.vdot(a, b)) / (np.linalg.norm(a) * np.linalg.norm(b))


def eigpair_errors(M, B, vin, u, vd, tau, resid):
    """(direction, tau, norm, residual) errors of one item of an eigenpair step against u = M^-1 B vin."""
    t = np.vdot(vin, u)
    return (1.0 - overlap(vd, u), abs(tau - t) / abs(t), abs(np.linalg.norm(vd) - 1.0),
            abs(resid - np.linalg.norm(M @ vin) / np.linalg.norm(M)))


def null_member(rng, n, gap):
    """One matrix U diag(s) V^H with s in [0.3, 3] and s_n = gap, and its right singular vector V[:, -1]."""
    U = np.linalg.qr(_cplx(rng, n, n))[0]
    V = np.linalg.qr(_cplx(rng, n, n))[0]
    s = np.sort(rng.uniform(0.3, 3.0, n))[::-1].copy()
    s[-1] = gap
    return (U * s) @ V.conj().T, V[:, -1].copy(), s


def null_family(n, nb=3):
    """(M, want): nb non-symmetric nearly singular matrices, s_n = 1e-4, 1e-6, ..., and their null vectors."""
    def make():
        rng = np.random.default_rng(n)
        out = [null_member(rng, n, 10.0 ** (-4 - 2 * b)) for b in range(nb)]
        return np.array([o[0] for o in out]), np.array([o[1] for o in out])
    return _cached(("null", n, nb), make)


class PdmFamily:
    """nb matrices M_b = P_b D_b M_0[b % 2] (see the module docstring).  base / want / kappa: the two base matrices,
    their null vectors and condition numbers; perm[b] / phase[b]: row i of M_b is phase[b][i] times row perm[b][i] of
    its base."""

    def __init__(self, n, nb, seed):
        rng = np.random.default_rng(seed)
        members = [null_member(rng, n, 1e-4) for _ in range(2)]
        self.n, self.nb = n, nb
        self.base = np.array([m[0] for m in members])
        self.want = np.array([m[1] for m in members])
        self.kappa = np.array([m[2][0] / m[2][-1] for m in members])
        self.perm = np.array([rng.permutation(n) for _ in range(nb)])
        self.phase = np.exp(2j * np.pi * rng.random((nb, n)))
        self.M = np.empty((nb, n, n), dtype=np.complex128)
        for b in range(nb):
            np.multiply(self.base[b % 2][self.perm[b]], self.phase[b][:, None], out=self.M[b])
        for a in (self.base, self.want, self.perm, self.phase, self.M):
            a.setflags(write=False)

    def solve(self, b, rhs):
        """M_b^-1 rhs through the base matrix: M_0^-1 (D_b^-1 P_b^T rhs)."""
        y = np.empty_like(rhs)
        y[self.perm[b]] = rhs / self.phase[b].reshape((-1,) + (1,) * (rhs.ndim - 1))
        return np.linalg.solve(self.base[b % 2], y)

    def moments(self, V, z, w, items=None):
        """(sum_b w_b M_b^-1 V, sum_b w_b z_b M_b^-1 V) over `items` (default: all).  The sums are linear in the
        right-hand sides, so each base matrix is solved once for its items' summed right-hand sides
        sum_b c_b D_b^-1 P_b^T V, taken in extended precision.  The base matrices have kappa = 3e4, where a plain
        double-precision solve is itself wrong by several 1e-12 -- the size of the moments' bar -- so each solve is
        refined three times on its extended-precision residual: what comes back is right to a few eps."""
        n, L = V.shape
        items = range(self.nb) if items is None else items
        out = []
        for coef in (w, w * z):
            total = np.zeros((n, L), dtype=np.clongdouble)
            for k in range(2):
                Y = np.zeros((n, L), dtype=np.clongdouble)
                for b in items:
                    if b % 2 == k:
                        Y[self.perm[b]] += (np.clongdouble(coef[b]) / self.phase[b].astype(np.clongdouble))[:, None] * V
                A = self.base[k]
                Ald = A.astype(np.clongdouble)
                x = np.linalg.solve(A, Y.astype(np.complex128)).astype(np.clongdouble)
                for _ in range(3):
                    r = Y - Ald @ x
                    x = x + np.linalg.solve(A, r.astype(np.complex128))
                total += x
            out.append(total.astype(np.complex128))
        return out[0], out[1]


def pdm_family(n, nb):
    return _cached(("pdm", n, nb), lambda: PdmFamily(n, nb, 7000 + n))


def fold_inputs(n, nb):
    """(M, M_old, domega, numpy's tr(M^-1 (M - M_old) / domega)) of nb structured_pair items of order n."""
    def make():
        rng = np.random.default_rng(1000 * n + nb)
        pairs = [structured_pair(rng, n) for _ in range(nb)]
        M, Mo = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
        dw = (0.2 + 0.3 * rng.random(nb)) * np.exp(2j * np.pi * rng.random(nb))
        ref = np.array([np.trace(np.linalg.solve(M[b], (M[b] - Mo[b]) / dw[b])) for b in range(nb)])
        return M, Mo, dw, ref
    return _cached(("fold", n, nb), make)


def near_singular(rng, n, gap):
    """Random complex matrix whose smallest singular value is `gap` times the largest."""
    a = _cplx(rng, n, n)
    u, s, vh = np.linalg.svd(a)
    s[-1] = gap * s[0]
    return (u * s) @ vh


def qr_inputs(n):
    """(A, B): item 0 generic, item 1 near_singular(..., 1e-7), and a random B."""
    def make():
        rng = np.random.default_rng(100 + n)
        A = np.stack([near_singular(rng, n, 1e-7) if b % 2 else _cplx(rng, n, n) for b in range(2)])
        return A, _cplx(rng, 2, n, n)
    return _cached(("qr", n), make)


def contour_inputs(n, nq=4, L=8):
    """(M, z, w, V) of test_contour_moments_match_numpy: M = I + G / sqrt(n), random nodes, weights and probes."""
    def make():
        rng = np.random.default_rng(n)
        M = _cplx(rng, nq, n, n) / np.sqrt(n) + np.eye(n)[None]
        return M, _cplx(rng, nq), _cplx(rng, nq), _cplx(rng, n, L)
    return _cached(("contour", n, nq, L), make)


def moments_of(X, z, w):
    """A0 = sum w_j X_j, A1 = sum w_j z_j X_j of X [nq, n, L] = M_j^-1 V."""
    return np.einsum("j,jil->il", w, X), np.einsum("j,jil->il", w * z, X)


def contour_errors(A0, A1, ld, R0, R1, sgn, lab):
    """(moment 0, moment 1, log|det|, arg det) errors, each divided by its bar (1e-11 relative in norm for the moments,
    1e-10 max(1, |log|det||) and 1e-10 rad for the log-determinant): R0, R1 the reference moments, (sgn, lab) = slogdet."""
    e0 = np.linalg.norm(A0 - R0) / (1e-11 * np.linalg.norm(R0))
    e1 = np.linalg.norm(A1 - R1) / (1e-11 * np.linalg.norm(R1))
    el = (np.abs(ld.real - lab) / (1e-10 * np.maximum(1.0, np.abs(lab)))).max()
    ea = (np.abs(np.angle(np.exp(1j * (ld.imag - np.angle(sgn))))) / 1e-10).max()
    return e0, e1, el, ea


# ---- the halves of the folded step and matrices with a singular half -------------------------------------------------
def fold_halves(X):
    """(S+, S-, u) as k_fold_pass and k_fold_edges read them from the upper triangle of X."""
    n = X.shape[0]
    m = n // 2
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    up = np.triu(X) + np.triu(X, 1).T
    P, Q = up[:m, :m].copy(), up[i, n - 1 - j].copy()
    lo = i > j
    Q[lo] = Q.T[lo]
    u = np.array([up[k, n - 1] - up[0, n - 1 - k] for k in range(n)])
    u[n - 1] = 0.5 * (up[n - 1, n - 1] - up[0, 0])
    return P + Q, P - Q, u


def lu_stop_column(S):
    """Partial-pivot LU as the kernels run it: 0, or the 1-based column whose pivot candidates are all exactly zero."""
    a = np.array(S, dtype=np.complex128)
    n = a.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        if a[p, k] == 0.0:
            return k + 1
        a[[k, p]] = a[[p, k]]
        a[k + 1:, k] /= a[k, k]
        a[k + 1:, k + 1:] -= np.outer(a[k + 1:, k], a[k, k + 1:])
    return 0


def with_singular_half(M, k, odd):
    """A copy of the structured matrix M whose even (odd: odd) half has an exactly zero row and column k, 1 <= k < n / 2:
    the entries X(i, n-1-j) that the fold pairs with X(i, j) are set to -X(i, j) (odd: +X(i, j)) along row and column k
    of the half, in every image that symmetry and centrosymmetry give them.  Negation and copying are exact, so
    S+ = P + Q (S- = P - Q) is zero there bit for bit; k >= 1 keeps the last row and column out of it."""
    X = np.array(M)
    n = X.shape[0]
    m = n // 2
    assert 1 <= k < m
    sign = 1.0 if odd else -1.0
    for t in range(m):
        i, j = min(t, k), max(t, k)  # entry (i, j) of the half, i <= j
        val = sign * X[i, j]
        for r, c in ((i, n - 1 - j), (n - 1 - j, i), (n - 1 - i, j), (j, n - 1 - i)):
            if r != n - 1 and c != n - 1:  # (k >= 1: only images outside the upper wedge touch the last row / column)
                X[r, c] = val
    return X


def singular_k_matrix(n):
    """(M, M_old) of even order n with both halves regular and det K = 0 exactly (info n + 1): M = diag(d) with
    d = (2, 4, 8, 2, 4, 8, ...) mirrored about the centre and the last entry replaced by 0, so C = diag(d) with
    C(n-1, n-1) = C(0, 0) = 2 and the edge u = -e_{n-1}: M = C - 2 e e^T has a zero last row and column.  Both halves
    are diag(d), every solve divides by a power of two, and K = [[1/2, 1/2], [1/2, 1/2]] bit for bit.  M_old is any
    matrix of the structure."""
    m = n // 2
    d = np.array([2.0, 4.0, 8.0] * m)[:m]
    M = np.diag(np.concatenate([d, d[::-1]])).astype(np.complex128)
    M[n - 1, n - 1] = 0.0
    rng = np.random.default_rng(n)
    return M, M + 0.05 * structured(rng, n, 0.0)


def fold_k_matrix(M):
    """K = I + [[e.a, e.b], [u.a, u.b]] of DESIGN.md 5.4c from the halves of M, with the kernels' unnormalised folds."""
    Sp, Sm, u = fold_halves(M)
    n = M.shape[0]
    m = n // 2
    e = np.zeros(n, dtype=complex)
    e[n - 1] = 1.0
    fold = lambda v: (v[:m] + v[::-1][:m], v[:m] - v[::-1][:m])
    (up, um), (ep, em) = fold(u), fold(e)
    ap, am = np.linalg.solve(Sp, up), np.linalg.solve(Sm, um)
    bp, bm = np.linalg.solve(Sp, ep), np.linalg.solve(Sm, em)
    both = lambda xp, xm, yp, ym: 0.5 * (xp @ yp + xm @ ym)
    return np.array([[1 + both(ep, em, ap, am), both(ep, em, bp, bm)],
                     [both(up, um, ap, am), 1 + both(up, um, bp, bm)]])
