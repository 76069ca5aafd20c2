"""The folded trace-secant formula of DESIGN.md §5.4c in numpy, and random matrices of the structure it is for: shared
by test_fold_host.py and test_gpu_fold.py."""
import numpy as np


def folded_trace(M, M_old, dw, rank2=True):
    """tr(M^-1 (M - M_old) / dw) for symmetric M, M_old that are centrosymmetric apart from their last row and column,
    from the upper triangles alone: the even and the odd block of order n / 2 and the rank-2 correction of the last row
    and column (rank2 = False leaves that correction out)."""
    n = M.shape[0]
    m = n // 2
    assert n == 2 * m
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")

    def parts(X):
        up = np.triu(X) + np.triu(X, 1).T  # only the upper triangle is looked at
        P, Q = up[:m, :m].copy(), up[i, n - 1 - j].copy()
        lo = i > j  # entry (i, j) below the diagonal: the one at (j, i)
        Q[lo] = Q.T[lo]
        u = np.array([up[k, n - 1] - up[0, n - 1 - k] for k in range(n)])
        u[n - 1] = 0.5 * (up[n - 1, n - 1] - up[0, 0])
        return P + Q, P - Q, u

    Sp, Sm, u = parts(M)
    Spo, Smo, uo = parts(M_old)
    Dp, Dm, ud = (Sp - Spo) / dw, (Sm - Smo) / dw, (u - uo) / dw
    tr = np.trace(np.linalg.solve(Sp, Dp)) + np.trace(np.linalg.solve(Sm, Dm))
    if not rank2:
        return tr

    def fold(v):  # unnormalised: every bilinear form of two folds is twice the form of the vectors
        return v[:m] + v[::-1][:m], v[:m] - v[::-1][:m]

    e = np.zeros(n, dtype=complex)
    e[n - 1] = 1.0
    (up_, um_), (ep, em), (dp, dm) = fold(u), fold(e), fold(ud)
    ap, am = np.linalg.solve(Sp, up_), np.linalg.solve(Sm, um_)
    bp, bm = np.linalg.solve(Sp, ep), np.linalg.solve(Sm, em)

    def both(xp, xm, yp, ym):
        return 0.5 * (xp @ yp + xm @ ym)

    ea, eb = both(ep, em, ap, am), both(ep, em, bp, bm)
    ua, ub = both(up_, um_, ap, am), both(up_, um_, bp, bm)
    au, bu = both(dp, dm, ap, am), both(dp, dm, bp, bm)
    fba = 0.5 * (bp @ Dp @ ap + bm @ Dm @ am)
    faa = 0.5 * (ap @ Dp @ ap + am @ Dm @ am)
    fbb = 0.5 * (bp @ Dp @ bp + bm @ Dm @ bm)
    g11 = fba + bu * ea + eb * au
    g12 = fbb + 2 * bu * eb
    g21 = faa + 2 * au * ea
    K = np.array([[1 + ea, eb], [ua, 1 + ub]])
    G = np.array([[g11, g12], [g21, g11]])
    return tr + 2 * bu - np.trace(np.linalg.solve(K, G))


def structured(rng, n, shift):
    """A random complex symmetric matrix of order n, centrosymmetric apart from its last row and column, its diagonal
    raised by `shift`."""
    A = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    A = A + A.T
    A = A + A[::-1, ::-1]  # C: symmetric and centrosymmetric
    A = A + shift * np.eye(n)
    u = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    A[:, n - 1] += u
    A[n - 1, :] += u
    return A


def structured_pair(rng, n, cond_max=1e3):
    """(M, M_old) of that structure with cond(M) <= cond_max: the diagonal is raised until it is."""
    shift = 2.0 * np.sqrt(n)
    while True:
        M = structured(rng, n, shift)
        if np.linalg.cond(M) <= cond_max:
            break
        shift *= 2.0
    M_old = M + 0.05 * structured(rng, n, 0.0)
    return M, M_old
