"""The folded secant eigenpair step of DESIGN.md §14.2 in numpy, from the wedge and the last column alone: shared by
test_eigpair_fold_host.py and test_gpu_eigpair_fold.py.  Notation of §5.4c: n = 2m, e = e_{n-1}, J the flip, folds
unnormalised (x+- = x1 +- J x2), so every form of two folds is twice the form of the vectors."""
import numpy as np


def fold(x):
    m = x.shape[0] // 2
    return x[:m] + x[::-1][:m], x[:m] - x[::-1][:m]


def unfold(xp, xm):
    return np.concatenate([0.5 * (xp + xm), (0.5 * (xp - xm))[::-1]])


def parts(X):
    """S+, S-, u of one matrix: only the wedge i <= j <= n-1-i of the upper triangle and the last column are read."""
    n = X.shape[0]
    m = n // 2
    assert n == 2 * m
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    up = np.triu(X) + np.triu(X, 1).T
    P, Q = up[:m, :m].copy(), up[i, n - 1 - j].copy()
    lo = i > j
    Q[lo] = Q.T[lo]
    u = np.array([up[k, n - 1] - up[0, n - 1 - k] for k in range(n)])
    u[n - 1] = 0.5 * (up[n - 1, n - 1] - up[0, 0])
    return P + Q, P - Q, u


def direct_step(M, M_old, dw, v):
    """The unfolded step: (u / |u|, tau, |M v| / |M|_F) by numpy's solve on the whole matrices."""
    uh = np.linalg.solve(M, (M - M_old) @ v / dw)
    return uh / np.linalg.norm(uh), np.vdot(v, uh), np.linalg.norm(M @ v) / np.linalg.norm(M), uh


def folded_step(M, M_old, dw, v, rank2=True):
    """(u / |u|, tau, resid, u, parity of v) of one chain; rank2 = False takes u = u' = 0 (the last-column rule left
    out)."""
    n = M.shape[0]
    m = n // 2
    Sp, Sm, u = parts(M)
    Spo, Smo, uo = parts(M_old)
    Dp, Dm, ud = (Sp - Spo) / dw, (Sm - Smo) / dw, (u - uo) / dw
    if not rank2:
        u, ud = np.zeros_like(u), np.zeros_like(ud)
    e = np.zeros(n, dtype=complex)
    e[n - 1] = 1.0
    halves = []
    for S, D, us, uds, es, vs in zip((Sp, Sm), (Dp, Dm), fold(u), fold(ud), fold(e), fold(v)):
        halves.append(dict(y=S @ vs, c=np.linalg.solve(S, D @ vs), a=np.linalg.solve(S, us), ap=np.linalg.solve(S, uds),
                           b=np.linalg.solve(S, es), u=us, ud=uds, e=es, v=vs, fro=np.linalg.norm(S) ** 2))

    def both(p, q):  # bilinear form of two folded vectors
        return 0.5 * sum(h[p] @ h[q] for h in halves)

    vlast, upv, uv = v[n - 1], both("ud", "v"), both("u", "v")
    for h in halves:
        h["x"] = h["c"] + vlast * h["ap"] + upv * h["b"]
    K = np.eye(2) + np.array([[both("e", "a"), both("e", "b")], [both("u", "a"), both("u", "b")]])
    g1, g2 = np.linalg.solve(K, np.array([both("e", "x"), both("u", "x")]))
    for h in halves:
        h["uh"] = h["x"] - g1 * h["a"] - g2 * h["b"]
        h["mv"] = h["y"] + vlast * h["u"] + uv * h["e"]
    tau = 0.5 * sum(np.vdot(h["v"], h["uh"]) for h in halves)
    nrm = np.sqrt(0.5 * sum(np.linalg.norm(h["uh"]) ** 2 for h in halves))
    mv = np.sqrt(0.5 * sum(np.linalg.norm(h["mv"]) ** 2 for h in halves))
    up = np.triu(M)
    fro2 = (halves[0]["fro"] + halves[1]["fro"]
            + 2.0 * sum(abs(up[i, n - 1]) ** 2 - abs(up[0, n - 1 - i]) ** 2 for i in range(1, n - 1))
            + abs(up[n - 1, n - 1]) ** 2 - abs(up[0, 0]) ** 2)
    if not rank2:
        fro2 = halves[0]["fro"] + halves[1]["fro"]
    uh = unfold(halves[0]["uh"], halves[1]["uh"])
    parity = 0.5 * np.linalg.norm(halves[0]["v"]) ** 2 / np.linalg.norm(v) ** 2
    return uh / nrm, tau, mv / np.sqrt(fro2), uh, parity


def parity(v):
    """|v1 + J v2|^2 / (2 |v|^2); for odd n the middle entry counts as even."""
    v = np.asarray(v, dtype=complex)
    n = v.shape[0]
    k = n // 2
    ev = np.linalg.norm(v[:k] + v[::-1][:k]) ** 2 + (2.0 * abs(v[k]) ** 2 if n % 2 else 0.0)
    return ev / (2.0 * np.linalg.norm(v) ** 2)
