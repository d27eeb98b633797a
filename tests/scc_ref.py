"""Dense restatement of the stratum-adjusted correlation: the
definition as written, with plain loops over the cells of the two N x N
matrices, box sums by direct loops over the window, ``math.fsum`` for the five
moments and the two-pass formula (means first) for rho.  It shares no code
with the package."""
import math

import numpy as np


def dense(bin1, bin2, count, weight, lo, N):
    """The symmetric N x N list of lists of ``(count * w[bin1]) * w[bin2]``
    (NaN -> 0; the raw count without weights) of the pixels with both ends in
    global bins [lo, lo + N)."""
    M = [[0.0] * N for _ in range(N)]
    for i, j, c in zip(bin1.tolist(), bin2.tolist(), count.tolist()):
        if not (lo <= i < lo + N and lo <= j < lo + N):
            continue
        v = float(c)
        if weight is not None:
            v = (v * float(weight[i])) * float(weight[j])
            if v != v:
                v = 0.0
        M[i - lo][j - lo] = v
        M[j - lo][i - lo] = v
    return M


def validity(weight, lo, N, bad):
    return [(weight is None or math.isfinite(weight[lo + j])) and (bad is None or not bad[j]) for j in range(N)]


def masked(M, valid, g):
    """x(a, b): 0 at an invalid bin and for |a - b| < g."""
    N = len(M)
    return [[M[a][b] if valid[a] and valid[b] and abs(a - b) >= g else 0.0 for b in range(N)] for a in range(N)]


def box(x, a, b, h):
    """SX(a, b): the window's cells inside [0, N)^2, row by row."""
    N = len(x)
    s = 0.0
    for p in range(max(0, a - h), min(N, a + h + 1)):
        s += sum(x[p][max(0, b - h):min(N, b + h + 1)])
    return s


def smoothed(MA, MB, valid, h, g, D):
    """Per stratum d = 0 .. D the lists of X and of Y over the kept cells."""
    N = len(MA)
    x, y = masked(MA, valid, g), masked(MB, valid, g)
    nv = [sum(1 for p in range(max(0, a - h), min(N, a + h + 1)) if valid[p]) for a in range(N)]
    out = []
    for d in range(D + 1):
        X, Y = [], []
        if d >= g:
            for a in range(N - d):
                b = a + d
                if not (valid[a] and valid[b]):
                    continue
                sx, sy = box(x, a, b, h), box(y, a, b, h)
                if sx == 0 and sy == 0:
                    continue
                X.append(sx / (nv[a] * nv[b]))
                Y.append(sy / (nv[a] * nv[b]))
        out.append((X, Y))
    return out


def moments(strata):
    """``(n, S, T)``: the counts, the five sums Sx, Sy, Sxx, Syy, Sxy by
    ``math.fsum`` and the sums of the terms' absolute values."""
    D1 = len(strata)
    n = np.zeros(D1, np.int64)
    S, T = np.zeros((5, D1)), np.zeros((5, D1))
    for d, (X, Y) in enumerate(strata):
        n[d] = len(X)
        terms = (X, Y, [u * u for u in X], [v * v for v in Y], [u * v for u, v in zip(X, Y)])
        for k, t in enumerate(terms):
            S[k, d] = math.fsum(t)
            T[k, d] = math.fsum(abs(u) for u in t)
    return n, S, T


def correlations(strata):
    """Two-pass: ``(rho, weight, usable, cond)`` per stratum, ``cond`` the
    larger of ``n Sxx / vx`` and ``n Syy / vy`` (the conditioning of the
    one-pass formula), NaN / 0 / False / NaN where the stratum is not usable
    (n < 3 or a zero variance)."""
    D1 = len(strata)
    rho, weight, cond = np.full(D1, np.nan), np.zeros(D1), np.full(D1, np.nan)
    usable = np.zeros(D1, bool)
    for d, (X, Y) in enumerate(strata):
        m = len(X)
        if m < 3:
            continue
        mx, my = math.fsum(X) / m, math.fsum(Y) / m
        dx, dy = [u - mx for u in X], [v - my for v in Y]
        vx, vy = math.fsum(u * u for u in dx), math.fsum(v * v for v in dy)
        if not (vx > 0 and vy > 0):
            continue
        usable[d] = True
        rho[d] = math.fsum(u * v for u, v in zip(dx, dy)) / math.sqrt(vx * vy)
        weight[d] = (m + 1) / 12.0
        cond[d] = max(math.fsum(u * u for u in X) / vx, math.fsum(v * v for v in Y) / vy)
    return rho, weight, usable, cond


def scc(rhos, weights, usables):
    """The weighted mean over the usable strata of every chromosome given."""
    num = math.fsum(w * r for rho, wt, us in zip(rhos, weights, usables) for r, w, u in zip(rho, wt, us) if u)
    den = math.fsum(w for wt, us in zip(weights, usables) for w, u in zip(wt, us) if u)
    return num / den if den > 0 else float("nan")


def generator(seed, N=300, block=25):
    """The intensity of the end-to-end tests: ``lambda = 400 (d + 1)^-1.08 (1 +
    0.3 s_i s_j) v_i v_j`` with compartment blocks of ``block`` bins (s = +-1)
    and ``v ~ LogNormal(0, 0.3)``."""
    rng = np.random.default_rng(seed)
    s = np.repeat(rng.choice([-1.0, 1.0], (N + block - 1) // block), block)[:N]
    v = rng.lognormal(0.0, 0.3, N)
    i, j = np.indices((N, N))
    return 400.0 * (np.abs(i - j) + 1.0) ** -1.08 * (1 + 0.3 * np.outer(s, s)) * np.outer(v, v)


def draw(lam, depth, seed):
    """One Poisson draw of the upper triangle as a sorted pixel table."""
    H = np.triu(np.random.default_rng(seed).poisson(lam * depth))
    b1, b2 = np.nonzero(H)
    return b1.astype(np.int64), b2.astype(np.int64), H[b1, b2].astype(np.int32)
