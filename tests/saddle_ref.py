"""Dense restatement of the cis expected and the compartment saddle (DESIGN.md
§4m): the definitions as plain loops over the cells of the N x N matrix.  It
shares no code with ``hichap_master_amd.saddle``; the tests pin the GPU sums
and the host rules to it."""
import math

import numpy as np


def dense(b1, b2, count, weight, lo, N):
    """The chromosome's symmetric matrix as cooler balances it: ``count *
    w[bin1] * w[bin2]`` in that order, NaN -> 0 (raw counts with weight None);
    pixels with an end outside [lo, lo + N) are dropped."""
    M = np.zeros((N, N))
    for p, q, c in zip(np.asarray(b1).tolist(), np.asarray(b2).tolist(), np.asarray(count, float).tolist()):
        if p < lo or q >= lo + N or p >= lo + N or q < lo:
            continue
        v = c
        if weight is not None:
            v = (c * float(weight[p])) * float(weight[q])
            if v != v:
                v = 0.0
        M[p - lo, q - lo] = v
        M[q - lo, p - lo] = v
    return M


def validity(weight, lo, N, bad):
    v = np.ones(N, bool)
    if weight is not None:
        v &= np.isfinite(np.asarray(weight)[lo:lo + N])
    if bad is not None:
        v &= np.asarray(bad) == 0
    return v


def expected_sums(M, valid, g, D):
    """sum[d], nvalid[d] for d = 0..D (0 below g) over the cells (a, a + d) with
    both bins valid.  An unstored cell is 0 in M and adds nothing."""
    N = len(M)
    M = [row.tolist() for row in np.asarray(M, dtype=np.float64)]
    s, n = [0.0] * (D + 1), [0] * (D + 1)
    for d in range(g, D + 1):
        for a in range(N - d):
            if valid[a] and valid[a + d]:
                n[d] += 1
                s[d] += M[a][a + d]
    return np.array(s), np.array(n, dtype=np.int64)


def expected(s, n, g):
    return np.array([s[d] / n[d] if n[d] > 0 and d >= g else math.nan for d in range(len(s))])


def saddle_sums(M, valid, e, cls, K, min_dist, D):
    """U, Cu (K x K) over the cells a < b with min_dist <= b - a <= D on usable
    diagonals (e finite and > 0), both bins valid, both classes != 255."""
    N = len(M)
    M = [row.tolist() for row in np.asarray(M, dtype=np.float64)]
    U = [[0.0] * K for _ in range(K)]
    Cu = [[0] * K for _ in range(K)]
    for a in range(N):
        if not valid[a] or cls[a] == 255:
            continue
        for b in range(a + min_dist, min(N, a + D + 1)):
            x = float(e[b - a])
            if not (math.isfinite(x) and x > 0) or not valid[b] or cls[b] == 255:
                continue
            Cu[cls[a]][cls[b]] += 1
            U[cls[a]][cls[b]] += M[a][b] / x
    return np.array(U), np.array(Cu, dtype=np.int64)


def symmetric(U, Cu):
    """S, C and the saddle S / C (NaN where C = 0)."""
    S, C = U + U.T, Cu + Cu.T
    sad = np.array([[S[i, j] / C[i, j] if C[i, j] else math.nan for j in range(len(S))] for i in range(len(S))])
    return S, C, sad


def digitize(tracks, valids, n_bins, qlo, qhi):
    """tracks / valids: lists in file order.  Returns ([cls], edges)."""
    x = [v for t in tracks for v in np.asarray(t, float).tolist() if math.isfinite(v) and v != 0]
    edges = np.quantile(np.array(x), np.linspace(qlo, qhi, n_bins + 1))
    out = []
    for t, ok in zip(tracks, valids):
        c = []
        for i, v in enumerate(np.asarray(t, float).tolist()):
            if not math.isfinite(v) or v == 0 or not ok[i]:
                c.append(255)
            else:
                c.append(sum(1 for e in edges.tolist() if e <= v))   # searchsorted(edges, v, 'right')
        out.append(np.array(c, dtype=np.uint8))
    return out, edges


def strength(S, C):
    """[intra(k) / inter(k) for k = 1 .. n // 2] on the interior of S, C."""
    Si, Ci = np.asarray(S, float)[1:-1, 1:-1], np.asarray(C, float)[1:-1, 1:-1]
    n = len(Si)
    out = []
    for k in range(1, n // 2 + 1):
        lo, hi = range(k), range(n - k, n)

        def tot(A, rows, cols):
            return sum(A[i, j] for i in rows for j in cols)

        with np.errstate(divide="ignore", invalid="ignore"):
            intra = np.float64(tot(Si, lo, lo) + tot(Si, hi, hi)) / np.float64(tot(Ci, lo, lo) + tot(Ci, hi, hi))
            inter = np.float64(tot(Si, lo, hi) + tot(Si, hi, lo)) / np.float64(tot(Ci, lo, hi) + tot(Ci, hi, lo))
            out.append(intra / inter)
    return np.array(out)


def planted(seed=7, N=240):
    """The planted compartment chromosome of the end-to-end tests: blocks of
    12-30 bins with alternating signs s, counts floor(4000 / (d + 1) * (1 +
    0.5 s_a s_b)) on the whole upper triangle, weights in [0.5, 2) with five
    NaN, track s * (1 + u), u uniform in [0, 1).  The ideal AA BB / AB^2
    contrast is 3.  Returns (bin1, bin2, count, weight, track), local bins."""
    rng = np.random.default_rng(seed)
    s = np.empty(N)
    at, sign = 0, 1.0
    while at < N:
        L = int(rng.integers(12, 31))
        s[at:at + L] = sign
        at, sign = at + L, -sign
    a, b = np.nonzero(np.triu(np.ones((N, N))))
    count = np.floor(4000.0 / (b - a + 1) * (1 + 0.5 * s[a] * s[b])).astype(np.int64)
    weight = rng.uniform(0.5, 2.0, N)
    weight[rng.choice(N, 5, replace=False)] = np.nan
    track = s * (1 + rng.random(N))
    return a.astype(np.int64), b.astype(np.int64), count, weight, track
