"""Dense restatement of the trans block sums, the trans expected, the cis /
trans totals and the trans saddle: the definitions as plain
loops over the cells of the n_bins x n_bins upper matrix.  It shares no code
with ``hichap_master_amd.trans``; the tests pin the GPU sums and the host
rules to it."""
import math

import numpy as np


def chrom_of(off):
    """c(x) for every global bin."""
    out = []
    for q in range(len(off) - 1):
        out += [q] * int(off[q + 1] - off[q])
    return out


def validity(off, weight, use, bad):
    c = chrom_of(off)
    v = []
    for x in range(int(off[-1])):
        ok = use is None or bool(use[c[x]])
        if ok and weight is not None and not math.isfinite(float(weight[x])):
            ok = False
        if ok and bad is not None and bad[x]:
            ok = False
        v.append(ok)
    return v


def dense_upper(b1, b2, count, weight, n_bins):
    """(M, stored): the upper matrix of ``count * w[bin1] * w[bin2]`` in that
    order (NaN -> 0, raw counts with weight None) and which cells are stored
    pixels."""
    M = [[0.0] * n_bins for _ in range(n_bins)]
    stored = [[False] * n_bins for _ in range(n_bins)]
    for a, b, c in zip(np.asarray(b1).tolist(), np.asarray(b2).tolist(), np.asarray(count, float).tolist()):
        v = c
        if weight is not None:
            v = (c * float(weight[a])) * float(weight[b])
            if v != v:
                v = 0.0
        M[a][b] = v
        stored[a][b] = True
    return M, stored


def block_sums(M, stored, off, valid, g):
    """sum, npix (C x C) over the stored cells a <= b with both bins valid;
    the cis cells take b - a >= g; below the diagonal both are 0.  The number
    of terms per block is npix."""
    C = len(off) - 1
    c = chrom_of(off)
    s = [[0.0] * C for _ in range(C)]
    n = [[0] * C for _ in range(C)]
    for a in range(int(off[-1])):
        if not valid[a]:
            continue
        for b in range(a, int(off[-1])):
            if not stored[a][b] or not valid[b]:
                continue
            if c[a] == c[b] and b - a < g:
                continue
            s[c[a]][c[b]] += M[a][b]
            n[c[a]][c[b]] += 1
    return np.array(s), np.array(n, dtype=np.int64)


def n_valid(off, valid):
    return [sum(1 for x in range(int(off[q]), int(off[q + 1])) if valid[x]) for q in range(len(off) - 1)]


def expected(s, nvb):
    C = len(nvb)
    return np.array([[s[p][q] / float(nvb[p] * nvb[q]) if p < q and nvb[p] * nvb[q] > 0 else math.nan
                      for q in range(C)] for p in range(C)])


def usable(e):
    C = len(e)
    return [[q > p and math.isfinite(float(e[p][q])) and float(e[p][q]) > 0 for q in range(C)] for p in range(C)]


def saddle_sums(M, stored, off, valid, e, cls, K):
    """U, Cu, Un (C x K x K): per row chromosome p, over every cell (a in p, b
    in q) of the usable blocks q > p with both bins valid and both classes !=
    255: Cu counts the cell, U adds M[a][b] / e[p][q] where it is stored and Un
    counts those terms."""
    C = len(off) - 1
    c = chrom_of(off)
    us = usable(e)
    U = [[[0.0] * K for _ in range(K)] for _ in range(C)]
    Cu = [[[0] * K for _ in range(K)] for _ in range(C)]
    Un = [[[0] * K for _ in range(K)] for _ in range(C)]
    for a in range(int(off[-1])):
        if not valid[a] or cls[a] == 255:
            continue
        for b in range(a + 1, int(off[-1])):
            p, q = c[a], c[b]
            if not us[p][q] or not valid[b] or cls[b] == 255:
                continue
            Cu[p][int(cls[a])][int(cls[b])] += 1
            if stored[a][b]:
                U[p][int(cls[a])][int(cls[b])] += M[a][b] / float(e[p][q])
                Un[p][int(cls[a])][int(cls[b])] += 1
    return np.array(U), np.array(Cu, dtype=np.int64), np.array(Un, dtype=np.int64)


def totals(s):
    """cis[p], trans[p], fraction[p] and the genome's (cis, trans, fraction)."""
    C = len(s)
    cis, trans, frac = [], [], []
    for p in range(C):
        t = 0.0
        for q in range(C):
            if q != p:
                t += float(s[min(p, q)][max(p, q)])
        cis.append(float(s[p][p]))
        trans.append(t)
        frac.append(cis[p] / (cis[p] + t) if cis[p] + t != 0 else math.nan)
    gc = 0.0
    for p in range(C):
        gc += float(s[p][p])
    gt = 0.0
    for p in range(C):
        for q in range(p + 1, C):
            gt += float(s[p][q])
    return cis, trans, frac, (gc, gt, gc / (gc + gt) if gc + gt != 0 else math.nan)


def symmetric(U, Cu):
    """S, C over the chromosomes in file order and the saddle S / C."""
    K = U.shape[1]
    S, Cn = np.zeros((K, K)), np.zeros((K, K), np.int64)
    for p in range(len(U)):
        S += U[p] + U[p].T
        Cn += Cu[p] + Cu[p].T
    sad = np.array([[S[i, j] / Cn[i, j] if Cn[i, j] else math.nan for j in range(K)] for i in range(K)])
    return S, Cn, sad
