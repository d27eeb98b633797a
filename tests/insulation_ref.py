"""Dense NumPy restatement of the insulation score: the
definition's loops over bins and windows on the N x N matrix, and scipy for
the boundaries.  It shares no code with ``hichap_master_amd.insulation``; the
tests pin the GPU sums and the host rules to it."""
import numpy as np
from scipy.signal import find_peaks, peak_prominences


def diamond_sums(M, valid, windows, g, bins=None):
    """S[k][i], n[k][i] over C_w(i) = {(a, b): i - w < a <= i <= b < i + w,
    0 <= a, b < N, b - a >= g} with valid[a] and valid[b]; M dense, NaN
    already 0.  ``bins``: only these i (the others stay 0)."""
    M = np.asarray(M, dtype=np.float64)
    N = M.shape[0]
    valid = np.ones(N, bool) if valid is None else np.asarray(valid) != 0
    S = np.zeros((len(windows), N))
    n = np.zeros((len(windows), N), np.int32)
    for k, w in enumerate(windows):
        for i in (range(N) if bins is None else bins):
            a = np.arange(max(0, i - w + 1), i + 1)
            b = np.arange(i, min(N, i + w))
            cell = (b[None, :] - a[:, None] >= g) & valid[a][:, None] & valid[b][None, :]
            S[k, i] = M[a[0]:i + 1, i:b[-1] + 1][cell].sum()
            n[k, i] = np.count_nonzero(cell)
    return S, n


def full(w, g):
    return sum(1 for s in range(w) for t in range(w) if s + t >= g)


def track(S, n, valid, w, g, min_frac_valid=0.66):
    """log2(score / nanmedian(score)), score = S / n under the three conditions."""
    N = len(S)
    score = np.full(N, np.nan)
    for i in range(N):
        if valid[i] and n[i] > 0 and n[i] >= min_frac_valid * full(w, g):
            score[i] = S[i] / n[i]
    if np.all(np.isnan(score)):
        return score
    with np.errstate(divide="ignore", invalid="ignore"):
        L = np.log2(score / np.nanmedian(score))
    L[~np.isfinite(L)] = np.nan
    return L


def boundaries(L):
    """(index into L, strength) of every strict local minimum of the finite entries."""
    L = np.asarray(L, dtype=np.float64)
    where = np.nonzero(np.isfinite(L))[0]
    x = L[where]
    peaks, _ = find_peaks(-x)
    prom = peak_prominences(-x, peaks)[0]
    return where[peaks], prom


def tables(mats, Res, wbins, g, min_frac_valid=0.66, min_strength=0.1):
    """What run_Insulation writes, as data: {chrom: (L[n_w][N], n[n_w][N])}
    and the boundary list [(chrom, pos, window_bp, strength)].  ``mats``:
    {chrom: (M with NaN -> 0, valid)} in file order."""
    tr, bnd = {}, []
    for chro, (M, valid) in mats.items():
        S, n = diamond_sums(M, valid, wbins, g)
        Ls = []
        for k, w in enumerate(wbins):
            L = track(S[k], n[k], valid, w, g, min_frac_valid)
            Ls.append(L)
            idx, prom = boundaries(L)
            bnd += [(chro, int(i) * Res, w * Res, float(p)) for i, p in zip(idx, prom) if p >= min_strength]
        tr[chro] = (np.array(Ls), n)
    return tr, bnd
