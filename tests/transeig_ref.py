"""Dense restatement of the trans eigenvectors in plain NumPy
on the n x n matrix, and the two test genomes.

T[i][j] = v(min, max) for valid i, j on different chromosomes (v = count *
w[a] * w[b] in that order, NaN -> 0), 0 elsewhere; the normalisation loop as
the definition words it; E = D T D - M; ``np.linalg.eigh`` sorted by descending
eigenvalue; the sign rule; the two row-compressed tables by ``np.lexsort``.
Nothing here imports the package under test.
"""
import functools

import numpy as np

SIZES_A = (11, 130, 1, 70, 9, 40)     # a 1-bin chromosome, nothing a multiple of 64, rows of more than 64 entries
SIZES_B = tuple(1 + (7 * i) % 3 for i in range(130))   # very short rows; every row's partners span > 100 chromosomes
BIG = 11                              # first bin of A's 130-bin chromosome
INVALID = {"A": [BIG + 0, BIG + 129, BIG + 90, BIG + 91, 3, 142 + 5], "B": [0, 5, 6, 100, 258]}
EMPTY_ROW = {"A": BIG + 40, "B": 40}  # a valid bin with no pixel at all
NO_TRANS = {"A": BIG + 60, "B": 77}   # a valid bin with cis pixels only: the normalisation must drop it
EMPTY_BLOCKS = {"A": [(0, 4), (2, 4)], "B": [(3, 9)]}   # chromosome pairs with no stored pixel


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def planted(n):
    x = np.arange(n)
    s = np.sign(np.sin(0.9 * x + 0.3))
    t = np.sign(np.cos(0.37 * x))
    return s, t


@functools.lru_cache(maxsize=None)
def genome(name, junk_seed=0):
    """(off, bin1, bin2, count): the sorted upper-triangle table.  Trans
    counts are Poisson around 40 (1 + 0.5 s_i s_j + 0.2 t_i t_j) cov_i cov_j,
    70 % of the trans cells stored; every cis cell holds Poisson(300) junk from
    ``junk_seed`` (it must not reach any output)."""
    sizes = SIZES_A if name == "A" else SIZES_B
    off = offsets(sizes)
    n = int(off[-1])
    rng = np.random.default_rng(31 if name == "A" else 32)
    chrom = np.repeat(np.arange(len(sizes)), sizes)
    s, t = planted(n)
    cov = rng.uniform(0.5, 2.0, n)
    lam = 40.0 * (1 + 0.5 * np.outer(s, s) + 0.2 * np.outer(t, t)) * np.outer(cov, cov)
    H = rng.poisson(lam).astype(np.float64)
    cis = chrom[:, None] == chrom[None, :]
    stored = (rng.random((n, n)) < 0.7) & ~cis
    for p, q in EMPTY_BLOCKS[name]:
        stored[np.ix_(chrom == p, chrom == q)] = False
    for x in (EMPTY_ROW[name], NO_TRANS[name]):
        stored[x, :] = False
        stored[:, x] = False
    junk = np.random.default_rng(1000 + junk_seed).poisson(300.0, (n, n)).astype(np.float64)
    H = np.where(cis, junk, H)
    stored |= cis
    stored[EMPTY_ROW[name], :] = False
    stored[:, EMPTY_ROW[name]] = False
    stored = np.triu(stored)
    b1, b2 = np.nonzero(stored)
    cnt = H[b1, b2]
    tr = np.nonzero(chrom[b1] != chrom[b2])[0]
    cnt[tr[::97]] = 0.0                     # a stored count of 0 is a pixel
    for a in (off, b1, b2, cnt):
        a.setflags(write=False)
    return off, b1.astype(np.int64), b2.astype(np.int64), cnt


def weights(name, kind):
    """(weight, bad, use).  The invalid bins come through NaN weights ('nan')
    or through bad ('bad'); '..._nouse' switches chromosome 3 off; 'exact_...'
    gives powers of two, 'general_...' uniform (0.05, 3), otherwise ones."""
    off = genome(name)[0]
    n = int(off[-1])
    rng = np.random.default_rng(5)
    if kind.startswith("exact"):
        w = 2.0 ** rng.integers(-3, 1, n)
    elif kind.startswith("general"):
        w = rng.uniform(0.05, 3.0, n)
    else:
        w = np.ones(n)
    bad = None
    if "nan" in kind:
        w[INVALID[name]] = np.nan
    else:
        bad = np.zeros(n, np.uint8)
        bad[INVALID[name]] = 1
    use = None
    if kind.endswith("nouse"):
        use = np.ones(len(off) - 1, np.uint8)
        use[3] = 0
    return w, bad, use


def chrom_of(off):
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def validity(off, weight=None, use=None, bad=None):
    n = int(off[-1])
    v = np.ones(n, bool)
    if use is not None:
        v &= np.asarray(use)[chrom_of(off)] != 0
    if weight is not None:
        v &= np.isfinite(weight[:n])
    if bad is not None:
        v &= np.asarray(bad) == 0
    return v


def pixel_values(b1, b2, cnt, weight):
    v = np.asarray(cnt, dtype=np.float64).copy()
    if weight is not None:
        with np.errstate(invalid="ignore"):
            v = v * weight[b1] * weight[b2]
        v[np.isnan(v)] = 0.0
    return v


def kept(b1, b2, off, valid):
    ch = chrom_of(off)
    return valid[b1] & valid[b2] & (ch[b1] != ch[b2])


def dense_T(b1, b2, cnt, weight, off, valid):
    n = int(off[-1])
    k = kept(b1, b2, off, valid)
    T = np.zeros((n, n))
    v = pixel_values(b1, b2, cnt, weight)
    T[b1[k], b2[k]] = v[k]
    T[b2[k], b1[k]] = v[k]
    return T


def tables(b1, b2, cnt, weight, off, valid):
    """{'upper': (rowptr, partner, value), 'lower': ...} by np.lexsort."""
    n = int(off[-1])
    k = kept(b1, b2, off, valid)
    a, b, v = b1[k], b2[k], pixel_values(b1, b2, cnt, weight)[k]
    out = {}
    for name, row, par in (("upper", a, b), ("lower", b, a)):
        o = np.lexsort((par, row))
        rp = np.searchsorted(row[o], np.arange(n + 1)).astype(np.int64)
        out[name] = (rp, par[o].astype(np.int32), v[o])
    return out


def partners(off, valid):
    per = np.add.reduceat(valid.astype(np.int64), off[:-1])
    return np.where(valid, per.sum() - per[chrom_of(off)], 0)


def normalise(T, off, valid, tol=1e-6, max_iter=500):
    """The definition's loop on the dense T: (d, valid_now, ntp, iterations,
    deviation, converged)."""
    valid = valid.copy()
    d = valid.astype(np.float64)
    ntp = partners(off, valid)
    it, dev, conv = 0, np.nan, False
    while valid.any() and it < max_iter:
        s = d * (T @ d)
        dead = valid & (s == 0)
        if dead.any():
            valid &= ~dead
            d[dead] = 0.0
            ntp = partners(off, valid)
            continue
        it += 1
        r = s[valid] / ntp[valid]
        dev = float(np.abs(r - 1).max())
        if dev < tol:
            conv = True
            break
        d[valid] /= np.sqrt(r)
    return d, valid, ntp, it, dev, conv


def mask_matrix(off, valid):
    ch = chrom_of(off)
    return (np.outer(valid, valid) & (ch[:, None] != ch[None, :])).astype(np.float64)


def operator(T, d, off, valid):
    return T * np.outer(d, d) - mask_matrix(off, valid)     # (d_i d_j = d_j d_i: symmetric to the bit)


def eigh_desc(E, valid):
    """(values, vectors[n, nv]) of E on the valid bins, descending; the
    vectors are 0 on the other bins."""
    idx = np.nonzero(valid)[0]
    lam, V = np.linalg.eigh(E[np.ix_(idx, idx)])
    out = np.zeros((E.shape[0], idx.size))
    out[idx] = V[:, ::-1]
    return lam[::-1], out


def pearson(x, y, ok):
    ok = ok & np.isfinite(x) & np.isfinite(y)
    return float(np.corrcoef(x[ok], y[ok])[0, 1])


def sign_of(x, valid, phasing=None):
    """+1 / -1: what the vector must be multiplied by."""
    if phasing is not None:
        r = pearson(x, phasing, valid)
        if np.isfinite(r) and r != 0:
            return 1.0 if r > 0 else -1.0
    mag = np.where(valid & np.isfinite(x), np.abs(x), -1.0)
    return 1.0 if x[int(np.argmax(mag))] >= 0 else -1.0


@functools.lru_cache(maxsize=None)
def solved(name, kind, tol=1e-9):
    """The whole restatement for one genome and weight kind:
    dict(off, valid0, T, d, valid, ntp, iterations, deviation, E, values, vectors)."""
    off, b1, b2, cnt = genome(name)
    w, bad, use = weights(name, kind)
    valid0 = validity(off, w, use, bad)
    T = dense_T(b1, b2, cnt, w, off, valid0)
    d, valid, ntp, it, dev, conv = normalise(T, off, valid0, tol)
    E = operator(T, d, off, valid)
    lam, V = eigh_desc(E, valid)
    return dict(off=off, valid0=valid0, T=T, d=d, valid=valid, ntp=ntp, iterations=it, deviation=dev, converged=conv,
                E=E, values=lam, vectors=V)
