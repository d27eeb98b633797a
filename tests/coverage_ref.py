"""Dense restatement of the per-bin coverage and the virtual 4C (DESIGN.md
§4v) in plain NumPy on the n x n matrix.

A[i][j] = v(min, max) for valid i, j with a stored pixel (v = count * w[a] *
w[b] in that order, NaN -> 0), 0 elsewhere; a diagonal pixel is one cell and
enters its row once.  With d = |i - j| a cell is trans (different
chromosomes), dropped (cis, d < ignore_diags), near (cis, ignore_diags <= d <
near_bins) or far (cis, d >= max(near_bins, ignore_diags)).  S / n are the row
sums per class, P the sum of the rows of a viewpoint without the dropped
cells; the lower table comes from ``np.lexsort``.  The genomes, weights and
validity are tests/transeig_ref.py's.  Nothing here imports the package under
test.
"""
import functools

import numpy as np

from tests.transeig_ref import chrom_of, genome, offsets, pixel_values, validity, weights  # noqa: F401

CLASSES = ("near", "far", "trans")


def in_table(b1, b2, n):
    """The pixels a row of A can hold: both ids in range and bin1 <= bin2."""
    return (b1 >= 0) & (b1 < n) & (b2 >= 0) & (b2 < n) & (b1 <= b2)


def dense_A(b1, b2, cnt, weight, off, valid):
    """(A, stored): the symmetric matrix and the cells with a stored pixel
    between two valid bins."""
    n = int(off[-1])
    k = in_table(b1, b2, n)
    a, b = b1[k], b2[k]
    v = pixel_values(a, b, np.asarray(cnt)[k], weight)
    ok = valid[a] & valid[b]
    a, b, v = a[ok], b[ok], v[ok]
    A, stored = np.zeros((n, n)), np.zeros((n, n), bool)
    A[a, b] = v
    A[b, a] = v
    stored[a, b] = True
    stored[b, a] = True
    return A, stored


def class_masks(off, ignore_diags, near_bins):
    """{'near', 'far', 'trans', 'dropped'}: n x n bool, a partition of the cells."""
    n = int(off[-1])
    ch = chrom_of(off)
    cis = ch[:, None] == ch[None, :]
    d = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
    dropped = cis & (d < ignore_diags)
    near = cis & ~dropped & (d < near_bins)
    far = cis & ~dropped & ~near
    return dict(near=near, far=far, trans=~cis, dropped=dropped)


def coverage(A, stored, off, valid, ignore_diags, near_bins):
    """(S float64[n, 3], n int64[n, 3]) in the order near, far, trans; an
    invalid row is 0 (A and stored are empty there)."""
    M = class_masks(off, ignore_diags, near_bins)
    S = np.stack([(A * M[k]).sum(axis=1) for k in CLASSES], axis=1)
    cnt = np.stack([(stored & M[k]).sum(axis=1) for k in CLASSES], axis=1).astype(np.int64)
    return S, cnt


def abs_terms(A, off, ignore_diags, near_bins):
    """sum_j |A[x][j]| per class: the scale of the rounding bound."""
    M = class_masks(off, ignore_diags, near_bins)
    return np.stack([(np.abs(A) * M[k]).sum(axis=1) for k in CLASSES], axis=1)


def viewpoint(A, off, ignore_diags, lo, hi):
    """P[y] = sum over x in [lo, hi) of A[x][y] without the dropped cells."""
    keep = ~class_masks(off, ignore_diags, 0)["dropped"]
    return (A * keep)[lo:hi].sum(axis=0)


def tracks(S, valid):
    """cov_cis, cov_tot, ICF, DLR as the definition words them."""
    n = S.shape[0]
    cis = S[:, 0] + S[:, 1]
    tot = cis + S[:, 2]
    icf, dlr = np.full(n, np.nan), np.full(n, np.nan)
    ok = np.asarray(valid, bool)
    a, b = ok & (tot != 0), ok & (S[:, 0] != 0)
    icf[a] = S[a, 2] / tot[a]
    with np.errstate(divide="ignore"):
        dlr[b] = np.log2(S[b, 1] / S[b, 0])
    return dict(cov_cis=cis, cov_tot=tot, ICF=icf, DLR=dlr)


def sym_tables(b1, b2, n):
    """dict(rowptr_u, rowptr_l, partner_l, src_l) by np.searchsorted / np.lexsort:
    the lower table holds the pixels with bin1 < bin2 and both ids in range,
    sorted by (bin2, bin1)."""
    rpu = np.searchsorted(b1, np.arange(n + 1)).astype(np.int64)
    idx = np.nonzero(in_table(b1, b2, n) & (b1 < b2))[0]
    o = np.lexsort((b1[idx], b2[idx]))
    idx = idx[o]
    rpl = np.searchsorted(b2[idx], np.arange(n + 1)).astype(np.int64)
    return dict(rowptr_u=rpu, rowptr_l=rpl, partner_l=b1[idx].astype(np.int32), src_l=idx.astype(np.uint32))


@functools.lru_cache(maxsize=None)
def degenerate(kind):
    """(off, bin1, bin2, count) of the tables the two genomes lack: 'empty'
    (nnz = 0), 'one_chrom' (C = 1), 'no_diag' (no diagonal pixel), 'all_diag'
    (every pixel diagonal) and 'malformed' (ids out of range on either side and
    pixels with bin1 > bin2, still sorted by bin1)."""
    off, b1, b2, cnt = genome("A")
    n = int(off[-1])
    if kind == "empty":
        return off, b1[:0], b2[:0], cnt[:0]
    if kind == "one_chrom":
        return np.array([0, n], np.int64), b1, b2, cnt
    if kind == "no_diag":
        k = b1 != b2
        return off, b1[k], b2[k], cnt[k]
    if kind == "all_diag":
        k = b1 == b2
        return off, b1[k], b2[k], cnt[k]
    if kind == "malformed":
        a, b = b1.copy(), b2.copy()
        b[5::37] = n + 3                       # bin2 past the end
        b[7::41] = -2                          # negative
        b[11::43] = 2 ** 40
        sw = np.arange(13, a.size, 29)         # bin1 > bin2: the row stays, the partner lies below it
        b[sw] = a[sw] // 2 - 1
        a[-3:] = [n, n + 1, 2 ** 35]           # bin1 past the end, still ascending
        return off, a, b, cnt
    raise KeyError(kind)


PLANTED = (50, 37, 64, 21)


@functools.lru_cache(maxsize=None)
def planted():
    """Four chromosomes for run_Coverage / run_Virtual4C: cis counts decay
    with the distance inside a band of 30 bins, 40 % of the trans cells are
    stored with counts 1..8, three bins are empty.  Returns (off, bin1, bin2,
    count int64)."""
    rng = np.random.default_rng(17)
    off = offsets(PLANTED)
    n = int(off[-1])
    ch = chrom_of(off)
    a, b = np.nonzero(np.triu(np.ones((n, n), bool)))
    cis = ch[a] == ch[b]
    keep = np.where(cis, b - a < 30, rng.random(a.size) < 0.4)
    for x in (7, 60, 150):
        keep &= (a != x) & (b != x)
    a, b, cis = a[keep], b[keep], cis[keep]
    count = np.where(cis, 200 // (b - a + 1) + rng.integers(0, 5, a.size), rng.integers(1, 9, a.size)).astype(np.int64)
    return off, a.astype(np.int64), b.astype(np.int64), count
