"""NumPy restatement of cooler's ``coarsen`` on cooler's pixel table: the check
of hichap_master_amd/coarsen.py and csrc/coarsen.hip.  It does
not use the package: the bin map is built here from its definition."""
import numpy as np


def ref_offsets(chrom_offsets, k):
    off = np.asarray(chrom_offsets, dtype=np.int64)
    nb = np.diff(off)
    return np.concatenate([[0], np.cumsum((nb + k - 1) // k)]).astype(np.int64)


def ref_bin_map(chrom_offsets, k):
    """map[i] = coff_c + (i - off_c) // k, chromosome by chromosome."""
    off = np.asarray(chrom_offsets, dtype=np.int64)
    coff = ref_offsets(off, k)
    m = np.empty(int(off[-1]), dtype=np.int64)
    for c in range(off.size - 1):
        lo, hi = int(off[c]), int(off[c + 1])
        m[lo:hi] = coff[c] + (np.arange(lo, hi) - lo) // k
    return m


def coarsen_ref(bin1, bin2, count, chrom_offsets, k):
    """``(bin1, bin2, count int64, coarse_offsets)``: ids through the bin map,
    keys I * NBc + J, counts summed per unique key (np.unique's inverse +
    bincount in int64).  A cell exists where a fine pixel maps to it."""
    m = ref_bin_map(chrom_offsets, k)
    coff = ref_offsets(chrom_offsets, k)
    nbc = int(coff[-1])
    I = m[np.asarray(bin1, dtype=np.int64)]
    J = m[np.asarray(bin2, dtype=np.int64)]
    keys, inv = np.unique(I * nbc + J, return_inverse=True)
    cnt = np.asarray(count).astype(np.int64)
    # bincount's weights are float64: sum the two 31-bit halves apart, each exact
    # below 2^53 / 2^31 addends per cell
    lo = np.bincount(inv, weights=(cnt & 0x7FFFFFFF).astype(np.float64), minlength=keys.size).astype(np.int64)
    hi = np.bincount(inv, weights=(cnt >> 31).astype(np.float64), minlength=keys.size).astype(np.int64)
    return keys // nbc, keys % nbc, lo + (hi << 31), coff


def dense_block_sum(M, chrom_offsets, k):
    """The coarse symmetric dense matrix of a symmetric dense matrix: the sum
    of every (coarse bin x coarse bin) block, except that a diagonal block
    counts its upper triangle once (cooler sums stored pixels, and stores the
    upper triangle)."""
    M = np.asarray(M)
    m = ref_bin_map(chrom_offsets, k)
    nbc = int(ref_offsets(chrom_offsets, k)[-1])
    U = np.triu(M).astype(np.int64)
    i, j = np.indices(U.shape)
    C = np.zeros((nbc, nbc), dtype=np.int64)
    np.add.at(C, (m[i.ravel()], m[j.ravel()]), U.ravel())
    C = np.triu(C)
    return C + np.triu(C, 1).T


def table_to_dense(b1, b2, c, n):
    M = np.zeros((n, n), dtype=np.int64)
    M[b1, b2] = c
    M[b2, b1] = c
    return M
