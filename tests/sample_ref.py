"""NumPy restatement of the down-sampling rule of DESIGN.md §4r, expanded per
contact: the check of hichap_master_amd/sample.py and csrc/sample.hip.  It does
not use the package.

    base = mix64(seed ^ mix64((uint64(bin1) << 32) | uint64(bin2)))
    kept = #{ t in [0, c) : mix64(base + t) < thr }       (uint64, wrapping)
"""
import numpy as np

U = np.uint64
RAGGED = (37, 5, 1, 64)        # bins per chromosome
BIG = (3, 90)                  # the pixel of 200 000 contacts
EDGE = {(10, 20): 63, (10, 21): 64, (10, 22): 65,              # the lane / wave cut of csrc/sample.hip
        (50, 60): 65535, (50, 61): 65536, (50, 62): 65537,     # the wave / block cut
        (40, 41): 0, BIG: 200000}


def mix64(z):
    """splitmix64's finaliser on a uint64 array (wrapping)."""
    z = np.asarray(z, dtype=U)
    with np.errstate(over="ignore"):
        z = z + U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def kept_ref(bin1, bin2, count, thr, seed, chunk=1 << 20):
    """kept of every pixel (int64), one hash per contact, ``chunk`` contacts at a time."""
    b1 = np.asarray(bin1).astype(U)
    b2 = np.asarray(bin2).astype(U)
    c = np.asarray(count).astype(np.int64)
    base = mix64(U(int(seed)) ^ mix64((b1 << U(32)) | b2))
    end = np.cumsum(c)
    kept = np.zeros(c.size, dtype=np.int64)
    total = int(end[-1]) if c.size else 0
    for s in range(0, total, chunk):
        g = np.arange(s, min(s + chunk, total), dtype=np.int64)      # contacts, numbered through the table
        p = np.searchsorted(end, g, side="right")                    # their pixels
        t = (g - (end[p] - c[p])).astype(U)
        with np.errstate(over="ignore"):
            flag = mix64(base[p] + t) < U(int(thr))
        kept += np.bincount(p[flag], minlength=c.size)
    return kept


def sample_ref(bin1, bin2, count, thr, seed):
    """``(bin1, bin2, kept)`` of the pixels with kept > 0, in the input's
    order: int64 ids; counts int32 while the largest is <= 2^31 - 1, else
    int64.  ``thr`` = 2^64 (frac = 1): the table as it is."""
    b1, b2 = np.asarray(bin1, dtype=np.int64), np.asarray(bin2, dtype=np.int64)
    if int(thr) >= 1 << 64:
        k, keep = np.asarray(count).astype(np.int64), slice(None)
    else:
        k = kept_ref(b1, b2, count, thr, seed)
        keep = k > 0
    k = k[keep]
    wide = k.size and int(k.max()) > 2 ** 31 - 1
    return b1[keep], b2[keep], k.astype(np.int64 if wide else np.int32)


def table107(seed=5):
    """The 107-bin test table: sorted unique upper triangle, cis and trans,
    density 0.25, counts 1 .. 59, and the forced pixels of ``EDGE``:
    ``(bin1, bin2, count int32, chrom_offsets)``."""
    off = np.concatenate([[0], np.cumsum(RAGGED)]).astype(np.int64)
    n = int(off[-1])
    rng = np.random.default_rng(seed)
    i, j = np.triu_indices(n)
    keep = rng.random(i.size) < 0.25
    for a, b in EDGE:
        keep[np.flatnonzero((i == a) & (j == b))] = True
    b1, b2 = i[keep].astype(np.int64), j[keep].astype(np.int64)
    c = rng.integers(1, 60, b1.size).astype(np.int32)
    for (a, b), v in EDGE.items():
        c[np.flatnonzero((b1 == a) & (b2 == b))] = v
    return b1, b2, c, off
