"""NumPy restatement of ``cooler merge`` on pixel tables: the check of
hichap_master_amd/merge.py and csrc/merge.hip.  It does not use
the package."""
import numpy as np


def merge_ref(tables, n_bins):
    """``(bin1, bin2, count int64)``: the tables concatenated, keys bin1 *
    n_bins + bin2, counts summed per unique key (np.unique's inverse +
    bincount in int64).  A pixel exists where a table stores it."""
    n_bins = int(n_bins)
    b1 = np.concatenate([np.asarray(t[0], dtype=np.int64) for t in tables])
    b2 = np.concatenate([np.asarray(t[1], dtype=np.int64) for t in tables])
    cnt = np.concatenate([np.asarray(t[2]).astype(np.int64) for t in tables])
    keys, inv = np.unique(b1 * n_bins + b2, return_inverse=True)
    # bincount's weights are float64: sum the two 31-bit halves apart, each exact
    # below 2^53 / 2^31 addends per pixel (tests/coarsen_ref.py)
    lo = np.bincount(inv, weights=(cnt & 0x7FFFFFFF).astype(np.float64), minlength=keys.size).astype(np.int64)
    hi = np.bincount(inv, weights=(cnt >> 31).astype(np.float64), minlength=keys.size).astype(np.int64)
    return keys // n_bins, keys % n_bins, lo + (hi << 31)
