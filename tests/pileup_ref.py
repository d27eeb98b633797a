"""Dense restatement of the pileup sums: the definition as
plain loops over the features and the cells of their windows on the N x N
matrix.  It shares no code with ``hichap_master_amd.pileup``; the tests pin
the GPU sums to it.  The matrix and the validity come from
``tests/saddle_ref.py`` (the same conventions)."""
import math

import numpy as np

from tests.saddle_ref import dense, validity  # noqa: F401  (re-exported: the conventions are §4m's)


def pileup_sums(M, valid, row, col, flank, expected, min_dist, chunk):
    """``(S, Cn)``, W x W.  Window cell (u, v) of feature k is the cell i =
    row[k] - flank + u, j = col[k] - flank + v of the symmetric matrix M; it is
    eligible when both are inside the chromosome and valid, |i - j| >=
    min_dist and, with an expected, |i - j| < len(expected) and the expected
    is finite and > 0.  Cn counts the eligible cells, S adds M[i][j] (over the
    expected); an unstored cell is 0 in M and adds nothing.  The association
    is §4n's: chunks of ``chunk`` consecutive features are summed in
    ascending k from 0.0, then the chunk sums in ascending chunk order from
    0.0 -- with Python floats, so no pairwise summation takes part."""
    N, f = len(M), int(flank)
    W = 2 * f + 1
    Ml = [r.tolist() for r in np.asarray(M, dtype=np.float64)]
    vl = [bool(x) for x in valid]
    el = None if expected is None else [float(x) for x in expected]
    row, col = [int(x) for x in row], [int(x) for x in col]
    S = [[0.0] * W for _ in range(W)]
    Cn = [[0] * W for _ in range(W)]
    for k0 in range(0, len(row), chunk):
        part = [[0.0] * W for _ in range(W)]
        for k in range(k0, min(k0 + chunk, len(row))):
            for u in range(W):
                i = row[k] - f + u
                if i < 0 or i >= N or not vl[i]:
                    continue
                Mi, pu, cu = Ml[i], part[u], Cn[u]
                for v in range(W):
                    j = col[k] - f + v
                    if j < 0 or j >= N or not vl[j]:
                        continue
                    d = abs(i - j)
                    if d < min_dist:
                        continue
                    t = Mi[j]
                    if el is not None:
                        if d >= len(el):
                            continue
                        x = el[d]
                        if not (math.isfinite(x) and x > 0):
                            continue
                        t = t / x
                    cu[v] += 1
                    pu[v] += t
        for u in range(W):
            Su, pu = S[u], part[u]
            for v in range(W):
                Su[v] += pu[v]
    return np.array(S).reshape(W, W), np.array(Cn, dtype=np.int64).reshape(W, W)
