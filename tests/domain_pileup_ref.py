"""Dense restatement of the domain pileup sums: the definition
as plain loops over the features, the cells of the output grid and the bins
under each cell, on the N x N matrix.  It shares no code with
``hichap_master_amd.domain_pileup``; the tests pin the GPU sums to it.  The
matrix and the validity come from ``tests/saddle_ref.py`` (§4m's conventions).
"""
import math

import numpy as np

from tests.saddle_ref import dense, validity  # noqa: F401  (re-exported: the conventions are §4m's)


def overlaps(start, L, R, P, N):
    """Per output index u = 0 .. R + 2 P - 1 the list of ``(bin, o)``: the bins
    inside [0, N) that meet [start R + (u - P) L, + L) (units of 1/R bin; bin
    i is [i R, (i + 1) R)) and the integer length o > 0 of the meeting."""
    out = []
    for u in range(R + 2 * P):
        x0 = start * R + (u - P) * L
        x1 = x0 + L
        cells = []
        for i in range(x0 // R, (x1 - 1) // R + 1):       # Python's // floors, also below zero
            o = min(x1, (i + 1) * R) - max(x0, i * R)
            assert 0 < o <= min(L, R)
            if 0 <= i < N:
                cells.append((i, o))
        out.append(cells)
    return out


def domain_pileup_sums(M, valid, start, end, R, P, expected, min_dist, chunk, number=float):
    """``(S, Wn, m)``, G x G with G = R + 2 P.  Feature k is the half-open
    interval [start[k], end[k]) of local bins, L = end - start.  Upper form:
    output cell (u, v), u <= v, takes the matrix cells a <= b with the integer
    weight c = o(u, a) o(v, b), doubled where a != b and u == v; a cell is
    eligible when both bins are valid, b - a >= min_dist and, with an
    expected, b - a < len(expected) and the expected is finite and > 0.  A_k
    is the integer sum of c over the eligible cells, T_k the sum of t * (c /
    L^2) over the eligible cells that are stored (M != 0), from 0 in ascending
    (a, b); t = M[a][b], over the expected.  S adds T_k and Wn adds A_k / L^2
    in §4n's order: chunks of ``chunk`` consecutive features in ascending k
    from 0, then the chunk sums in ascending chunk order from 0; the lower
    triangle is the mirror.  m[u][v] counts the stored terms of the cell.
    ``number``: ``float`` (Python floats: IEEE, no pairwise summation) or
    ``fractions.Fraction`` (exact) -- the type of every sum, product and
    quotient."""
    N, G = len(M), R + 2 * P
    Ml = [[number(x) for x in r] for r in np.asarray(M, dtype=np.float64).tolist()]
    vl = [bool(x) for x in valid]
    ok = [d >= min_dist for d in range(N)]
    el = None
    if expected is not None:
        raw = [float(x) for x in expected]
        ok = [ok[d] and d < len(raw) and math.isfinite(raw[d]) and raw[d] > 0 for d in range(N)]
        el = [number(x) if ok[d] else None for d, x in enumerate(raw)]
    zero = number(0)
    S = [[zero] * G for _ in range(G)]
    Wn = [[zero] * G for _ in range(G)]
    m = [[0] * G for _ in range(G)]
    start, end = [int(x) for x in start], [int(x) for x in end]
    for k0 in range(0, len(start), chunk):
        part = [[zero] * G for _ in range(G)]
        wpart = [[zero] * G for _ in range(G)]
        for k in range(k0, min(k0 + chunk, len(start))):
            L = end[k] - start[k]
            assert 0 <= start[k] < end[k] <= N
            LL = number(L * L)
            cells = [[(i, o) for i, o in c if vl[i]] for c in overlaps(start[k], L, R, P, N)]
            for u in range(G):
                for v in range(u, G):
                    A, T = 0, zero
                    for a, oa in cells[u]:
                        Ma = Ml[a]
                        for b, ob in cells[v]:
                            if b < a:
                                assert u == v                # (a < b never feeds u > v: only the diagonal cell)
                                continue
                            if not ok[b - a]:
                                continue
                            c = oa * ob
                            if u == v and a != b:
                                c *= 2
                            A += c
                            t = Ma[b]
                            if t != 0:
                                if el is not None:
                                    t = t / el[b - a]
                                T += t * (number(c) / LL)
                                m[u][v] += 1
                    part[u][v] += T
                    wpart[u][v] += number(A) / LL
        for u in range(G):
            for v in range(u, G):
                S[u][v] += part[u][v]
                Wn[u][v] += wpart[u][v]
    for u in range(G):
        for v in range(u):
            S[u][v], Wn[u][v], m[u][v] = S[v][u], Wn[v][u], m[v][u]
    if number is float:
        return np.array(S).reshape(G, G), np.array(Wn).reshape(G, G), np.array(m, dtype=np.int64).reshape(G, G)
    return S, Wn, np.array(m, dtype=np.int64).reshape(G, G)
