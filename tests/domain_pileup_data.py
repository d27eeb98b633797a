"""Inputs shared by tests/test_domain_pileup_cpu.py and
tests/test_domain_pileup_gpu.py: the pixel table of three
chromosomes, the weights, the invalid bins, the expected vector (generated the
way tests/test_pileup_gpu.py generates its own), two lists of about 150
domains and the planted chromosome of the ``run_DomainPileup`` tests.
Everything is cached and read-only."""
import functools

import numpy as np

from tests import domain_pileup_ref as ref

RES = 10000
N = 300
LO, NB = 11, 11 + N + 9                       # 'a' 11 bins, 'b' N bins (queried), 'c' 9 bins
INVALID = [0, N - 1, 90, 91, 92, 93, 150]     # both ends, a run of 4, a single bin
EMPTY_ROW = 40                                # a bin with no pixels at all
N_EXP = 200                                   # n_expected < N: far cells are cut
CHUNK, DEFAULT_CHUNK = 16, 64
GRIDS = [(8, 4), (7, 3), (5, 0), (1, 0), (63, 32)]   # (R, P); the last one is the cap, G = 127
POW2 = (1, 2, 4, 8, 16, 32, 64)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def table():
    """Sorted upper-triangle pixel table of the three chromosomes, counts in
    1/64: dense near the diagonal of 'b', sparse far from it, trans pixels
    into 'b' and out of it."""
    rng = np.random.default_rng(2025)
    i, j = np.indices((NB, NB))
    H = np.triu(rng.integers(1, 4000, (NB, NB)) * (rng.random((NB, NB)) < np.where(j - i < 140, 0.7, 0.15)))
    H[LO + EMPTY_ROW, :] = 0
    H[:, LO + EMPTY_ROW] = 0
    H[LO + 2, LO + N - 3] = 77
    assert np.count_nonzero(H[:LO, LO:LO + N]) > 20 and np.count_nonzero(H[LO:LO + N, LO + N:]) > 20
    b1, b2 = np.nonzero(H)
    return _frozen(b1.astype(np.int64), b2.astype(np.int64), H[b1, b2] / 64.0)


def weights(kind):
    """Global weights (None for 'raw') and the 'bad' list of chromosome 'b'.
    exact: powers of two in 2^-3 .. 2^0; general: uniform in [0.05, 3)."""
    rng = np.random.default_rng(5)
    w = 2.0 ** rng.integers(-3, 1, NB) if kind.startswith("exact") else rng.uniform(0.05, 3.0, NB)
    bad = None
    if kind.endswith("nan"):
        w[LO + np.array(INVALID)] = np.nan
        w[3] = np.nan                         # a masked bin of 'a': its trans pixels must not matter
    else:
        bad = np.zeros(N, np.uint8)
        bad[INVALID] = 1
    return (None if kind.startswith("raw") else w), bad


@functools.lru_cache(maxsize=None)
def dense(kind):
    w, bad = weights(kind)
    return _frozen(ref.dense(*table(), w, LO, N), ref.validity(w, LO, N, bad))


def expected_vector(kind, use):
    """None, or N_EXP entries with a zero and two NaN: powers of two in 2^-2 ..
    2^2 for the exact and raw kinds, random positive values otherwise."""
    if not use:
        return None
    rng = np.random.default_rng(8)
    if kind.startswith("exact") or kind.startswith("raw"):
        e = 2.0 ** rng.integers(-2, 3, N_EXP).astype(np.float64)
    else:
        e = rng.uniform(0.1, 5.0, N_EXP)
    e[3] = np.nan
    e[50] = np.nan
    e[6] = 0.0
    return e


@functools.lru_cache(maxsize=None)
def features(which):
    """``(start, end)``, int32, 150 domains in a fixed shuffled order (a
    partial last chunk at 16 per chunk).  'general': lengths 1 .. 126 -- below,
    at, multiples of and between multiples of every R of GRIDS -- and the whole
    chromosome; 'pow2': every length a power of two up to 64; 'seven': every
    length 7.  Each list has domains at start = 0 and end = N, flanks that
    leave the chromosome at either end, domains over the invalid run, the
    single invalid bin and the empty row, overlaps and three exact repeats."""
    rng = np.random.default_rng({"general": 78, "pow2": 79, "seven": 80}[which])
    if which == "general":
        fixed = [(0, N), (0, 1), (0, 8), (0, 63), (0, 120), (N - 1, N), (N - 7, N), (N - 64, N), (N - 126, N),
                 (2, 60), (5, 125), (10, 130), (250, 298), (180, 299), (60, 186),
                 (85, 100), (88, 96), (90, 94), (91, 92), (148, 153), (150, 151), (89, 152),
                 (35, 45), (40, 41), (38, 42), (40, 103), (1, 41),
                 (100, 105), (100, 107), (100, 108), (100, 110), (100, 114), (100, 116), (100, 121), (100, 163),
                 (100, 226), (200, 203), (200, 209), (200, 211), (200, 213), (200, 265)]
        lengths = rng.integers(1, 121, 150)
    elif which == "pow2":
        fixed = [(0, 1), (0, 8), (0, 64), (N - 1, N), (N - 2, N), (N - 32, N), (N - 64, N), (2, 66), (4, 36),
                 (230, 294), (266, 298), (88, 96), (90, 94), (91, 92), (86, 102), (150, 151), (148, 152), (120, 184),
                 (36, 44), (40, 41), (39, 41), (24, 56), (100, 108), (100, 116), (100, 164), (104, 112)]
        lengths = rng.choice(POW2, 150)
    else:
        fixed = [(0, 7), (N - 7, N), (1, 8), (N - 8, N - 1), (88, 95), (90, 97), (146, 153), (150, 157), (36, 43),
                 (40, 47), (34, 41), (100, 107), (103, 110), (107, 114)]
        lengths = np.full(150, 7)
    F = list(fixed)
    for L in lengths[:150 - 3 - len(fixed)].tolist():
        s = int(rng.integers(0, N - L + 1))
        F.append((s, s + L))
    F += [F[0], F[len(fixed)], F[len(fixed) + 20]]          # three exact repeats
    F = [F[k] for k in rng.permutation(len(F))]
    assert len(F) == 150 and len(F) % CHUNK != 0 and len(set(F)) <= 147
    start, end = np.array([a for a, _ in F], np.int32), np.array([b for _, b in F], np.int32)
    assert start.min() == 0 and end.max() == N and (start < end).all()
    if which == "pow2":
        assert set((end - start).tolist()) == set(POW2)
    return _frozen(start, end)


@functools.lru_cache(maxsize=None)
def want(kind, which, R, P, use_e, min_dist, chunk=CHUNK):
    """The restatement's (S, Wn, m) on the shared input."""
    start, end = features(which)
    return _frozen(*ref.domain_pileup_sums(*dense(kind), start, end, R, P, expected_vector(kind, use_e), min_dist,
                                           chunk))


# ten domains of different sizes on a chromosome of 400 bins; bins 3, 7, 395 and 398 are masked
PLANTED = [(12, 30), (30, 70), (75, 83), (90, 150), (150, 171), (180, 185), (200, 262), (270, 300), (300, 345),
           (350, 390)]


@functools.lru_cache(maxsize=None)
def planted(domains=True, seed=3, Nc=400):
    """A chromosome whose balanced matrix is a distance decay 2e5 / (d + 1),
    three times that inside the PLANTED domains (none with ``domains=False``),
    under multiplicative noise of 5 %: counts = round(balanced / (w_a w_b)),
    weights in [0.5, 2) with four NaN.  Returns (bin1, bin2, count, weight)."""
    rng = np.random.default_rng(seed)
    a, b = np.nonzero(np.triu(np.ones((Nc, Nc))))
    bal = 2e5 / (b - a + 1.0) * rng.uniform(0.95, 1.05, a.size)
    if domains:
        dom = np.full(Nc, -1)
        for k, (s, e) in enumerate(PLANTED):
            dom[s:e] = k
        bal[(dom[a] >= 0) & (dom[a] == dom[b])] *= 3.0
    weight = rng.uniform(0.5, 2.0, Nc)
    count = np.rint(bal / (weight[a] * weight[b])).astype(np.int64)
    weight[[3, 7, Nc - 5, Nc - 2]] = np.nan
    return _frozen(a.astype(np.int64), b.astype(np.int64), count, weight)
