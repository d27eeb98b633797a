"""Cis expected and compartment saddle on the GPU (csrc/saddle.hip, DESIGN.md
§4m): ``hh_expected_pixels`` and ``hh_saddle_pixels`` against the dense
restatement (tests/saddle_ref.py) -- exactly where every product, quotient and
sum is exact in fp64, within a bound derived from the number of terms
otherwise -- then ``run_Saddle`` on a planted compartment chromosome, through
the traditional (balanced) path and the haplotype (raw) path."""
import functools
import os

import numpy as np
import pytest

from hichap_master_amd import _lib, coolio, h5
from hichap_master_amd import saddle as sd
from hichap_master_amd._lib import HipLibraryError, ptr
from hichap_master_amd.StructureFind import StructureFind, py2_float_str
from tests import saddle_ref as ref
from tests.knobs import tuned

pytestmark = pytest.mark.gpu

RES = 10000
N = 300                                       # not a multiple of 64: the masks' tail word is partial
LO, NB = 11, 11 + N + 9                       # 'a' 11 bins, 'b' N bins (queried), 'c' 9 bins
INVALID = [0, N - 1, 90, 91, 92, 93, 150]     # both ends, a run of 4, a single bin
EMPTY_ROW = 40                                # a bin with no pixels at all
HH_ERR_ARG = -1
DEFAULT_TILE = 256                            # HH_SADDLE_DIAG_TILE
U53 = 2.0 ** -53


@pytest.fixture(autouse=True)
def small_tile():
    """64 diagonals per wave: five sub-tiles, two blocks of sub-tiles and three
    row chunks have their edges inside the 300-bin table."""
    with tuned(saddle_diag_tile=64):
        yield


@functools.lru_cache(maxsize=None)
def _table():
    """Sorted upper-triangle pixel table of the three chromosomes, counts in
    1/64: dense near the diagonal of 'b', sparse far from it (every distance
    up to N - 1 is hit), trans pixels into 'b' (bin1 < LO) and out of it
    (bin2 >= LO + N)."""
    rng = np.random.default_rng(2025)
    i, j = np.indices((NB, NB))
    H = np.triu(rng.integers(1, 4000, (NB, NB)) * (rng.random((NB, NB)) < np.where(j - i < 140, 0.7, 0.15)))
    H[LO + EMPTY_ROW, :] = 0
    H[:, LO + EMPTY_ROW] = 0
    H[LO + 2, LO + N - 3] = 77                # a far corner pixel between valid bins
    assert np.count_nonzero(H[:LO, LO:LO + N]) > 20 and np.count_nonzero(H[LO:LO + N, LO + N:]) > 20
    b1, b2 = np.nonzero(H)
    cnt = H[b1, b2] / 64.0
    for a in (b1, b2, cnt):
        a.setflags(write=False)
    return b1.astype(np.int64), b2.astype(np.int64), cnt


def _weights(kind):
    """Global weights and the 'bad' list of chromosome 'b'.  exact: powers of
    two, so every product of the k/64 counts is exact in fp64."""
    rng = np.random.default_rng(5)
    if kind.startswith("exact"):
        w = 2.0 ** rng.integers(-3, 1, NB)
    else:
        w = rng.uniform(0.05, 3.0, NB)
    bad = None
    if kind.endswith("nan"):
        w[LO + np.array(INVALID)] = np.nan
        w[3] = np.nan                         # a masked bin of 'a': its trans pixels must not matter
    else:
        bad = np.zeros(N, np.uint8)
        bad[INVALID] = 1
    return w, bad


@functools.lru_cache(maxsize=None)
def _dense(kind):
    w, bad = _weights(kind)
    M = ref.dense(*_table(), w, LO, N)
    valid = ref.validity(w, LO, N, bad)
    M.setflags(write=False)
    valid.setflags(write=False)
    return M, valid


@functools.lru_cache(maxsize=None)
def _want_expected(kind, g, D):
    out = ref.expected_sums(*_dense(kind), g, D)
    for a in out:
        a.setflags(write=False)
    return out


def _classes(K):
    """A class per bin of 'b', 255 for about one bin in ten."""
    rng = np.random.default_rng(K)
    cls = rng.integers(0, K, N).astype(np.uint8)
    cls[rng.random(N) < 0.1] = 255
    cls[7] = K - 1                            # the largest id is in use
    return cls


def _expected_vector(kind, D):
    """exact: powers of two, two diagonals NaN and one 0 (unusable); general:
    the restatement's own expected."""
    if kind.startswith("exact"):
        e = 2.0 ** np.random.default_rng(8).integers(-2, 3, D + 1).astype(np.float64)
        e[3] = np.nan
        e[min(50, D)] = np.nan
        e[6] = 0.0
        return e
    s, n = _want_expected(kind, 1, D)
    return ref.expected(s, n, 1)


@functools.lru_cache(maxsize=None)
def _want_saddle(kind, K, min_dist, D):
    out = ref.saddle_sums(*_dense(kind), _expected_vector(kind, D), _classes(K), K, min_dist, D)
    for a in out:
        a.setflags(write=False)
    return out


def _dev(*arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.array(a)).cuda() for a in arrays]


def _expected(kind, g, D, device=False):
    b1, b2, cnt = _table()
    w, bad = _weights(kind)
    if device:
        b1, b2, cnt, w, bad = _dev(b1, b2, cnt, w, bad)
    s, n = sd.expected_pixels(b1, b2, cnt, w, LO, N, g, D, bad)
    if device:
        assert s.is_cuda and n.is_cuda
        s, n = s.cpu().numpy(), n.cpu().numpy()
    assert s.dtype == np.float64 and n.dtype == np.int64 and s.shape == n.shape == (D + 1,)
    return s, n


def _saddle(kind, K, min_dist, D, device=False):
    b1, b2, cnt = _table()
    w, bad = _weights(kind)
    e, cls = _expected_vector(kind, D), _classes(K)
    if device:
        b1, b2, cnt, w, bad, e, cls = _dev(b1, b2, cnt, w, bad, e, cls)
    U, Cu = sd.saddle_pixels(b1, b2, cnt, w, LO, N, e, cls, K, min_dist, D, bad)
    if device:
        assert U.is_cuda and Cu.is_cuda
        U, Cu = U.cpu().numpy(), Cu.cpu().numpy()
    assert U.dtype == np.float64 and Cu.dtype == np.int64 and U.shape == Cu.shape == (K, K)
    return U, Cu


# ------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("kind", ["exact_nan", "exact_bad"])
@pytest.mark.parametrize("D", [0, 7, N - 1])
@pytest.mark.parametrize("g", [0, 1, 2])
def test_expected_exact(kind, g, D):
    s, n = _want_expected(kind, g, D)
    if D == N - 1:
        assert n[N - 1] == 0 and s[N - 5] > 0             # both ends are invalid bins; the far corner pixel
        assert g > 1 or n[1] == N - 1 - 9                 # 9 neighbour pairs touch one of the 7 invalid bins
    for device in (False, True):
        got_s, got_n = _expected(kind, g, D, device)
        assert np.array_equal(got_n, n)
        assert np.array_equal(got_s, s)


@pytest.mark.parametrize("kind", ["exact_nan", "exact_bad"])
@pytest.mark.parametrize("D", [7, N - 1])
@pytest.mark.parametrize("K", [2, 12, 64])
@pytest.mark.parametrize("min_dist", [1, 5])
def test_saddle_exact(kind, min_dist, K, D):
    U, Cu = _want_saddle(kind, K, min_dist, D)
    assert Cu.sum() > 0 and U.sum() > 0
    for device in (False, True):
        got_U, got_Cu = _saddle(kind, K, min_dist, D, device)
        assert np.array_equal(got_Cu, Cu)
        assert np.array_equal(got_U, U)


def test_exact_at_the_default_tile():
    with tuned(saddle_diag_tile=DEFAULT_TILE):
        for g, D in ((0, N - 1), (2, 7)):
            s, n = _want_expected("exact_nan", g, D)
            got_s, got_n = _expected("exact_nan", g, D)
            assert np.array_equal(got_n, n) and np.array_equal(got_s, s)
        U, Cu = _want_saddle("exact_nan", 12, 1, N - 1)
        got_U, got_Cu = _saddle("exact_nan", 12, 1, N - 1)
    assert np.array_equal(got_Cu, Cu) and np.array_equal(got_U, U)


# -------------------------------------------------- 2. random positive weights
def _rtol(m):
    """Both sides sum the same m non-negative IEEE terms in different orders;
    either sum is within m * 2^-53 (relative) of the true one, so the two are
    within 2 (m + 2) 2^-53 of each other.  Derived from the input, not measured."""
    return 2.0 * (int(m) + 2) * U53


@pytest.mark.parametrize("kind", ["general_nan", "general_bad"])
@pytest.mark.parametrize("g,D", [(0, N - 1), (2, N - 1), (1, 7)])
def test_expected_general(kind, g, D):
    s, n = _want_expected(kind, g, D)
    rtol = _rtol(n.max())
    for device in (False, True):
        got_s, got_n = _expected(kind, g, D, device)
        assert np.array_equal(got_n, n)
        err = np.abs(got_s - s) / np.where(s > 0, s, 1.0)
        print(f"{kind} g={g} D={D}: max relative error {err.max():.3g}, bound {rtol:.3g}")
        np.testing.assert_allclose(got_s, s, rtol=rtol, atol=0)


@pytest.mark.parametrize("kind", ["general_nan", "general_bad"])
@pytest.mark.parametrize("K,min_dist,D", [(12, 1, N - 1), (64, 5, N - 1), (2, 1, 7), (52, 2, N - 1)])
def test_saddle_general(kind, K, min_dist, D):
    U, Cu = _want_saddle(kind, K, min_dist, D)
    rtol = _rtol(Cu.max())
    for device in (False, True):
        got_U, got_Cu = _saddle(kind, K, min_dist, D, device)
        assert np.array_equal(got_Cu, Cu)
        err = np.abs(got_U - U) / np.where(U > 0, U, 1.0)
        print(f"{kind} K={K} min_dist={min_dist} D={D}: max relative error {err.max():.3g}, bound {rtol:.3g}")
        np.testing.assert_allclose(got_U, U, rtol=rtol, atol=0)


# ----------------------------------------------------------------- 3. bitwise
def test_bitwise():
    kind, g, K = "general_nan", 1, 12
    s1, n1 = _expected(kind, g, N - 1)
    s2, n2 = _expected(kind, g, N - 1)
    s3, n3 = _expected(kind, g, N - 1, device=True)
    assert s1.tobytes() == s2.tobytes() == s3.tobytes()                   # two calls; host form = device form
    assert n1.tobytes() == n2.tobytes() == n3.tobytes()
    U1, C1 = _saddle(kind, K, 1, N - 1)
    U2, C2 = _saddle(kind, K, 1, N - 1)
    U3, C3 = _saddle(kind, K, 1, N - 1, device=True)
    assert U1.tobytes() == U2.tobytes() == U3.tobytes()
    assert C1.tobytes() == C2.tobytes() == C3.tobytes()
    # The default tile is another partition of the diagonals among the waves, which the
    # interface does not promise to sum in the same order: it is held to the bound of
    # test_expected_general only, the integer counts to equality.
    with tuned(saddle_diag_tile=DEFAULT_TILE):
        s4, n4 = _expected(kind, g, N - 1)
        U4, C4 = _saddle(kind, K, 1, N - 1)
    assert np.array_equal(n4, n1) and np.array_equal(C4, C1)
    np.testing.assert_allclose(s4, s1, rtol=_rtol(n1.max()), atol=0)
    np.testing.assert_allclose(U4, U1, rtol=_rtol(C1.max()), atol=0)


# ------------------------------------------------------------------- 4. edges
def test_no_pixels():
    none = (np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0))
    w, bad = _weights("exact_nan")
    e, cls = _expected_vector("exact_nan", N - 1), _classes(12)
    for device in (False, True):
        b1, b2, cnt, wt, ex, cl = _dev(*none, w, e, cls) if device else (*none, w, e, cls)
        s, n = sd.expected_pixels(b1, b2, cnt, wt, LO, N, 1, N - 1)
        U, Cu = sd.saddle_pixels(b1, b2, cnt, wt, LO, N, ex, cl, 12, 1, N - 1)
        if device:
            s, n, U, Cu = (t.cpu().numpy() for t in (s, n, U, Cu))
        assert not s.any() and np.array_equal(n, _want_expected("exact_nan", 1, N - 1)[1])
        assert not U.any() and np.array_equal(Cu, _want_saddle("exact_nan", 12, 1, N - 1)[1])


def test_every_bin_invalid():
    b1, b2, cnt = _table()
    w = _weights("exact_bad")[0]
    bad = np.ones(N, np.uint8)
    s, n = sd.expected_pixels(b1, b2, cnt, w, LO, N, 0, N - 1, bad)
    assert not s.any() and not n.any()
    U, Cu = sd.saddle_pixels(b1, b2, cnt, w, LO, N, np.ones(N), _classes(12), 12, 1, N - 1, bad)
    assert not U.any() and not Cu.any()
    s, n = sd.expected_pixels(b1, b2, cnt, np.full(NB, np.nan), LO, N, 0, N - 1)      # the same through the weights
    assert not s.any() and not n.any()


def test_one_bin_chromosome():
    b1 = np.array([0, 0, 1, 1, 2], np.int64)             # chromosomes of 1, 1 and 1 bins; the middle one is queried
    b2 = np.array([0, 1, 1, 2, 2], np.int64)
    cnt = np.array([3.0, 5.0, 7.0, 11.0, 13.0])
    for g, want in ((0, 7.0), (1, 0.0)):
        s, n = sd.expected_pixels(b1, b2, cnt, None, 1, 1, g, 0)
        assert s.tolist() == [want] and n.tolist() == [1 - g]
    s, n = sd.expected_pixels(b1, b2, cnt, np.array([1.0, 0.5, 1.0]), 1, 1, 0, 0)
    assert s.tolist() == [1.75] and n.tolist() == [1]
    with pytest.raises(HipLibraryError, match="min_dist"):            # no distance >= 1 exists: no saddle
        sd.saddle_pixels(b1, b2, cnt, None, 1, 1, np.ones(1), np.zeros(1, np.uint8), 2, 1, 0)


def test_all_classes_left_out():
    b1, b2, cnt = _table()
    w, bad = _weights("exact_bad")
    U, Cu = sd.saddle_pixels(b1, b2, cnt, w, LO, N, np.ones(N), np.full(N, 255, np.uint8), 12, 1, N - 1, bad)
    assert not U.any() and not Cu.any()
    # and no usable diagonal
    U, Cu = sd.saddle_pixels(b1, b2, cnt, w, LO, N, np.full(N, np.nan), _classes(12), 12, 1, N - 1, bad)
    assert not U.any() and not Cu.any()


def test_argument_errors_leave_outputs_untouched():
    b1, b2, cnt = _table()
    w = _weights("exact_nan")[0]
    lib = _lib.load()
    s, n = np.full(N, -7.5), np.full(N, -3, np.int64)
    U, Cu = np.full((64, 64), -7.5), np.full((64, 64), -3, np.int64)
    e = _expected_vector("exact_nan", N - 1)

    def expected(N_=N, g=1, D=N - 1, n_weight=NB):
        return lib.hh_expected_pixels(ptr(b1), ptr(b2), ptr(cnt), b1.size, ptr(w), n_weight, LO, N_, None, g, D,
                                      ptr(s), ptr(n), 0, None)

    def saddle(N_=N, K=12, min_dist=1, D=N - 1, n_weight=NB, cls=None):
        cls = _classes(12) if cls is None else cls
        return lib.hh_saddle_pixels(ptr(b1), ptr(b2), ptr(cnt), b1.size, ptr(w), n_weight, LO, N_, None, ptr(e),
                                    ptr(cls), K, min_dist, D, ptr(U), ptr(Cu), 0, None)

    assert expected(N_=0, D=0) == HH_ERR_ARG and saddle(N_=0) == HH_ERR_ARG                  # N < 1
    assert expected(D=-1) == HH_ERR_ARG and expected(D=N) == HH_ERR_ARG                      # max_dist
    assert b"max_dist" in lib.hh_last_error()
    assert saddle(D=N) == HH_ERR_ARG and saddle(D=-1) == HH_ERR_ARG
    assert expected(g=-1) == HH_ERR_ARG                                                      # ignore_diags < 0
    assert b"ignore_diags" in lib.hh_last_error()
    assert saddle(min_dist=0) == HH_ERR_ARG and saddle(min_dist=8, D=7) == HH_ERR_ARG        # min_dist
    assert b"min_dist" in lib.hh_last_error()
    assert saddle(K=1) == HH_ERR_ARG and saddle(K=65) == HH_ERR_ARG                          # K
    assert b"K outside" in lib.hh_last_error()
    for wrong in (12, 200, 254):                                                             # a class in [K, 254]
        cls = _classes(12)
        cls[N - 2] = wrong
        assert saddle(cls=cls) == HH_ERR_ARG, wrong
        assert b"cls entry" in lib.hh_last_error()
    assert expected(n_weight=LO + N - 1) == HH_ERR_ARG and saddle(n_weight=LO + N - 1) == HH_ERR_ARG
    assert b"weights do not cover" in lib.hh_last_error()
    assert np.all(s == -7.5) and np.all(n == -3) and np.all(U == -7.5) and np.all(Cu == -3)
    import torch                                                                             # the device form too
    dcls = _classes(12)
    dcls[5] = 100
    tb1, tb2, tc, tw, te, tcls = _dev(b1, b2, cnt, w, e, dcls)
    tU, tCu = torch.full((12, 12), -7.5, dtype=torch.float64).cuda(), torch.full((12, 12), -3).cuda()
    assert lib.hh_saddle_pixels(ptr(tb1), ptr(tb2), ptr(tc), b1.size, ptr(tw), NB, LO, N, None, ptr(te), ptr(tcls),
                                12, 1, N - 1, ptr(tU), ptr(tCu), 1, None) == HH_ERR_ARG
    assert bool((tU == -7.5).all()) and bool((tCu == -3).all())
    with pytest.raises(HipLibraryError, match="K outside"):
        sd.saddle_pixels(b1, b2, cnt, w, LO, N, e, _classes(12), 65)
    # the library is still usable, and only the K x K head of the outputs is written
    assert expected(g=1) == 0 and saddle(K=12) == 0
    want = _want_expected("exact_nan", 1, N - 1)
    assert np.array_equal(s, want[0]) and np.array_equal(n, want[1])
    want = _want_saddle("exact_nan", 12, 1, N - 1)
    assert np.array_equal(U.ravel()[:144].reshape(12, 12), want[0])
    assert np.array_equal(Cu.ravel()[:144].reshape(12, 12), want[1])
    assert np.all(U.ravel()[144:] == -7.5) and np.all(Cu.ravel()[144:] == -3)


# ---------------------------------------------------------- 5, 6. run_Saddle
def _read(out):
    prefix = os.path.basename(out)
    res = StructureFind.properU(RES)
    return [[ln.rstrip("\n").split("\t") for ln in open(os.path.join(out, f"{prefix}_{what}_{res}.txt"))]
            for what in ("Expected", "Saddle", "SaddleStrength")]


def _check_run(r, out, chrom, shown, M, valid, track, g, n_bins):
    """``run_Saddle``'s arrays against the restatement on the dense matrix M,
    and the three files as the text of those arrays.  The chain has two links.
    The expected sums are held to 2 (m + 2) 2^-53, m the largest nvalid.  The
    saddle's terms v / expected[d] then differ between the two sides by the
    relative difference of the two expected vectors, and a sum of non-negative
    terms each perturbed by at most delta is perturbed by at most delta: so
    the restatement fed with the call's own expected is held to 2 (m + 2)
    2^-53, m the largest Cu cell (the +2: the addition U + U^T and the division
    by C), and the restatement's own chain to the sum of the two bounds.
    strength(k) is a ratio of two ratios, each of a sum of 2 k^2 such cells over
    a count: 2 k^2 + 1 roundings per ratio and one for the last division, on
    either side, on top of twice the cells' bound."""
    Nc, K = len(M), n_bins + 2
    bound_k = 2 * (2 * (2 * (n_bins // 2) ** 2 + 1) + 1) * U53
    rc = r["chroms"][chrom]
    s, n = ref.expected_sums(M, valid, g, Nc - 1)
    e = ref.expected(s, n, g)
    (cls,), edges = ref.digitize([track], [valid], n_bins, 0.025, 0.975)
    assert list(r["chroms"]) == [chrom] and np.array_equal(rc["valid"] != 0, valid)
    assert np.array_equal(rc["nvalid"], n) and np.array_equal(rc["cls"], cls) and np.array_equal(r["edges"], edges)
    bound_e = _rtol(n.max())
    np.testing.assert_allclose(rc["sum"], s, rtol=bound_e, atol=0)
    assert np.array_equal(np.isnan(rc["expected"]), np.isnan(e))
    np.testing.assert_allclose(rc["expected"], e, rtol=bound_e, atol=0, equal_nan=True)
    dmin = max(1, g)
    U, Cu = ref.saddle_sums(M, valid, rc["expected"], cls, K, dmin, Nc - 1)   # the call's own expected
    S, C, sad = ref.symmetric(U, Cu)
    bound_s = _rtol(Cu.max())
    assert np.array_equal(rc["Cu"], Cu) and np.array_equal(r["C"], C)
    np.testing.assert_allclose(rc["U"], U, rtol=bound_s, atol=0)
    np.testing.assert_allclose(r["saddle"], sad, rtol=bound_s, atol=0, equal_nan=True)
    U2, Cu2 = ref.saddle_sums(M, valid, e, cls, K, dmin, Nc - 1)              # the restatement's own chain
    S2, C2, sad2 = ref.symmetric(U2, Cu2)
    assert np.array_equal(C2, C)
    np.testing.assert_allclose(r["saddle"], sad2, rtol=bound_s + bound_e, atol=0, equal_nan=True)
    k_want = ref.strength(S2, C2)
    np.testing.assert_allclose(r["strength"], k_want, rtol=2 * (bound_s + bound_e) + bound_k, atol=0)
    print(f"{chrom}: strength(k) = {r['strength']}, restatement {k_want}")
    assert k_want[1] > 2 and r["strength"][1] > 2
    interior = r["saddle"][1:-1, 1:-1]
    same = (interior[:2, :2].mean() + interior[-2:, -2:].mean()) / 2
    cross = (interior[:2, -2:].mean() + interior[-2:, :2].mean()) / 2
    assert same > cross
    # the files are the text of these arrays
    exp, sadf, strf = _read(out)
    assert exp[0] == ["chrom", "dist_bins", "dist_bp", "n_valid", "balanced_sum", "balanced_avg"]
    assert exp[1:] == [[shown, str(d), str(d * RES), str(int(n[d])), py2_float_str(rc["sum"][d]),
                        py2_float_str(rc["expected"][d])] for d in range(Nc)]
    assert sadf[0] == [py2_float_str(x) for x in edges] and len(sadf[0]) == K - 1
    assert sadf[1:] == [[py2_float_str(x) for x in row] for row in r["saddle"]] and len(sadf) == 1 + K
    assert strf == [["k", "strength"]] + [[str(k + 1), py2_float_str(x)] for k, x in enumerate(r["strength"])]
    # and, parsed back, the restatement's values: '%.12g' rounds to 5e-12 (relative)
    got = np.array([[float(x) for x in row] for row in sadf[1:]])
    np.testing.assert_allclose(got, sad2, rtol=bound_s + bound_e + 5e-12, atol=0, equal_nan=True)
    np.testing.assert_allclose([float(t[5]) for t in exp[1:]], e, rtol=bound_e + 5e-12, atol=0, equal_nan=True)
    np.testing.assert_allclose([float(t[1]) for t in strf[1:]], k_want,
                               rtol=2 * (bound_s + bound_e) + bound_k + 5e-12, atol=0)


def test_run_saddle_traditional(tmp_path):
    b1, b2, count, weight, track = ref.planted()
    Nc = track.size
    path = str(tmp_path / "trad.cool")
    coolio.create_cooler(path, {RES: ([("chr1", Nc * RES)], b1, b2, count)})
    out = str(tmp_path / "planted")
    sf = StructureFind(path, Res=RES)
    with pytest.raises(ValueError, match="no bins/weight"):
        sf.run_Saddle(out, track={"chr1": track})
    h5.append_dataset(path, f"{RES}/bins", "weight", weight)
    with pytest.raises(ValueError, match="239 values"):
        sf.run_Saddle(out, track={"chr1": track[:-1]}, n_bins=10)
    r = sf.run_Saddle(out, track={"chr1": track}, n_bins=10, ignore_diags=2)
    assert r is sf.Saddle_dict
    M = ref.dense(b1, b2, count, weight, 0, Nc)
    _check_run(r, out, "chr1", "chr1", M, ref.validity(weight, 0, Nc, None), track, 2, 10)
    # distances in bp: min_dist / max_dist select the diagonals
    r2 = sf.run_Saddle(str(tmp_path / "near"), track={"chr1": track}, n_bins=10, ignore_diags=2,
                       min_dist=5 * RES, max_dist=40 * RES)
    rc = r2["chroms"]["chr1"]
    assert rc["sum"].shape == (41,)
    want = ref.saddle_sums(M, rc["valid"] != 0, rc["expected"], rc["cls"], 12, 5, 40)
    assert np.array_equal(rc["Cu"], want[1])
    np.testing.assert_allclose(rc["U"], want[0], rtol=_rtol(want[1].max()), atol=0)


def test_run_saddle_haplotype(tmp_path):
    """The same planted chromosome as the maternal haplotype 'Mb' (raw counts,
    no weights), the NaN-weight bins as its gap list, next to a paternal 'Pb'
    that must not be read; the track comes from a PC file without prefixes."""
    b1, b2, count, weight, track = ref.planted()
    Nc = track.size
    gap = np.nonzero(~np.isfinite(weight))[0]
    pb = Nc + np.arange(30)
    path = str(tmp_path / "hap.cool")
    coolio.create_cooler(path, {RES: ([("Mb", Nc * RES), ("Pb", 30 * RES)], np.concatenate([b1, pb]),
                                      np.concatenate([b2, pb]), np.concatenate([count, np.full(30, 9)]))})
    pc = str(tmp_path / "pc.txt")
    with open(pc, "w") as f:
        for x in track:
            f.write(f"b\t{float(x)!r}\n")
        for x in range(30):
            f.write("c\t0.5\n")
    out = str(tmp_path / "hap")
    sf = StructureFind(path, Res=RES, Allelic="Maternal", GapFile={str(RES): {"Mb": gap, "Pb": np.array([0])}})
    with pytest.raises(ValueError, match="no track"):
        sf.run_Saddle(out)
    r = sf.run_Saddle(out, PC_file=pc, n_bins=10, ignore_diags=2)
    bad = np.zeros(Nc, np.uint8)
    bad[gap] = 1
    M = ref.dense(b1, b2, count, None, 0, Nc)
    _check_run(r, out, "Mb", "b", M, ref.validity(None, 0, Nc, bad), track, 2, 10)
