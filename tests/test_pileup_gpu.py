"""Pileups on the GPU (csrc/pileup.hip): ``hh_pileup_pixels``
against the dense restatement (tests/pileup_ref.py) -- exactly where every
product, quotient and sum is exact in fp64, and with the same chunked
association otherwise, next to a bound derived from the number of terms --
then ``run_Pileup`` on a chromosome with planted loops, through the
traditional (balanced) path, the haplotype (raw) path and a boundary file."""
import functools
import os

import numpy as np
import pytest

from hichap_master_amd import _lib, coolio, h5
from hichap_master_amd import pileup as pu
from hichap_master_amd._lib import HipLibraryError, ptr
from hichap_master_amd.StructureFind import StructureFind, py2_float_str
from tests import pileup_ref as ref
from tests.knobs import tuned

pytestmark = pytest.mark.gpu

RES = 10000
N = 300                                       # the table of test_saddle_gpu.py
LO, NB = 11, 11 + N + 9                       # 'a' 11 bins, 'b' N bins (queried), 'c' 9 bins
INVALID = [0, N - 1, 90, 91, 92, 93, 150]     # both ends, a run of 4, a single bin
EMPTY_ROW = 40                                # a bin with no pixels at all
HH_ERR_ARG = -1
CHUNK, DEFAULT_CHUNK = 16, 64                 # HH_PILEUP_CHUNK
N_EXP = 200                                   # n_expected < N: far cells are cut
U53 = 2.0 ** -53
KINDS_EXACT = ["exact_nan", "exact_bad", "raw_bad"]
KINDS_GENERAL = ["general_nan", "general_bad"]


@pytest.fixture(autouse=True)
def small_chunk():
    """16 features per chunk: ten chunks, the last one partial, lie inside the
    list of 150 features."""
    with tuned(pileup_chunk=CHUNK):
        yield


@functools.lru_cache(maxsize=None)
def _table():
    """Sorted upper-triangle pixel table of the three chromosomes, counts in
    1/64: dense near the diagonal of 'b', sparse far from it, trans pixels
    into 'b' (bin1 < LO) and out of it (bin2 >= LO + N)."""
    rng = np.random.default_rng(2025)
    i, j = np.indices((NB, NB))
    H = np.triu(rng.integers(1, 4000, (NB, NB)) * (rng.random((NB, NB)) < np.where(j - i < 140, 0.7, 0.15)))
    H[LO + EMPTY_ROW, :] = 0
    H[:, LO + EMPTY_ROW] = 0
    H[LO + 2, LO + N - 3] = 77
    assert np.count_nonzero(H[:LO, LO:LO + N]) > 20 and np.count_nonzero(H[LO:LO + N, LO + N:]) > 20
    b1, b2 = np.nonzero(H)
    cnt = H[b1, b2] / 64.0
    for a in (b1, b2, cnt):
        a.setflags(write=False)
    return b1.astype(np.int64), b2.astype(np.int64), cnt


def _weights(kind):
    """Global weights (None for 'raw') and the 'bad' list of chromosome 'b'.
    exact: powers of two, so every product of the k/64 counts is exact."""
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
def _dense(kind):
    w, bad = _weights(kind)
    M = ref.dense(*_table(), w, LO, N)
    valid = ref.validity(w, LO, N, bad)
    M.setflags(write=False)
    valid.setflags(write=False)
    return M, valid


@functools.lru_cache(maxsize=None)
def _features():
    """150 features in a fixed shuffled order: far loops, near-diagonal loops
    (their windows cross the diagonal at f >= 10), on-diagonal features,
    centres at the ends and at the corner (0, N - 1), centres on and next to
    invalid bins and on the empty row, and three exact repeats."""
    rng = np.random.default_rng(77)
    F = []
    for lo_d, hi_d, n in ((130, 290, 24), (21, 126, 30), (1, 21, 36)):
        d = rng.integers(lo_d, hi_d, n)
        r = (rng.random(n) * (N - d)).astype(np.int64)
        F += list(zip(r.tolist(), (r + d).tolist()))
    F += [(int(x), int(x)) for x in rng.integers(0, N, 22)]
    F += [(0, 0), (N - 1, N - 1), (0, N - 1), (0, 5), (3, N - 2), (N - 4, N - 1), (2, 2), (N - 3, N - 3),
          (1, N - 2), (5, N - 6), (8, 12), (N - 9, N - 1)]
    F += [(90, 90), (89, 94), (91, 150), (150, 150), (149, 151), (93, 200), (94, 94), (88, 152),
          (EMPTY_ROW, EMPTY_ROW), (EMPTY_ROW, 100), (10, EMPTY_ROW), (EMPTY_ROW - 1, EMPTY_ROW + 1),
          (EMPTY_ROW, EMPTY_ROW + 3)]
    F += [(60, 60), (60, 61), (100, 230), (120, 120), (200, 207), (250, 299), (30, 130), (17, 17), (210, 260),
          (275, 280)]
    F += [F[0], F[30], F[95]]                 # three exact repeats
    F = [F[k] for k in rng.permutation(len(F))]
    assert len(F) == 150 and len(F) % CHUNK != 0 and len(set(F)) <= 147
    row = np.array([a for a, _ in F], np.int32)
    col = np.array([b for _, b in F], np.int32)
    assert (row <= col).all() and row.min() == 0 and col.max() == N - 1
    row.setflags(write=False)
    col.setflags(write=False)
    return row, col


def _expected_vector(kind, use):
    """None, or N_EXP entries with a zero and two NaN: powers of two for the
    exact kinds, random positive values otherwise."""
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
def _want(kind, f, use_e, min_dist, chunk=CHUNK, order=None):
    row, col = _features()
    if order is not None:
        row, col = row[list(order)], col[list(order)]
    out = ref.pileup_sums(*_dense(kind), row, col, f, _expected_vector(kind, use_e), min_dist, chunk)
    for a in out:
        a.setflags(write=False)
    return out


def _dev(*arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.array(a)).cuda() for a in arrays]


def _pileup(kind, f, use_e, min_dist, device=False, order=None):
    b1, b2, cnt = _table()
    w, bad = _weights(kind)
    row, col = _features()
    if order is not None:
        row, col = row[list(order)], col[list(order)]
    e = _expected_vector(kind, use_e)
    if device:
        b1, b2, cnt, w, bad, row, col, e = _dev(b1, b2, cnt, w, bad, row, col, e)
    S, Cn = pu.pileup_pixels(b1, b2, cnt, w, LO, N, row, col, f, e, min_dist, bad)
    if device:
        assert S.is_cuda and Cn.is_cuda
        S, Cn = S.cpu().numpy(), Cn.cpu().numpy()
    W = 2 * f + 1
    assert S.dtype == np.float64 and Cn.dtype == np.int64 and S.shape == Cn.shape == (W, W)
    return S, Cn


def _census(kind, f, use_e, min_dist):
    """What the reference input exercises, counted on the dense matrix: cells
    left ineligible by each of the four reasons, and stored contributing
    pixels in the upper (j >= i) and the mirrored (j < i) part."""
    M, valid = _dense(kind)
    row, col = _features()
    e = _expected_vector(kind, use_e)
    u = np.arange(2 * f + 1)
    i = row[:, None, None].astype(np.int64) - f + u[None, :, None] + 0 * u[None, None, :]
    j = col[:, None, None].astype(np.int64) - f + u[None, None, :] + 0 * u[None, :, None]
    inside = (i >= 0) & (i < N) & (j >= 0) & (j < N)
    ic, jc = np.clip(i, 0, N - 1), np.clip(j, 0, N - 1)
    ok_valid = valid[ic] & valid[jc]
    d = np.abs(ic - jc)
    ok_dist = d >= min_dist
    ok_e = np.ones(d.shape, bool)
    if e is not None:
        x = e[np.minimum(d, N_EXP - 1)]
        ok_e = (d < N_EXP) & np.isfinite(x) & (x > 0)
    elig = inside & ok_valid & ok_dist & ok_e
    stored = elig & (M[ic, jc] != 0)
    return dict(off=int((~inside).sum()), invalid=int((inside & ~ok_valid).sum()),
                near=int((inside & ok_valid & ~ok_dist).sum()),
                unusable=int((inside & ok_valid & ok_dist & ~ok_e).sum()),
                upper=int((stored & (j >= i)).sum()), mirrored=int((stored & (j < i)).sum()), elig=elig)


def test_reference_is_not_vacuous():
    c = _census("exact_nan", 10, True, 2)
    assert min(c["off"], c["invalid"], c["near"], c["unusable"]) > 50, c
    assert c["upper"] > 1000 and c["mirrored"] > 1000
    for use_e in (False, True):
        for min_dist in (0, 2, 25):
            S, Cn = _want("exact_nan", 10, use_e, min_dist)
            assert Cn.min() > 0 and (S > 0).all()
            assert np.array_equal(Cn, _census("exact_nan", 10, use_e, min_dist)["elig"].sum(0))
    c = _census("general_bad", 40, False, 0)
    assert c["mirrored"] > 1000 and c["upper"] > 1000 and c["off"] > 1000


# ------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("kind", KINDS_EXACT)
@pytest.mark.parametrize("min_dist", [0, 2, 25])
@pytest.mark.parametrize("use_e", [False, True])
@pytest.mark.parametrize("f", [0, 1, 10, 40, 63])
def test_exact(kind, f, use_e, min_dist):
    S, Cn = _want(kind, f, use_e, min_dist)
    assert Cn.sum() > 0 and S.sum() > 0
    got_S, got_Cn = _pileup(kind, f, use_e, min_dist)
    assert np.array_equal(got_Cn, Cn)
    assert np.array_equal(got_S, S)


# -------------------------------------------------- 2. random positive weights
def _rtol(m):
    """Both sides sum the same m non-negative IEEE terms in different orders;
    either sum is within m * 2^-53 (relative) of the true one, so the two are
    within 2 (m + 2) 2^-53 of each other (§4m's bound).  Derived from the
    input, not measured."""
    return 2.0 * (m + 2) * U53


@pytest.mark.parametrize("kind", KINDS_GENERAL)
@pytest.mark.parametrize("f,use_e,min_dist", [(10, True, 2), (10, False, 0), (40, True, 0), (63, False, 2), (1, True, 25)])
def test_general(kind, f, use_e, min_dist):
    S, Cn = _want(kind, f, use_e, min_dist)
    S1, Cn1 = _want(kind, f, use_e, min_dist, chunk=1 << 20)          # one chunk: plain ascending k
    assert np.array_equal(Cn1, Cn)
    for device in (False, True):
        got_S, got_Cn = _pileup(kind, f, use_e, min_dist, device)
        assert np.array_equal(got_Cn, Cn)
        err = np.abs(got_S - S1)
        bound = _rtol(Cn) * np.abs(S1)
        print(f"{kind} f={f} expected={use_e} min_dist={min_dist}: max error / bound "
              f"{(err / np.where(bound > 0, bound, 1.0)).max():.3g}, cells differing from the chunked restatement "
              f"{int((got_S != S).sum())}")
        assert (err <= bound).all()
        assert np.array_equal(got_S, S)                               # the same association: the same bits


# ----------------------------------------------------------------- 3. bitwise
def test_bitwise():
    kind, f = "general_nan", 40
    S1, C1 = _pileup(kind, f, True, 2)
    S2, C2 = _pileup(kind, f, True, 2)
    S3, C3 = _pileup(kind, f, True, 2, device=True)
    assert S1.tobytes() == S2.tobytes() == S3.tobytes()               # two calls; host form = device form
    assert C1.tobytes() == C2.tobytes() == C3.tobytes()
    order = tuple(np.random.default_rng(1).permutation(150).tolist())
    for kind in ("exact_nan", "raw_bad"):                             # exact terms: any association, any order
        S1, C1 = _pileup(kind, f, True, 2)
        Sp, Cp = _pileup(kind, f, True, 2, order=order)
        assert Sp.tobytes() == S1.tobytes() and Cp.tobytes() == C1.tobytes()
        with tuned(pileup_chunk=DEFAULT_CHUNK):
            S4, C4 = _pileup(kind, f, True, 2)
        assert S4.tobytes() == S1.tobytes() and C4.tobytes() == C1.tobytes()
    # general terms at the default chunk: the restatement's association with chunk 64
    with tuned(pileup_chunk=DEFAULT_CHUNK):
        S5, C5 = _pileup("general_bad", 10, True, 0)
    want = _want("general_bad", 10, True, 0, chunk=DEFAULT_CHUNK)
    assert np.array_equal(S5, want[0]) and np.array_equal(C5, want[1])
    with pytest.raises(HipLibraryError, match="pileup_chunk"), tuned(pileup_chunk=DEFAULT_CHUNK + 1):
        pass
    with pytest.raises(HipLibraryError, match="pileup_chunk"), tuned(pileup_chunk=0):
        pass
    with tuned(pileup_chunk=1):                                       # one feature per chunk
        S6, C6 = _pileup("general_bad", 10, True, 0)
    want = _want("general_bad", 10, True, 0, chunk=1)
    assert np.array_equal(S6, want[0]) and np.array_equal(C6, want[1])


# ------------------------------------------------------------------- 4. edges
def test_no_features_and_no_pixels():
    b1, b2, cnt = _table()
    w, bad = _weights("exact_nan")
    none = (np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0))
    row, col = _features()
    e = _expected_vector("exact_nan", True)
    for device in (False, True):
        t = _dev(b1, b2, cnt, w, e, row, col, *none) if device else (b1, b2, cnt, w, e, row, col, *none)
        tb1, tb2, tc, tw, te, trow, tcol, n1, n2, nc = t
        S, Cn = pu.pileup_pixels(tb1, tb2, tc, tw, LO, N, trow[:0], tcol[:0], 10, te, 2)      # M = 0
        S0, Cn0 = pu.pileup_pixels(n1, n2, nc, tw, LO, N, trow, tcol, 10, te, 2)              # nnz = 0
        if device:
            S, Cn, S0, Cn0 = (x.cpu().numpy() for x in (S, Cn, S0, Cn0))
        assert S.shape == (21, 21) and not S.any() and not Cn.any()
        assert not S0.any() and np.array_equal(Cn0, _want("exact_nan", 10, True, 2)[1])


def test_whole_table_and_one_bin():
    b1, b2, cnt = _table()                    # the three chromosomes as one: lo = 0, N = NB, no weights
    M = ref.dense(b1, b2, cnt, None, 0, NB)
    row, col = _features()
    row, col = np.concatenate([row, [0, NB - 1]]).astype(np.int32), np.concatenate([col, [NB - 1, NB - 1]]).astype(np.int32)
    S, Cn = pu.pileup_pixels(b1, b2, cnt, None, 0, NB, row, col, 10)
    want = ref.pileup_sums(M, np.ones(NB, bool), row, col, 10, None, 0, CHUNK)
    assert np.array_equal(S, want[0]) and np.array_equal(Cn, want[1])
    # chromosomes of 1, 1 and 1 bins; the middle one is queried
    b1 = np.array([0, 0, 1, 1, 2], np.int64)
    b2 = np.array([0, 1, 1, 2, 2], np.int64)
    cnt = np.array([3.0, 5.0, 7.0, 11.0, 13.0])
    z = np.zeros(3, np.int32)
    S, Cn = pu.pileup_pixels(b1, b2, cnt, None, 1, 1, z, z, 0)
    assert S.tolist() == [[21.0]] and Cn.tolist() == [[3]]
    S, Cn = pu.pileup_pixels(b1, b2, cnt, np.array([1.0, 0.5, 1.0]), 1, 1, z[:1], z[:1], 0, np.array([0.25]))
    assert S.tolist() == [[7.0]] and Cn.tolist() == [[1]]
    S, Cn = pu.pileup_pixels(b1, b2, cnt, None, 1, 1, z[:1], z[:1], 0, None, 1)               # min_dist cuts d = 0
    assert S.tolist() == [[0.0]] and Cn.tolist() == [[0]]
    S, Cn = pu.pileup_pixels(b1, b2, cnt, None, 1, 1, z[:1], z[:1], 2)                        # the window leaves it
    assert S[2, 2] == 7.0 and S.sum() == 7.0 and Cn.sum() == 1


def test_every_bin_invalid():
    b1, b2, cnt = _table()
    row, col = _features()
    S, Cn = pu.pileup_pixels(b1, b2, cnt, None, LO, N, row, col, 10, None, 0, np.ones(N, np.uint8))
    assert not S.any() and not Cn.any()
    S, Cn = pu.pileup_pixels(b1, b2, cnt, np.full(NB, np.nan), LO, N, row, col, 10)
    assert not S.any() and not Cn.any()
    S, Cn = pu.pileup_pixels(b1, b2, cnt, None, LO, N, row, col, 10, np.full(N, np.nan))      # no usable expected
    assert not S.any() and not Cn.any()


# ------------------------------------------------------------------ 5. errors
def test_argument_errors_leave_outputs_untouched():
    b1, b2, cnt = _table()
    w = _weights("exact_nan")[0]
    row, col = _features()
    e = _expected_vector("exact_nan", True)
    lib = _lib.load()
    S, Cn = np.full((127, 127), -7.5), np.full((127, 127), -3, np.int64)

    def run(N_=N, f=10, min_dist=0, n_weight=NB, n_exp=N_EXP, row_=row, col_=col, ex=e):
        return lib.hh_pileup_pixels(ptr(b1), ptr(b2), ptr(cnt), b1.size, ptr(w), n_weight, LO, N_, None, ptr(row_),
                                    ptr(col_), row_.size, f, ptr(ex), n_exp, min_dist, ptr(S), ptr(Cn), 0, None)

    assert run(N_=0) == HH_ERR_ARG                                                           # N < 1
    assert run(f=-1) == HH_ERR_ARG and run(f=64) == HH_ERR_ARG                               # flank
    assert b"flank" in lib.hh_last_error()
    assert run(min_dist=-1) == HH_ERR_ARG                                                    # min_dist
    assert b"min_dist" in lib.hh_last_error()
    assert run(n_exp=0) == HH_ERR_ARG and run(n_exp=N + 1) == HH_ERR_ARG                     # n_expected
    assert b"n_expected" in lib.hh_last_error()
    assert run(n_exp=0, ex=None) == 0                                                        # (ignored without one)
    S[:], Cn[:] = -7.5, -3
    for k, (r, c) in ((0, (5, 4)), (149, (-1, 3)), (70, (10, N)), (33, (N, N))):             # a bad feature
        r2, c2 = row.copy(), col.copy()
        r2[k], c2[k] = r, c
        assert run(row_=r2, col_=c2) == HH_ERR_ARG, (r, c)
        assert b"feature" in lib.hh_last_error()
    assert run(n_weight=LO + N - 1) == HH_ERR_ARG                                            # weights
    assert b"weights do not cover" in lib.hh_last_error()
    assert np.all(S == -7.5) and np.all(Cn == -3)
    import torch                                                                             # the device form too
    tb1, tb2, tc, tw, te = _dev(b1, b2, cnt, w, e)
    tS, tCn = torch.full((21, 21), -7.5, dtype=torch.float64).cuda(), torch.full((21, 21), -3).cuda()
    for r, c in ((5, 4), (-1, 3), (10, N)):
        r2, c2 = row.copy(), col.copy()
        r2[100], c2[100] = r, c
        tr, tcl = _dev(r2, c2)
        assert lib.hh_pileup_pixels(ptr(tb1), ptr(tb2), ptr(tc), b1.size, ptr(tw), NB, LO, N, None, ptr(tr), ptr(tcl),
                                    150, 10, ptr(te), N_EXP, 0, ptr(tS), ptr(tCn), 1, None) == HH_ERR_ARG
        assert b"feature" in lib.hh_last_error()
    assert bool((tS == -7.5).all()) and bool((tCn == -3).all())
    with pytest.raises(HipLibraryError, match="flank"):
        pu.pileup_pixels(b1, b2, cnt, w, LO, N, row, col, 64)
    # the library is still usable, and only the W x W head of the outputs is written
    assert run(f=10, min_dist=2) == 0
    want = _want("exact_nan", 10, True, 2)
    assert np.array_equal(S.ravel()[:441].reshape(21, 21), want[0])
    assert np.array_equal(Cn.ravel()[:441].reshape(21, 21), want[1])
    assert np.all(S.ravel()[441:] == -7.5) and np.all(Cn.ravel()[441:] == -3)


# ------------------------------------------------------- 6, 7, 8. run_Pileup
def _planted(seed=3, Nc=400, n_loops=20):
    """A chromosome whose balanced matrix is a distance decay 2e5 / (d + 1)
    with ``n_loops`` single-pixel loops of 8 x the background at distances
    15..60: counts = round(balanced / (w_a w_b)), weights in [0.5, 2) with
    four NaN away from the loops.  Returns (bin1, bin2, count, weight,
    (rows, cols))."""
    rng = np.random.default_rng(seed)
    rows = np.sort(rng.choice(np.arange(30, Nc - 100, 12), n_loops, replace=False))
    cols = rows + rng.integers(15, 61, n_loops)
    a, b = np.nonzero(np.triu(np.ones((Nc, Nc))))
    bal = 2e5 / (b - a + 1.0)
    loop = np.zeros((Nc, Nc), bool)
    loop[rows, cols] = True
    bal[loop[a, b]] *= 8.0
    weight = rng.uniform(0.5, 2.0, Nc)
    count = np.rint(bal / (weight[a] * weight[b])).astype(np.int64)
    weight[[3, 7, Nc - 5, Nc - 2]] = np.nan
    return a.astype(np.int64), b.astype(np.int64), count, weight, (rows, cols)


def _read(out):
    prefix = os.path.basename(out)
    res = StructureFind.properU(RES)
    return [[ln.rstrip("\n").split("\t") for ln in open(os.path.join(out, f"{prefix}_{what}_{res}.txt"))]
            for what in ("Pileup", "PileupCount", "APA")]


def _check_files(r, out):
    pil, cnt, apa = _read(out)
    assert pil == [[py2_float_str(x) for x in row] for row in r["pileup"]]
    assert cnt == [[str(int(x)) for x in row] for row in r["Cn"]]
    want = [[k, py2_float_str(r["apa"][k])] for k in pu.APA_NAMES] + [["n_features", str(r["n_features"])]]
    if "apa_ratio" in r:
        want += [[k + "_over_controls", py2_float_str(r["apa_ratio"][k])] for k in pu.APA_NAMES]
    assert apa == want
    got = np.array([[float(x) for x in row] for row in pil])            # '%.12g' rounds to 5e-12 (relative)
    np.testing.assert_allclose(got, r["pileup"], rtol=5e-12, atol=0, equal_nan=True)


def _check_sums(r, chrom, M, valid, f, dmin):
    """The call's sums against the restatement fed with the call's own
    expected and features: the same association, so the same bits."""
    rc = r["chroms"][chrom]
    S, Cn = ref.pileup_sums(M, valid, rc["row"], rc["col"], f, rc["expected"], dmin, CHUNK)
    assert np.array_equal(rc["Cn"], Cn) and np.array_equal(rc["S"], S)
    assert np.array_equal(r["Cn"], Cn) and np.array_equal(r["S"], S)
    with np.errstate(invalid="ignore", divide="ignore"):
        np.testing.assert_array_equal(r["pileup"], np.where(Cn > 0, S / Cn, np.nan))


def test_run_pileup_traditional(tmp_path):
    b1, b2, count, weight, (rows, cols) = _planted()
    Nc = weight.size
    path = str(tmp_path / "trad.cool")
    coolio.create_cooler(path, {RES: ([("chr1", Nc * RES)], b1, b2, count)})
    h5.append_dataset(path, f"{RES}/bins", "weight", weight)
    out = str(tmp_path / "planted")
    sf = StructureFind(path, Res=RES)
    # pos1 > pos2 for every other loop (swapped back), positions inside their bins (floored)
    p1, p2 = rows * RES + 123, cols * RES + RES - 1
    p1[::2], p2[::2] = p2[::2].copy(), p1[::2].copy()
    r = sf.run_Pileup(out, features={"chr1": (p1, p2)}, flank=5 * RES, n_shifts=5, seed=4)
    assert r is sf.Pileup_dict and r["flank"] == 5 and r["n_features"] == rows.size
    rc = r["chroms"]["chr1"]
    assert np.array_equal(rc["row"], rows) and np.array_equal(rc["col"], cols)
    M = ref.dense(b1, b2, count, weight, 0, Nc)
    valid = ref.validity(weight, 0, Nc, None)
    _check_sums(r, "chr1", M, valid, 5, 2)
    _check_files(r, out)
    P = r["pileup"]
    print("traditional: apa", r["apa"], "controls", pu.apa_scores(r["pileup_c"]), "ratio", r["apa_ratio"])
    assert np.nanargmax(P) == 5 * 11 + 5 and 6.0 < P[5, 5] < 10.0          # the centre is the maximum: ~8 x expected
    assert r["apa"]["P2LL"] > 1 and r["apa"]["P2M"] > 1
    # the controls: the same distances away from the loops, a flat pileup
    assert r["n_controls"] == rc["row_c"].size > 50
    Sc, Cc = ref.pileup_sums(M, valid, rc["row_c"], rc["col_c"], 5, rc["expected"], 2, CHUNK)
    assert np.array_equal(r["S_c"], Sc) and np.array_equal(r["Cn_c"], Cc)
    assert 0.5 < pu.apa_scores(r["pileup_c"])["P2LL"] < 2.0
    assert r["apa_ratio"]["P2LL"] > 1
    # a loop file and distances in bp: the same features through run_Loops' format, observed only
    lf = str(tmp_path / "loops.txt")
    with open(lf, "w") as f:
        f.write("chromLabel\tloc_1\tloc_2\tIF\n")
        for a, b in zip(rows, cols):
            f.write(f"chr1\t{a * RES}\t{b * RES}\t1.0\n")
    out2 = str(tmp_path / "observed")
    r2 = sf.run_Pileup(out2, loop_file=lf, flank=3 * RES, expected=False, min_dist=4 * RES)
    assert r2["flank"] == 3 and "pileup_c" not in r2 and r2["chroms"]["chr1"]["expected"] is None
    _check_sums(r2, "chr1", M, valid, 3, 4)
    _check_files(r2, out2)
    assert np.nanargmax(r2["pileup"]) == 3 * 7 + 3


def test_run_pileup_haplotype(tmp_path):
    """The planted chromosome as the maternal haplotype 'Mb' (raw counts, no
    weights), the NaN-weight bins as its gap list, next to a paternal 'Pb'
    that must not be read; the features are named 'b'."""
    b1, b2, count, weight, (rows, cols) = _planted()
    Nc = weight.size
    gap = np.nonzero(~np.isfinite(weight))[0]
    pb = Nc + np.arange(30)
    path = str(tmp_path / "hap.cool")
    coolio.create_cooler(path, {RES: ([("Mb", Nc * RES), ("Pb", 30 * RES)], np.concatenate([b1, pb]),
                                      np.concatenate([b2, pb]), np.concatenate([count, np.full(30, 9)]))})
    out = str(tmp_path / "hap")
    sf = StructureFind(path, Res=RES, Allelic="Maternal", GapFile={str(RES): {"Mb": gap, "Pb": np.array([0])}})
    with pytest.raises(ValueError, match="Mb"):
        sf.run_Pileup(out, features={"Mb": (rows * RES, cols * RES)}, flank=5 * RES)          # names carry no prefix
    r = sf.run_Pileup(out, features={"b": (rows * RES, cols * RES)}, flank=5 * RES)
    bad = np.zeros(Nc, np.uint8)
    bad[gap] = 1
    M = ref.dense(b1, b2, count, None, 0, Nc)
    assert list(r["chroms"]) == ["Mb"]
    _check_sums(r, "Mb", M, ref.validity(None, 0, Nc, bad), 5, 2)
    _check_files(r, out)
    assert r["Cn"].max() == rows.size and r["apa"]["peak"] > 0


def test_run_pileup_boundary_file(tmp_path):
    b1, b2, count, weight, _ = _planted()
    Nc = weight.size
    path = str(tmp_path / "trad.cool")
    coolio.create_cooler(path, {RES: ([("chr1", Nc * RES)], b1, b2, count)})
    h5.append_dataset(path, f"{RES}/bins", "weight", weight)
    bins = [2, 40, 41, 150, 151, 152, 290, Nc - 3]
    bf = str(tmp_path / "x_Filtered_Boundary_10K.txt")
    with open(bf, "w") as f:
        for b in bins:
            f.write(f"chr1\t{b * RES}\n")
    out = str(tmp_path / "bnd")
    r = StructureFind(path, Res=RES).run_Pileup(out, boundary_file=bf, flank=12 * RES)
    rc = r["chroms"]["chr1"]
    assert rc["row"].tolist() == bins and rc["col"].tolist() == bins and r["flank"] == 12
    _check_sums(r, "chr1", ref.dense(b1, b2, count, weight, 0, Nc), ref.validity(weight, 0, Nc, None), 12, 2)
    _check_files(r, out)
    assert r["S"].tobytes() == r["S"].T.copy().tobytes() and np.array_equal(r["Cn"], r["Cn"].T)
    assert r["Cn"][12, 12] == 0 and r["Cn"][12, 14] == len(bins)          # d < ignore_diags is left out
