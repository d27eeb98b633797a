"""Trans block sums and trans saddle on the GPU (csrc/trans.hip, DESIGN.md
§4s): ``hh_trans_blocks`` and ``hh_trans_saddle`` against the dense
restatement (tests/trans_ref.py) for every row chromosome of two genomes --
exactly where every product, quotient and sum is exact in fp64, within a bound
derived from the number of terms otherwise -- then ``run_Trans`` on a planted
four-chromosome cooler, through the traditional (balanced) path and the
haplotype (raw) path."""
import functools
import os

import numpy as np
import pytest

from hichap_master_amd import _lib, coolio, h5
from hichap_master_amd import trans as tr
from hichap_master_amd._lib import HipLibraryError, ptr
from hichap_master_amd.StructureFind import StructureFind, py2_float_str
from tests import saddle_ref
from tests import trans_ref as ref
from tests.knobs import tuned

pytestmark = pytest.mark.gpu

RES = 10000
HH_ERR_ARG = -1
DEFAULT_TRIPS, MAX_TRIPS = 8, 256                # HH_TRANS_TRIPS, HH_TRANS_MAX_TRIPS
U53 = 2.0 ** -53
K = 12

# genome A: a 1-bin chromosome, nothing a multiple of 64
SIZES_A = (11, 130, 1, 70, 9, 40)
BIG = 11                                       # first bin of the 130-bin chromosome
INVALID_A = [BIG + 0, BIG + 129, BIG + 90, BIG + 91, BIG + 92, BIG + 93, 3, 142 + 5]   # both ends, a run of 4
EMPTY_ROW = BIG + 40                           # a bin with no pixels at all
CIS_ONLY_ROW = BIG + 60                        # a row with no trans pixels
# genome B: 130 chromosomes of 1-3 bins: the partner index crosses 64 and 128
SIZES_B = tuple(1 + (7 * i) % 3 for i in range(130))
INVALID_B = [0, 5, 6, 100, 258]


@pytest.fixture(autouse=True)
def small_spans():
    """One trip of 64 pixels per span: about two hundred span edges inside the
    rows of the 130-bin chromosome, and two levels of the tree over the span
    sums (more than 64 spans)."""
    with tuned(trans_trips=1):
        yield


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _genome(name):
    """(off, bin1, bin2, count): the sorted upper-triangle table, counts in
    1/64.  A: cis dense near the diagonal, trans density 0.6 between the first
    two chromosomes (a row's segment into the 130-bin one exceeds 64 pixels),
    about 0.5 in (1, 3), sparse elsewhere, nothing in block (3, 4).  B: 0.4
    everywhere."""
    sizes = SIZES_A if name == "A" else SIZES_B
    off = _offsets(sizes)
    n = int(off[-1])
    rng = np.random.default_rng(2026 if name == "A" else 2027)
    chrom = np.repeat(np.arange(len(sizes)), sizes)
    i, j = np.indices((n, n))
    ci, cj = chrom[i], chrom[j]
    if name == "A":
        dens = np.where(ci == cj, np.where(j - i < 20, 0.8, 0.1), 0.2)
        dens[(ci == 0) & (cj == 1)] = 0.6
        dens[(ci == 1) & (cj == 3)] = 0.5
        dens[(ci == 3) & (cj == 4)] = 0.0
    else:
        dens = np.full((n, n), 0.4)
    H = rng.integers(1, 4000, (n, n))
    stored = np.triu(rng.random((n, n)) < dens)
    if name == "A":
        stored[EMPTY_ROW, :] = False
        stored[:, EMPTY_ROW] = False
        stored[CIS_ONLY_ROW, off[2]:] = False
        assert stored[CIS_ONLY_ROW, CIS_ONLY_ROW:off[2]].sum() > 5
        assert stored[:off[1], off[1]:off[2]].sum(axis=1).max() > 64          # a (row, q) segment of more than 64
        assert not stored[off[3]:off[4], off[4]:off[5]].any()
        assert stored[off[1]:off[2]].sum() > 20 * 64
    b1, b2 = np.nonzero(stored)
    cnt = H[b1, b2] / 64.0
    cnt[::97] = 0.0                               # a stored count of 0 is a pixel
    for a in (off, b1, b2, cnt):
        a.setflags(write=False)
    return off, b1.astype(np.int64), b2.astype(np.int64), cnt


def _weights(name, kind):
    """Global weights, the global 'bad' list and 'use'.  exact: powers of two,
    so every product of the k/64 counts is exact in fp64.  The invalid bins
    come through NaN weights (nan) or through bad (bad); nouse switches
    chromosome 3 off."""
    off = _genome(name)[0]
    n = int(off[-1])
    rng = np.random.default_rng(5)
    w = 2.0 ** rng.integers(-3, 1, n) if kind.startswith("exact") else rng.uniform(0.05, 3.0, n)
    invalid = INVALID_A if name == "A" else INVALID_B
    bad = None
    if "nan" in kind:
        w[invalid] = np.nan
    else:
        bad = np.zeros(n, np.uint8)
        bad[invalid] = 1
    use = None
    if kind.endswith("nouse"):
        use = np.ones(len(off) - 1, np.uint8)
        use[3] = 0
    return w, bad, use


def _classes(name):
    """A global class per bin, 255 for about one bin in ten."""
    n = int(_genome(name)[0][-1])
    rng = np.random.default_rng(K)
    cls = rng.integers(0, K, n).astype(np.uint8)
    cls[rng.random(n) < 0.1] = 255
    cls[BIG + 7] = K - 1                          # the largest id is in use
    return cls


@functools.lru_cache(maxsize=None)
def _want(name, kind, g):
    """The restatement's (sum, npix, expected, U, Cu, Un) for every row
    chromosome at once.  exact: the expected is powers of two with a NaN and a
    zero block; general: the restatement's own expected."""
    off, b1, b2, cnt = _genome(name)
    w, bad, use = _weights(name, kind)
    n, C = int(off[-1]), len(off) - 1
    valid = ref.validity(off, w, use, bad)
    M, stored = ref.dense_upper(b1, b2, cnt, w, n)
    s, npx = ref.block_sums(M, stored, off, valid, g)
    if kind.startswith("exact"):
        e = 2.0 ** np.random.default_rng(8).integers(-2, 3, (C, C)).astype(np.float64)
        e[0, 1], e[1, 4], e[2, 3] = np.nan, 0.0, -1.0
    else:
        e = ref.expected(s, ref.n_valid(off, valid))
    U, Cu, Un = ref.saddle_sums(M, stored, off, valid, e, _classes(name), K)
    out = (s, npx, e, U, Cu, Un)
    for a in out:
        a.setflags(write=False)
    return out


def _dev(*arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.array(a)).cuda() for a in arrays]


def _rows(name, p):
    """The pixel_rows-style slice of chromosome p."""
    off, b1, b2, cnt = _genome(name)
    lo, hi = np.searchsorted(b1, [off[p], off[p + 1]])
    return b1[lo:hi], b2[lo:hi], cnt[lo:hi]


def _blocks(name, kind, p, g, device=False, rows=False):
    off, b1, b2, cnt = _genome(name)
    if rows:
        b1, b2, cnt = _rows(name, p)
    w, bad, use = _weights(name, kind)
    if device:
        b1, b2, cnt, w, bad = _dev(b1, b2, cnt, w, bad)
    s, n = tr.trans_blocks_pixels(b1, b2, cnt, w, off, p, g, use, bad)
    if device:
        assert s.is_cuda and n.is_cuda
        s, n = s.cpu().numpy(), n.cpu().numpy()
    assert s.dtype == np.float64 and n.dtype == np.int64 and s.shape == n.shape == (len(off) - 1,)
    return s, n


def _saddle(name, kind, p, e, device=False, rows=False):
    off, b1, b2, cnt = _genome(name)
    if rows:
        b1, b2, cnt = _rows(name, p)
    w, bad, use = _weights(name, kind)
    cls = _classes(name)
    if device:
        b1, b2, cnt, w, bad, e, cls = _dev(b1, b2, cnt, w, bad, e, cls)
    U = tr.trans_saddle_pixels(b1, b2, cnt, w, off, p, e, cls, K, use, bad)
    if device:
        assert U.is_cuda
        U = U.cpu().numpy()
    assert U.dtype == np.float64 and U.shape == (K, K)
    return U


def _rtol(m):
    """Both sides sum the same m IEEE terms of one sign in different orders;
    either sum is within m * 2^-53 (relative) of the true one, so the two are
    within 2 (m + 2) 2^-53 of each other.  Derived from the input, not measured."""
    return 2.0 * (int(m) + 2) * U53


CASES = [("A", "nan"), ("A", "bad"), ("A", "nan_nouse"), ("B", "nan"), ("B", "bad")]


# ------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("name,kind", CASES)
@pytest.mark.parametrize("g", [0, 2])
def test_exact_for_every_row_chromosome(name, kind, g):
    kind = "exact_" + kind
    s, n, e, U, Cu, Un = _want(name, kind, g)
    C = len(s)
    assert n.sum() > 0 and Un.sum() > 0 and not np.tril(n, -1).any()
    if name == "A":
        assert n[3, 4] == 0 and n[0, 1] > 64 * 11 * 0.4
    if kind.endswith("nouse"):
        assert not n[3].any() and not n[:, 3].any() and not Un[3].any()
    for p in range(C):                                     # the last one too: only its cis cell is set
        for device in (False, True):
            got_s, got_n = _blocks(name, kind, p, g, device)
            assert np.array_equal(got_n, n[p]), p
            assert np.array_equal(got_s, s[p]), p
            if g == 0:
                got_U = _saddle(name, kind, p, e[p], device)
                assert np.array_equal(got_U, U[p]), p
    assert not n[C - 1, :C - 1].any() and not Un[C - 1].any()


def test_exact_at_other_span_lengths():
    for trips in (3, DEFAULT_TRIPS, MAX_TRIPS):
        with tuned(trans_trips=trips):
            for name, p in (("A", 0), ("A", 1), ("A", 3), ("B", 64)):
                s, n, e, U, _, _ = _want(name, "exact_nan", 2)
                got_s, got_n = _blocks(name, "exact_nan", p, 2)
                assert np.array_equal(got_n, n[p]) and np.array_equal(got_s, s[p])
                assert np.array_equal(_saddle(name, "exact_nan", p, e[p]), U[p])


# -------------------------------------------------- 2. random positive weights
@pytest.mark.parametrize("name,kind", CASES)
def test_general_for_every_row_chromosome(name, kind):
    kind, g = "general_" + kind, 2
    s, n, e, U, Cu, Un = _want(name, kind, g)
    worst = 0.0
    for p in range(len(s)):
        rs, ru = _rtol(n[p].max()), _rtol(Un[p].max())
        for device in (False, True):
            got_s, got_n = _blocks(name, kind, p, g, device)
            got_U = _saddle(name, kind, p, e[p], device)
            assert np.array_equal(got_n, n[p]), p
            err_s = (np.abs(got_s - s[p]) / np.where(s[p] > 0, s[p], 1.0)).max()
            err_u = (np.abs(got_U - U[p]) / np.where(U[p] > 0, U[p], 1.0)).max()
            worst = max(worst, err_s / rs, err_u / ru)
            np.testing.assert_allclose(got_s, s[p], rtol=rs, atol=0, err_msg=f"p={p}")
            np.testing.assert_allclose(got_U, U[p], rtol=ru, atol=0, err_msg=f"p={p}")
    print(f"{name} {kind}: worst error / bound {worst:.3g}; largest sums of {n.max()} and {Un.max()} terms")


# ----------------------------------------------------------------- 3. bitwise
@pytest.mark.parametrize("name,p", [("A", 0), ("A", 1), ("A", 3), ("B", 17), ("B", 129)])
def test_bitwise(name, p):
    kind, g = "general_nan", 2
    e = _want(name, kind, g)[2][p]
    s1, n1 = _blocks(name, kind, p, g)
    s2, n2 = _blocks(name, kind, p, g)
    s3, n3 = _blocks(name, kind, p, g, device=True)
    s4, n4 = _blocks(name, kind, p, g, rows=True)
    s5, n5 = _blocks(name, kind, p, g, device=True, rows=True)
    # two calls; host form = device form; the whole table = the rows of p alone
    assert s1.tobytes() == s2.tobytes() == s3.tobytes() == s4.tobytes() == s5.tobytes()
    assert n1.tobytes() == n2.tobytes() == n3.tobytes() == n4.tobytes() == n5.tobytes()
    U = [_saddle(name, kind, p, e), _saddle(name, kind, p, e), _saddle(name, kind, p, e, device=True),
         _saddle(name, kind, p, e, rows=True), _saddle(name, kind, p, e, device=True, rows=True)]
    assert all(u.tobytes() == U[0].tobytes() for u in U)
    # trans_trips regroups the block sums (last bits, the header says so): held to the bound,
    # npix to equality; no key touches the saddle sums: the same bits
    for trips in (2, DEFAULT_TRIPS, MAX_TRIPS):
        with tuned(trans_trips=trips):
            s6, n6 = _blocks(name, kind, p, g)
            U6 = _saddle(name, kind, p, e)
        assert np.array_equal(n6, n1) and U6.tobytes() == U[0].tobytes()
        np.testing.assert_allclose(s6, s1, rtol=_rtol(n1.max()), atol=0)


# ------------------------------------------------------------------- 4. edges
def test_no_pixels():
    off = _genome("A")[0]
    none = (np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0))
    w, bad, use = _weights("A", "exact_nan")
    e, cls = np.ones(len(off) - 1), _classes("A")
    for device in (False, True):
        b1, b2, cnt, wt, ex, cl = _dev(*none, w, e, cls) if device else (*none, w, e, cls)
        s, n = tr.trans_blocks_pixels(b1, b2, cnt, wt, off, 1, 2)
        U = tr.trans_saddle_pixels(b1, b2, cnt, wt, off, 1, ex, cl, K)
        if device:
            s, n, U = (t.cpu().numpy() for t in (s, n, U))
        assert s.shape == (6,) and not s.any() and not n.any() and U.shape == (K, K) and not U.any()
    # and a table whose rows of p hold nothing (the empty row as a one-bin "chromosome")
    off2 = np.array([0, EMPTY_ROW, EMPTY_ROW + 1, off[-1]])
    s, n = tr.trans_blocks_pixels(*_genome("A")[1:], w, off2, 1, 0)
    assert not s.any() and not n.any()


def test_single_chromosome_and_every_bin_invalid():
    off, b1, b2, cnt = _genome("A")
    n = int(off[-1])
    s, npx = tr.trans_blocks_pixels(b1, b2, cnt, None, np.array([0, n]), 0, 0)         # C = 1: the whole table is cis
    assert npx.tolist() == [b1.size] and s.tolist() == [float(np.sum(cnt * 64)) / 64]
    s, npx = tr.trans_blocks_pixels(b1, b2, cnt, None, off, 1, 0, bad=np.ones(n, np.uint8))
    assert not s.any() and not npx.any()
    s, npx = tr.trans_blocks_pixels(b1, b2, cnt, np.full(n, np.nan), off, 1, 0)
    assert not s.any() and not npx.any()
    U = tr.trans_saddle_pixels(b1, b2, cnt, None, off, 1, np.ones(6), np.full(n, 255, np.uint8), K)
    assert not U.any()
    U = tr.trans_saddle_pixels(b1, b2, cnt, None, off, 1, np.full(6, np.nan), _classes("A"), K)   # no usable block
    assert not U.any()


def test_argument_errors_leave_outputs_untouched():
    off, b1, b2, cnt = _genome("A")
    n, C = int(off[-1]), len(off) - 1
    w = _weights("A", "exact_nan")[0]
    lib = _lib.load()
    s, npx, U = np.full(600, -7.5), np.full(600, -3, np.int64), np.full((64, 64), -7.5)
    e = np.array(_want("A", "exact_nan", 2)[2][1])
    long_off = np.arange(514, dtype=np.int64)

    def blocks(off_=off, C_=C, p=1, g=2, n_weight=n, bin1=b1):
        return lib.hh_trans_blocks(ptr(bin1), ptr(b2), ptr(cnt), b1.size, ptr(w), n_weight, ptr(off_), C_, None,
                                   None, p, g, ptr(s), ptr(npx), 0, None)

    def saddle(off_=off, C_=C, p=1, K_=K, n_weight=n, cls=None, bin1=b1):
        cls = _classes("A") if cls is None else cls
        return lib.hh_trans_saddle(ptr(bin1), ptr(b2), ptr(cnt), b1.size, ptr(w), n_weight, ptr(off_), C_, None,
                                   None, p, ptr(e), ptr(cls), K_, ptr(U), 0, None)

    for call in (blocks, saddle):
        assert call(C_=0) == HH_ERR_ARG and call(off_=long_off, C_=513) == HH_ERR_ARG          # C outside 1..512
        assert b"C outside" in lib.hh_last_error()
        flat = off.copy()
        flat[3] = flat[2]
        assert call(off_=flat) == HH_ERR_ARG                                                   # not strictly ascending
        assert b"ascending" in lib.hh_last_error()
        assert call(off_=off + 1) == HH_ERR_ARG                                                # not starting at 0
        assert b"start at 0" in lib.hh_last_error()
        assert call(p=-1) == HH_ERR_ARG and call(p=C) == HH_ERR_ARG                            # p outside [0, C)
        assert b"p outside" in lib.hh_last_error()
        assert call(n_weight=n - 1) == HH_ERR_ARG                                              # weights
        assert b"weights do not cover" in lib.hh_last_error()
        assert call(bin1=None) == HH_ERR_ARG                                                   # null pixels, nnz > 0
        assert b"null pixel arrays" in lib.hh_last_error()
    assert blocks(g=-1) == HH_ERR_ARG                                                          # ignore_diags < 0
    assert b"ignore_diags" in lib.hh_last_error()
    assert saddle(K_=1) == HH_ERR_ARG and saddle(K_=65) == HH_ERR_ARG                          # K
    assert b"K outside" in lib.hh_last_error()
    for wrong in (K, 200, 254):                                                                # a class in [K, 254]
        cls = _classes("A")
        cls[n - 2] = wrong
        assert saddle(cls=cls) == HH_ERR_ARG, wrong
        assert b"cls entry" in lib.hh_last_error()
    assert np.all(s == -7.5) and np.all(npx == -3) and np.all(U == -7.5)
    import torch                                                                               # the device form too
    dcls = _classes("A")
    dcls[5] = 100
    tb1, tb2, tc, tw, te, tcls = _dev(b1, b2, cnt, w, e, dcls)
    tU = torch.full((K, K), -7.5, dtype=torch.float64).cuda()
    assert lib.hh_trans_saddle(ptr(tb1), ptr(tb2), ptr(tc), b1.size, ptr(tw), n, ptr(off), C, None, None, 1, ptr(te),
                               ptr(tcls), K, ptr(tU), 1, None) == HH_ERR_ARG
    assert bool((tU == -7.5).all())
    with pytest.raises(HipLibraryError, match="K outside"):
        tr.trans_saddle_pixels(b1, b2, cnt, w, off, 1, e, _classes("A"), 65)
    with pytest.raises(ValueError, match="bad must have one entry per bin of the genome"):
        tr.trans_blocks_pixels(b1, b2, cnt, w, off, 1, bad=np.zeros(130, np.uint8))            # a cis call's bad
    # the library is still usable, and only the heads of the outputs are written
    assert blocks() == 0 and saddle() == 0
    want = _want("A", "exact_nan", 2)
    assert np.array_equal(s[:C], want[0][1]) and np.array_equal(npx[:C], want[1][1])
    assert np.array_equal(U.ravel()[:K * K].reshape(K, K), want[3][1])
    assert np.all(s[C:] == -7.5) and np.all(npx[C:] == -3) and np.all(U.ravel()[K * K:] == -7.5)


# ------------------------------------------------------------- 5, 6. run_Trans
PLANTED = (50, 37, 64, 21)


@functools.lru_cache(maxsize=None)
def _planted():
    """Four chromosomes with a +-1 track in runs of 5-11 bins.  Cis counts
    decay with the distance; every trans cell is stored, 8 between bins of the
    same sign and 2 between bins of opposite signs.  Weights are powers of two
    (every block sum is exact) with five NaN.  Returns (off, bin1, bin2, count,
    weight, track)."""
    rng = np.random.default_rng(7)
    off = _offsets(PLANTED)
    n = int(off[-1])
    sign = np.empty(n)
    at, s = 0, 1.0
    while at < n:
        L = int(rng.integers(5, 12))
        sign[at:at + L] = s
        at, s = at + L, -s
    chrom = np.repeat(np.arange(4), PLANTED)
    a, b = np.nonzero(np.triu(np.ones((n, n))))
    cis = chrom[a] == chrom[b]
    keep = ~cis | (b - a < 25)
    a, b, cis = a[keep], b[keep], cis[keep]
    count = np.where(cis, 100 // (b - a + 1) + 1, np.where(sign[a] == sign[b], 8, 2)).astype(np.int64)
    weight = 2.0 ** rng.integers(-2, 2, n)
    weight[[0, 49, 60, 61, 171]] = np.nan
    track = sign * (1 + rng.random(n))
    return off, a.astype(np.int64), b.astype(np.int64), count, weight, track


def _read(out, saddle=True):
    prefix = os.path.basename(out)
    res = StructureFind.properU(RES)
    kinds = ("TransExpected", "CisTrans") + (("TransSaddle", "TransSaddleStrength") if saddle else ())
    return [[ln.rstrip("\n").split("\t") for ln in open(os.path.join(out, f"{prefix}_{what}_{res}.txt"))]
            for what in kinds]


def _check_run(r, out, shown, off, table, weight, use, bad, track, g, n_bins):
    """``run_Trans``'s arrays and its four files against the restatement.
    The weights are powers of two or absent and the counts integers, so the
    block sums, the totals and the expected (one division of an exact sum by
    an exact integer) are equal to the restatement's; the saddle's terms v /
    expected are then the same IEEE numbers on both sides and only the order
    of the additions differs: U is held to 2 (m + 2) 2^-53, m the largest
    number of terms of a cell."""
    n, C, Kc = int(off[-1]), len(off) - 1, n_bins + 2
    sel = [q for q in range(C) if use is None or use[q]]
    valid = ref.validity(off, weight, use, bad)
    M, stored = ref.dense_upper(*table, weight, n)
    s, npx = ref.block_sums(M, stored, off, valid, g)
    nvb = ref.n_valid(off, valid)
    e = ref.expected(s, nvb)
    cis, trans, frac, genome = ref.totals(s)
    assert r["selected"] == sel and r["n_valid"].tolist() == nvb and np.array_equal(r["valid"] != 0, valid)
    assert np.array_equal(r["npix"], npx) and np.array_equal(r["sum"], s)
    assert np.array_equal(r["expected"], e, equal_nan=True)
    assert r["cis"].tolist() == cis and r["trans"].tolist() == trans and r["genome"] == genome
    assert np.array_equal(r["cis_fraction"], np.array(frac), equal_nan=True)
    cls_sel, edges = saddle_ref.digitize([track[off[q]:off[q + 1]] for q in sel],
                                         [valid[off[q]:off[q + 1]] for q in sel], n_bins, 0.025, 0.975)
    cls = np.full(n, 255, np.uint8)
    for q, c in zip(sel, cls_sel):
        cls[off[q]:off[q + 1]] = c
    assert np.array_equal(r["cls"], cls) and np.array_equal(r["edges"], edges)
    U, Cu, Un = ref.saddle_sums(M, stored, off, valid, e, cls, Kc)
    S, Cn, sad = ref.symmetric(U, Cu)
    bound = _rtol(Un.max())
    assert np.array_equal(r["Cu"], Cu) and np.array_equal(r["C"], Cn)
    np.testing.assert_allclose(r["U"], U, rtol=bound, atol=0)
    np.testing.assert_allclose(r["saddle"], sad, rtol=bound, atol=0, equal_nan=True)
    k_want = saddle_ref.strength(S, Cn)
    bound_k = 2 * (2 * (2 * (n_bins // 2) ** 2 + 1) + 1) * U53          # as tests/test_saddle_gpu.py derives it
    np.testing.assert_allclose(r["strength"], k_want, rtol=2 * bound + bound_k, atol=0)
    print(f"trans saddle strength(k) = {r['strength']}, restatement {k_want}; genome cis fraction {genome[2]:.4f}")
    assert k_want[max(1, n_bins // 5) - 1] > 1 and r["strength"][max(1, n_bins // 5) - 1] > 1
    # the files are the restatement's numbers as Python 2 printed them
    exp, ct, sadf, strf = _read(out)
    assert exp[0] == ["chrom1", "chrom2", "n_valid1", "n_valid2", "n_pixels", "balanced_sum", "balanced_avg"]
    assert exp[1:] == [[shown[p], shown[q], str(nvb[p]), str(nvb[q]), str(npx[p, q]), py2_float_str(s[p, q]),
                        py2_float_str(e[p, q])] for i, p in enumerate(sel) for q in sel[i + 1:]]
    assert ct[0] == ["chrom", "cis_sum", "trans_sum", "cis_fraction"]
    assert ct[1:] == [[shown[p], py2_float_str(cis[p]), py2_float_str(trans[p]), py2_float_str(frac[p])]
                      for p in sel] + [["genome"] + [py2_float_str(x) for x in genome]]
    assert sadf[0] == [py2_float_str(x) for x in edges] and len(sadf) == 1 + Kc
    assert sadf[1:] == [[py2_float_str(x) for x in row] for row in sad]
    assert strf == [["k", "strength"]] + [[str(k + 1), py2_float_str(x)] for k, x in enumerate(k_want)]


def test_run_trans_traditional(tmp_path):
    off, b1, b2, count, weight, track = _planted()
    names = ["chr1", "chr2", "chr3", "chr4"]
    path = str(tmp_path / "trad.cool")
    coolio.create_cooler(path, {RES: ([(x, L * RES) for x, L in zip(names, PLANTED)], b1, b2, count)})
    h5.append_dataset(path, f"{RES}/bins", "weight", weight)
    tracks = {x: track[off[q]:off[q + 1]] for q, x in enumerate(names)}
    sf = StructureFind(path, Res=RES)
    out = str(tmp_path / "planted")
    with pytest.raises(ValueError, match="36 values"):
        sf.run_Trans(out, track=dict(tracks, chr2=tracks["chr2"][:-1]), n_bins=10)
    r = sf.run_Trans(out, track=tracks, n_bins=10, ignore_diags=2)
    assert r is sf.Trans_dict
    _check_run(r, out, names, off, (b1, b2, count), weight, None, None, track, 2, 10)
    # without a track: the first two files only, the same text
    r2 = sf.run_Trans(str(tmp_path / "plain"), ignore_diags=2)
    assert "U" not in r2 and np.array_equal(r2["sum"], r["sum"])
    assert _read(str(tmp_path / "plain"), saddle=False) == _read(out)[:2]
    assert sorted(os.listdir(str(tmp_path / "plain"))) == [f"plain_CisTrans_{StructureFind.properU(RES)}.txt",
                                                           f"plain_TransExpected_{StructureFind.properU(RES)}.txt"]


def test_run_trans_haplotype(tmp_path):
    """The same four chromosomes as the maternal haplotype (raw counts, no
    weights), the NaN-weight bins as their gap lists, next to two paternal
    chromosomes with cis and maternal-paternal pixels that must not be read;
    the track comes from a PC file without prefixes."""
    off, b1, b2, count, weight, track = _planted()
    n = int(off[-1])
    sizes = PLANTED + (13, 8)
    off2 = _offsets(sizes)
    rng = np.random.default_rng(9)
    extra = np.array([(a, b) for a in range(int(off2[-1])) for b in range(max(a, n), int(off2[-1]))
                      if rng.random() < 0.3])
    t1, t2 = np.concatenate([b1, extra[:, 0]]), np.concatenate([b2, extra[:, 1]])
    tc = np.concatenate([count, rng.integers(1, 9, len(extra))])
    o = np.lexsort((t2, t1))
    t1, t2, tc = t1[o], t2[o], tc[o]
    names = ["Ma", "Mb", "Mc", "Md", "Pa", "Pb"]
    path = str(tmp_path / "hap.cool")
    coolio.create_cooler(path, {RES: ([(x, L * RES) for x, L in zip(names, sizes)], t1, t2, tc)})
    gap = np.nonzero(~np.isfinite(weight))[0]
    gaps = {x: gap[(gap >= off2[q]) & (gap < off2[q + 1])] - off2[q] for q, x in enumerate(names)}
    pc = str(tmp_path / "pc.txt")
    with open(pc, "w") as f:
        for q, x in enumerate(names[:4]):
            for v in track[off[q]:off[q + 1]]:
                f.write(f"{x[1:]}\t{float(v)!r}\n")
    out = str(tmp_path / "hap")
    sf = StructureFind(path, Res=RES, Allelic="Maternal", GapFile={str(RES): gaps})
    r = sf.run_Trans(out, PC_file=pc, n_bins=10, ignore_diags=2)
    bad = np.zeros(int(off2[-1]), np.uint8)
    bad[gap] = 1
    use = np.array([1, 1, 1, 1, 0, 0], np.uint8)
    full_track = np.concatenate([track, np.zeros(21)])
    _check_run(r, out, [x[1:] for x in names], off2, (t1, t2, tc), None, use, bad, full_track, 2, 10)
    assert not r["sum"][4:].any() and not r["sum"][:, 4:].any()
