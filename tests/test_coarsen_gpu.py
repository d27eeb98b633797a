"""``hh_coarsen_*`` (csrc/coarsen.hip) through
``coarsen.coarsen_pixels`` against the NumPy restatement (tests/coarsen_ref.py).
Every comparison is exact: the counts are integer sums."""
import ctypes as C
import functools

import numpy as np
import pytest

from hichap_master_amd import coarsen as co
from hichap_master_amd._lib import HipLibraryError, call, ptr
from tests import knobs
from tests.coarsen_ref import coarsen_ref, ref_bin_map

pytestmark = pytest.mark.gpu

HH_ERR_ARG = -1
RAGGED = (37, 5, 1, 64)            # bins per chromosome: odd, tiny, single-bin, a power of two
EMPTY_BIN = 20                     # a bin with no pixels at all
FACTORS = (1, 2, 4, 5, 50, 100)    # 1 = identity; 50 / 100: every chromosome collapses to one or two bins
BLOCK = 512                        # pixels one block handles per trip of its walk (kCoBlock in coarsen.hip)


def _off(nbins):
    return np.concatenate([[0], np.cumsum(nbins)]).astype(np.int64)


def _random_table(nbins, seed, density, extra=(), empty=(), hi=60):
    """Sorted unique upper-triangle table (cis and trans) + forced pixels."""
    off = _off(nbins)
    n = int(off[-1])
    rng = np.random.default_rng(seed)
    i, j = np.triu_indices(n)
    keep = rng.random(i.size) < density
    for a, b in extra:
        keep[np.flatnonzero((i == a) & (j == b))] = True
    for e in empty:
        keep[(i == e) | (j == e)] = False
    b1, b2 = i[keep].astype(np.int64), j[keep].astype(np.int64)
    c = rng.integers(1, hi, b1.size).astype(np.int32)
    for a in (b1, b2, c, off):
        a.setflags(write=False)
    return b1, b2, c, off


@functools.lru_cache(maxsize=None)
def _ragged():
    b1, b2, c, off = _random_table(RAGGED, 1, 0.25, extra=((0, 0), (0, 106), (106, 106)), empty=(EMPTY_BIN,))
    n = int(off[-1])
    assert np.any((b1 < 37) & (b2 >= 43)) and np.any(b1 == b2)      # trans and diagonal pixels
    assert not np.any((b1 == EMPTY_BIN) | (b2 == EMPTY_BIN)) and b2.max() == n - 1
    return b1, b2, c, off


@functools.lru_cache(maxsize=None)
def _ref(table, k):
    b1, b2, c, off = table()
    out = coarsen_ref(b1, b2, c, off, k)
    for a in out:
        a.setflags(write=False)
    return out


def _check(got, want):
    (g1, g2, gc, goff), (w1, w2, wc, woff) = got, want
    np.testing.assert_array_equal(goff, woff)
    np.testing.assert_array_equal(g1, w1)
    np.testing.assert_array_equal(g2, w2)
    np.testing.assert_array_equal(gc.astype(np.int64), wc)
    assert gc.dtype == (np.int32 if (wc.size == 0 or wc.max() <= 2 ** 31 - 1) else np.int64)
    nbc = int(woff[-1])
    assert np.all(g1 <= g2) and np.all(np.diff(g1 * nbc + g2) > 0)    # sorted, unique, upper triangle


def _dev(table):
    import torch
    b1, b2, c, off = table
    f = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt)).cuda()
    return f(b1, np.int32), f(b2, np.int32), f(c, c.dtype if c.dtype == np.int64 else np.int32), off


def _host(out):
    return tuple(x.cpu().numpy() if hasattr(x, "cpu") else x for x in out)


@pytest.fixture
def tile64():
    """Column tiles of 64 coarse bins for the test, the default after it."""
    assert co.tile_width() == co.TILE == 8192
    with knobs.tuned(coarsen_tile=64):
        assert co.tile_width() == 64
        yield 64


@pytest.mark.parametrize("k", FACTORS)
def test_ragged_equals_restatement(k):
    b1, b2, c, off = _ragged()
    got = co.coarsen_pixels(b1, b2, c, off, k)
    _check(got, _ref(_ragged, k))
    assert got[0].dtype == np.int64 and int(got[2].sum()) == int(c.sum())   # total count conserved
    if k == 1:
        np.testing.assert_array_equal(got[0], b1)
        np.testing.assert_array_equal(got[2], c)


@pytest.mark.parametrize("k", FACTORS)
def test_ragged_tile64(tile64, k):
    b1, b2, c, off = _ragged()          # 107 bins: two tiles of 64 at k = 1, one otherwise
    _check(co.coarsen_pixels(b1, b2, c, off, k), _ref(_ragged, k))


EDGE_GENOME = (37, 5, 1, 64, 300)     # 407 fine bins; 407 (k = 1) and 205 (k = 2) coarse bins: > 2 T at T = 64


def _edge_pixels(nbins, k, T, rows):
    """Fine pixels at the coarse columns T-1, T, T+1, 2T-1, 2T from the given coarse rows."""
    m = ref_bin_map(_off(nbins), k)
    px = []
    for I in rows:
        r = int(np.searchsorted(m, I))
        for e in (T - 1, T, T + 1, 2 * T - 1, 2 * T):
            f = int(np.searchsorted(m, e))
            if e >= I:
                px.append((r, f))
                if k > 1 and m[f + 1] == e and f + 1 > r:
                    px.append((r, f + 1))     # two addends in an edge cell
    return tuple(px)


@pytest.mark.parametrize("k", (1, 2))
def test_tile_edges_tile64(tile64, k):
    T = tile64
    extra = _edge_pixels(EDGE_GENOME, k, T, (0, 3, T - 1, T, T + 1, 2 * T - 1, 2 * T))
    b1, b2, c, off = _random_table(EDGE_GENOME, 10 + k, 0.05, extra=extra)
    want = coarsen_ref(b1, b2, c, off, k)
    assert int(want[3][-1]) > 2 * T
    for e in (T - 1, T, T + 1, 2 * T - 1, 2 * T):
        assert np.any((want[0] == 0) & (want[1] == e)) and np.any((want[0] == e) & (want[1] == e))
    _check(co.coarsen_pixels(b1, b2, c, off, k), want)


def test_tile_edges_default_tile():
    """2 T + 3 coarse bins in two chromosomes at the default width (T = 8192,
    k = 2: 32 773 fine bins, ~2e5 random pixels), the edge columns populated."""
    T, k = co.tile_width(), 2
    assert T == co.TILE
    nbins = (2 * T + 3617, 2 * T - 3612)                 # 20 001 + 12 772 fine, 10 001 (ragged) + 6 386 coarse bins
    off = _off(nbins)
    assert int(np.sum([-(-x // k) for x in nbins])) == 2 * T + 3
    n = int(off[-1])
    rng = np.random.default_rng(77)
    r = np.sort(rng.integers(0, n, 200_000))
    cc = np.minimum(r + (rng.pareto(0.7, r.size) * 3).astype(np.int64), n - 1)
    edge = _edge_pixels(nbins, k, T, (0, 5, T - 1, T, T + 1, 2 * T - 1, 2 * T))
    r = np.concatenate([r, [a for a, _ in edge]])
    cc = np.concatenate([cc, [b for _, b in edge]])
    key = np.unique(r * n + cc)
    b1, b2 = key // n, key % n
    c = rng.integers(1, 1000, b1.size).astype(np.int32)
    want = coarsen_ref(b1, b2, c, off, k)
    assert int(want[3][-1]) == 2 * T + 3
    for e in (T - 1, T, T + 1, 2 * T - 1, 2 * T):
        assert np.any((want[0] == 0) & (want[1] == e)) and np.any((want[0] == e) & (want[1] == e))
    _check(co.coarsen_pixels(b1, b2, c, off, k), want)


@pytest.mark.parametrize("k", (1, 3, 40))
def test_empty_single_and_gaps(k):
    off = _off((10, 7, 12))
    e = np.empty(0, np.int64)
    g1, g2, gc, goff = co.coarsen_pixels(e, e, e.astype(np.int32), off, k)
    assert g1.size == g2.size == gc.size == 0 and gc.dtype == np.int32
    np.testing.assert_array_equal(goff, _off([-(-x // k) for x in (10, 7, 12)]))
    import torch
    z = torch.empty(0, dtype=torch.int32, device="cuda")
    d = co.coarsen_pixels(z, z, z, off, k)
    assert d[0].numel() == 0 and d[0].is_cuda and d[2].dtype == torch.int32
    # one pixel: on the diagonal, off it, trans, in the last bin
    for a, b in ((0, 0), (3, 9), (2, 28), (28, 28)):
        t = (np.array([a]), np.array([b]), np.array([7], np.int32), off)
        _check(co.coarsen_pixels(*t, k), coarsen_ref(*t, k))
    # a whole chromosome without pixels between two that have some
    b1, b2, c, _ = _random_table((10, 7, 12), 3, 0.4, empty=tuple(range(10, 17)))
    assert b1.size > 50 and not np.any((b1 >= 10) & (b1 < 17)) and np.any((b1 < 10) & (b2 >= 17))
    _check(co.coarsen_pixels(b1, b2, c, off, k), coarsen_ref(b1, b2, c, off, k))


@functools.lru_cache(maxsize=None)
def _heavy():
    """One chromosome of 3 200 bins whose first 100 rows are half full, the
    50 x 50 block rows 0-49 x columns 50-99 completely."""
    n = 3200
    rng = np.random.default_rng(8)
    keep = rng.random((100, n)) < 0.5
    keep[:50, 50:100] = True
    keep &= np.arange(n)[None, :] >= np.arange(100)[:, None]
    b1, b2 = np.nonzero(keep)
    c = rng.integers(1, 2 ** 20, b1.size).astype(np.int32)
    return b1.astype(np.int64), b2.astype(np.int64), c, _off((n,))


@pytest.mark.parametrize("k,tuned", [(50, True), (50, False), (100, True), (100, False)])
def test_heavy_item(k, tuned):
    """One (coarse row x tile) item far beyond one trip of the block's walk:
    coarse row 0 at k = 50 is one item of ~80 000 pixels in both tilings (64
    coarse bins = one tile of 64), over 100 x the 512 pixels of a trip (at
    least 4 x is asked for); its cell (0, 1) sums 2 500 pixels.  k = 100 walks 100
    fine rows per item, more than the 64 whose segments are staged at once."""
    b1, b2, c, off = _heavy()
    assert int(np.sum(b1 < 50)) >= 100 * BLOCK and int(np.sum((b1 < 50) & (b2 >= 50) & (b2 < 100))) == 2500
    with knobs.tuned(coarsen_tile=64 if tuned else co.TILE):
        got = co.coarsen_pixels(b1, b2, c, off, k)
    _check(got, _ref(_heavy, k))


@pytest.mark.parametrize("total,dtype", [(2 ** 31 - 1, np.int32), (2 ** 31, np.int64), (2 ** 32, np.int64)])
def test_count_width(total, dtype):
    """A 4 x 4 fine block whose 16 counts sum to 2^31 - 1 stays int32, 2^31
    needs int64, 16 x 2^28 is exactly 2^32."""
    b1, b2 = (x.ravel().astype(np.int64) for x in np.meshgrid(np.arange(4), np.arange(4, 8), indexing="ij"))
    c = np.full(16, 2 ** 28 if total == 2 ** 32 else 2 ** 27, dtype=np.int64)
    c[-1] += total - int(c.sum())
    assert int(c.sum()) == total and c.max() <= 2 ** 31 - 1
    c = c.astype(np.int32)
    for form in ("host", "device"):
        t = (b1, b2, c, _off((8,)))
        g1, g2, gc, goff = _host(co.coarsen_pixels(*(_dev(t) if form == "device" else t), 4))
        assert gc.dtype == dtype and gc.tolist() == [total] and (g1.tolist(), g2.tolist()) == ([0], [1])


def test_int64_source_counts():
    """A level whose counts are int64 is a valid source (zoomify's later levels)."""
    b1 = np.array([0, 0, 1, 5], dtype=np.int64)
    b2 = np.array([2, 3, 3, 7], dtype=np.int64)
    c = np.array([2 ** 40, 2 ** 33 + 1, 5, 2 ** 31], dtype=np.int64)
    t = (b1, b2, c, _off((8,)))
    want = coarsen_ref(*t, 2)
    _check(co.coarsen_pixels(*t, 2), want)
    _check(_host(co.coarsen_pixels(*_dev(t), 2)), want)


@pytest.mark.parametrize("ks", [(2, 2), (4, 5)])
def test_composition_on_device(ks):
    """k = 2 then 2 is bitwise k = 4, k = 4 then 5 bitwise k = 20: a level is
    as good a source as the base table (zoomify relies on it)."""
    t = _dev(_random_table((137, 45, 1, 264), 4, 0.2))
    a = co.coarsen_pixels(*t, ks[0])
    two = _host(co.coarsen_pixels(a[0], a[1], a[2], a[3], ks[1]))
    one = _host(co.coarsen_pixels(*t, ks[0] * ks[1]))
    for g, w in zip(two, one):
        assert g.dtype == w.dtype
        np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("k", (2, 5))
def test_host_device_and_reruns_bitwise(k):
    import torch
    t = _ragged()
    h = co.coarsen_pixels(*t, k)
    d = co.coarsen_pixels(*_dev(t), k)
    assert d[0].is_cuda and d[0].dtype == d[1].dtype == torch.int32
    d2 = co.coarsen_pixels(*_dev(t), k)
    for a, b, c in zip(h, _host(d), _host(d2)):
        np.testing.assert_array_equal(a, b)
        assert b.tobytes() == c.tobytes()
    assert h[2].dtype == _host(d)[2].dtype


def _malformed(kind):
    """(table, first offending pixel, words of the message)."""
    b1, b2, c, off = (np.array(a) for a in _ragged())
    n = int(off[-1])
    p = int(np.flatnonzero((b1[:-1] == b1[1:]) & (b1[:-1] == 40))[3])     # p, p + 1 in one row, inside the table
    if kind == "unsorted":
        b2[[p, p + 1]] = b2[[p + 1, p]]
        return (b1, b2, c, off), p + 1, "not sorted"
    if kind == "unsorted_rows":
        q = int(np.flatnonzero(b1[:-1] != b1[1:])[30])                     # the last pixel of a row
        b1[q], b2[q] = b1[q + 1] + 1, n - 1
        return (b1, b2, c, off), q + 1, "not sorted"
    if kind == "duplicate":
        b2[p + 1] = b2[p]
        return (b1, b2, c, off), p + 1, "duplicate pixel"
    if kind == "lower":
        assert b1[p] < b2[p]
        b1[p], b2[p] = b2[p], b1[p]
        return (b1, b2, c, off), p, "bin1 > bin2"
    if kind == "range":
        q = int(np.flatnonzero(b1[:-1] != b1[1:])[30])
        b2[q] = n
        return (b1, b2, c, off), q, "out of range"
    if kind == "range_negative":
        b1[0] = -1
        return (b1, b2, c, off), 0, "out of range"
    assert kind == "negative"
    c[p] = -3
    return (b1, b2, c, off), p, "non-negative"


@pytest.mark.parametrize("k", (1, 4))
@pytest.mark.parametrize("kind", ["unsorted", "unsorted_rows", "duplicate", "lower", "range", "range_negative",
                                  "negative"])
def test_malformed_tables(kind, k):
    t, at, words = _malformed(kind)
    for form in ("host", "device"):
        with pytest.raises(HipLibraryError) as e:
            co.coarsen_pixels(*(_dev(t) if form == "device" else t), k)
        assert e.value.code == HH_ERR_ARG
        assert words in str(e.value) and str(e.value).endswith(f"at pixel {at}"), str(e.value)
    # the C-ABI leaves its outputs alone: no handle, no sizes
    d1, d2, dc, off = _dev(t)
    h, n, mx = C.c_void_p(), C.c_int64(-7), C.c_int64(-7)
    with pytest.raises(HipLibraryError):
        call("hh_coarsen_count", ptr(d1), ptr(d2), ptr(dc), 0, d1.numel(), int(off[-1]), ptr(off), off.size - 1, k, 1,
             None, C.byref(h), C.byref(n), C.byref(mx))
    assert h.value is None and n.value == -7 and mx.value == -7
    # and a good table still runs afterwards
    _check(co.coarsen_pixels(*_ragged(), k), _ref(_ragged, k))


def test_argument_errors():
    b1, b2, c, off = _ragged()
    with pytest.raises(HipLibraryError) as e:
        co.coarsen_pixels(b1, b2, c, off[:-1], 2)           # offsets that stop short of the ids
    assert e.value.code == HH_ERR_ARG
    with pytest.raises(ValueError):
        co.coarsen_pixels(b1, b2, c, off, 0)
    with pytest.raises(HipLibraryError), knobs.tuned(coarsen_tile=63):
        pass
    with pytest.raises(HipLibraryError), knobs.tuned(coarsen_tile=co.TILE + 1):
        pass
    assert co.tile_width() == co.TILE
