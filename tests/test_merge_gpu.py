"""``merge.merge_pixels`` (hh_merge_count / hh_merge_write, csrc/merge.hip)
against the NumPy restatement tests/merge_ref.py: every comparison is exact."""
import functools

import numpy as np
import pytest

from hichap_master_amd import coarsen as co
from hichap_master_amd._lib import HipLibraryError
from hichap_master_amd.merge import merge_pixels
from tests import knobs
from tests.merge_ref import merge_ref

pytestmark = pytest.mark.gpu

HH_ERR_ARG = -1
RAGGED = (37, 5, 1, 64)            # bins per chromosome: odd, tiny, single-bin, a power of two
N = sum(RAGGED)
EMPTY_BIN = 20                     # a bin with no pixels in any table
ALL, LAST, ZERO_SUM, ZERO_ONLY = (5, 9), (7, 99), (30, 31), (6, 6)
DENSITY = (0.25, 0.1, 0.4, 0.05, 0.3)
BLOCK = 512                        # pixels one block handles per trip of its walk (kCoBlock)


def _table(n, seed, density, extra=(), drop=(), empty=(), zero=(), rows=None, hi=60, dtype=np.int32):
    """Sorted unique upper-triangle table over n bins (cis and trans alike)."""
    rng = np.random.default_rng(seed)
    i, j = np.triu_indices(n)
    keep = rng.random(i.size) < density
    for a, b in extra:
        keep[(i == a) & (j == b)] = True
    for a, b in drop:
        keep[(i == a) & (j == b)] = False
    for e in empty:
        keep[(i == e) | (j == e)] = False
    if rows is not None:
        keep &= (i >= rows[0]) & (i < rows[1])
    b1, b2 = i[keep].astype(np.int64), j[keep].astype(np.int64)
    c = rng.integers(1, hi, b1.size).astype(dtype)
    for a, b in zero:
        c[(b1 == a) & (b2 == b)] = 0
    for a in (b1, b2, c):
        a.setflags(write=False)
    return b1, b2, c


EMPTY = tuple(np.zeros(0, dt) for dt in (np.int64, np.int64, np.int32))


@functools.lru_cache(maxsize=None)
def _ragged(K):
    """K tables of different densities: ALL is in every one, LAST in the last
    only, ZERO_SUM is stored as 0 in table 0 (and counted in the others),
    ZERO_ONLY is a stored 0 of table 0 alone."""
    out = []
    for t in range(K):
        extra = (ALL, ZERO_SUM) + ((LAST,) if t == K - 1 else ()) + ((ZERO_ONLY,) if t == 0 else ())
        drop = (() if t == K - 1 else (LAST,)) + (() if t == 0 else (ZERO_ONLY,))
        out.append(_table(N, 10 + t, DENSITY[t], extra, drop, (EMPTY_BIN,), (ZERO_SUM, ZERO_ONLY) if t == 0 else ()))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _case(name):
    if name.startswith("ragged"):
        return _ragged(int(name[-1])), N
    if name == "one_empty":
        a, b = _ragged(2)
        return (a, EMPTY, b), N
    if name == "all_empty":
        return (EMPTY, EMPTY), N
    if name == "disjoint_rows":
        return (_table(N, 3, 0.3, rows=(0, 50)), _table(N, 4, 0.3, rows=(50, N))), N
    assert name == "edges"             # 150 bins: tile edges of 64 at columns 63 / 64 / 127 / 128
    e = ((0, 63), (0, 64), (0, 127), (0, 128), (63, 63), (63, 64), (64, 64), (127, 127), (127, 128), (128, 128),
         (64, 127), (64, 128), (149, 149))
    return (_table(150, 5, 0.05, e), _table(150, 6, 0.1, e[::2]), _table(150, 7, 0.02, e[1::2])), 150


CASES = ("ragged1", "ragged2", "ragged5", "one_empty", "all_empty", "disjoint_rows", "edges")


@functools.lru_cache(maxsize=None)
def _ref(name):
    tables, n = _case(name)
    out = merge_ref(tables, n)
    for a in out:
        a.setflags(write=False)
    return out


def _check(got, want, n):
    (g1, g2, gc), (w1, w2, wc) = got, want
    np.testing.assert_array_equal(g1, w1)
    np.testing.assert_array_equal(g2, w2)
    np.testing.assert_array_equal(gc.astype(np.int64), wc)
    assert gc.dtype == (np.int32 if (wc.size == 0 or wc.max() <= 2 ** 31 - 1) else np.int64)
    assert np.all(g1 <= g2) and np.all(np.diff(g1 * n + g2) > 0)      # sorted, unique, upper triangle


def _dev(t):
    import torch
    f = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt)).cuda()
    return f(t[0], np.int32), f(t[1], np.int32), f(t[2], t[2].dtype if t[2].dtype == np.int64 else np.int32)


def _host(out):
    return tuple(x.cpu().numpy() for x in out)


@pytest.fixture
def tile64():
    assert co.tile_width() == co.TILE == 8192
    with knobs.tuned(coarsen_tile=64):
        assert co.tile_width() == 64
        yield 64


def test_fixture_covers_the_cases():
    ts = _ragged(5)
    has = lambda t, p: bool(np.any((t[0] == p[0]) & (t[1] == p[1])))
    assert all(has(t, ALL) for t in ts) and [has(t, LAST) for t in ts] == [False] * 4 + [True]
    assert [has(t, ZERO_ONLY) for t in ts] == [True] + [False] * 4
    assert not any(np.any((t[0] == EMPTY_BIN) | (t[1] == EMPTY_BIN)) for t in ts)
    assert any(np.any((t[0] < 37) & (t[1] >= 43)) for t in ts)          # trans pixels
    w1, w2, wc = _ref("ragged5")
    assert wc[(w1 == ZERO_ONLY[0]) & (w2 == ZERO_ONLY[1])].tolist() == [0]
    assert wc[(w1 == ZERO_SUM[0]) & (w2 == ZERO_SUM[1])][0] > 0
    assert len({t[0].size for t in ts}) == 5


@pytest.mark.parametrize("name", CASES)
def test_equals_restatement(name):
    tables, n = _case(name)
    got = merge_pixels(tables, n)
    _check(got, _ref(name), n)
    assert got[0].dtype == np.int64 and int(got[2].sum()) == sum(int(t[2].sum()) for t in tables)
    if name == "ragged1":              # one table: the identity, through the same kernels
        for g, a in zip(got, tables[0]):
            np.testing.assert_array_equal(g, a)


@pytest.mark.parametrize("name", CASES)
def test_equals_restatement_tile64(tile64, name):
    tables, n = _case(name)            # 107 or 150 bins: two or three column tiles of 64
    _check(merge_pixels(tables, n), _ref(name), n)
    _check(_host(merge_pixels([_dev(t) for t in tables], n)), _ref(name), n)


@pytest.mark.parametrize("tile", (64, 8192))
def test_long_row_takes_several_trips(tile):
    n = 700
    tabs = []
    for t in range(3):
        b1, b2, c = (np.array(a) for a in _table(n, 20 + t, 0.002))
        rest = b1 > 0
        b1 = np.concatenate([np.zeros(n, np.int64), b1[rest]])       # row 0 dense
        b2 = np.concatenate([np.arange(n), b2[rest]])
        c = np.concatenate([np.arange(1, n + 1, dtype=np.int32) * (t + 1), c[rest]])
        tabs.append((b1, b2, c))
    assert 3 * n > BLOCK
    with knobs.tuned(coarsen_tile=tile):
        got = merge_pixels(tabs, n)
    _check(got, merge_ref(tabs, n), n)
    np.testing.assert_array_equal(got[2][:n], np.arange(1, n + 1) * 6)


def test_count_width():
    big = 2 ** 30 + 5
    a = (np.array([0, 1]), np.array([1, 1]), np.array([big, 3], np.int32))
    b = (np.array([0, 2]), np.array([1, 2]), np.array([big, 4], np.int32))
    for tabs in ([a, b], [_dev(a), _dev(b)]):
        o1, o2, oc = merge_pixels(tabs, 3)
        if hasattr(oc, "cpu"):
            o1, o2, oc = _host((o1, o2, oc))
        assert oc.dtype == np.int64 and oc.tolist() == [2 * big, 3, 4] and o1.tolist() == [0, 1, 2]
    o = merge_pixels([a, (b[0], b[1], np.array([big - 11, 4], np.int32))], 3)      # 2^31 - 1 still fits int32
    assert o[2].dtype == np.int32 and o[2].tolist() == [2 ** 31 - 1, 3, 4]
    # an int64 device table next to an int32 one
    a64 = (a[0], a[1], np.array([2 ** 40, 3], np.int64))
    got = _host(merge_pixels([_dev(a64), _dev(b)], 3))
    assert got[2].dtype == np.int64 and got[2].tolist() == [2 ** 40 + big, 3, 4]
    _check(_host(merge_pixels([_dev(b), _dev(a64), _dev(a)], 3)), merge_ref([b, a64, a], 3), 3)


@pytest.mark.parametrize("name", ("ragged5", "edges"))
def test_host_device_and_reruns_bitwise(tile64, name):
    tables, n = _case(name)
    h = merge_pixels(tables, n)
    d = merge_pixels([_dev(t) for t in tables], n)
    import torch
    assert d[0].dtype == torch.int32 and d[0].is_cuda
    for x, y, z in zip(h, _host(d), merge_pixels(tables, n)):
        assert x.astype(np.int64).tobytes() == y.astype(np.int64).tobytes() == z.astype(np.int64).tobytes()
    assert h[2].dtype == _host(d)[2].dtype


def test_algebra_on_device():
    import torch
    (A, B, C), n = _case("edges")
    dA, dB, dC = _dev(A), _dev(B), _dev(C)
    eq = lambda x, y: all(torch.equal(a, b) for a, b in zip(x, y))
    ab = merge_pixels([dA, dB], n)
    assert eq(ab, merge_pixels([dB, dA], n))                              # commutes
    abc = merge_pixels([dA, dB, dC], n)
    assert eq(merge_pixels([ab, dC], n), abc)                             # composes, on the device
    assert eq(merge_pixels([dC, ab], n), abc)
    aa = merge_pixels([dA, dA], n)
    assert torch.equal(aa[0], dA[0]) and torch.equal(aa[1], dA[1]) and torch.equal(aa[2], 2 * dA[2])
    _check(_host(abc), _ref("edges"), n)


def test_merge_then_coarsen_is_coarsen_then_merge():
    tables = _ragged(5)[:3]
    off = np.concatenate([[0], np.cumsum(RAGGED)]).astype(np.int64)
    m = merge_pixels(tables, N)
    a1, a2, ac, coff = co.coarsen_pixels(*m, off, 4)
    parts = [co.coarsen_pixels(*t, off, 4)[:3] for t in tables]
    b1, b2, bc = merge_pixels(parts, int(coff[-1]))
    np.testing.assert_array_equal(a1, b1)
    np.testing.assert_array_equal(a2, b2)
    np.testing.assert_array_equal(ac, bc)


def _malformed(kind):
    """(table, first offending pixel, words of the message)."""
    b1, b2, c = (np.array(a) for a in _ragged(5)[0])
    p = int(np.flatnonzero((b1[:-1] == b1[1:]) & (b1[:-1] == 40))[3])     # p, p + 1 in one row, inside the table
    if kind == "unsorted":
        b2[[p, p + 1]] = b2[[p + 1, p]]
        return (b1, b2, c), p + 1, "not sorted"
    if kind == "duplicate":
        b2[p + 1] = b2[p]
        return (b1, b2, c), p + 1, "duplicate pixel"
    if kind == "lower":
        assert b1[p] < b2[p]
        b1[p], b2[p] = b2[p], b1[p]
        return (b1, b2, c), p, "bin1 > bin2"
    if kind == "range":
        q = int(np.flatnonzero(b1[:-1] != b1[1:])[30])                     # the last pixel of a row
        b2[q] = N
        return (b1, b2, c), q, "out of range"
    if kind == "range_negative":
        b1[0] = -1
        return (b1, b2, c), 0, "out of range"
    assert kind == "negative"
    c[p] = -3
    return (b1, b2, c), p, "non-negative"


@pytest.mark.parametrize("kind", ["unsorted", "duplicate", "lower", "range", "range_negative", "negative"])
@pytest.mark.parametrize("tile", (64, 8192))
def test_malformed_table_is_named(kind, tile):
    bad, at, words = _malformed(kind)
    good = _ragged(5)
    tabs = [good[1], bad, good[2]]
    with knobs.tuned(coarsen_tile=tile):
        for form in ("host", "device"):
            with pytest.raises(HipLibraryError) as e:
                merge_pixels([_dev(t) for t in tabs] if form == "device" else tabs, N)
            assert e.value.code == HH_ERR_ARG
            msg = str(e.value)
            assert "table 1:" in msg and words in msg and msg.endswith(f"at pixel {at}"), msg
        # and good tables still run afterwards
        _check(merge_pixels([good[1], good[2]], N), merge_ref([good[1], good[2]], N), N)
