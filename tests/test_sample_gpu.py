"""``sample.downsample_pixels`` (hh_sample_count / hh_sample_write,
csrc/sample.hip) against the per-contact NumPy restatement tests/sample_ref.py
on the 107-bin table, whose forced counts sit on both sides of the kernel's
path cuts (64: lane / wave; 65536: wave / block).  Every comparison is exact."""
import functools
from fractions import Fraction

import numpy as np
import pytest

from hichap_master_amd._lib import HipLibraryError
from hichap_master_amd.sample import downsample_pixels, sample_threshold
from tests.sample_ref import EDGE, sample_ref, table107

pytestmark = pytest.mark.gpu

HH_ERR_ARG = -1
FRACS = (Fraction(0), Fraction(1, 1000), Fraction(37, 100), Fraction(1, 2), 1 - Fraction(1, 2 ** 20), Fraction(1))
SEEDS = (0, 1)


@functools.lru_cache(maxsize=None)
def _table():
    b1, b2, c, off = table107()
    for a in (b1, b2, c, off):
        a.setflags(write=False)
    return b1, b2, c, off


@functools.lru_cache(maxsize=None)
def _ref(frac, seed):
    b1, b2, c, _ = _table()
    out = sample_ref(b1, b2, c, sample_threshold(frac=frac), seed)
    for a in out:
        a.setflags(write=False)
    return out


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        np.testing.assert_array_equal(g, w)


def _dev(b1, b2, c):
    import torch
    f = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt)).cuda()
    return f(b1, np.int32), f(b2, np.int32), f(c, c.dtype if c.dtype == np.int64 else np.int32)


def _host(out):
    return tuple(x.cpu().numpy() for x in out)


def test_table_sits_on_the_path_cuts():
    b1, b2, c, _ = _table()
    got = {(int(a), int(b)): int(v) for a, b, v in zip(b1, b2, c) if (int(a), int(b)) in EDGE}
    assert got == EDGE and {63, 64, 65, 65535, 65536, 65537, 0, 200000} == set(EDGE.values())


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("frac", FRACS, ids=str)
def test_equals_restatement(frac, seed):
    b1, b2, c, _ = _table()
    want = _ref(frac, seed)
    got = downsample_pixels(b1, b2, c, frac=frac, seed=seed)
    _same(got, want)
    assert got[0].dtype == np.int64 and got[2].dtype == np.int32
    if frac == 0:
        assert got[0].size == 0
    elif frac < 1:
        assert got[2].min() > 0 and got[0].size < b1.size       # the stored 0 is gone at least
    else:
        assert got[0].size == b1.size


@pytest.mark.parametrize("frac", (Fraction(37, 100), 1 - Fraction(1, 2 ** 20)), ids=str)
def test_host_device_and_reruns_bitwise(frac):
    import torch
    b1, b2, c, _ = _table()
    want = _ref(frac, 1)
    d = downsample_pixels(*_dev(b1, b2, c), frac=frac, seed=1)
    assert d[0].dtype == torch.int32 and d[0].is_cuda and d[2].dtype == torch.int32
    h = _host(d)
    _same((h[0].astype(np.int64), h[1].astype(np.int64), h[2]), want)
    _same(downsample_pixels(b1, b2, c, frac=frac, seed=1), want)          # a second run
    # int64 counts, host and device
    _same(downsample_pixels(b1, b2, c.astype(np.int64), frac=frac, seed=1), want)
    h = _host(downsample_pixels(*_dev(b1, b2, c.astype(np.int64)), frac=frac, seed=1))
    _same((h[0].astype(np.int64), h[1].astype(np.int64), h[2]), want)


def test_wide_counts_give_int64():
    b1, b2 = np.array([3, 4]), np.array([90, 4])
    c = np.array([2 ** 31 + 2 ** 16, 5], np.int64)
    thr = 2 ** 64 - 2 ** 40                                  # drops a contact in 2^24: ~128 of the large pixel
    frac = Fraction(thr, 2 ** 64)
    o1, o2, oc = downsample_pixels(b1, b2, c, frac=frac, seed=0)
    assert oc.dtype == np.int64 and o1.tolist() == [3, 4]
    assert 2 ** 31 - 1 < oc[0] < c[0] and abs(int(c[0] - oc[0]) - 128) < 5 * np.sqrt(128) and oc[1] == 5
    d = _host(downsample_pixels(*_dev(b1, b2, c), frac=frac, seed=0))
    assert d[2].dtype == np.int64 and d[2].tolist() == oc.tolist()
    # the same rule on the part of the count the restatement can expand: nested below the whole
    part = sample_ref(b1[:1], b2[:1], np.array([1 << 22]), thr, 0)[2][0]
    assert (1 << 22) - part <= c[0] - oc[0]


def test_one_chromosome_alone_equals_its_rows_of_the_whole():
    b1, b2, c, off = _table()
    w1, w2, wc = _ref(Fraction(37, 100), 0)
    for q in range(off.size - 1):
        lo, hi = int(off[q]), int(off[q + 1])
        m, mw = (b1 >= lo) & (b1 < hi), (w1 >= lo) & (w1 < hi)
        _same(downsample_pixels(b1[m], b2[m], c[m], frac=Fraction(37, 100), seed=0), (w1[mw], w2[mw], wc[mw]))


def test_nested_fractions():
    b1, b2, c, off = _table()
    n = int(off[-1])
    dense = []
    for frac in (Fraction(1, 1000), Fraction(3, 10), Fraction(6, 10), 1 - Fraction(1, 2 ** 20)):
        o1, o2, oc = downsample_pixels(b1, b2, c, frac=frac, seed=1)
        M = np.zeros((n, n), np.int64)
        M[o1, o2] = oc
        dense.append(M)
    S = np.zeros((n, n), np.int64)
    S[b1, b2] = c
    for lo, hi in zip(dense, dense[1:] + [S]):
        assert np.all(lo <= hi)
    # (1 - 2^-20 drops 0.4 contacts of this table on average: it may equal the source)
    assert dense[0].sum() < dense[1].sum() < dense[2].sum() < dense[3].sum() <= S.sum()


def test_count_target_is_the_equivalent_fraction():
    b1, b2, c, _ = _table()
    total = int(c.sum(dtype=np.int64))
    target = total // 3 + 1
    got = downsample_pixels(b1, b2, c, count_target=target, seed=1)
    _same(got, downsample_pixels(b1, b2, c, frac=Fraction(target, total), seed=1))
    _same(got, sample_ref(b1, b2, c, (target << 64) // total, 1))
    d = _host(downsample_pixels(*_dev(b1, b2, c), count_target=target, seed=1))
    np.testing.assert_array_equal(d[2], got[2])
    # binomial around the target, not equal to it
    p = target / total
    assert abs(int(got[2].sum()) - target) <= 5 * np.sqrt(total * p * (1 - p))


def test_unsorted_input_keeps_its_order():
    b1, b2, c, off = _table()
    o = np.random.default_rng(3).permutation(b1.size)
    w1, w2, wc = _ref(Fraction(1, 2), 0)
    kept = np.zeros((int(off[-1]),) * 2, np.int64)
    kept[w1, w2] = wc
    g1, g2, gc = downsample_pixels(b1[o], b2[o], c[o], frac=Fraction(1, 2), seed=0)
    keep = kept[b1[o], b2[o]] > 0
    _same((g1, g2, gc), (b1[o][keep], b2[o][keep], kept[b1[o], b2[o]][keep].astype(np.int32)))
    # a table with a repeated pixel is no cooler table, but it samples: each copy like the pixel alone
    r1, r2, rc = downsample_pixels(np.array([3, 3]), np.array([90, 90]), np.array([200000, 200000]), frac=0.5)
    assert rc[0] == rc[1] == kept[3, 90]


@pytest.mark.parametrize("kind", ("count", "id", "wide_id"))
def test_malformed_table(kind):
    b1, b2, c, _ = (np.array(a) for a in _table())
    c = c.astype(np.int64)
    at = 777
    if kind == "count":
        c[at], c[at + 100], words = -1, -5, "non-negative"
    elif kind == "id":
        b2[at], c[at + 1], words = -4, -1, "bin id"
    else:
        b1[at], words = 2 ** 31, "bin id"
    forms = ("host",) if kind == "wide_id" else ("host", "device")
    for form in forms:
        with pytest.raises(HipLibraryError) as e:
            downsample_pixels(*((b1, b2, c) if form == "host" else _dev(b1, b2, c)), frac=0.5)
        assert e.value.code == HH_ERR_ARG
        assert words in str(e.value) and str(e.value).endswith(f"at pixel {at}"), str(e.value)
    _same(downsample_pixels(*_table()[:3], frac=Fraction(1, 2), seed=0), _ref(Fraction(1, 2), 0))
