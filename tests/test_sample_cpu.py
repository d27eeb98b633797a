"""The down-sampling rule of DESIGN.md §4r without a GPU: the exact threshold
arithmetic of ``sample.sample_threshold``, the argument errors, and the
statistics of the rule itself (tests/sample_ref.py) on the 107-bin table --
a condition on the rule, not on the kernel."""
import functools
from fractions import Fraction

import numpy as np
import pytest

from hichap_master_amd import coolio
from hichap_master_amd.sample import KEEP_ALL, downsample_pixels, sample_threshold
from tests.sample_ref import BIG, kept_ref, table107

ZMAX = 5.0      # |z| of a kept total against its binomial; the restatement measured stays below 2.0


def test_threshold_values():
    assert sample_threshold(frac=Fraction(1, 2)) == 2 ** 63 == sample_threshold(frac=0.5)
    assert sample_threshold(frac=0) == 0 == sample_threshold(frac=0.0)
    assert sample_threshold(frac=Fraction(1, 3)) == (2 ** 64 - 1) // 3
    assert sample_threshold(frac=Fraction(37, 100)) == (37 << 64) // 100
    assert sample_threshold(frac=1 - Fraction(1, 2 ** 20)) == 2 ** 64 - 2 ** 44
    assert sample_threshold(frac="1/4") == 2 ** 62


def test_threshold_count_over_total_is_exact_past_2_53():
    total = 2 ** 53 + 1                                  # no float64 holds it
    for count in (1, 1234567890123457, total - 1):
        assert sample_threshold(count=count, total=total) == (count << 64) // total
    assert sample_threshold(count=2 ** 60, total=2 ** 61 + 2) == (2 ** 124) // (2 ** 61 + 2)
    assert sample_threshold(count=0, total=0) == 0


def test_frac_one_is_keep_all():
    assert KEEP_ALL == 2 ** 64
    assert sample_threshold(frac=1) == sample_threshold(frac=1.0) == sample_threshold(count=7, total=7) == KEEP_ALL
    # ... and returns the table without a library call (there is no GPU here to call)
    b1, b2, c, _ = table107()
    o1, o2, oc = downsample_pixels(b1, b2, c, frac=1)
    assert np.array_equal(o1, b1) and np.array_equal(o2, b2) and np.array_equal(oc, c)
    assert o1.dtype == np.int64 and oc.dtype == np.int32
    o1, o2, oc = downsample_pixels(b1, b2, c, count_target=int(c.sum()))
    assert np.array_equal(oc, c)


@pytest.mark.parametrize("kw", [dict(frac=-0.1), dict(frac=1.0000001), dict(frac=Fraction(3, 2)), dict(frac=float("nan")),
                                dict(), dict(frac=0.5, count=3, total=10), dict(count=11, total=10),
                                dict(count=-1, total=10), dict(count=3)])
def test_threshold_argument_errors(kw):
    with pytest.raises(ValueError):
        sample_threshold(**kw)


@pytest.mark.parametrize("kw", [dict(frac=-0.1), dict(frac=2), dict(), dict(frac=0.5, count_target=3),
                                dict(count_target=10 ** 9), dict(frac=0.5, seed=-1), dict(frac=0.5, seed=2 ** 64)])
def test_downsample_argument_errors(kw):
    b1, b2, c, _ = table107()
    with pytest.raises(ValueError):           # before any GPU call
        downsample_pixels(b1, b2, c, **kw)
    with pytest.raises(ValueError, match="GPU down-sampling takes integer counts"):
        downsample_pixels(b1, b2, c.astype(np.float64) + 0.5, frac=0.5)


def test_downsample_rejects_mixed_host_and_device_columns():
    import torch
    b1, b2, c, _ = table107()
    t = torch.from_numpy
    for cols in ((b1, b2, t(c)), (t(b1), t(b2), c), (b1, t(b2), c), (t(b1), b2, t(c))):
        with pytest.raises(ValueError, match="all NumPy arrays or all GPU tensors"):
            downsample_pixels(*cols, frac=0.5)


def test_downsample_cooler_argument_errors(tmp_path):
    b1, b2, c, off = table107()
    src = str(tmp_path / "a.cool")
    coolio.create_cooler(src, {1000: ([("1", 37000), ("2", 5000), ("3", 1000), ("4", 64000)], b1, b2, c)})
    for kw in (dict(), dict(frac=0.5, count=3), dict(frac=1.5), dict(count=int(c.sum()) + 1)):
        with pytest.raises(ValueError):
            coolio.downsample_cooler(f"{src}::1000", str(tmp_path / "b.cool"), **kw)
    with pytest.raises(ValueError):
        coolio.downsample_cooler(f"{src}::1000", str(tmp_path / "b.cool") + "::2000", frac=0.5)


@functools.lru_cache(maxsize=None)
def _kept(frac, seed):
    b1, b2, c, _ = table107()
    k = kept_ref(b1, b2, c, sample_threshold(frac=frac), seed)
    k.setflags(write=False)
    return k


def _z(kept, n, frac):
    p = float(frac)
    return (float(kept) - n * p) / np.sqrt(n * p * (1 - p))


@pytest.mark.parametrize("seed", (0, 1))
@pytest.mark.parametrize("frac", (Fraction(37, 100), Fraction(1, 1000)))
def test_rule_statistics(frac, seed):
    b1, b2, c, _ = table107()
    c = c.astype(np.int64)
    assert b1.size > 1000 and c.sum() > 200000 + 3 * 65536
    k = _kept(frac, seed)
    assert np.all(k >= 0) and np.all(k <= c)
    zs = {"total": _z(k.sum(), c.sum(), frac)}
    for lo, hi in ((1, 10), (10, 30), (30, 60)):
        m = (c >= lo) & (c < hi)
        assert m.sum() > 100
        zs[f"[{lo},{hi})"] = _z(k[m].sum(), c[m].sum(), frac)
    big = (b1 == BIG[0]) & (b2 == BIG[1])
    assert c[big].tolist() == [200000]
    zs["200000"] = _z(k[big].sum(), 200000, frac)
    print(frac, seed, {a: round(v, 2) for a, v in zs.items()})
    assert all(abs(v) <= ZMAX for v in zs.values()), zs


def test_rule_nested_and_seeded():
    b1, b2, c, _ = table107()
    for seed in (0, 1):
        lo, hi = _kept(Fraction(3, 10), seed), _kept(Fraction(6, 10), seed)
        assert np.all(lo <= hi) and lo.sum() < hi.sum()
    a, b = _kept(Fraction(37, 100), 0), _kept(Fraction(37, 100), 1)
    assert np.mean(a != b) > 0.5               # two seeds differ on most pixels
    # the keep flags inside the 200 000-count pixel are not serially correlated
    from tests.sample_ref import U, mix64
    base = mix64(U(0) ^ mix64((U(BIG[0]) << U(32)) | U(BIG[1])))
    with np.errstate(over="ignore"):
        f = (mix64(base + np.arange(200000, dtype=U)) < U(sample_threshold(frac=Fraction(37, 100)))).astype(float)
    assert abs(np.corrcoef(f[:-1], f[1:])[0, 1]) < 5 / np.sqrt(200000)
