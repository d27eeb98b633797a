"""The arithmetic of the upper-band sweep's fast walk, restated
in NumPy: a count n in the high dword of a double whose low dword is 0 is
n * 2^-1042 exactly, so with the biases staged times 2^512 every product and
sum is the converted-count one times 2^-530, rounded at the same bit, as long
as the biases are 0 or of magnitude in [2^-400, 2^400] (the kernel's guard)."""
from fractions import Fraction

import numpy as np

K = 512
UP = np.ldexp(1.0, K)           # staging scale
DOWN = np.ldexp(1.0, 1042 - K)  # back out of the scaled domain
LO, HI = np.ldexp(1.0, -400), np.ldexp(1.0, 400)


def operand(n):
    """uint counts -> the doubles with high dword n, low dword 0"""
    return (np.asarray(n, dtype=np.uint64) << np.uint64(32)).view(np.float64)


def in_range(v):
    """the guard on a staged bias (NaN biases are staged as 0 before it)"""
    v = np.where(np.isnan(v), 0.0, np.asarray(v, dtype=np.float64))
    m = np.abs(v)
    return (v == 0.0) | ((m >= LO) & (m <= HI))


def biases(rng, shape):
    """log-uniform over the whole guard range, either sign, some zeros, the
    range's ends"""
    b = np.ldexp(rng.uniform(1.0, 2.0, shape), rng.integers(-400, 400, shape))
    b *= rng.choice([-1.0, 1.0], shape)
    b[rng.random(shape) < 0.05] = 0.0
    flat = b.reshape(-1)
    flat[:4] = [LO, HI, -LO, -HI]
    assert in_range(b).all()
    return b


def fma(a, b, c):
    """a * b + c rounded once (exact rationals; int / int rounds correctly,
    subnormal results included)"""
    f = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    return f.numerator / f.denominator


def test_operand_is_the_count_times_2_pow_minus_1042():
    n = np.concatenate([np.arange(256), [4095, 65535, (1 << 20) - 1]])
    np.testing.assert_array_equal(operand(n), np.ldexp(n.astype(np.float64), -1042))
    assert operand(1) > 0 and operand(255) < np.finfo(np.float64).tiny  # subnormal: exponent field 0


def test_scaled_sums_equal_converted_sums():
    rng = np.random.default_rng(20250311)
    trials, terms = 2000, 64
    w = biases(rng, (trials, terms))
    n = rng.integers(0, 256, (trials, terms))
    n[:, ::9] = 255
    n[:, 4::9] = 0
    conv = np.zeros(trials)
    fast = np.zeros(trials)
    for k in range(terms):  # the walk's order: one term after the other
        conv = conv + n[:, k].astype(np.float64) * w[:, k]
        fast = fast + operand(n[:, k]) * (w[:, k] * UP)
        np.testing.assert_array_equal((fast * DOWN).view(np.uint64), conv.view(np.uint64))
    # same-sign rows: sums that grow over all 64 terms
    wp = np.abs(w)
    conv = np.cumsum(n * wp, axis=1)[:, -1]
    fast = np.cumsum(operand(n) * (wp * UP), axis=1)[:, -1]
    np.testing.assert_array_equal((fast * DOWN).view(np.uint64), conv.view(np.uint64))


def test_scaled_fused_sums_equal_converted_sums():
    """the kernel's own operation, one rounding per term"""
    rng = np.random.default_rng(7)
    trials, terms = 150, 16
    w = biases(rng, (trials, terms))
    n = rng.integers(0, 256, (trials, terms))
    for t in range(trials):
        conv = fast = 0.0
        for k in range(terms):
            conv = fma(float(n[t, k]), w[t, k], conv)
            fast = fma(operand(n[t, k]), w[t, k] * UP, fast)
            assert np.float64(fast * DOWN).view(np.uint64) == np.float64(conv).view(np.uint64), (t, k)


def test_all_counts_against_one_bias_and_sum():
    rng = np.random.default_rng(3)
    w = biases(rng, (512,))[None, :]
    acc = (rng.random((1, 512)) - 0.3) * 4096.0 * np.abs(w)
    n = np.arange(256)[:, None]
    conv = n.astype(np.float64) * w + acc
    fast = operand(n) * (w * UP) + acc / DOWN
    np.testing.assert_array_equal((fast * DOWN).view(np.uint64), conv.view(np.uint64))


def test_guard_rejects_biases_outside_the_range():
    ok = np.array([0.0, -0.0, LO, HI, -LO, -HI, 1.0, np.nan])  # (NaN is staged as 0)
    assert in_range(ok).all()
    out = np.array([np.ldexp(1.0, 450), np.ldexp(1.0, -450), -np.ldexp(1.0, 450), np.inf, -np.inf,
                    np.nextafter(HI, np.inf), np.nextafter(LO, 0.0), np.finfo(np.float64).tiny, 5e-324])
    assert not in_range(out).any()
    # and it has to: outside the range the scaled domain is not exact
    with np.errstate(over="ignore", under="ignore"):
        tiny = np.ldexp(1.0 + 2.0 ** -52, -600)
        assert operand(200) * (tiny * UP) * DOWN != 200.0 * tiny
        assert not np.isfinite(operand(200) * (np.ldexp(1.0, 600) * UP) * DOWN)
