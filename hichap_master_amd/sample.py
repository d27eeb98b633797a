"""Down-sampling of cooler's pixel table on the GPU: binomial thinning by a
counter-based rule (the normative text).

With ``mix64`` the splitmix64 finaliser of ``csrc/hh_common.hpp`` and ``thr``
a uint64 threshold, pixel ``(bin1, bin2)`` of count ``c`` keeps

    base = mix64(seed ^ mix64((uint64(bin1) << 32) | uint64(bin2)))
    kept = #{ t in [0, c) : mix64(base + t) < thr }      (uint64, wrapping)

contacts; pixels with ``kept == 0`` are dropped, the others keep their order.
``thr = floor(frac * 2^64)`` in exact integers.  Every contact's fate is a pure
function of ``(seed, bin1, bin2, t)``: the sample does not depend on the launch
geometry or on host versus device input, a part of the table samples to the
same pixels as the whole, and samples of one seed are nested (``frac_a <=
frac_b`` gives ``kept_a <= kept_b`` for every pixel).

The kept total is binomial around ``frac * total``, not equal to it: this is
cooltools' ``sample(exact=False)``.  Exact-size sampling without replacement
is not built.

* ``sample_threshold``: ``frac`` or ``count / total`` -> ``thr`` (pure Python).
* ``downsample_pixels``: host arrays or device tensors
  (``hh_sample_count`` / ``hh_sample_write``, csrc/sample.hip).

The file level (``downsample_cooler``) is in ``coolio.py``.
"""
from __future__ import annotations

import ctypes as C
from fractions import Fraction

import numpy as np

from ._lib import call, ptr, require_gpu
from ._pixels import is_dev
from .coarsen import INT32_MAX, integer_counts

KEEP_ALL = 1 << 64    # sample_threshold's value for frac = 1: no uint64 holds it, the table is returned as it is


def _fraction(frac=None, count=None, total=None):
    if (frac is None) == (count is None):
        raise ValueError("give exactly one of frac and a target count")
    if frac is not None:
        try:
            f = Fraction(frac)
        except (TypeError, ValueError, OverflowError) as e:
            raise ValueError(f"frac must be a number in [0, 1]: {frac!r}") from e
        if not 0 <= f <= 1:
            raise ValueError(f"frac must lie in [0, 1]: {frac!r}")
        return f
    if total is None:
        raise ValueError("a target count needs the table's total")
    count, total = int(count), int(total)
    if count < 0 or total < 0:
        raise ValueError("the target count and the total must be >= 0")
    if count > total:
        raise ValueError(f"the target count {count} is larger than the table's total {total}")
    return Fraction(count, total) if total else Fraction(0)


def sample_threshold(frac=None, count=None, total=None):
    """``floor(frac * 2^64)`` in exact integers; ``frac`` a number in [0, 1]
    (a float stands for its exact binary value, a ``Fraction`` for itself), or
    ``count / total`` as an exact rational.  ``frac = 1`` gives ``KEEP_ALL`` (2^64):
    every contact is kept and the library is not called.  ``ValueError``: both
    or neither of ``frac`` / ``count``, ``frac`` outside [0, 1], ``count`` >
    ``total``."""
    f = _fraction(frac, count, total)
    return (f.numerator << 64) // f.denominator


def _seed(seed):
    if int(seed) != seed or not 0 <= int(seed) < (1 << 64):
        raise ValueError("seed must be an integer in [0, 2^64)")
    return int(seed)


def downsample_pixels(bin1, bin2, count, frac=None, count_target=None, seed=0, stream=None):
    """Thin a pixel table: every contact is kept with probability ``frac``, or
    ``count_target / sum(count)`` (an exact rational), by the rule above:
    ``(bin1, bin2, count)`` of the pixels that keep at least one contact, in
    the input's order.  The kept total is binomial around the target, not equal
    to it (cooltools' ``sample(exact=False)``); exact-size sampling is not
    built.  NumPy inputs return NumPy arrays (int64 ids); torch tensors on the
    GPU are used in place (int32 ids; int32 or int64 counts) and the result
    stays on the device (int32 ids).  Counts come back int32 while the largest
    is <= 2^31 - 1, int64 otherwise.  The table need not be sorted; ids outside
    [0, 2^31) or a negative count raise ``HipLibraryError`` (HH_ERR_ARG) naming
    the first offending pixel.  ``frac = 1`` returns the table as it is (with
    those dtypes) without calling the library.  ``ValueError`` before any GPU
    call: ``frac`` outside [0, 1], both or neither of ``frac`` /
    ``count_target``, a target larger than the total, a mix of NumPy and
    tensor columns."""
    seed = _seed(seed)
    if (frac is None) == (count_target is None):
        raise ValueError("give exactly one of frac and count_target")
    dev = is_dev(bin1)
    if any(is_dev(x) != dev for x in (bin2, count)):
        raise ValueError("downsample_pixels: bin1, bin2 and count must be all NumPy arrays or all GPU tensors")
    if dev:
        import torch
        b1, b2 = (x.to(torch.int32).contiguous() for x in (bin1, bin2))
        c = count
        if c.dtype.is_floating_point:
            if not bool(torch.all(torch.isfinite(c) & (c == torch.floor(c)))):
                raise ValueError("GPU down-sampling takes integer counts")
            c = c.to(torch.int64)
        elif c.dtype not in (torch.int32, torch.int64):
            c = c.to(torch.int64)
        c = c.contiguous()
        if not (b1.ndim == 1 and tuple(b1.shape) == tuple(b2.shape) == tuple(c.shape)):
            raise ValueError("bin1, bin2 and count must be 1-D of the same length")
    else:
        b1 = np.ascontiguousarray(bin1, dtype=np.int64)
        b2 = np.ascontiguousarray(bin2, dtype=np.int64)
        c = integer_counts(count, "GPU down-sampling")
        if not (b1.ndim == 1 and b1.shape == b2.shape == c.shape):
            raise ValueError("bin1, bin2 and count must be 1-D of the same length")
    if frac is not None:
        thr = sample_threshold(frac=frac)
    else:
        total = int(c.sum(dtype=torch.int64)) if dev else int(c.sum(dtype=np.int64))
        thr = sample_threshold(count=count_target, total=total)
    if thr == KEEP_ALL:
        mx = int(c.max()) if len(c) else 0
        if dev:
            return b1, b2, c.to(torch.int64 if mx > INT32_MAX else torch.int32)
        return b1, b2, c.astype(np.int64 if mx > INT32_MAX else np.int32)
    require_gpu()
    h, n, tot, mx = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    if dev:
        call("hh_sample_count", ptr(b1), ptr(b2), ptr(c), int(c.dtype == torch.int64), b1.numel(), thr, seed, 1,
             stream, C.byref(h), C.byref(n), C.byref(tot), C.byref(mx))
        try:
            wide = mx.value > INT32_MAX
            o1 = torch.empty(n.value, dtype=torch.int32, device=b1.device)
            o2 = torch.empty(n.value, dtype=torch.int32, device=b1.device)
            oc = torch.empty(n.value, dtype=torch.int64 if wide else torch.int32, device=b1.device)
            call("hh_sample_write", h, ptr(o1), ptr(o2), ptr(oc), int(wide), stream)
        finally:
            call("hh_sample_free", h)
        return o1, o2, oc
    call("hh_sample_count_host", ptr(b1), ptr(b2), ptr(c), b1.size, thr, seed, stream, C.byref(h), C.byref(n),
         C.byref(tot), C.byref(mx))
    try:
        wide = mx.value > INT32_MAX
        o1, o2 = np.empty(n.value, np.int64), np.empty(n.value, np.int64)
        oc = np.empty(n.value, np.int64 if wide else np.int32)
        call("hh_sample_write_host", h, ptr(o1), ptr(o2), ptr(oc), int(wide), stream)
    finally:
        call("hh_sample_free", h)
    return o1, o2, oc
