"""``cooler merge`` on the GPU, straight from cooler's pixel tables (DESIGN.md
§4r).

The union of K (1 .. 64) pixel tables over the same bin table: every pixel
present in at least one input, its count the exact integer sum over the
inputs; a stored count of 0 keeps its pixel.  Inputs and output are cooler's
tables (sorted by (bin1, bin2), upper triangle, unique).  The sums run in
``hh_merge_count`` / ``hh_merge_write`` (csrc/merge.hip): coarsening by 1 over
several tables, no key sort, bitwise the same on every run and for every
order of the tables.

* ``merge_pixels``: host arrays or device tensors.

The file level (``merge_coolers``) is in ``coolio.py``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import call, ptr, require_gpu
from ._pixels import is_dev
from .coarsen import INT32_MAX, integer_counts

MAX_TABLES = 64


def _pointers(arrays):
    return (C.c_void_p * len(arrays))(*[(ptr(a).value if a is not None and _numel(a) else None) for a in arrays])


def _numel(a):
    return int(a.numel()) if hasattr(a, "numel") else int(a.size)


def merge_pixels(tables, n_bins, stream=None):
    """Merge ``tables``, a sequence of 1 .. 64 ``(bin1, bin2, count)`` over one
    bin table of ``n_bins`` bins: ``(bin1, bin2, count)``.  All NumPy, or all
    torch tensors on the GPU.  NumPy inputs return NumPy arrays (int64 ids);
    tensors are used in place (int32 ids; int32 or int64 counts per table) and
    the result stays on the device (int32 ids).  Counts come back int32 while
    the largest sum is <= 2^31 - 1, int64 otherwise.  Float counts that are
    all integer-valued are cast; other float counts raise ``ValueError``, as
    do no tables, more than 64, and a mix of host and device tables.  A table
    that is not sorted unique upper-triangle with ids in ``[0, n_bins)`` and
    counts >= 0 raises ``HipLibraryError`` (HH_ERR_ARG) naming the table and
    its first offending pixel."""
    tables = [tuple(t) for t in tables]
    K = len(tables)
    if K < 1:
        raise ValueError("merge_pixels: no tables")
    if K > MAX_TABLES:
        raise ValueError(f"merge_pixels: {K} tables; at most {MAX_TABLES} are merged in one call")
    if any(len(t) != 3 for t in tables):
        raise ValueError("merge_pixels: every table is (bin1, bin2, count)")
    dev = [any(is_dev(x) for x in t) for t in tables]
    if any(dev) and not all(is_dev(x) for t in tables for x in t):
        raise ValueError("merge_pixels: the tables must be all NumPy arrays or all GPU tensors")
    if int(n_bins) != n_bins or int(n_bins) < 1:
        raise ValueError("merge_pixels: n_bins must be an integer >= 1")
    n_bins = int(n_bins)
    h, n, mx = C.c_void_p(), C.c_int64(0), C.c_int64(0)
    if dev[0]:
        import torch
        b1s, b2s, cs = [], [], []
        for t, (b1, b2, c) in enumerate(tables):
            b1, b2 = (x.to(torch.int32).contiguous() for x in (b1, b2))
            if c.dtype.is_floating_point:
                if not bool(torch.all(torch.isfinite(c) & (c == torch.floor(c)))):
                    raise ValueError("GPU merging takes integer counts")
                c = c.to(torch.int64)
            elif c.dtype not in (torch.int32, torch.int64):
                c = c.to(torch.int64)
            c = c.contiguous()
            if not (b1.ndim == 1 and tuple(b1.shape) == tuple(b2.shape) == tuple(c.shape)):
                raise ValueError(f"merge_pixels: table {t}: bin1, bin2 and count must be 1-D of the same length")
            if b1.device != tables[0][0].device:
                raise ValueError("merge_pixels: the tables must be on one device")
            b1s.append(b1), b2s.append(b2), cs.append(c)
        require_gpu()
        device = b1s[0].device
        nnz = np.array([x.numel() for x in b1s], dtype=np.int64)
        c64 = np.array([c.dtype == torch.int64 for c in cs], dtype=np.int32)
        call("hh_merge_count", _pointers(b1s), _pointers(b2s), _pointers(cs), ptr(c64), ptr(nnz), K, n_bins, 1,
             stream, C.byref(h), C.byref(n), C.byref(mx))
        try:
            wide = mx.value > INT32_MAX
            o1 = torch.empty(n.value, dtype=torch.int32, device=device)
            o2 = torch.empty(n.value, dtype=torch.int32, device=device)
            oc = torch.empty(n.value, dtype=torch.int64 if wide else torch.int32, device=device)
            call("hh_merge_write", h, ptr(o1), ptr(o2), ptr(oc), int(wide), stream)
        finally:
            call("hh_merge_free", h)
        return o1, o2, oc
    b1s, b2s, cs = [], [], []
    for t, (b1, b2, c) in enumerate(tables):
        b1 = np.ascontiguousarray(b1, dtype=np.int64)
        b2 = np.ascontiguousarray(b2, dtype=np.int64)
        c = integer_counts(c, "GPU merging")
        if not (b1.ndim == 1 and b1.shape == b2.shape == c.shape):
            raise ValueError(f"merge_pixels: table {t}: bin1, bin2 and count must be 1-D of the same length")
        b1s.append(b1), b2s.append(b2), cs.append(c)
    require_gpu()
    nnz = np.array([x.size for x in b1s], dtype=np.int64)
    call("hh_merge_count_host", _pointers(b1s), _pointers(b2s), _pointers(cs), ptr(nnz), K, n_bins, stream,
         C.byref(h), C.byref(n), C.byref(mx))
    try:
        wide = mx.value > INT32_MAX
        o1, o2 = np.empty(n.value, np.int64), np.empty(n.value, np.int64)
        oc = np.empty(n.value, np.int64 if wide else np.int32)
        call("hh_merge_write_host", h, ptr(o1), ptr(o2), ptr(oc), int(wide), stream)
    finally:
        call("hh_merge_free", h)
    return o1, o2, oc
