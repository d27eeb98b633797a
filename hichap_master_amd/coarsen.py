"""``cooler coarsen`` / ``cooler zoomify`` on the GPU, straight from cooler's
pixel table.

Fine bin ``i`` of chromosome ``c`` maps to coarse bin ``coff_c + (i - off_c)
// k`` with ``coff`` the running sum of ``ceil(nbins_c / k)``: a coarse bin
never spans two chromosomes and the last one of a chromosome may hold fewer
than ``k`` fine bins.  The coarse table is again cooler's (sorted by (bin1,
bin2), upper triangle, unique), every count the exact integer sum of the fine
pixels of its cell.  The sums run in ``hh_coarsen_count`` / ``hh_coarsen_write``
(csrc/coarsen.hip): no key sort, bitwise the same on every run.

* ``coarse_offsets`` / ``coarse_bin_map``: the map, pure NumPy.
* ``coarsen_pixels``: one level, host arrays or device tensors.
* ``zoom_plan``: which level each resolution of a zoomify is taken from.

The file level (``coarsen_cooler``, ``zoomify``) is in ``coolio.py``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import call, ptr, require_gpu
from ._pixels import is_dev

TILE = 8192  # HH_COARSEN_TILE: coarse columns per work item (the default of hh_tune "coarsen_tile")
INT32_MAX = 2 ** 31 - 1


def tile_width():
    """The column-tile width in force (``hh_tune("coarsen_tile", T)`` lowers it)."""
    t = C.c_int32(0)
    call("hh_coarsen_tile", C.byref(t))
    return int(t.value)


def _offsets(chrom_offsets, k):
    off = np.ascontiguousarray(chrom_offsets, dtype=np.int64).ravel()
    if int(k) != k or int(k) < 1:
        raise ValueError("the coarsening factor must be an integer >= 1")
    if off.size < 2 or off[0] != 0 or np.any(np.diff(off) < 0):
        raise ValueError("chrom_offsets must start at 0 and not decrease")
    return off, int(k)


def coarse_offsets(chrom_offsets, k):
    """Chromosome offsets of the coarse bin table: the running sum of
    ``ceil(nbins_c / k)``."""
    off, k = _offsets(chrom_offsets, k)
    return np.concatenate([[0], np.cumsum(-(-np.diff(off) // k))]).astype(np.int64)


def coarse_bin_map(chrom_offsets, k):
    """``map[i]`` = coarse bin of fine bin ``i`` (int64[n_bins])."""
    off, k = _offsets(chrom_offsets, k)
    coff = coarse_offsets(off, k)
    i = np.arange(int(off[-1]), dtype=np.int64)
    c = np.searchsorted(off, i, side="right") - 1
    return coff[c] + (i - off[c]) // k


def zoom_plan(base_res, resolutions):
    """``[(res, src_res, factor)]`` in ascending ``res``: every level is taken
    from the largest resolution already there (the base or an earlier target)
    that divides it.  A target that is not a multiple of the base, or is <=
    it, raises ``ValueError``."""
    base = int(base_res)
    if base < 1:
        raise ValueError("the base resolution must be >= 1")
    have, plan = [base], []
    for res in sorted({int(r) for r in resolutions}):
        if res <= base or res % base:
            raise ValueError(f"resolution {res} is not a multiple of the base resolution {base} larger than it")
        src = max(h for h in have if res % h == 0)
        plan.append((res, src, res // src))
        have.append(res)
    return plan


def integer_counts(count, who="GPU coarsening"):
    """Host counts as int64; float counts only when all are integer-valued
    (``who``: the operation the message speaks for; merging and down-sampling
    share this)."""
    count = np.asarray(count)
    if count.dtype.kind == "f":
        if not np.all(np.isfinite(count)) or np.any(count != np.floor(count)):
            raise ValueError(f"{who} takes integer counts (the float64 haplotype coolers are written at "
                             "every resolution by their construction driver)")
    elif count.dtype.kind not in "iub":
        raise ValueError(f"{who} takes integer counts")
    return np.ascontiguousarray(count, dtype=np.int64)


def coarsen_device(p1, p2, pc, count_is_i64, nnz, chrom_offsets, k, device, stream=None):
    """One level from raw device pointers (int32 ids, int32 / int64 counts) to
    torch tensors on ``device``: ``(bin1, bin2, count, coarse_offsets)``."""
    import torch
    require_gpu()
    off, k = _offsets(chrom_offsets, k)
    h, n, mx = C.c_void_p(), C.c_int64(0), C.c_int64(0)
    call("hh_coarsen_count", C.c_void_p(p1), C.c_void_p(p2), C.c_void_p(pc), int(bool(count_is_i64)), int(nnz),
         int(off[-1]), ptr(off), off.size - 1, k, 1, stream, C.byref(h), C.byref(n), C.byref(mx))
    try:
        wide = mx.value > INT32_MAX
        o1 = torch.empty(n.value, dtype=torch.int32, device=device)
        o2 = torch.empty(n.value, dtype=torch.int32, device=device)
        oc = torch.empty(n.value, dtype=torch.int64 if wide else torch.int32, device=device)
        call("hh_coarsen_write", h, ptr(o1), ptr(o2), ptr(oc), int(wide), stream)
    finally:
        call("hh_coarsen_free", h)
    return o1, o2, oc, coarse_offsets(off, k)


def coarsen_pixels(bin1, bin2, count, chrom_offsets, k, stream=None):
    """Coarsen cooler's pixel table by the integer factor ``k``: ``(bin1,
    bin2, count, coarse_chrom_offsets)``.  NumPy inputs return NumPy arrays
    (int64 ids); torch tensors on the GPU are used in place (int32 ids; int32
    or int64 counts) and the result stays on the device (int32 ids).  Counts
    come back int32 while the largest sum is <= 2^31 - 1, int64 otherwise.
    Float counts that are all integer-valued are cast; other float counts
    raise ``ValueError``.  A table that is not sorted unique upper-triangle
    with ids in range and counts >= 0 raises ``HipLibraryError`` (HH_ERR_ARG)
    naming the first offending pixel."""
    off, k = _offsets(chrom_offsets, k)
    if is_dev(bin1):
        import torch
        b1, b2 = (x.to(torch.int32).contiguous() for x in (bin1, bin2))
        c = count
        if c.dtype.is_floating_point:
            if not bool(torch.all(torch.isfinite(c) & (c == torch.floor(c)))):
                raise ValueError("GPU coarsening takes integer counts")
            c = c.to(torch.int64)
        elif c.dtype not in (torch.int32, torch.int64):
            c = c.to(torch.int64)
        c = c.contiguous()
        if not (b1.ndim == 1 and tuple(b1.shape) == tuple(b2.shape) == tuple(c.shape)):
            raise ValueError("bin1, bin2 and count must be 1-D of the same length")
        return coarsen_device(b1.data_ptr(), b2.data_ptr(), c.data_ptr(), c.dtype == torch.int64, b1.numel(), off, k,
                              b1.device, stream)
    b1 = np.ascontiguousarray(bin1, dtype=np.int64)
    b2 = np.ascontiguousarray(bin2, dtype=np.int64)
    c = integer_counts(count)
    if not (b1.ndim == 1 and b1.shape == b2.shape == c.shape):
        raise ValueError("bin1, bin2 and count must be 1-D of the same length")
    require_gpu()
    h, n, mx = C.c_void_p(), C.c_int64(0), C.c_int64(0)
    call("hh_coarsen_count_host", ptr(b1), ptr(b2), ptr(c), b1.size, int(off[-1]), ptr(off), off.size - 1, k, stream,
         C.byref(h), C.byref(n), C.byref(mx))
    try:
        wide = mx.value > INT32_MAX
        o1, o2 = np.empty(n.value, np.int64), np.empty(n.value, np.int64)
        oc = np.empty(n.value, np.int64 if wide else np.int32)
        call("hh_coarsen_write_host", h, ptr(o1), ptr(o2), ptr(oc), int(wide), stream)
    finally:
        call("hh_coarsen_free", h)
    return o1, o2, oc, coarse_offsets(off, k)
