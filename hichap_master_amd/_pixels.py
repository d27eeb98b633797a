"""One chromosome of cooler's pixel table as the ``*_pixels`` calls take it
(``bin1, bin2, count, weight, lo, N[, bad]``, NumPy or torch tensors on the
GPU), and the chromosomes a cooler holds for one ``Allelic`` setting."""
from __future__ import annotations

import numpy as np


def is_dev(a):
    return hasattr(a, "data_ptr")


def host_or_dev(a, dtype, dev):
    """``a`` as a contiguous array of ``dtype`` on the side the call runs on."""
    if a is None:
        return None
    if dev is None:
        return np.ascontiguousarray(a, dtype=dtype)
    import torch
    if not is_dev(a):
        a = torch.from_numpy(np.array(a, dtype=dtype))
    return a.to(device=dev, dtype=getattr(torch, np.dtype(dtype).name)).contiguous()


def empty(shape, dtype, dev):
    if dev is None:
        return np.empty(shape, dtype)
    import torch
    return torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=dev)


def table(bin1, bin2, count, weight, N, bad):
    """The call's side (None = host, or the torch device of ``bin1``) and the
    table, weights and ``bad`` as contiguous arrays on that side."""
    dev = bin1.device if is_dev(bin1) else None
    b1, b2 = host_or_dev(bin1, np.int64, dev), host_or_dev(bin2, np.int64, dev)
    c = host_or_dev(count, np.float64, dev)
    if not (tuple(b1.shape) == tuple(b2.shape) == tuple(c.shape)) or b1.ndim != 1:
        raise ValueError("bin1, bin2 and count must be 1-D of the same length")
    wt = host_or_dev(weight, np.float64, dev)
    bad = host_or_dev(bad, np.uint8, dev)
    if bad is not None and tuple(bad.shape) != (int(N),):
        raise ValueError("bad must have one entry per bin")
    return dev, b1, b2, c, wt, bad


def allelic_chroms(allelic, chromnames=()):
    """The chromosomes of ``chromnames`` that ``allelic`` reads: all for
    False, those with the M / P prefix for 'Maternal' / 'Paternal'."""
    if allelic is False:
        return list(chromnames)
    if allelic in ("Maternal", "Paternal"):
        return [x for x in chromnames if x.startswith(allelic[0])]
    raise ValueError(f"Unkonwn key word {allelic}, Only Maternal, Paternal, False allowed")


def chrom_label(allelic, chro):
    """The chromosome's name in output files: without its M / P prefix."""
    return chro if allelic is False else chro[1:]
