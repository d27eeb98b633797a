"""Diamond insulation score and insulation boundaries.

HiCHap has no insulation score: the definition is this project's.  For bin i
of a chromosome, a window of w bins and ``ignore_diags = g`` the diamond is
``C_w(i) = {(a, b): i - w < a <= i <= b < i + w, b - a >= g}`` clipped to the
chromosome; ``S_w(i)`` is the sum of the balanced matrix over the diamond's
cells with both bins valid and ``n_w(i)`` their number.  The sums run on the
GPU for up to 8 windows in one launch (``hh_insulation_scan`` /
``hh_insulation_pixels``, K11 in csrc/comp.hip), straight from cooler's pixel
table: the N x N matrix never exists.  The rest is O(N) host code:

* ``insulation_track``: ``score = S / n`` where enough of the diamond is
  valid, ``log2(score / nanmedian(score))``;
* ``insulation_boundaries``: strict local minima of the finite entries with
  their topographic prominence, what ``scipy.signal.find_peaks(-x)`` and
  ``peak_prominences`` give (scipy is not used: it is the tests' check).

``InsulationCalling`` is mixed into ``StructureFind`` (``Get_Insulation``,
``run_Insulation``) the way ``tads.TADCalling`` is.
"""
from __future__ import annotations

import numpy as np

from ._lib import call, ptr, require_gpu
from ._pixels import host_or_dev, is_dev, table

MAX_WINDOWS, MAX_WINDOW = 8, 256


def _out(n_w, N, dev):
    """S (float64) and n (int32), n_w x N: torch tensors on ``dev`` or NumPy."""
    if dev is None:
        return np.empty((n_w, N), np.float64), np.empty((n_w, N), np.int32)
    import torch
    return (torch.empty((n_w, N), dtype=torch.float64, device=dev),
            torch.empty((n_w, N), dtype=torch.int32, device=dev))


def diamond_sums_band(band, valid, windows, ignore_diags=1, stream=None):
    """``(S, n)`` of the diamonds from the diagonal-major band of the DI scans
    (``column_band``; (2B+1) x N with B >= 2 * max(windows) - 2).  ``windows``
    in bins, ascending; ``valid`` uint8[N] or None.  A torch band on the GPU
    is scanned in place and the results stay there."""
    require_gpu()
    dev = band.device if is_dev(band) else None
    band = host_or_dev(band, np.float64, dev)
    if band.ndim != 2 or band.shape[0] % 2 != 1:
        raise ValueError("band must be (2B+1) x N")
    B, N = band.shape[0] // 2, band.shape[1]
    valid = host_or_dev(valid, np.uint8, dev)
    if valid is not None and tuple(valid.shape) != (N,):
        raise ValueError("valid must have one entry per bin")
    w = np.ascontiguousarray(windows, dtype=np.int32).ravel()
    S, n = _out(w.size, N, dev)
    call("hh_insulation_scan", ptr(band), N, B, ptr(valid), ptr(w), w.size, int(ignore_diags), ptr(S), ptr(n),
         0 if dev is None else 1, stream)
    return S, n


def diamond_sums(M, windows, ignore_diags=1, valid=None, stream=None):
    """``(S, n)`` of the diamonds of one dense N x N matrix (NaN already 0):
    its band goes through ``column_band``, so N x N never crosses PCIe."""
    from .StructureFind import column_band
    w = np.ascontiguousarray(windows, dtype=np.int32).ravel()
    B = 2 * int(w.max()) - 2 if w.size and 1 <= w.max() <= MAX_WINDOW else 0
    return diamond_sums_band(column_band(M, B), valid, w, ignore_diags, stream)


def diamond_sums_pixels(bin1, bin2, count, weight, lo, N, windows, ignore_diags=1, bad=None, stream=None):
    """``(S, n)`` of one chromosome's diamonds straight from cooler's pixel
    table: ``bin1 <= bin2`` are global bin ids of unique pixels, the
    chromosome is bins [lo, lo + N), the value of a cell is
    ``count * weight[bin1] * weight[bin2]`` (NaN -> 0), or the raw count with
    ``weight=None``.  A bin is invalid where its weight is not finite or
    ``bad`` (uint8[N]) is set.  Torch tensors on the GPU are used in place and
    the results stay on the device."""
    require_gpu()
    dev, b1, b2, c, wt, bad = table(bin1, bin2, count, weight, N, bad)
    w = np.ascontiguousarray(windows, dtype=np.int32).ravel()
    S, n = _out(w.size, int(N), dev)
    call("hh_insulation_pixels", ptr(b1), ptr(b2), ptr(c), int(b1.shape[0]), ptr(wt),
         0 if wt is None else int(wt.shape[0]), int(lo), int(N), ptr(bad), ptr(w), w.size, int(ignore_diags),
         ptr(S), ptr(n), 0 if dev is None else 1, stream)
    return S, n


def full_cells(w, g):
    """``#{(s, t) in [0, w)^2 : s + t >= g}``: the cells of an unclipped diamond."""
    w, g = int(w), int(g)
    below = sum(min(d, w - 1) - max(0, d - w + 1) + 1 for d in range(min(g, 2 * w - 1)))
    return w * w - below


def insulation_track(S, n, valid, w, g, min_frac_valid=0.66):
    """``log2(score / nanmedian(score))`` of one window: ``score = S / n``
    where the bin is valid, n > 0 and n >= min_frac_valid * full(w, g), NaN
    elsewhere (the clipped diamonds at the chromosome's ends among them);
    non-finite values -- those of a score of 0 too -- are NaN, and so is
    everything when no score is finite."""
    S = np.asarray(S, dtype=np.float64)
    n = np.asarray(n)
    ok = (np.asarray(valid) != 0) & (n > 0) & (n >= min_frac_valid * full_cells(w, g))
    score = np.full(S.shape, np.nan)
    score[ok] = S[ok] / n[ok]
    L = np.full(S.shape, np.nan)
    if not np.isnan(score).all():
        med = np.nanmedian(score)
        with np.errstate(divide="ignore", invalid="ignore"):
            L = np.log2(score / med)
        L[~np.isfinite(L)] = np.nan
    return L


def _reach_max(x):
    """out[p] = max of x over (j, p], j the nearest index left of p with
    x[j] < x[p] (or -1): one pass with a stack of increasing values."""
    out = [0.0] * len(x)
    stack = []  # (value, max over the stretch it stands for), values increasing
    for p, v in enumerate(x):
        m = v
        while stack and stack[-1][0] >= v:
            m = max(m, stack.pop()[1])
        out[p] = m
        stack.append((v, m))
    return out


def insulation_boundaries(L, min_strength=0.1):
    """Insulation boundaries of one log2 track: ``(index, strength, called)``.
    x = the finite entries of L (NaNs are skipped, not walls); a boundary is a
    strict local minimum of x -- a plateau counts once, at its midpoint
    rounded down, the first and last entries never -- and its strength the
    topographic prominence of the minimum: min(highest x on the way left to
    the first lower value, the same to the right) - x.  ``index`` points into
    L, ``called = strength >= min_strength``."""
    L = np.asarray(L, dtype=np.float64)
    where = np.nonzero(np.isfinite(L))[0]
    x = L[where].tolist()
    m = len(x)
    peaks = []
    i = 1
    while i < m - 1:
        if x[i - 1] > x[i]:
            j = i + 1
            while j < m - 1 and x[j] == x[i]:
                j += 1
            if x[j] > x[i]:
                peaks.append((i + j - 1) // 2)
                i = j
        i += 1
    left, right = _reach_max(x), _reach_max(x[::-1])[::-1]
    idx = where[np.array(peaks, dtype=np.int64)] if peaks else np.empty(0, np.int64)
    strength = np.array([min(left[p], right[p]) - x[p] for p in peaks], dtype=np.float64)
    return idx.astype(np.int64), strength, strength >= min_strength


def write_insulation(track_fil, boundary_fil, results, Res, wbins, min_strength=0.1, name=lambda chro: chro):
    """The two text files of ``run_Insulation`` (tab-separated, floats as
    Python 2 printed them, NaN as 'nan').  ``results``: {chrom: dict(size=bp,
    valid=uint8[N], L=[n_w][N], n=[n_w][N], strength=[n_w][N])} in file order,
    ``strength`` the prominence at every local minimum and NaN elsewhere;
    ``wbins`` the windows in bins."""
    from .StructureFind import StructureFind, py2_float_str
    units = [StructureFind.properU(w * Res) for w in wbins]
    with open(track_fil, "w") as f:
        head = ["chrom", "start", "end", "valid"]
        for u in units:
            head += [f"log2_insulation_{u}", f"n_valid_{u}", f"boundary_strength_{u}"]
        f.write("\t".join(head) + "\n")
        for chro, r in results.items():
            for i in range(len(r["valid"])):
                row = [name(chro), str(i * Res), str(min((i + 1) * Res, int(r["size"]))), str(int(r["valid"][i]))]
                for k in range(len(wbins)):
                    row += [py2_float_str(r["L"][k][i]), str(int(r["n"][k][i])), py2_float_str(r["strength"][k][i])]
                f.write("\t".join(row) + "\n")
    with open(boundary_fil, "w") as f:
        f.write("chrom\tpos\twindow\tstrength\n")
        for chro, r in results.items():
            for k, w in enumerate(wbins):
                s = np.asarray(r["strength"][k])
                for i in np.nonzero(s >= min_strength)[0]:
                    f.write(f"{name(chro)}\t{int(i) * Res}\t{w * Res}\t{py2_float_str(s[i])}\n")


def _tracks(S, n, valid, wbins, g, min_frac_valid):
    """Per window the log2 track and the strength column (NaN off the minima)."""
    Ls, Ss = [], []
    for k, w in enumerate(wbins):
        L = insulation_track(S[k], n[k], valid, w, g, min_frac_valid)
        idx, strength, _ = insulation_boundaries(L, 0.0)
        col = np.full(L.shape, np.nan)
        col[idx] = strength
        Ls.append(L)
        Ss.append(col)
    return np.array(Ls), np.array(Ss)


class InsulationCalling:
    """The insulation-score methods of ``StructureFind``."""

    def Get_Insulation(self, M, windows, ignore_diags=1, min_frac_valid=0.66):
        """The log2 insulation tracks ([len(windows)][N]) of one dense matrix,
        beside ``Get_DI``.  ``windows`` in bins, ascending.  Rows that are NaN
        on the diagonal (cooler's masked bins) are invalid; NaN counts as 0."""
        M = np.asarray(M, dtype=np.float64)
        valid = np.isfinite(np.diagonal(M)).astype(np.uint8)
        wbins = [int(w) for w in windows]
        S, n = diamond_sums(np.nan_to_num(M), wbins, ignore_diags, valid, getattr(self, "stream", None))
        return _tracks(S, n, valid, wbins, ignore_diags, min_frac_valid)[0]

    def run_Insulation(self, OutPath, windows=(600000,), ignore_diags=1, min_frac_valid=0.66, min_strength=0.1):
        """Insulation score and boundaries to text files, per chromosome
        straight from the cooler's pixel table.  ``windows`` in bp (each
        ``int(window / Res)`` >= 1 bins, distinct).  Traditional data uses
        ``bins/weight``; haplotype data ('Maternal' / 'Paternal') the raw
        counts, with the chromosome's gap list as invalid bins when a
        ``GapFile`` was given.  Writes ``<prefix>_Insulation_<res>.txt`` (one
        line per bin: chrom, start, end, valid and per window the log2 score,
        the diamond's valid cells and the prominence at local minima) and
        ``<prefix>_InsulationBoundary_<res>.txt`` (chrom, pos = start of the
        boundary bin, window in bp, strength; minima with strength >=
        min_strength), haplotype chromosomes without their M/P prefix.
        Returns (and keeps as ``Insulation_dict``) the per-chromosome arrays."""
        from .coolio import Cooler
        self._chroms()
        wbins = sorted(int(w / self.Res) for w in windows)
        if not wbins or wbins[0] < 1 or len(set(wbins)) != len(wbins):
            raise ValueError("run_Insulation: every window must span >= 1 bin and the bin counts must be distinct")
        if len(wbins) > MAX_WINDOWS or wbins[-1] > MAX_WINDOW:
            raise ValueError(f"run_Insulation: at most {MAX_WINDOWS} windows of at most {MAX_WINDOW} bins")
        results = {}
        with Cooler(self.cooler_fil) as c:
            for chro, lo, N, wt, bad, valid in self._cooler_walk(c, "run_Insulation"):
                b1, b2, v = c.pixel_rows(lo, lo + N)
                S, n = diamond_sums_pixels(b1, b2, v, wt, lo, N, wbins, ignore_diags, bad,
                                           getattr(self, "stream", None))
                L, strength = _tracks(S, n, valid, wbins, ignore_diags, min_frac_valid)
                results[chro] = dict(size=c.chromsizes[chro], valid=valid, S=S, n=n, L=L, strength=strength)
        write_insulation(self._out_path(OutPath, "Insulation"), self._out_path(OutPath, "InsulationBoundary"),
                         results, self.Res, wbins, min_strength, self._name)
        self.Insulation_dict = results
        return results
