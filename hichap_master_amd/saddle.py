"""Cis expected and compartment saddle.

HiCHap has neither quantity: the definitions are this project's.  Both are
sums over cooler's pixel table of one chromosome, global bins [lo, lo + N);
the value of a cell is ``v(a, b) = count * weight[bin1] * weight[bin2]`` (NaN
-> 0; the raw count with ``weight=None``) and a bin is invalid where its
weight is not finite or ``bad`` is set.  The sums run on the GPU
(``hh_expected_pixels`` / ``hh_saddle_pixels``, csrc/saddle.hip), the table is
streamed once per call and the N x N matrix never exists:

* expected: for ``ignore_diags <= d <= max_dist`` the fp64 sum of the stored
  ``v(a, a + d)`` with both bins valid and the number of cells ``(a, a + d)``
  with both bins valid, stored or not; ``expected_from_sums`` divides them;
* saddle: with a class per bin (``digitize_track``: quantile bins of a track,
  255 = left out), ``U[cls[a]][cls[b]]`` adds ``v(a, b) / expected[b - a]``
  over the stored pixels and ``Cu[cls[a]][cls[b]]`` counts every cell
  ``a < b``, both on the usable diagonals (``min_dist <= d <= max_dist``,
  expected finite and > 0); the saddle is ``(U + U.T) / (Cu + Cu.T)``.

The rest is host code on K x K arrays: ``saddle_strength`` (corner contrast
``intra(k) / inter(k)``) and ``write_saddle`` (the three text files).
``SaddleCalling`` is mixed into ``StructureFind`` (``run_Saddle``) the way
``insulation.InsulationCalling`` is.
"""
from __future__ import annotations

import numpy as np

from ._lib import call, ptr, require_gpu
from ._pixels import empty, host_or_dev, table

MAX_CLASSES = 64
LEFT_OUT = 255


def expected_pixels(bin1, bin2, count, weight, lo, N, ignore_diags=2, max_dist=None, bad=None, stream=None):
    """``(sum, nvalid)`` per diagonal 0..max_dist (default N - 1) of one
    chromosome straight from cooler's pixel table: ``sum[d]`` (float64) the sum
    of the balanced stored pixels on diagonal d with both bins valid,
    ``nvalid[d]`` (int64) the cells of the diagonal with both bins valid; both
    0 for ``d < ignore_diags``.  Torch tensors on the GPU are used in place and
    the results stay on the device."""
    require_gpu()
    dev, b1, b2, c, wt, bad = table(bin1, bin2, count, weight, N, bad)
    D = int(N) - 1 if max_dist is None else int(max_dist)
    n_out = max(D + 1, 0)
    s, n = empty((n_out,), np.float64, dev), empty((n_out,), np.int64, dev)
    call("hh_expected_pixels", ptr(b1), ptr(b2), ptr(c), int(b1.shape[0]), ptr(wt),
         0 if wt is None else int(wt.shape[0]), int(lo), int(N), ptr(bad), int(ignore_diags), D, ptr(s), ptr(n),
         0 if dev is None else 1, stream)
    return s, n


def saddle_pixels(bin1, bin2, count, weight, lo, N, expected, cls, K, min_dist=1, max_dist=None, bad=None,
                  stream=None):
    """``(U, Cu)``, K x K (float64, int64): the upper-triangle saddle sums of
    one chromosome.  ``expected``: float64[max_dist + 1]; ``cls``: uint8[N],
    class ids 0..K-1 or 255 for a bin left out.  The symmetric sums are
    ``U + U.T`` and ``Cu + Cu.T``.  Torch tensors on the GPU are used in place
    and the results stay on the device."""
    require_gpu()
    dev, b1, b2, c, wt, bad = table(bin1, bin2, count, weight, N, bad)
    D = int(N) - 1 if max_dist is None else int(max_dist)
    e = host_or_dev(expected, np.float64, dev)
    k = host_or_dev(cls, np.uint8, dev)
    if tuple(e.shape) != (D + 1,):
        raise ValueError("expected must have max_dist + 1 entries")
    if tuple(k.shape) != (int(N),):
        raise ValueError("cls must have one entry per bin")
    K = int(K)
    kk = (max(K, 0), max(K, 0))
    U, Cu = empty(kk, np.float64, dev), empty(kk, np.int64, dev)
    call("hh_saddle_pixels", ptr(b1), ptr(b2), ptr(c), int(b1.shape[0]), ptr(wt),
         0 if wt is None else int(wt.shape[0]), int(lo), int(N), ptr(bad), ptr(e), ptr(k), K, int(min_dist), D,
         ptr(U), ptr(Cu), 0 if dev is None else 1, stream)
    return U, Cu


def expected_from_sums(s, nvalid, ignore_diags=0):
    """``sum / nvalid`` where ``nvalid > 0`` and ``d >= ignore_diags``, NaN
    elsewhere.  No smoothing."""
    s = np.asarray(s, dtype=np.float64)
    n = np.asarray(nvalid)
    ok = (n > 0) & (np.arange(s.size) >= ignore_diags)
    out = np.full(s.shape, np.nan)
    out[ok] = s[ok] / n[ok]
    return out


def digitize_track(tracks, valid=None, n_bins=50, qrange=(0.025, 0.975)):
    """Quantile classes of a track, cooltools' shape.  ``tracks``: {chrom:
    values} in file order; ``valid``: {chrom: uint8} or None.  ``x`` = the
    finite, non-zero values of all chromosomes (gap bins are 0 in this
    project's PC files), ``edges = np.quantile(x, linspace(qlo, qhi, n_bins +
    1))``, ``cls = searchsorted(edges, value, 'right')`` (K = n_bins + 2
    classes, 0 and K - 1 the outliers) and 255 where the value is 0 or not
    finite or the bin is invalid.  Returns ``({chrom: uint8 cls}, edges)``."""
    n_bins = int(n_bins)
    if not 1 <= n_bins <= MAX_CLASSES - 2:
        raise ValueError(f"n_bins must be 1..{MAX_CLASSES - 2}")
    vals = {k: np.asarray(v, dtype=np.float64) for k, v in tracks.items()}
    x = np.concatenate([v[np.isfinite(v) & (v != 0)] for v in vals.values()]) if vals else np.empty(0)
    if x.size == 0:
        raise ValueError("the track has no finite non-zero value")
    edges = np.quantile(x, np.linspace(qrange[0], qrange[1], n_bins + 1))
    out = {}
    for k, v in vals.items():
        ok = np.isfinite(v) & (v != 0)
        if valid is not None and valid.get(k) is not None:
            ok &= np.asarray(valid[k]) != 0
        c = np.full(v.shape, LEFT_OUT, np.uint8)
        c[ok] = np.searchsorted(edges, v[ok], side="right").astype(np.uint8)
        out[k] = c
    return out, edges


def saddle_strength(S, C):
    """``strength[k - 1] = intra(k) / inter(k)`` for k = 1 .. n // 2 on the
    interior (outlier classes dropped) of the symmetric sums S and counts C:
    ``intra(k)`` = the two same-sign k x k corners' sum over their count,
    ``inter(k)`` the two cross corners'.  The headline value is at
    ``k = max(1, n // 5)``."""
    Si = np.asarray(S, dtype=np.float64)[1:-1, 1:-1]
    Ci = np.asarray(C, dtype=np.float64)[1:-1, 1:-1]
    n = Si.shape[0]
    out = np.full(n // 2, np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(1, n // 2 + 1):
            intra = (Si[:k, :k].sum() + Si[-k:, -k:].sum()) / (Ci[:k, :k].sum() + Ci[-k:, -k:].sum())
            inter = (Si[:k, -k:].sum() + Si[-k:, :k].sum()) / (Ci[:k, -k:].sum() + Ci[-k:, :k].sum())
            out[k - 1] = intra / inter
    return out


def write_saddle(expected_fil, saddle_fil, strength_fil, results, Res, edges, S, C, name=lambda chro: chro):
    """The three text files of ``run_Saddle`` (tab-separated, floats as Python 2
    printed them, NaN as 'nan').  ``results``: {chrom: dict(sum=, nvalid=,
    expected=)} in file order; ``edges`` the K - 1 quantile edges; S, C the
    symmetric K x K sums and counts of the genome."""
    from .StructureFind import py2_float_str
    with open(expected_fil, "w") as f:
        f.write("chrom\tdist_bins\tdist_bp\tn_valid\tbalanced_sum\tbalanced_avg\n")
        for chro, r in results.items():
            for d in range(len(r["sum"])):
                f.write("\t".join([name(chro), str(d), str(d * Res), str(int(r["nvalid"][d])),
                                   py2_float_str(r["sum"][d]), py2_float_str(r["expected"][d])]) + "\n")
    S = np.asarray(S, dtype=np.float64)
    C = np.asarray(C)
    sad = np.full(S.shape, np.nan)
    sad[C > 0] = S[C > 0] / C[C > 0]
    with open(saddle_fil, "w") as f:
        f.write("\t".join(py2_float_str(e) for e in edges) + "\n")
        for row in sad:
            f.write("\t".join(py2_float_str(x) for x in row) + "\n")
    with open(strength_fil, "w") as f:
        f.write("k\tstrength\n")
        for k, x in enumerate(saddle_strength(S, C), start=1):
            f.write(f"{k}\t{py2_float_str(x)}\n")


class SaddleCalling:
    """The expected / saddle methods of ``StructureFind``."""

    def _saddle_track(self, track, PC_file, chroms, name):
        """{chrom: track} for the cooler's chromosomes: ``track``, else the
        last ``Compartment`` run, else ``PC_file`` (haplotype chromosomes are
        looked up without their M/P prefix there)."""
        if track is not None:
            src, key = track, (lambda chro: chro)
        elif getattr(self, "Compartment_Dict", None):
            src, key = self.Compartment_Dict, (lambda chro: chro)
        elif PC_file is not None:
            src, key = self.Loading_Tranditional_PC(PC_file), name
        else:
            raise ValueError("run_Saddle: no track (pass track=, run Compartment first, or pass PC_file=)")
        missing = [chro for chro in chroms if key(chro) not in src]
        if missing:
            raise ValueError(f"run_Saddle: the track has no values for {missing}")
        return {chro: np.asarray(src[key(chro)], dtype=np.float64) for chro in chroms}

    def run_Saddle(self, OutPath, track=None, PC_file=None, n_bins=50, qrange=(0.025, 0.975), ignore_diags=2,
                   min_dist=None, max_dist=None):
        """Cis expected, compartment saddle and saddle strength to text files,
        per chromosome straight from the cooler's pixel table.  The track is
        ``track`` ({chrom: array}), else ``Compartment_Dict`` of an earlier
        ``Compartment`` run, else ``PC_file`` (``Loading_Tranditional_PC``);
        it is cut into ``n_bins`` quantile classes between ``qrange`` plus two
        outlier classes.  Distances in bp: ``min_dist`` defaults to
        ``max(1, ignore_diags)`` bins, ``max_dist`` to the whole chromosome.
        Traditional data uses ``bins/weight``; haplotype data ('Maternal' /
        'Paternal') the raw counts, with the chromosome's gap list as invalid
        bins when a ``GapFile`` was given.  Writes
        ``<prefix>_Expected_<res>.txt`` (chrom, dist_bins, dist_bp, n_valid,
        balanced_sum, balanced_avg), ``<prefix>_Saddle_<res>.txt`` (the K - 1
        quantile edges, then the K rows of S / C) and
        ``<prefix>_SaddleStrength_<res>.txt`` (k, strength), haplotype
        chromosomes without their M/P prefix.  Returns (and keeps as
        ``Saddle_dict``) the arrays."""
        from .coolio import Cooler
        self._chroms()
        g = int(ignore_diags)
        dmin = max(1, g) if min_dist is None else int(min_dist / self.Res)
        if g < 0 or dmin < 1:
            raise ValueError("run_Saddle: ignore_diags must be >= 0 and min_dist at least one bin")
        stream = getattr(self, "stream", None)
        K = int(n_bins) + 2
        S, C = np.zeros((K, K)), np.zeros((K, K), np.int64)
        results = {}
        with Cooler(self.cooler_fil) as c:
            geom = list(self._cooler_walk(c, "run_Saddle"))  # the classes need every chromosome's valid bins
            valid = {row[0]: row[5] for row in geom}
            tracks = self._saddle_track(track, PC_file, list(valid), self._name)
            for chro, _, N, *_ in geom:
                if tracks[chro].shape != (N,):
                    raise ValueError(f"run_Saddle: the track of {chro} has {tracks[chro].size} values, "
                                     f"the chromosome {N} bins")
            cls, edges = digitize_track(tracks, valid, n_bins, qrange)
            for chro, lo, N, wt, bad, _ in geom:
                b1, b2, cnt = c.pixel_rows(lo, lo + N)
                D = N - 1 if max_dist is None else min(N - 1, int(max_dist / self.Res))
                s, n = expected_pixels(b1, b2, cnt, wt, lo, N, g, D, bad, stream)
                e = expected_from_sums(s, n, g)
                r = dict(size=c.chromsizes[chro], valid=valid[chro], cls=cls[chro], sum=s, nvalid=n, expected=e)
                if dmin <= D:                              # (a chromosome shorter than min_dist adds nothing)
                    U, Cu = saddle_pixels(b1, b2, cnt, wt, lo, N, e, cls[chro], K, dmin, D, bad, stream)
                    S += U + U.T
                    C += Cu + Cu.T
                    r.update(U=U, Cu=Cu)
                results[chro] = r
        write_saddle(self._out_path(OutPath, "Expected"), self._out_path(OutPath, "Saddle"),
                     self._out_path(OutPath, "SaddleStrength"), results, self.Res, edges, S, C, self._name)
        with np.errstate(divide="ignore", invalid="ignore"):
            saddle = np.where(C > 0, S / C, np.nan)
        self.Saddle_dict = dict(chroms=results, edges=edges, S=S, C=C, saddle=saddle, strength=saddle_strength(S, C))
        return self.Saddle_dict
