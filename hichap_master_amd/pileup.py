"""Pileups: aggregate loop and boundary analysis.

HiCHap has no pileup: the definition is this project's.  A pileup is the mean
observed or observed-over-expected contact map in a ``W x W`` window (``W = 2
flank + 1`` bins) around a list of features of the same kind -- loops, domain
corners, boundaries -- also called aggregate peak analysis (APA) or the
"average loop" / "average boundary" plot.  The sums run on the GPU
(``hh_pileup_pixels``, csrc/pileup.hip) straight from cooler's pixel table of
one chromosome, global bins [lo, lo + N), with ``saddle.expected_pixels``'
conventions: the value of a cell is ``v(a, b) = count * weight[bin1] *
weight[bin2]`` (NaN -> 0; the raw count with ``weight=None``) and a bin is
invalid where its weight is not finite or ``bad`` is set.  Neither the N x N
matrix nor the stack of the M windows exists.

Feature k has the chromosome-local centre ``(row[k], col[k])``, ``row <= col``
(``row == col``: an on-diagonal feature); window cell ``(u, v)`` is the cell
``i = row[k] - flank + u, j = col[k] - flank + v`` of the symmetric matrix, at
distance ``d = |i - j|``.  It is eligible when both bins are inside the
chromosome and valid, ``d >= min_dist`` and, with an expected, ``d <
len(expected)`` and ``expected[d]`` is finite and > 0.  ``Cn[u][v]`` counts
the features whose cell is eligible, ``S[u][v]`` adds ``v`` (over
``expected[d]``) of those that are stored pixels as well; the pileup is ``S /
Cn``.

The rest is host code on W x W arrays: ``pileup_from_sums``, ``apa_scores``,
``shifted_controls`` (features moved along the diagonal: the normalisation
when no expected is wanted) and ``write_pileup``.  ``PileupCalling`` is mixed
into ``StructureFind`` (``run_Pileup``) the way ``saddle.SaddleCalling`` is.
"""
from __future__ import annotations

import numpy as np

from ._lib import call, ptr, require_gpu
from ._pixels import empty, host_or_dev, table
from .saddle import expected_from_sums, expected_pixels

MAX_FLANK = 63
APA_NAMES = ("peak", "P2M", "P2UL", "P2UR", "P2LL", "P2LR", "ZscoreLL")


def pileup_pixels(bin1, bin2, count, weight, lo, N, row, col, flank, expected=None, min_dist=0, bad=None,
                  stream=None):
    """``(S, Cn)``, W x W (float64, int64), ``W = 2 * flank + 1``: the pileup
    sums of one chromosome around the features ``(row[k], col[k])`` (local
    bins, ``row <= col``; any order, repeats allowed; a window may leave the
    chromosome).  ``expected``: float64[n], 1 <= n <= N, or None for an
    observed pileup; ``min_dist`` in bins.  Torch tensors on the GPU are used
    in place and the results stay on the device."""
    require_gpu()
    dev, b1, b2, c, wt, bad = table(bin1, bin2, count, weight, N, bad)
    r, q = host_or_dev(row, np.int32, dev), host_or_dev(col, np.int32, dev)
    if r.ndim != 1 or tuple(r.shape) != tuple(q.shape):
        raise ValueError("row and col must be 1-D of the same length")
    e = host_or_dev(expected, np.float64, dev)
    if e is not None and e.ndim != 1:
        raise ValueError("expected must be 1-D")
    W = 2 * int(flank) + 1 if 0 <= int(flank) <= MAX_FLANK else 0
    S, Cn = empty((W, W), np.float64, dev), empty((W, W), np.int64, dev)
    call("hh_pileup_pixels", ptr(b1), ptr(b2), ptr(c), int(b1.shape[0]), ptr(wt),
         0 if wt is None else int(wt.shape[0]), int(lo), int(N), ptr(bad), ptr(r), ptr(q), int(r.shape[0]),
         int(flank), ptr(e), 0 if e is None else int(e.shape[0]), int(min_dist), ptr(S), ptr(Cn),
         0 if dev is None else 1, stream)
    return S, Cn


def pileup_from_sums(S, Cn):
    """``S / Cn``, NaN where ``Cn == 0``."""
    S = np.asarray(S, dtype=np.float64)
    Cn = np.asarray(Cn)
    out = np.full(S.shape, np.nan)
    ok = Cn > 0
    out[ok] = S[ok] / Cn[ok]
    return out


def _nanmean(x):
    x = np.asarray(x, dtype=np.float64).ravel()
    x = x[~np.isnan(x)]
    return float(x.mean()) if x.size else float("nan")


def _ratio(a, b):
    return a / b if b == b and b != 0 else float("nan")


def apa_scores(P, corner=None):
    """The APA scores of a W x W pileup (W odd, flank = W // 2), as a dict:
    ``peak = P[f][f]``; ``P2M`` = peak over the mean of all other cells;
    ``P2UL``, ``P2UR``, ``P2LL``, ``P2LR`` = peak over the mean of the q x q
    corner, ``q = corner or max(1, flank // 2)`` (the lower-left corner
    ``P[W - q:, :q]`` is the one nearer the diagonal for ``row < col``);
    ``ZscoreLL = (peak - mean(LL)) / std(LL, ddof=1)``.  Means and deviations
    skip NaN cells; a score is NaN where its denominator is 0 or has no
    cells."""
    P = np.asarray(P, dtype=np.float64)
    W = P.shape[0]
    if P.ndim != 2 or P.shape != (W, W) or W % 2 != 1:
        raise ValueError("the pileup must be W x W with W odd")
    f = W // 2
    q = int(corner) if corner else max(1, f // 2)
    if not 1 <= q <= W:
        raise ValueError("corner must be 1..W")
    peak = float(P[f, f])
    rest = np.ones((W, W), bool)
    rest[f, f] = False
    corners = dict(UL=P[:q, :q], UR=P[:q, W - q:], LL=P[W - q:, :q], LR=P[W - q:, W - q:])
    out = {"peak": peak, "P2M": _ratio(peak, _nanmean(P[rest]))}
    for k in ("UL", "UR", "LL", "LR"):
        out["P2" + k] = _ratio(peak, _nanmean(corners[k]))
    ll = corners["LL"].ravel()
    ll = ll[~np.isnan(ll)]
    sd = float(ll.std(ddof=1)) if ll.size >= 2 else float("nan")
    out["ZscoreLL"] = _ratio(peak - _nanmean(ll), sd)
    return out


def shifted_controls(row, col, N, flank, n_shifts, seed=0):
    """``(row_c, col_c)``: for each feature ``n_shifts`` copies moved along the
    diagonal (the same offset on both ends: ``col - row`` is kept).  Offsets
    come from ``numpy.random.default_rng(seed)``, ``|offset|`` uniform in ``[W,
    100 W]`` with ``W = 2 * flank + 1`` and a random sign; a draw whose centre
    leaves [0, N) is redrawn at most 16 times and the copy is dropped if it is
    still outside.  ``pileup(features) / pileup(controls)`` is the
    normalisation when no expected is wanted."""
    row = np.repeat(np.asarray(row, dtype=np.int64), int(n_shifts))
    col = np.repeat(np.asarray(col, dtype=np.int64), int(n_shifts))
    W = 2 * int(flank) + 1
    rng = np.random.default_rng(seed)

    def draw(n):
        return rng.integers(W, 100 * W + 1, n) * (2 * rng.integers(0, 2, n) - 1)

    def outside(off):
        return (row + off < 0) | (col + off >= int(N))

    off = draw(row.size)
    for _ in range(16):
        out = outside(off)
        if not out.any():
            break
        off[out] = draw(int(out.sum()))
    keep = ~outside(off)
    return (row + off)[keep].astype(np.int32), (col + off)[keep].astype(np.int32)


def read_loop_file(fil):
    """{chrom: (pos1, pos2)} in bp from any of ``run_Loops``' three files: one
    header line, then ``chrom, pos1, pos2`` in the first three columns."""
    out = {}
    with open(fil) as f:
        next(f, None)
        for line in f:
            t = line.split()
            if t:
                out.setdefault(t[0], []).append((int(float(t[1])), int(float(t[2]))))
    return {k: (np.array([a for a, _ in v], np.int64), np.array([b for _, b in v], np.int64)) for k, v in out.items()}


def read_boundary_file(fil):
    """{chrom: (pos, pos)} from ``run_TADs``' ``_Filtered_Boundary_`` or
    ``_All_Boundary_`` file: ``chrom<TAB>value`` without a header, the value a
    position in bp (``tads.BoundaryCall`` stores bin * Res)."""
    out = {}
    with open(fil) as f:
        for line in f:
            t = line.split()
            if t:
                out.setdefault(t[0], []).append(int(float(t[1])))
    return {k: (np.array(v, np.int64), np.array(v, np.int64)) for k, v in out.items()}


def write_pileup(pileup_fil, count_fil, apa_fil, P, Cn, scores, n_features, control_scores=None):
    """The three text files of ``run_Pileup`` (tab-separated, floats as Python
    2 printed them, NaN as 'nan'): the W rows of the pileup, the W rows of Cn,
    and one ``name<TAB>value`` line per APA score plus ``n_features``; with
    controls the same scores of features-over-controls as ``<name>_over_controls``."""
    from .StructureFind import py2_float_str
    with open(pileup_fil, "w") as f:
        for r in np.asarray(P, dtype=np.float64):
            f.write("\t".join(py2_float_str(x) for x in r) + "\n")
    with open(count_fil, "w") as f:
        for r in np.asarray(Cn):
            f.write("\t".join(str(int(x)) for x in r) + "\n")
    with open(apa_fil, "w") as f:
        for k in APA_NAMES:
            f.write(f"{k}\t{py2_float_str(scores[k])}\n")
        f.write(f"n_features\t{int(n_features)}\n")
        if control_scores is not None:
            for k in APA_NAMES:
                f.write(f"{k}_over_controls\t{py2_float_str(control_scores[k])}\n")


class PileupCalling:
    """The pileup method of ``StructureFind``."""

    def run_Pileup(self, OutPath, features=None, loop_file=None, boundary_file=None, flank=100000, expected=True,
                   min_dist=None, ignore_diags=2, n_shifts=0, seed=0):
        """Pileup of the cooler around a list of features, per chromosome
        straight from the pixel table.  Exactly one source: ``features``
        ({chrom: (pos1, pos2)} in bp), ``loop_file`` (any of ``run_Loops``'
        files: a header line, then chrom, pos1, pos2 in bp) or
        ``boundary_file`` (``run_TADs``' ``_Filtered_Boundary_`` /
        ``_All_Boundary_`` file: ``chrom<TAB>position`` in bp -- the writer
        stores bin * Res -- for on-diagonal features).  Chromosome names are
        those of the files: haplotype chromosomes ('Maternal' / 'Paternal')
        are looked up without their M/P prefix.  Positions are floored to
        bins and swapped where pos1 > pos2.  ``flank`` and ``min_dist`` in bp
        (``min_dist`` defaults to ``ignore_diags`` bins; at most 63 bins of
        flank); ``expected=True`` divides by the chromosome's own cis
        expected (``ignore_diags`` diagonals left out); ``n_shifts > 0`` also
        piles up that many shifted controls per feature
        (``shifted_controls``, ``seed``).  Traditional data uses
        ``bins/weight``; haplotype data the raw counts, with the chromosome's
        gap list as invalid bins when a ``GapFile`` was given.  Writes
        ``<prefix>_Pileup_<res>.txt`` (the W rows of S / Cn),
        ``<prefix>_PileupCount_<res>.txt`` (Cn) and ``<prefix>_APA_<res>.txt``
        (name, value per score, ``n_features`` and, with controls, the scores
        of features-over-controls).  Returns (and keeps as ``Pileup_dict``)
        the arrays."""
        from .coolio import Cooler
        if sum(x is not None for x in (features, loop_file, boundary_file)) != 1:
            raise ValueError("run_Pileup: give exactly one of features=, loop_file=, boundary_file=")
        self._chroms()
        f = int(flank // self.Res)
        g = int(ignore_diags)
        dmin = g if min_dist is None else int(min_dist // self.Res)
        if not 0 <= f <= MAX_FLANK:
            raise ValueError(f"run_Pileup: flank must be 0..{MAX_FLANK} bins")
        if g < 0 or dmin < 0 or int(n_shifts) < 0:
            raise ValueError("run_Pileup: ignore_diags, min_dist and n_shifts must be >= 0")
        if loop_file is not None:
            features = read_loop_file(loop_file)
        elif boundary_file is not None:
            features = read_boundary_file(boundary_file)
        name = self._name
        stream = getattr(self, "stream", None)
        W = 2 * f + 1
        S, Cn = np.zeros((W, W)), np.zeros((W, W), np.int64)
        Sc, Cc = np.zeros((W, W)), np.zeros((W, W), np.int64)
        results, n_features, n_controls = {}, 0, 0
        with Cooler(self.cooler_fil) as c:
            walk = self._cooler_walk(c, "run_Pileup", lambda chro: name(chro) in features)
            missing = sorted(set(features) - {name(chro) for chro in self._chroms(c.chromnames)})
            if missing:
                raise ValueError(f"run_Pileup: features on chromosomes the cooler lacks: {missing}")
            for chro, lo, N, wt, bad, _ in walk:
                p1, p2 = (np.asarray(x, dtype=np.int64) // self.Res for x in features[name(chro)])
                if p1.shape != p2.shape or p1.ndim != 1:
                    raise ValueError(f"run_Pileup: the features of {name(chro)} must be two 1-D arrays of one length")
                row, col = np.minimum(p1, p2).astype(np.int32), np.maximum(p1, p2).astype(np.int32)
                if row.size and (row.min() < 0 or col.max() >= N):
                    raise ValueError(f"run_Pileup: a feature of {name(chro)} lies outside the chromosome")
                b1, b2, cnt = c.pixel_rows(lo, lo + N)
                e = None
                if expected:
                    es, en = expected_pixels(b1, b2, cnt, wt, lo, N, g, N - 1, bad, stream)
                    e = expected_from_sums(es, en, g)
                s, n = pileup_pixels(b1, b2, cnt, wt, lo, N, row, col, f, e, dmin, bad, stream)
                S += s
                Cn += n
                n_features += int(row.size)
                r = dict(row=row, col=col, expected=e, S=s, Cn=n)
                if n_shifts:
                    rc, cc = shifted_controls(row, col, N, f, n_shifts, seed)
                    s2, n2 = pileup_pixels(b1, b2, cnt, wt, lo, N, rc, cc, f, e, dmin, bad, stream)
                    Sc += s2
                    Cc += n2
                    n_controls += int(rc.size)
                    r.update(row_c=rc, col_c=cc, S_c=s2, Cn_c=n2)
                results[chro] = r
        P = pileup_from_sums(S, Cn)
        out = dict(chroms=results, flank=f, S=S, Cn=Cn, pileup=P, apa=apa_scores(P), n_features=n_features)
        if n_shifts:
            Pc = pileup_from_sums(Sc, Cc)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(Pc > 0, P / Pc, np.nan)
            out.update(S_c=Sc, Cn_c=Cc, pileup_c=Pc, n_controls=n_controls, ratio=ratio, apa_ratio=apa_scores(ratio))
        write_pileup(self._out_path(OutPath, "Pileup"), self._out_path(OutPath, "PileupCount"),
                     self._out_path(OutPath, "APA"), P, Cn, out["apa"], n_features, out.get("apa_ratio"))
        self.Pileup_dict = out
        return out
