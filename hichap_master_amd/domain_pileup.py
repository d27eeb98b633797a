"""Domain pileups: the average domain, rescaled.

HiCHap has no pileup: the definition is this project's.  ``run_TADs`` writes a
list of domains of very different sizes; a domain pileup stretches every
domain (and a flank on each side, in units of the domain's own length) to the
same ``G x G`` grid and averages them.  The sums run on the GPU
(``hh_domain_pileup_pixels``, csrc/pileup.hip) straight from cooler's pixel
table of one chromosome, global bins [lo, lo + N), with ``pileup_pixels``'
conventions for the value of a cell, the validity of a bin, ``expected`` and
``min_dist``.  Neither the N x N matrix nor a stack of per-domain sub-matrices
exists.

Feature k is the half-open interval ``[start[k], end[k])`` of local bins, ``L
= end - start``.  ``body`` (R) output cells span the domain, ``pad`` (P) cells
of flank lie on each side, ``G = R + 2 P <= 127``; every output cell spans ``L
/ R`` bins.  A matrix cell feeds an output cell with the area of their
intersection as weight (exact integers in units of 1/R bin); ``S`` adds the
weighted values of the eligible stored cells over ``L^2`` and ``Wn`` the
weighted eligible area over ``L^2`` -- a domain has weight 1 in a cell it
covers with eligible bins only -- and the pileup is ``S / Wn``.

The rest is host code on G x G arrays: ``domain_pileup_from_sums``,
``domain_scores`` and ``write_domain_pileup``.  ``DomainPileupCalling`` is
mixed into ``StructureFind`` (``run_DomainPileup``) the way
``pileup.PileupCalling`` is.
"""
from __future__ import annotations

import numpy as np

from ._lib import call, ptr, require_gpu
from ._pixels import empty, host_or_dev, table
from .pileup import _nanmean, _ratio, shifted_controls
from .saddle import expected_from_sums, expected_pixels

MAX_GRID = 127
SCORE_NAMES = ("body", "cross", "strength")


def domain_pileup_pixels(bin1, bin2, count, weight, lo, N, start, end, body, pad, expected=None, min_dist=0,
                         bad=None, stream=None):
    """``(S, Wn)``, G x G float64, ``G = body + 2 * pad``: the rescaled pileup
    sums of one chromosome over the intervals ``[start[k], end[k])`` (local
    bins, ``0 <= start < end <= N``; any order, repeats and overlaps allowed;
    a flank may leave the chromosome).  ``expected``: float64[n], 1 <= n <= N,
    or None for an observed pileup; ``min_dist`` in bins.  Torch tensors on
    the GPU are used in place and the results stay on the device."""
    require_gpu()
    dev, b1, b2, c, wt, bad = table(bin1, bin2, count, weight, N, bad)
    s, t = host_or_dev(start, np.int32, dev), host_or_dev(end, np.int32, dev)
    if s.ndim != 1 or tuple(s.shape) != tuple(t.shape):
        raise ValueError("start and end must be 1-D of the same length")
    e = host_or_dev(expected, np.float64, dev)
    if e is not None and e.ndim != 1:
        raise ValueError("expected must be 1-D")
    R, P = int(body), int(pad)
    G = R + 2 * P if R >= 1 and P >= 0 and R + 2 * P <= MAX_GRID else 0
    S, Wn = empty((G, G), np.float64, dev), empty((G, G), np.float64, dev)
    call("hh_domain_pileup_pixels", ptr(b1), ptr(b2), ptr(c), int(b1.shape[0]), ptr(wt),
         0 if wt is None else int(wt.shape[0]), int(lo), int(N), ptr(bad), ptr(s), ptr(t), int(s.shape[0]), R, P,
         ptr(e), 0 if e is None else int(e.shape[0]), int(min_dist), ptr(S), ptr(Wn), 0 if dev is None else 1, stream)
    return S, Wn


def domain_pileup_from_sums(S, Wn):
    """``S / Wn``, NaN where ``Wn == 0``."""
    S = np.asarray(S, dtype=np.float64)
    Wn = np.asarray(Wn, dtype=np.float64)
    out = np.full(S.shape, np.nan)
    ok = Wn > 0
    out[ok] = S[ok] / Wn[ok]
    return out


def domain_scores(Pm, body, pad):
    """The scores of a G x G domain pileup (G = body + 2 pad), as a dict:
    ``body`` = the mean of the cells with both indices in the body ``[pad, pad
    + body)``; ``cross`` = the mean of the cells with exactly one index in the
    body (the domain against its flanks); ``strength = body / cross``.  Means
    skip NaN cells; a score is NaN where it has no cells or its denominator is
    0."""
    Pm = np.asarray(Pm, dtype=np.float64)
    R, P = int(body), int(pad)
    G = R + 2 * P
    if R < 1 or P < 0 or Pm.shape != (G, G):
        raise ValueError("the pileup must be G x G with G = body + 2 pad")
    inb = np.zeros(G, bool)
    inb[P:P + R] = True
    both = inb[:, None] & inb[None, :]
    one = inb[:, None] ^ inb[None, :]
    b, c = _nanmean(Pm[both]), _nanmean(Pm[one])
    return {"body": b, "cross": c, "strength": _ratio(b, c)}


def read_domain_file(fil):
    """{chrom: (start_bp, end_bp)} from ``run_TADs``' ``_Domain_`` file:
    ``chrom<TAB>start<TAB>end`` in bp without a header."""
    out = {}
    with open(fil) as f:
        for line in f:
            t = line.split()
            if t:
                out.setdefault(t[0], []).append((int(float(t[1])), int(float(t[2]))))
    return {k: (np.array([a for a, _ in v], np.int64), np.array([b for _, b in v], np.int64)) for k, v in out.items()}


def domain_bins(start_bp, end_bp, res, min_size=0, max_size=None):
    """``(start, end, n_dropped)``: the bin intervals ``[start_bp // res,
    ceil(end_bp / res))`` (int32) of the domains whose size ``end_bp -
    start_bp`` lies in ``[min_size, max_size]`` bp (``max_size=None``: no
    upper limit), in the order given, and the number left out."""
    s, e = np.asarray(start_bp, dtype=np.int64), np.asarray(end_bp, dtype=np.int64)
    if s.ndim != 1 or s.shape != e.shape:
        raise ValueError("the domains must be two 1-D arrays of one length")
    size = e - s
    keep = size >= int(min_size)
    if max_size is not None:
        keep &= size <= int(max_size)
    res = int(res)
    return (s[keep] // res).astype(np.int32), (-(-e[keep] // res)).astype(np.int32), int((~keep).sum())


def write_domain_pileup(pileup_fil, weight_fil, score_fil, Pm, Wn, scores, n_features, n_dropped,
                        control_scores=None):
    """The three text files of ``run_DomainPileup`` (tab-separated, floats as
    Python 2 printed them, NaN as 'nan'): the G rows of the pileup, the G rows
    of Wn, and one ``name<TAB>value`` line per score plus ``n_features`` and
    ``n_dropped``; with controls the same scores of features-over-controls as
    ``<name>_over_controls``."""
    from .StructureFind import py2_float_str
    for fil, arr in ((pileup_fil, Pm), (weight_fil, Wn)):
        with open(fil, "w") as f:
            for r in np.asarray(arr, dtype=np.float64):
                f.write("\t".join(py2_float_str(x) for x in r) + "\n")
    with open(score_fil, "w") as f:
        for k in SCORE_NAMES:
            f.write(f"{k}\t{py2_float_str(scores[k])}\n")
        f.write(f"n_features\t{int(n_features)}\n")
        f.write(f"n_dropped\t{int(n_dropped)}\n")
        if control_scores is not None:
            for k in SCORE_NAMES:
                f.write(f"{k}_over_controls\t{py2_float_str(control_scores[k])}\n")


class DomainPileupCalling:
    """The domain pileup method of ``StructureFind``."""

    def run_DomainPileup(self, OutPath, features=None, domain_file=None, body=40, pad=20, expected=True,
                         min_dist=None, ignore_diags=2, min_size=0, max_size=None, n_shifts=0, seed=0):
        """Rescaled pileup of the cooler over a list of domains, per
        chromosome straight from the pixel table.  Exactly one source:
        ``features`` ({chrom: (start_bp, end_bp)}) or ``domain_file``
        (``run_TADs``' ``_Domain_`` file: ``chrom<TAB>start<TAB>end`` in bp
        without a header).  Chromosome names are those of the files:
        haplotype chromosomes are looked up without their M/P prefix.  A
        domain is the bin interval ``[start_bp // Res, ceil(end_bp / Res))``;
        domains outside ``[min_size, max_size]`` bp are dropped and counted.
        ``body`` output cells span a domain and ``pad`` cells each flank
        (``body + 2 pad <= 127``); ``min_dist`` in bp (defaults to
        ``ignore_diags`` bins); ``expected=True`` divides by the chromosome's
        own cis expected (``ignore_diags`` diagonals left out); ``n_shifts >
        0`` also piles up that many copies of each domain moved along the
        diagonal (``pileup.shifted_controls`` with flank ``G // 2``,
        ``seed``).  Traditional data uses ``bins/weight``; haplotype data the
        raw counts, with the chromosome's gap list as invalid bins when a
        ``GapFile`` was given.  Writes ``<prefix>_DomainPileup_<res>.txt``
        (the G rows of S / Wn), ``<prefix>_DomainPileupWeight_<res>.txt`` (Wn)
        and ``<prefix>_DomainScore_<res>.txt`` (name, value per score,
        ``n_features``, ``n_dropped`` and, with controls, the scores of
        features-over-controls).  Returns (and keeps as ``DomainPileup_dict``)
        the arrays."""
        from .coolio import Cooler
        if (features is None) == (domain_file is None):
            raise ValueError("run_DomainPileup: give exactly one of features=, domain_file=")
        self._chroms()
        R, P = int(body), int(pad)
        G = R + 2 * P
        g = int(ignore_diags)
        dmin = g if min_dist is None else int(min_dist // self.Res)
        if R < 1 or P < 0 or G > MAX_GRID:
            raise ValueError(f"run_DomainPileup: body >= 1, pad >= 0 and body + 2 pad <= {MAX_GRID}")
        if g < 0 or dmin < 0 or int(n_shifts) < 0:
            raise ValueError("run_DomainPileup: ignore_diags, min_dist and n_shifts must be >= 0")
        if domain_file is not None:
            features = read_domain_file(domain_file)
        name = self._name
        stream = getattr(self, "stream", None)
        S, Wn = np.zeros((G, G)), np.zeros((G, G))
        Sc, Wc = np.zeros((G, G)), np.zeros((G, G))
        results, n_features, n_dropped, n_controls = {}, 0, 0, 0
        with Cooler(self.cooler_fil) as c:
            walk = self._cooler_walk(c, "run_DomainPileup", lambda chro: name(chro) in features)
            missing = sorted(set(features) - {name(chro) for chro in self._chroms(c.chromnames)})
            if missing:
                raise ValueError(f"run_DomainPileup: features on chromosomes the cooler lacks: {missing}")
            for chro, lo, N, wt, bad, _ in walk:
                start, end, dropped = domain_bins(*features[name(chro)], self.Res, min_size, max_size)
                if start.size and (start.min() < 0 or end.max() > N or (start >= end).any()):
                    raise ValueError(f"run_DomainPileup: a domain of {name(chro)} is empty or outside the chromosome")
                b1, b2, cnt = c.pixel_rows(lo, lo + N)
                e = None
                if expected:
                    es, en = expected_pixels(b1, b2, cnt, wt, lo, N, g, N - 1, bad, stream)
                    e = expected_from_sums(es, en, g)
                s, w = domain_pileup_pixels(b1, b2, cnt, wt, lo, N, start, end, R, P, e, dmin, bad, stream)
                S += s
                Wn += w
                n_features += int(start.size)
                n_dropped += dropped
                r = dict(start=start, end=end, expected=e, S=s, Wn=w, n_dropped=dropped)
                if n_shifts:
                    sc, lc = shifted_controls(start, end - 1, N, G // 2, n_shifts, seed)
                    ec = lc + 1
                    s2, w2 = domain_pileup_pixels(b1, b2, cnt, wt, lo, N, sc, ec, R, P, e, dmin, bad, stream)
                    Sc += s2
                    Wc += w2
                    n_controls += int(sc.size)
                    r.update(start_c=sc, end_c=ec, S_c=s2, Wn_c=w2)
                results[chro] = r
        Pm = domain_pileup_from_sums(S, Wn)
        out = dict(chroms=results, body=R, pad=P, S=S, Wn=Wn, pileup=Pm, scores=domain_scores(Pm, R, P),
                   n_features=n_features, n_dropped=n_dropped)
        if n_shifts:
            Pc = domain_pileup_from_sums(Sc, Wc)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(Pc > 0, Pm / Pc, np.nan)
            out.update(S_c=Sc, Wn_c=Wc, pileup_c=Pc, n_controls=n_controls, ratio=ratio,
                       scores_ratio=domain_scores(ratio, R, P))
        write_domain_pileup(self._out_path(OutPath, "DomainPileup"), self._out_path(OutPath, "DomainPileupWeight"),
                            self._out_path(OutPath, "DomainScore"), Pm, Wn, out["scores"], n_features, n_dropped,
                            out.get("scores_ratio"))
        self.DomainPileup_dict = out
        return out
