"""Reproducibility of two contact maps: the stratum-adjusted correlation
coefficient (SCC, HiCRep: Yang et al. 2017).

HiCHap has no reproducibility score: the definition is this project's.  Two
pixel tables A and B describe the same chromosome of N bins, at global bins
[lo_a, lo_a + N) and [lo_b, lo_b + N) of their files (the two differ for the
M and P copy inside one haplotype cooler).  The value of a cell is ``v(a, b) =
(count * weight[bin1]) * weight[bin2]`` (NaN -> 0; the raw count with
``weight=None``), a bin is valid where it is valid on both sides (weight
finite, ``bad`` not set), and ``x(a, b)`` / ``y(a, b)`` are the symmetric
values of A / B, 0 at an invalid bin or with ``|a - b| < ignore_diags``.
Both maps are smoothed by the mean over the valid cells of a (2h + 1)^2 box,
``X = SX / (nv(a) nv(b))``, and per stratum ``d`` the GPU
(``hh_scc_pixels``, csrc/scc.hip) returns the number of cells between valid
bins with ``SX`` or ``SY`` non-zero and the sums of X, Y, X^2, Y^2 and X Y
over them.  The tables are read straight from the pixel table: no N x N
matrix is made.

The rest is host code on (max_dist + 1)-vectors: ``scc_from_moments`` (the
per-stratum correlations and their variance-stabilising weights),
``default_h`` and ``write_scc`` (the two text files).
``ReproducibilityCalling`` is mixed into ``StructureFind``
(``run_Reproducibility``) the way ``saddle.SaddleCalling`` is.
"""
from __future__ import annotations

import copy

import numpy as np

from ._lib import call, ptr, require_gpu
from ._pixels import empty, table

MAX_H = 20  # HH_SCC_MAX_H
MOMENTS = ("Sx", "Sy", "Sxx", "Syy", "Sxy")  # the rows of S


def default_h(Res):
    """The smoothing half-width in bins: 200 kb, at most ``MAX_H`` bins."""
    return min(MAX_H, int(round(200000 / Res)))


def _side(t, N):
    """One side of ``scc_pixels``: ``(bin1, bin2, count, weight, lo[, bad])``."""
    b1, b2, c, w, lo = t[:5]
    bad = t[5] if len(t) > 5 else None
    dev, b1, b2, c, w, bad = table(b1, b2, c, w, N, bad)
    return dev, (ptr(b1), ptr(b2), ptr(c), int(b1.shape[0]), ptr(w), 0 if w is None else int(w.shape[0]), int(lo),
                 ptr(bad)), (b1, b2, c, w, bad)


def scc_pixels(tableA, tableB, N, h, ignore_diags=1, max_dist=None, stream=None):
    """``(n, S)`` of one chromosome from two pixel tables, each ``(bin1, bin2,
    count, weight, lo[, bad])`` as ``saddle.expected_pixels`` takes them:
    ``n[d]`` (int64) the kept cells of stratum d = 0 .. max_dist (default N -
    1) and ``S`` (float64, 5 x (max_dist + 1)) the rows Sx, Sy, Sxx, Syy, Sxy
    of the smoothed values over them; both 0 for ``d < ignore_diags``.  NumPy
    arrays, or torch tensors on the GPU on both sides: those are used in place
    and the results stay on the device."""
    require_gpu()
    dev_a, args_a, keep_a = _side(tableA, N)
    dev_b, args_b, keep_b = _side(tableB, N)
    if (dev_a is None) != (dev_b is None) or (dev_a is not None and dev_a != dev_b):
        raise ValueError("both tables must be NumPy arrays, or tensors on the same device")
    D = int(N) - 1 if max_dist is None else int(max_dist)
    n_out = max(D + 1, 0)
    n, S = empty((n_out,), np.int64, dev_a), empty((5, n_out), np.float64, dev_a)
    call("hh_scc_pixels", *args_a, *args_b, int(N), int(h), int(ignore_diags), D, ptr(n), ptr(S),
         0 if dev_a is None else 1, stream)
    del keep_a, keep_b
    return n, S


def scc_from_moments(n, S):
    """The correlations of the strata and their weighted mean.  With ``cov = n
    Sxy - Sx Sy``, ``vx = n Sxx - Sx^2``, ``vy = n Syy - Sy^2`` a stratum is
    usable when ``n >= 3``, ``vx > 0`` and ``vy > 0``; ``rho = cov / sqrt(vx
    vy)`` (NaN elsewhere), ``weight = (n + 1) / 12`` (0 elsewhere): HiCRep's
    ``n var(rank / n)`` of a tie-free stratum; ``scc = sum(weight rho) /
    sum(weight)``, NaN without a usable stratum.  The strata of several
    chromosomes concatenated give the genome's value."""
    n = np.asarray(n)
    S = np.asarray(S, dtype=np.float64).reshape(5, -1)
    nf = n.astype(np.float64)
    sx, sy, sxx, syy, sxy = S
    cov, vx, vy = nf * sxy - sx * sy, nf * sxx - sx * sx, nf * syy - sy * sy
    usable = (n >= 3) & (vx > 0) & (vy > 0)
    rho = np.full(nf.shape, np.nan)
    rho[usable] = cov[usable] / np.sqrt(vx[usable] * vy[usable])
    weight = np.where(usable, (nf + 1.0) / 12.0, 0.0)
    scc = float(np.sum(weight[usable] * rho[usable]) / np.sum(weight[usable])) if usable.any() else float("nan")
    return dict(rho=rho, weight=weight, usable=usable, scc=scc)


def pooled_scc(results):
    """``scc_from_moments`` of the strata of every chromosome of ``results``
    ({chrom: dict(n=, S=)}) together."""
    if not results:
        return scc_from_moments(np.zeros(0, np.int64), np.zeros((5, 0)))
    return scc_from_moments(np.concatenate([r["n"] for r in results.values()]),
                            np.concatenate([r["S"] for r in results.values()], axis=1))


def write_scc(scc_fil, strata_fil, results, Res, genome, name=lambda chro: chro):
    """The two text files of ``run_Reproducibility`` (tab-separated, floats as
    Python 2 printed them, NaN as 'nan').  ``results``: {chrom: dict(h=,
    max_dist=, n=, rho=, weight=, usable=, scc=)} in file order; ``genome``:
    the pooled ``scc_from_moments``."""
    from .StructureFind import py2_float_str
    with open(scc_fil, "w") as f:
        f.write("chrom\th\tmax_dist_bins\tn_usable\tscc\n")
        for chro, r in results.items():
            f.write("\t".join([name(chro), str(r["h"]), str(r["max_dist"]), str(int(r["usable"].sum())),
                               py2_float_str(r["scc"])]) + "\n")
        hs = sorted({r["h"] for r in results.values()})
        f.write("\t".join(["genome", ",".join(str(h) for h in hs),
                           str(max([r["max_dist"] for r in results.values()], default=0)),
                           str(int(genome["usable"].sum())), py2_float_str(genome["scc"])]) + "\n")
    with open(strata_fil, "w") as f:
        f.write("chrom\tdist_bins\tdist_bp\tn\trho\tweight\n")
        for chro, r in results.items():
            for d in range(len(r["n"])):
                f.write("\t".join([name(chro), str(d), str(d * Res), str(int(r["n"][d])), py2_float_str(r["rho"][d]),
                                   py2_float_str(r["weight"][d])]) + "\n")


def _same_bins(c, o, who="run_Reproducibility"):
    """``ValueError`` naming the first difference of two coolers' bin tables
    (``who``: the caller the message speaks for; ``coolio.merge_coolers`` shares it)."""
    if c.binsize != o.binsize:
        raise ValueError(f"{who}: bin sizes differ: {c.binsize} and {o.binsize}")
    for k, (x, y) in enumerate(zip(c.chromnames, o.chromnames)):
        if x != y:
            raise ValueError(f"{who}: chromosome {k} is {x} in one cooler and {y} in the other")
        if c.chromsizes[x] != o.chromsizes[y]:
            raise ValueError(f"{who}: {x} has {c.chromsizes[x]} bp in one cooler and "
                             f"{o.chromsizes[y]} in the other")
    if len(c.chromnames) != len(o.chromnames):
        raise ValueError(f"{who}: {len(c.chromnames)} chromosomes in one cooler and "
                         f"{len(o.chromnames)} in the other")


class ReproducibilityCalling:
    """The reproducibility method of ``StructureFind``."""

    def _scc_walk(self, c, balance):
        """``_cooler_walk``'s rows; traditional data with ``balance=False``:
        no weights, every bin valid."""
        if self.Allelic is False and not balance:
            return [(chro, *c.extent(chro), None, None) for chro in self._chroms(c.chromnames)]
        return [(chro, lo, lo + N, wt, bad) for chro, lo, N, wt, bad, _ in
                self._cooler_walk(c, "run_Reproducibility")]

    def run_Reproducibility(self, OutPath, other=None, h=None, max_dist=5000000, ignore_diags=1, balance=True):
        """Stratum-adjusted correlation (SCC) of two maps, per chromosome and
        for the genome, straight from the coolers' pixel tables.  Traditional
        data: this cooler against ``other`` (the URI or path of a second
        cooler at the same resolution, e.g. the other replicate) with
        ``bins/weight`` of either file, the raw counts with ``balance=False``.
        Haplotype data ('Maternal' / 'Paternal'): without ``other`` every
        chromosome of this haplotype against the other haplotype's copy in the
        same cooler (``M<c>`` against ``P<c>``), with ``other`` the same
        haplotype of the two files; raw counts, each side's gap list as its
        invalid bins when a ``GapFile`` was given.  ``h``: smoothing
        half-width in bins (default ``default_h(Res)``), ``max_dist`` in bp,
        ``ignore_diags`` in bins.  Writes ``<prefix>_SCC_<res>.txt`` (chrom, h,
        max_dist_bins, n_usable, scc; last row ``genome``) and
        ``<prefix>_SCCStrata_<res>.txt`` (chrom, dist_bins, dist_bp, n, rho,
        weight), haplotype chromosomes without their M/P prefix.  Returns (and
        keeps as ``Reproducibility_dict``) the arrays."""
        from .coolio import Cooler
        self._chroms()
        h = default_h(self.Res) if h is None else int(h)
        g = int(ignore_diags)
        if not 0 <= h <= MAX_H:
            raise ValueError(f"run_Reproducibility: h must be 0..{MAX_H} bins, got {h}")
        if g < 0 or max_dist < 0:
            raise ValueError("run_Reproducibility: ignore_diags and max_dist must be >= 0")
        if other is None and self.Allelic is False:
            raise ValueError("run_Reproducibility: traditional data needs other=, the cooler to compare with")
        stream = getattr(self, "stream", None)
        results = {}
        with Cooler(self.cooler_fil) as c:
            if other is not None:
                o = Cooler(other if "::" in str(other) else "{}::{}".format(other, self.Res))
                side_b = self
            else:
                o = c
                side_b = copy.copy(self)
                side_b.Allelic = "Paternal" if self.Allelic == "Maternal" else "Maternal"
            try:
                if o is not c:
                    _same_bins(c, o)
                rows_a = self._scc_walk(c, balance)
                rows_b = {self._name(r[0]): r for r in side_b._scc_walk(o, balance)}
                for chro, lo_a, hi_a, _, _ in rows_a:      # every pair is checked before the first is computed
                    if self._name(chro) not in rows_b:
                        raise ValueError(f"run_Reproducibility: {chro} has no copy of the other haplotype")
                    chro_b, lo_b, hi_b = rows_b[self._name(chro)][:3]
                    if hi_b - lo_b != hi_a - lo_a:
                        raise ValueError(f"run_Reproducibility: {chro} has {hi_a - lo_a} bins, {chro_b} "
                                         f"{hi_b - lo_b}")
                for chro, lo_a, hi_a, wt_a, bad_a in rows_a:
                    _, lo_b, hi_b, wt_b, bad_b = rows_b[self._name(chro)]
                    N = hi_a - lo_a
                    D = min(N - 1, int(max_dist / self.Res))
                    n, S = scc_pixels((*c.pixel_rows(lo_a, hi_a), wt_a, lo_a, bad_a),
                                      (*o.pixel_rows(lo_b, hi_b), wt_b, lo_b, bad_b), N, h, g, D, stream)
                    results[chro] = dict(h=h, max_dist=D, n=n, S=S, **scc_from_moments(n, S))
            finally:
                if o is not c:
                    o.close()
        genome = pooled_scc(results)
        write_scc(self._out_path(OutPath, "SCC"), self._out_path(OutPath, "SCCStrata"), results, self.Res, genome,
                  self._name)
        self.Reproducibility_dict = dict(chroms=results, h=h, ignore_diags=g, usable=genome["usable"],
                                         scc=genome["scc"])
        return self.Reproducibility_dict
