"""Trans expected, cis / trans totals and trans saddle.

HiCHap has none of these and cooltools is absent: the definitions are this
project's.  The genome is C chromosomes, chromosome q the global bins
``[chrom_offset[q], chrom_offset[q + 1])``; ``use`` (uint8[C] or None = all)
switches chromosomes off, as rows and as columns.  The value of a cell is
``v(a, b) = count * weight[bin1] * weight[bin2]`` (NaN -> 0; the raw count with
``weight=None``) and a bin is invalid where its chromosome is not used, its
weight is not finite or the GLOBAL ``bad`` (uint8[n_bins]) is set.  One GPU
call (``hh_trans_blocks`` / ``hh_trans_saddle``, csrc/trans.hip) takes the rows
of one chromosome p, the pixels with bin1 in p, from the whole table or from
``Cooler.pixel_rows``:

* blocks: ``sum[q]`` / ``npix[q]``, the fp64 sum and the number of the stored
  pixels between p and q with both bins valid (q = p: those with ``b - a >=
  ignore_diags``; q < p: 0);
* saddle: with a global class per bin (255 = left out) and row p of the trans
  expected, ``U[cls[a]][cls[b]]`` adds ``v(a, b) / expected[q]`` over the stored
  pixels of the usable blocks q > p (expected finite and > 0).

The rest is host arithmetic: ``valid_bins``, ``trans_expected_from_sums`` (sum
over the product of the two chromosomes' valid bins), ``cis_trans_totals``,
``trans_saddle_counts`` (the cells per class pair, which need no pixel) and
``write_trans`` (the four text files).  ``TransCalling`` is mixed into
``StructureFind`` (``run_Trans``) the way ``saddle.SaddleCalling`` is.
"""
from __future__ import annotations

import numpy as np

from ._lib import call, ptr, require_gpu
from ._pixels import empty, host_or_dev, is_dev
from .saddle import LEFT_OUT, digitize_track, saddle_strength

MAX_CHROMS = 512


def _genome_table(bin1, bin2, count, weight, chrom_offset, use, bad):
    """The call's side (None = host, or the torch device of ``bin1``), the
    table, the global weights and ``bad`` as contiguous arrays on that side,
    and the offsets and ``use`` as host arrays (they are arguments of the
    call, not data)."""
    dev = bin1.device if is_dev(bin1) else None
    b1, b2 = host_or_dev(bin1, np.int64, dev), host_or_dev(bin2, np.int64, dev)
    c = host_or_dev(count, np.float64, dev)
    if not (tuple(b1.shape) == tuple(b2.shape) == tuple(c.shape)) or b1.ndim != 1:
        raise ValueError("bin1, bin2 and count must be 1-D of the same length")
    off = np.ascontiguousarray(chrom_offset, dtype=np.int64)
    if off.ndim != 1 or off.size < 1:
        raise ValueError("chrom_offset must be 1-D with C + 1 entries")
    C = off.size - 1
    if use is not None:
        use = np.ascontiguousarray(np.asarray(use) != 0, dtype=np.uint8)
        if use.shape != (C,):
            raise ValueError("use must have one entry per chromosome")
    wt = host_or_dev(weight, np.float64, dev)
    bad = host_or_dev(bad, np.uint8, dev)
    if bad is not None and tuple(bad.shape) != (int(off[-1]),):
        raise ValueError("bad must have one entry per bin of the genome")
    return dev, b1, b2, c, wt, off, C, use, bad


def trans_blocks_pixels(bin1, bin2, count, weight, chrom_offset, p, ignore_diags=2, use=None, bad=None, stream=None):
    """``(sum, npix)`` (float64[C], int64[C]) of the rows of chromosome p:
    per partner chromosome q >= p the sum of the balanced stored pixels with
    both bins valid and their number; the cis cell q = p takes the pixels with
    ``b - a >= ignore_diags``.  Torch tensors on the GPU are used in place and
    the results stay on the device."""
    require_gpu()
    dev, b1, b2, c, wt, off, C, use, bad = _genome_table(bin1, bin2, count, weight, chrom_offset, use, bad)
    s, n = empty((C,), np.float64, dev), empty((C,), np.int64, dev)
    call("hh_trans_blocks", ptr(b1), ptr(b2), ptr(c), int(b1.shape[0]), ptr(wt),
         0 if wt is None else int(wt.shape[0]), ptr(off), C, ptr(use), ptr(bad), int(p), int(ignore_diags),
         ptr(s), ptr(n), 0 if dev is None else 1, stream)
    return s, n


def trans_saddle_pixels(bin1, bin2, count, weight, chrom_offset, p, expected, cls, K, use=None, bad=None,
                        stream=None):
    """``U`` (K x K float64): the trans saddle sums of the rows of chromosome
    p.  ``expected``: float64[C], row p of the trans expected; ``cls``:
    uint8[n_bins], global, class ids 0..K-1 or 255 for a bin left out.  Torch
    tensors on the GPU are used in place and the result stays on the device."""
    require_gpu()
    dev, b1, b2, c, wt, off, C, use, bad = _genome_table(bin1, bin2, count, weight, chrom_offset, use, bad)
    e = host_or_dev(expected, np.float64, dev)
    k = host_or_dev(cls, np.uint8, dev)
    if tuple(e.shape) != (C,):
        raise ValueError("expected must have one entry per chromosome")
    if tuple(k.shape) != (int(off[-1]),):
        raise ValueError("cls must have one entry per bin of the genome")
    K = int(K)
    U = empty((max(K, 0), max(K, 0)), np.float64, dev)
    call("hh_trans_saddle", ptr(b1), ptr(b2), ptr(c), int(b1.shape[0]), ptr(wt),
         0 if wt is None else int(wt.shape[0]), ptr(off), C, ptr(use), ptr(bad), int(p), ptr(e), ptr(k), K,
         ptr(U), 0 if dev is None else 1, stream)
    return U


def valid_bins(chrom_offset, weight=None, use=None, bad=None):
    """``(valid, nvb)``: uint8[n_bins] and the valid bins per chromosome
    (int64[C])."""
    off = np.asarray(chrom_offset, dtype=np.int64)
    n = int(off[-1])
    valid = np.ones(n, bool)
    if use is not None:
        valid &= np.repeat(np.asarray(use) != 0, np.diff(off))
    if weight is not None:
        valid &= np.isfinite(np.asarray(weight, dtype=np.float64)[:n])
    if bad is not None:
        valid &= np.asarray(bad) == 0
    csum = np.concatenate([[0], np.cumsum(valid, dtype=np.int64)])
    return valid.astype(np.uint8), csum[off[1:]] - csum[off[:-1]]


def trans_expected_from_sums(sums, nvb):
    """C x C: ``sums[p][q] / (nvb[p] * nvb[q])`` for p < q (an exact integer
    product, one IEEE division), NaN where the product is 0 and for p >= q."""
    s = np.asarray(sums, dtype=np.float64)
    n = np.asarray(nvb, dtype=np.int64)
    cells = np.multiply.outer(n, n)
    ok = np.triu(np.ones(s.shape, bool), 1) & (cells > 0)
    out = np.full(s.shape, np.nan)
    out[ok] = s[ok] / cells[ok].astype(np.float64)
    return out


def trans_usable(expected):
    """C x C bool: block (p, q) is usable when q > p and its expected is
    finite and > 0."""
    e = np.asarray(expected, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.triu(np.ones(e.shape, bool), 1) & np.isfinite(e) & (e > 0)


def cis_trans_totals(sums):
    """From the C x C block sums (upper triangle): ``cis[p] = sums[p][p]``,
    ``trans[p]`` the blocks (min(p, q), max(p, q)) of q != p added in ascending
    q, ``cis_fraction = cis / (cis + trans)`` (NaN for 0 / 0), and ``genome =
    (cis, trans, fraction)`` with cis the diagonal and trans the blocks p < q,
    both added in file order."""
    s = np.asarray(sums, dtype=np.float64)
    C = s.shape[0]
    cis, trans = np.zeros(C), np.zeros(C)
    g_cis = g_trans = np.float64(0.0)
    for p in range(C):
        cis[p] = s[p, p]
        g_cis = g_cis + s[p, p]
        t = np.float64(0.0)
        for q in range(C):
            if q != p:
                t = t + s[min(p, q), max(p, q)]
            if q > p:
                g_trans = g_trans + s[p, q]
        trans[p] = t
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = cis / (cis + trans)
        g_frac = g_cis / (g_cis + g_trans)
    return dict(cis=cis, trans=trans, cis_fraction=frac, genome=(float(g_cis), float(g_trans), float(g_frac)))


def trans_saddle_counts(chrom_offset, valid, cls, K, usable):
    """``Cu`` (int64[C, K, K]): ``Cu[p] = sum over the usable q > p of h_p (x)
    h_q``, ``h_q[i]`` the valid bins of q with class i: the cells behind
    ``U`` of ``trans_saddle_pixels``, stored or not."""
    off = np.asarray(chrom_offset, dtype=np.int64)
    C = off.size - 1
    ec = np.where(np.asarray(valid) != 0, np.asarray(cls), LEFT_OUT).astype(np.int64)
    if np.any((ec >= K) & (ec != LEFT_OUT)):
        raise ValueError("a cls entry is neither a class id below K nor 255")
    h = np.zeros((C, K), np.int64)
    for q in range(C):
        x = ec[off[q]:off[q + 1]]
        h[q] = np.bincount(x[x != LEFT_OUT], minlength=K)[:K]
    us = np.asarray(usable, bool)
    Cu = np.zeros((C, K, K), np.int64)
    for p in range(C):
        hq = h[[q for q in range(p + 1, C) if us[p, q]]].sum(axis=0) if us[p, p + 1:].any() else np.zeros(K, np.int64)
        Cu[p] = np.multiply.outer(h[p], hq)
    return Cu


def write_trans(expected_fil, cistrans_fil, names, sel, nvb, sums, npix, expected, totals, saddle_fil=None,
                strength_fil=None, edges=None, S=None, C=None):
    """The text files of ``run_Trans`` (tab-separated, floats as Python 2
    printed them, NaN as 'nan').  ``names``: the chromosomes' names as shown,
    ``sel`` the indices of the selected ones in file order; the saddle and its
    strength are written when ``saddle_fil`` is given (``edges`` the K - 1
    quantile edges, S and C the symmetric K x K sums and counts)."""
    from .StructureFind import py2_float_str
    with open(expected_fil, "w") as f:
        f.write("chrom1\tchrom2\tn_valid1\tn_valid2\tn_pixels\tbalanced_sum\tbalanced_avg\n")
        for i, p in enumerate(sel):
            for q in sel[i + 1:]:
                f.write("\t".join([names[p], names[q], str(int(nvb[p])), str(int(nvb[q])), str(int(npix[p][q])),
                                   py2_float_str(sums[p][q]), py2_float_str(expected[p][q])]) + "\n")
    with open(cistrans_fil, "w") as f:
        f.write("chrom\tcis_sum\ttrans_sum\tcis_fraction\n")
        for p in sel:
            f.write("\t".join([names[p], py2_float_str(totals["cis"][p]), py2_float_str(totals["trans"][p]),
                               py2_float_str(totals["cis_fraction"][p])]) + "\n")
        f.write("\t".join(["genome"] + [py2_float_str(x) for x in totals["genome"]]) + "\n")
    if saddle_fil is None:
        return
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


class TransCalling:
    """The trans methods of ``StructureFind``."""

    def run_Trans(self, OutPath, track=None, PC_file=None, n_bins=50, qrange=(0.025, 0.975), ignore_diags=2):
        """Trans expected, cis / trans ratio and, with a track, the trans
        saddle and its strength to text files, per chromosome straight from
        the cooler's pixel table (one ``pixel_rows`` read and one block call
        per chromosome; with a track a second read and one saddle call per
        chromosome once every block is known).  The track is ``track``
        ({chrom: array}), else ``Compartment_Dict`` of an earlier
        ``Compartment`` run, else ``PC_file``; without any of them only the
        first two files are written.  Traditional data uses ``bins/weight``;
        haplotype data ('Maternal' / 'Paternal') the chromosomes with that
        prefix and the raw counts, with the gap lists as invalid bins when a
        ``GapFile`` was given.  Writes ``<prefix>_TransExpected_<res>.txt``
        (chrom1, chrom2, n_valid1, n_valid2, n_pixels, balanced_sum,
        balanced_avg for the selected pairs p < q in file order),
        ``<prefix>_CisTrans_<res>.txt`` (chrom, cis_sum, trans_sum,
        cis_fraction and a last line 'genome'), ``<prefix>_TransSaddle_<res>.txt``
        and ``<prefix>_TransSaddleStrength_<res>.txt`` (``run_Saddle``'s
        layouts), haplotype chromosomes without their M/P prefix.  Returns
        (and keeps as ``Trans_dict``) the arrays."""
        from .coolio import Cooler
        self._chroms()
        g = int(ignore_diags)
        if g < 0:
            raise ValueError("run_Trans: ignore_diags must be >= 0")
        stream = getattr(self, "stream", None)
        with_track = track is not None or bool(getattr(self, "Compartment_Dict", None)) or PC_file is not None
        with Cooler(self.cooler_fil) as c:
            geom = list(self._cooler_walk(c, "run_Trans"))
            chroms = list(c.chromnames)
            off = c.chrom_offsets()
            C = len(chroms)
            if C > MAX_CHROMS:
                raise ValueError(f"run_Trans: {C} chromosomes, at most {MAX_CHROMS}")
            sel = [chroms.index(row[0]) for row in geom]
            use = None
            if len(sel) < C:
                use = np.zeros(C, np.uint8)
                use[sel] = 1
            wt = geom[0][3] if geom else None
            bad = None
            if any(row[4] is not None for row in geom):
                bad = np.zeros(int(off[-1]), np.uint8)
                for _, lo, N, _, b, _ in geom:
                    if b is not None:
                        bad[lo:lo + N] = b
            valid, nvb = valid_bins(off, wt, use, bad)
            sums, npix = np.zeros((C, C)), np.zeros((C, C), np.int64)
            for (_, lo, N, *_), p in zip(geom, sel):
                b1, b2, cnt = c.pixel_rows(lo, lo + N)
                sums[p], npix[p] = trans_blocks_pixels(b1, b2, cnt, wt, off, p, g, use, bad, stream)
            expected = trans_expected_from_sums(sums, nvb)
            totals = cis_trans_totals(sums)
            names = [self._name(x) if k in sel else x for k, x in enumerate(chroms)]
            r = dict(chroms=chroms, selected=sel, chrom_offset=off, valid=valid, n_valid=nvb, sum=sums, npix=npix,
                     expected=expected, **totals)
            files = {}
            if with_track:
                tracks = self._saddle_track(track, PC_file, [row[0] for row in geom], self._name)
                for chro, _, N, *_ in geom:
                    if tracks[chro].shape != (N,):
                        raise ValueError(f"run_Trans: the track of {chro} has {tracks[chro].size} values, "
                                         f"the chromosome {N} bins")
                cls_by, edges = digitize_track(tracks, {row[0]: row[5] for row in geom}, n_bins, qrange)
                K = int(n_bins) + 2
                cls = np.full(int(off[-1]), LEFT_OUT, np.uint8)
                for chro, lo, N, *_ in geom:
                    cls[lo:lo + N] = cls_by[chro]
                usable = trans_usable(expected)
                Cu = trans_saddle_counts(off, valid, cls, K, usable)
                U = np.zeros((C, K, K))
                S, Cn = np.zeros((K, K)), np.zeros((K, K), np.int64)
                for (_, lo, N, *_), p in zip(geom, sel):
                    if usable[p].any():                     # (the last chromosome has no block q > p)
                        b1, b2, cnt = c.pixel_rows(lo, lo + N)
                        U[p] = trans_saddle_pixels(b1, b2, cnt, wt, off, p, expected[p], cls, K, use, bad, stream)
                    S += U[p] + U[p].T
                    Cn += Cu[p] + Cu[p].T
                with np.errstate(divide="ignore", invalid="ignore"):
                    saddle = np.where(Cn > 0, S / Cn, np.nan)
                r.update(cls=cls, edges=edges, usable=usable, U=U, Cu=Cu, S=S, C=Cn, saddle=saddle,
                         strength=saddle_strength(S, Cn))
                files = dict(saddle_fil=self._out_path(OutPath, "TransSaddle"),
                             strength_fil=self._out_path(OutPath, "TransSaddleStrength"), edges=edges, S=S, C=Cn)
        write_trans(self._out_path(OutPath, "TransExpected"), self._out_path(OutPath, "CisTrans"), names, sel, nvb,
                    sums, npix, expected, totals, **files)
        self.Trans_dict = r
        return r
