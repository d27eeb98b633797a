"""Per-bin coverage tracks and virtual 4C.

HiCHap has neither and cooltools is absent: the definitions are this
project's.  The genome, the pixels, ``v(a, b) = count * weight[a] * weight[b]``
(NaN -> 0; the raw count with ``weight=None``), ``use``, ``bad`` and ``valid``
are ``trans.py``'s.  ``A[i][j] = v(min, max)`` for valid i, j with a stored
pixel, 0 elsewhere; a diagonal pixel enters its row ONCE (cooltools adds it
twice).  With ``d = |i - j|`` a cell is *trans* (different chromosomes),
dropped (cis, ``d < ignore_diags``), *near* (cis, ``ignore_diags <= d <
near_bins``) or *far* (cis, ``d >= max(near_bins, ignore_diags)``).

``SymTable`` owns the handle of the symmetric pixel table on the GPU
(``hh_symtab_*``, csrc/symtab.hip: the whole upper table and its transpose,
raw counts, nothing baked in) and has the two hot paths (csrc/coverage.hip):

* ``coverage``: ``S[x][k]`` / ``n[x][k]``, the fp64 sum and the number of the
  stored pixels of row x per class k = near, far, trans;
* ``viewpoints``: ``P[c][y]``, the sum of the rows ``[lo_c, hi_c)`` of A
  without the dropped cells, the contact profile of a viewpoint against the
  whole genome.

The rest is host arithmetic: ``coverage_tracks`` (cis and total coverage, the
inter-chromosomal fraction ICF and the distal-to-local ratio DLR),
``viewpoint_bins``, the writers and readers of the two text files, and
``CoverageCalling`` (``run_Coverage``, ``run_Virtual4C``), mixed into
``StructureFind`` the way ``transeig.TransEigCalling`` is.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import call, ptr, require_gpu
from ._pixels import empty, host_or_dev
from .trans import MAX_CHROMS, _genome_table

MAX_VIEWS = 64          # HH_SYMTAB_MAX_VIEWS
NEAR_BP = 3_000_000     # HOMER's boundary between local and distal contacts (DLR)
CLASSES = ("near", "far", "trans")
COVERAGE_COLUMNS = ("chrom", "start", "end", "valid", "n_cis", "n_trans", "cov_cis_raw", "cov_tot_raw", "cov_cis",
                    "cov_tot", "ICF", "DLR")


class SymTable:
    """The symmetric pixel table of one cooler on the GPU (a context manager
    over an ``hh_symtab`` handle).  The pixel arrays are host arrays or torch
    tensors on the GPU; they may be freed once the table exists.  Nothing
    depends on weights or validity: one table serves raw and balanced calls
    and any ``use`` / ``bad``."""

    def __init__(self, bin1, bin2, count, chrom_offset, stream=None):
        require_gpu()
        dev, b1, b2, c, _, off, C, _, _ = _genome_table(bin1, bin2, count, None, chrom_offset, None, None)
        self.stream, self.dev = stream, dev
        self._h = None
        self.chrom_offset, self.C, self.n = off, C, int(off[-1])
        h = ctypes.c_void_p()
        call("hh_symtab_create", ptr(b1), ptr(b2), ptr(c), int(b1.shape[0]), ptr(off), C, 0 if dev is None else 1,
             stream, ctypes.byref(h))
        self._h = h
        u, lo = ctypes.c_int64(), ctypes.c_int64()
        call("hh_symtab_nnz", self._h, ctypes.byref(u), ctypes.byref(lo))
        self.nnz, self.n_lower = int(u.value), int(lo.value)

    def close(self):
        if self._h is not None:
            call("hh_symtab_free", self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h is None:
            raise ValueError("the SymTable is closed")
        return self._h

    def tables(self):
        """``dict(rowptr_u, rowptr_l, partner_l, src_l)`` as host arrays
        (int64[n + 1] twice, int32[n_lower], uint32[n_lower])."""
        rpu, rpl = np.zeros(self.n + 1, np.int64), np.zeros(self.n + 1, np.int64)
        p, src = np.zeros(self.n_lower, np.int32), np.zeros(self.n_lower, np.uint32)
        call("hh_symtab_export", self._handle(), ptr(rpu), ptr(rpl), ptr(p) if self.n_lower else None,
             ptr(src) if self.n_lower else None)
        return dict(rowptr_u=rpu, rowptr_l=rpl, partner_l=p, src_l=src)

    def _genome_args(self, weight, use, bad):
        wt = host_or_dev(weight, np.float64, self.dev)
        bad = host_or_dev(bad, np.uint8, self.dev)
        if bad is not None and tuple(bad.shape) != (self.n,):
            raise ValueError("bad must have one entry per bin of the genome")
        if use is not None:
            use = np.ascontiguousarray(np.asarray(use) != 0, dtype=np.uint8)
            if use.shape != (self.C,):
                raise ValueError("use must have one entry per chromosome")
        return wt, 0 if wt is None else int(wt.shape[0]), use, bad

    def coverage(self, weight=None, use=None, bad=None, ignore_diags=2, near_bins=0):
        """``(S, n)``: float64[n_bins, 3] and int64[n_bins, 3], the columns
        near, far, trans.  A table made from torch tensors on the GPU takes
        ``weight`` / ``bad`` there and leaves the results on the device."""
        wt, nw, use, bad = self._genome_args(weight, use, bad)
        S, n = empty((self.n, 3), np.float64, self.dev), empty((self.n, 3), np.int64, self.dev)
        call("hh_symtab_coverage", self._handle(), ptr(wt), nw, ptr(use), ptr(bad), int(ignore_diags),
             int(near_bins), ptr(S), ptr(n), 0 if self.dev is None else 1, self.stream)
        return S, n

    def viewpoints(self, intervals, weight=None, use=None, bad=None, ignore_diags=2):
        """``P`` (float64[len(intervals), n_bins]): row c the contact profile
        of the half-open interval of global bins ``intervals[c] = (lo, hi)``.
        Any number of intervals: they go to the GPU in groups of 64, and a
        column has the same bits whatever shares its call."""
        iv = np.asarray(intervals, dtype=np.int64).reshape(-1, 2)
        wt, nw, use, bad = self._genome_args(weight, use, bad)
        parts = []
        for c0 in range(0, iv.shape[0], MAX_VIEWS):
            lo = np.ascontiguousarray(iv[c0:c0 + MAX_VIEWS, 0])
            hi = np.ascontiguousarray(iv[c0:c0 + MAX_VIEWS, 1])
            P = empty((lo.size, self.n), np.float64, self.dev)
            call("hh_symtab_viewpoints", self._handle(), ptr(wt), nw, ptr(use), ptr(bad), int(ignore_diags), ptr(lo),
                 ptr(hi), int(lo.size), ptr(P), 0 if self.dev is None else 1, self.stream)
            parts.append(P)
        if not parts:
            return empty((0, self.n), np.float64, self.dev)
        if len(parts) == 1:
            return parts[0]
        if self.dev is None:
            return np.concatenate(parts, axis=0)
        import torch
        return torch.cat(parts, dim=0)


def default_near_bins(res, near_bp=NEAR_BP):
    """``ceil(near_bp / res)``."""
    return -(-int(near_bp) // int(res))


def coverage_tracks(S, valid):
    """From ``S`` (float64[n_bins, 3]: near, far, trans) and ``valid``:
    ``cov_cis = near + far``, ``cov_tot = cov_cis + trans``, ``ICF = trans /
    cov_tot`` and ``DLR = log2(far / near)``, single IEEE operations; ICF and
    DLR are NaN where the denominator is 0 or the bin is invalid (a bin with
    near > 0 and far = 0 has DLR = -inf)."""
    S = np.asarray(S, dtype=np.float64)
    ok = np.asarray(valid) != 0
    near, far, trans = S[:, 0], S[:, 1], S[:, 2]
    cis = near + far
    tot = cis + trans
    icf, dlr = np.full(S.shape[0], np.nan), np.full(S.shape[0], np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = ok & (tot != 0)
        icf[a] = trans[a] / tot[a]
        b = ok & (near != 0)
        dlr[b] = np.log2(far[b] / near[b])
    return dict(cov_cis=cis, cov_tot=tot, ICF=icf, DLR=dlr)


def viewpoint_bins(viewpoints, chromnames, chrom_offset, res, allelic=False):
    """``[(name, chrom, lo, hi, start_bp, end_bp)]``: the global bins ``[lo,
    hi)`` that overlap ``[start_bp, end_bp)``.  ``viewpoints``: ``{name:
    (chrom, start_bp, end_bp)}`` or the path of a tab-separated file with the
    lines ``chrom start end [name]`` ('#' lines skipped; without a name column
    the name is ``chrom:start-end``).  With ``allelic`` 'Maternal' /
    'Paternal' a chromosome given by its bare name is taken on that parent's
    copy.  ``ValueError`` for an unknown chromosome, ``end <= start``, a
    negative start and a viewpoint that crosses the end of its chromosome."""
    if isinstance(viewpoints, (str, bytes)):
        items = []
        with open(viewpoints) as f:
            for ln in f:
                t = ln.split()
                if not t or t[0].startswith("#"):
                    continue
                if len(t) < 3:
                    raise ValueError(f"viewpoint file: expected 'chrom start end [name]', got {ln.strip()!r}")
                items.append((t[3] if len(t) > 3 else f"{t[0]}:{t[1]}-{t[2]}", (t[0], int(t[1]), int(t[2]))))
    else:
        items = list(dict(viewpoints).items())
    off = np.asarray(chrom_offset, dtype=np.int64)
    names = list(chromnames)
    res = int(res)
    out = []
    for name, (chrom, start, end) in items:
        start, end = int(start), int(end)
        full = chrom
        if allelic in ("Maternal", "Paternal") and allelic[0] + str(chrom) in names:
            full = allelic[0] + str(chrom)
        if full not in names:
            raise ValueError(f"viewpoint {name}: unknown chromosome {chrom}")
        if start < 0 or end <= start:
            raise ValueError(f"viewpoint {name}: needs 0 <= start < end, got {start}, {end}")
        q = names.index(full)
        N = int(off[q + 1] - off[q])
        lo, hi = start // res, -(-end // res)
        if hi > N:
            raise ValueError(f"viewpoint {name}: {chrom}:{start}-{end} crosses the end of the chromosome "
                             f"({N} bins of {res} bp)")
        out.append((str(name), full, int(off[q]) + lo, int(off[q]) + hi, start, end))
    return out


def _fmt(v):
    from .StructureFind import py2_float_str
    return py2_float_str(v)


def _bin_rows(names, chrom_offset, sel, res):
    off = np.asarray(chrom_offset, dtype=np.int64)
    for p in sel:
        for x in range(int(off[p]), int(off[p + 1])):
            r = x - int(off[p])
            yield x, [names[p], str(r * res), str((r + 1) * res)]


def write_coverage(fil, names, chrom_offset, sel, res, valid, n, S_raw, S):
    """``<prefix>_Coverage_<res>.txt``: one tab-separated line per bin of the
    selected chromosomes with ``COVERAGE_COLUMNS`` (floats as Python 2 printed
    them, NaN as 'nan').  ``n`` / ``S_raw``: the counts and sums of the raw
    call, ``S`` those of the balanced one (the same array for haplotype data);
    ICF and DLR come from ``S``.  For traditional data the raw call masks no
    bin, so ``n_cis``, ``n_trans`` and the ``*_raw`` columns count every stored
    pixel, while ``valid``, ``cov_cis``, ``cov_tot``, ICF and DLR are the
    balanced call's: a line with ``valid = 0`` may show pixels next to a
    balanced coverage of 0."""
    raw, bal = coverage_tracks(S_raw, valid), coverage_tracks(S, valid)
    n = np.asarray(n)
    with open(fil, "w") as f:
        f.write("\t".join(COVERAGE_COLUMNS) + "\n")
        for x, head in _bin_rows(names, chrom_offset, sel, res):
            f.write("\t".join(head + [str(int(valid[x])), str(int(n[x, 0] + n[x, 1])), str(int(n[x, 2])),
                                      _fmt(raw["cov_cis"][x]), _fmt(raw["cov_tot"][x]), _fmt(bal["cov_cis"][x]),
                                      _fmt(bal["cov_tot"][x]), _fmt(bal["ICF"][x]), _fmt(bal["DLR"][x])]) + "\n")


def read_coverage(fil):
    """The file of ``write_coverage`` as ``{column: array}`` (chrom: str,
    start / end / valid / n_cis / n_trans: int64, the rest float64)."""
    with open(fil) as f:
        head = f.readline().rstrip("\n").split("\t")
        rows = [ln.rstrip("\n").split("\t") for ln in f]
    if tuple(head) != COVERAGE_COLUMNS:
        raise ValueError(f"{fil}: not a coverage file")
    out = {}
    for k, name in enumerate(head):
        col = [r[k] for r in rows]
        out[name] = (np.array(col, dtype=str) if k == 0 else np.array(col, dtype=np.int64) if k < 6
                     else np.array([float(v) for v in col], dtype=np.float64))
    return out


def write_virtual4c(fil, names, chrom_offset, sel, res, views, P):
    """``<prefix>_Virtual4C_<res>.txt``: ``chrom start end`` and one column
    per viewpoint, headed ``name|chrom:start-end``; one line per bin of the
    selected chromosomes.  ``views``: ``[(name, chrom as shown, start_bp,
    end_bp)]``; ``P`` float64[len(views), n_bins]."""
    P = np.asarray(P, dtype=np.float64)
    with open(fil, "w") as f:
        f.write("\t".join(["chrom", "start", "end"] + [f"{nm}|{ch}:{s}-{e}" for nm, ch, s, e in views]) + "\n")
        for x, head in _bin_rows(names, chrom_offset, sel, res):
            f.write("\t".join(head + [_fmt(P[c, x]) for c in range(P.shape[0])]) + "\n")


def read_virtual4c(fil):
    """``(chrom, start, end, views, P)`` of a file of ``write_virtual4c``:
    ``views`` the column heads, ``P`` float64[len(views), rows]."""
    with open(fil) as f:
        head = f.readline().rstrip("\n").split("\t")
        rows = [ln.rstrip("\n").split("\t") for ln in f]
    if head[:3] != ["chrom", "start", "end"]:
        raise ValueError(f"{fil}: not a virtual 4C file")
    P = np.array([[float(v) for v in r[3:]] for r in rows], dtype=np.float64).reshape(len(rows), len(head) - 3).T
    return (np.array([r[0] for r in rows], dtype=str), np.array([r[1] for r in rows], dtype=np.int64),
            np.array([r[2] for r in rows], dtype=np.int64), head[3:], P)


class CoverageCalling:
    """The per-bin methods of ``StructureFind``."""

    def _coverage_genome(self, c, caller):
        """The geometry ``run_TransEig`` assembles: ``(geom, chroms, off, sel,
        use, weight, bad, valid, names)``."""
        geom = list(self._cooler_walk(c, caller))
        chroms = list(c.chromnames)
        off = c.chrom_offsets()
        C = len(chroms)
        if C > MAX_CHROMS:
            raise ValueError(f"{caller}: {C} chromosomes, at most {MAX_CHROMS}")
        sel = [chroms.index(row[0]) for row in geom]
        use = None
        if len(sel) < C:
            use = np.zeros(C, np.uint8)
            use[sel] = 1
        wt = geom[0][3] if geom else None
        n = int(off[-1])
        bad = None
        if any(row[4] is not None for row in geom):
            bad = np.zeros(n, np.uint8)
            for _, lo, N, _, b, _ in geom:
                if b is not None:
                    bad[lo:lo + N] = b
        valid = np.zeros(n, np.uint8)
        for _, lo, N, _, _, v in geom:
            valid[lo:lo + N] = v
        names = [self._name(x) if k in sel else x for k, x in enumerate(chroms)]
        return geom, chroms, off, sel, use, wt, bad, valid, names

    def run_Coverage(self, OutPath, ignore_diags=2, near_bp=NEAR_BP, store=False):
        """Per-bin coverage of the symmetric map: the whole
        pixel table read once, one ``SymTable``; traditional data takes two
        coverage calls, the raw counts (no bin masked) and the balanced values
        (``bins/weight``; a bin without a finite weight is invalid), haplotype
        data ('Maternal' / 'Paternal') one call on the raw counts of the
        chromosomes with that prefix, the gap lists as invalid bins when a
        ``GapFile`` was given.  ``near_bins = ceil(near_bp / Res)`` splits cis
        into near and far.  Writes ``<prefix>_Coverage_<res>.txt`` (chrom,
        start, end, valid, n_cis, n_trans: the stored pixels behind the raw
        columns; cov_cis_raw, cov_tot_raw; cov_cis, cov_tot, ICF, DLR from the
        balanced call, for haplotype data from the one call).  ``store`` (for
        traditional data with integer counts) appends ``bins/cov_cis_raw`` and
        ``bins/cov_tot_raw`` (int64) to the cooler, replacing columns of those
        names.  Returns (and keeps as ``Coverage_dict``) the arrays."""
        from . import h5
        from .coolio import Cooler, parse_uri
        self._chroms()
        stream = getattr(self, "stream", None)
        near_bins = default_near_bins(self.Res, near_bp)
        with Cooler(self.cooler_fil) as c:
            geom, chroms, off, sel, use, wt, bad, valid, names = self._coverage_genome(c, "run_Coverage")
            b1, b2, cnt = c.pixels_table()
        if store:
            if self.Allelic is not False:
                raise ValueError("run_Coverage: store=True is for traditional data")
            if np.asarray(cnt).dtype.kind == "f" and np.any(cnt != np.floor(cnt)):
                raise ValueError("run_Coverage: store=True needs integer counts")
        with SymTable(b1, b2, cnt, off, stream) as tab:
            S_raw, n = tab.coverage(None, use, bad, ignore_diags, near_bins)
            S = tab.coverage(wt, use, bad, ignore_diags, near_bins)[0] if wt is not None else S_raw
            nnz, n_lower = tab.nnz, tab.n_lower
        raw, bal = coverage_tracks(S_raw, valid if wt is None else np.ones_like(valid)), coverage_tracks(S, valid)
        r = dict(chroms=chroms, selected=sel, chrom_offset=off, valid=valid, n=n, S_raw=S_raw, S=S,
                 ignore_diags=int(ignore_diags), near_bins=near_bins, nnz=nnz, n_lower=n_lower,
                 n_cis=n[:, 0] + n[:, 1], n_trans=n[:, 2], cov_cis_raw=raw["cov_cis"], cov_tot_raw=raw["cov_tot"],
                 cov_cis=bal["cov_cis"], cov_tot=bal["cov_tot"], ICF=bal["ICF"], DLR=bal["DLR"])
        r["file"] = self._out_path(OutPath, "Coverage")
        write_coverage(r["file"], names, off, sel, int(self.Res), valid, n, S_raw, S)
        if store:
            path, group = parse_uri(self.cooler_fil)
            for key in ("cov_cis_raw", "cov_tot_raw"):
                h5.append_dataset(path, (group + "/bins") if group else "bins", key, np.rint(r[key]).astype(np.int64),
                                  {"ignore_diags": int(ignore_diags)})
        self.Coverage_dict = r
        return r

    def run_Virtual4C(self, OutPath, viewpoints, ignore_diags=2):
        """Virtual 4C: the contact profile of every viewpoint
        against the whole genome.  ``viewpoints``: ``{name: (chrom, start_bp,
        end_bp)}`` or a file of ``chrom start end [name]`` lines; a viewpoint
        lies in one chromosome and covers the bins that overlap its interval.
        Geometry, weights and invalid bins are ``run_Coverage``'s (balanced
        values for traditional data, raw counts for haplotype data, where a
        bare chromosome name means the selected parent's copy).  Writes
        ``<prefix>_Virtual4C_<res>.txt`` (chrom, start, end and one column per
        viewpoint, headed ``name|chrom:start-end``).  Returns (and keeps as
        ``Virtual4C_dict``) the arrays."""
        from .coolio import Cooler
        self._chroms()
        stream = getattr(self, "stream", None)
        with Cooler(self.cooler_fil) as c:
            geom, chroms, off, sel, use, wt, bad, valid, names = self._coverage_genome(c, "run_Virtual4C")
            views = viewpoint_bins(viewpoints, chroms, off, self.Res, self.Allelic)
            for name, full, *_ in views:
                if chroms.index(full) not in sel:
                    raise ValueError(f"run_Virtual4C: viewpoint {name} lies on {full}, which Allelic={self.Allelic!r} "
                                     f"does not read")
            if not views:
                raise ValueError("run_Virtual4C: no viewpoint given")
            b1, b2, cnt = c.pixels_table()
        with SymTable(b1, b2, cnt, off, stream) as tab:
            P = tab.viewpoints([(lo, hi) for _, _, lo, hi, _, _ in views], wt, use, bad, ignore_diags)
        shown = [(name, names[chroms.index(full)], s, e) for name, full, _, _, s, e in views]
        r = dict(chroms=chroms, selected=sel, chrom_offset=off, valid=valid, viewpoints=views, P=P,
                 ignore_diags=int(ignore_diags))
        r["file"] = self._out_path(OutPath, "Virtual4C")
        write_virtual4c(r["file"], names, off, sel, int(self.Res), shown, P)
        self.Virtual4C_dict = r
        return r
