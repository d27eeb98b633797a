"""HICCUPS loop calling on MI355X — StructureFind.CallPeaks / pcaller
(HiCHap/StructureFind.py:1596-2043).

Per chromosome:

1. host: the raw band (main diagonal removed), the balanced band, the
   isotonic expected per diagonal (``sklearn.isotonic.IsotonicRegression(
   increasing='auto')`` on the balanced diagonal means — the reference's own
   call, :2022-2031) and the candidate pixels (nonzero raw contacts at
   ww <= d <= maxapart / res; the allelic gap / blanking filter, :1727-1759).
   O(N * num) glue.
2. GPU (``hh_hiccups_*``, csrc/loops.hip): the window-widening loop
   (:1776-1830) — donut and lower-left sums of the balanced and expected
   bands from per-row prefix sums, one launch per width; the host applies
   the reference's stop rule (< 10 % of the pending pixels became valid).
3. host: expected = EM * ratio * bias_i * bias_j, lambda chunks, Poisson
   p-values and Benjamini-Hochberg per chunk, q <= sig, the +-5-bin gap
   filter, donut AND lower-left (:1832-1948).  Vectorised; the p-values are
   computed once per distinct (observed count, chunk) and BH once per
   distinct p-value of a chunk — the same functions on the same inputs as
   the reference, so the results are identical.

Deviations (the reference raises): no candidate pixels, or every pixel valid
before the widening stops (its ratio divides by zero), return no calls.

The second half of the file is what ``run_Loops`` does with that table:
``Loop_Selecting`` (:2063-2094; ``diag_rank`` on the GPU, ``loop_select``) and
``LoopCluster`` (:2097-2243; ``peak_cluster`` .. ``loop_cluster``, host).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import call, ptr
from ._pixels import allelic_chroms, chrom_label


def peaks_parameter(res):
    """Peaks_Parameter (:1596-1615): dict(pw, ww, maxww, maxapart, sig)."""
    if res >= 20000:
        pw, ww = 1, 3
    elif res >= 10000:
        pw, ww = 2, 5
    else:
        pw, ww = 4, 7
    return dict(pw=pw, ww=ww, maxww=20, maxapart=2000000, sig=0.05)


def biases_from_weights(weights):
    """CallPeaks (:2007-2010): 1 / weight; weight == 0 -> 0; NaN stays NaN."""
    tmp = np.asarray(weights, dtype=np.float64)
    mask = np.logical_not(tmp == 0) | np.isnan(tmp)
    biases = np.zeros_like(tmp)
    biases[mask] = 1 / tmp[mask]
    return biases


def band_width(res, params=None):
    """``num`` of CallPeaks (:2020): diagonals 0 .. maxapart // res + maxww."""
    p = params or peaks_parameter(res)
    return p["maxapart"] // res + p["maxww"] + 1


def raw_band_from_pixels(bin1, bin2, count, lo, N, num):
    """raw[r, d] = H[r, r + d] (d < num) of chromosome bins [lo, lo + N)
    straight from cooler's upper-triangle pixel table (global ids, unique
    pixels): the band CallPeaks reads from ``matrix(balance=False).fetch``
    (:2006), without the N x N matrix."""
    b1 = np.asarray(bin1, dtype=np.int64) - lo
    b2 = np.asarray(bin2, dtype=np.int64) - lo
    c = np.asarray(count)
    d = b2 - b1
    k = (b1 >= 0) & (b1 < N) & (b2 < N) & (d >= 0) & (d < num)
    raw = np.zeros((N, num), dtype=c.dtype if c.dtype.kind in "iu" else np.float64)
    raw[b1[k], d[k]] = c[k]
    return raw


def bands(H_raw, weights, res, allelic=False, params=None, raw=None):
    """Raw / balanced bands, expected per diagonal and biases (:2003-2032),
    from the dense raw matrix or (``raw``, ``H_raw=None``) from its band."""
    p = params or peaks_parameter(res)
    num = band_width(res, p)
    if raw is None:
        H = np.asarray(H_raw)
        N = H.shape[0]
        r = np.arange(N)[:, None]
        d = np.arange(num)[None, :]
        raw = np.where((r + d) < N, H[r, np.minimum(r + d, N - 1)], 0)
    return _bands_from_raw(np.asarray(raw), weights, res, allelic, p)


def _bands_from_raw(raw, weights, res, allelic, p):
    from sklearn import isotonic
    ww = p["ww"]
    N, num = raw.shape
    r = np.arange(N)[:, None]
    d = np.arange(num)[None, :]
    inside = (r + d) < N
    cc = np.minimum(r + d, N - 1)
    if not allelic:
        w = np.asarray(weights, dtype=np.float64)
        # cH = nan_to_num(H * w_i * w_j), evaluated on the band in the same order
        bal = np.nan_to_num(raw.astype(float) * w[:, None] * np.where(inside, w[cc], 0.0))
        biases = biases_from_weights(w)
    else:
        bal = raw.astype(float)
        biases = np.ones(N)
    Hb = raw.astype(np.float64)
    Hb[:, 0] = 0.0                      # H - diag(H) (:2018)
    x = np.arange(ww, num)
    y = [bal[:N - i, i].mean() if i < N else np.nan for i in x]   # np.diagonal(cH, i).mean()
    IR = isotonic.IsotonicRegression(increasing="auto")
    IR.fit(x, y)
    pe = IR.predict(x)
    pe[pe < 0] = 0
    Eall = np.zeros(num)
    Eall[ww:] = pe
    Cb = np.where(d >= ww, bal, 0.0)
    return dict(N=N, num=num, res=res, allelic=allelic, Hb=np.ascontiguousarray(Hb),
                Cb=np.ascontiguousarray(Cb), Eall=Eall, biases=biases, **p)


def candidates(B, gap=None):
    """M.nonzero() with ww <= y - x <= maxapart // res (:1727-1730); for
    allelic data also the gap and blanking filter (:1731-1759), whose
    neighbour lookups follow the reference's dense-band indexing (row -1
    wraps to the last row; a column past the end counts as 1; `left` and
    `right` are the same cell)."""
    Hb, N, num = B["Hb"], B["N"], B["num"]
    rr, dd = np.nonzero(Hb)
    m = (dd >= B["ww"]) & (dd <= B["maxapart"] // B["res"])
    xi, yi = rr[m].astype(np.int64), (rr[m] + dd[m]).astype(np.int64)
    if B["allelic"]:
        def band(R, Cc):
            D = Cc - R
            ok = (D >= 0) & (D < num)
            v = np.zeros(R.shape)
            v[ok] = Hb[R[ok], D[ok]]
            return v
        gs = np.asarray(gap if gap is not None else [], dtype=np.int64)
        keep = ~(np.isin(xi, gs) & np.isin(yi, gs))
        left = band((xi - 1) % N, yi)
        top = np.where(yi + 1 >= N, 1.0, band(xi, np.minimum(yi + 1, N - 1)))
        bottom = band(xi, yi - 1)
        keep &= (left * left * top * bottom) != 0
        xi, yi = xi[keep], yi[keep]
    return xi, yi


class Neighbourhood:
    """Device state of one chromosome (``hh_hiccups``)."""

    def __init__(self, B, stream=None):
        _lib.require_gpu()
        self.B = B
        self.stream = stream
        h = C.c_void_p()
        call("hh_hiccups_create", ptr(B["Hb"]), ptr(B["Cb"]), ptr(np.ascontiguousarray(B["Eall"])), int(B["N"]),
             int(B["num"]), int(B["pw"]), 0, stream, C.byref(h))
        self._h = h

    def set_pixels(self, xi, yi):
        self.n = int(xi.size)
        r32 = np.ascontiguousarray(xi, dtype=np.int32)
        c32 = np.ascontiguousarray(yi, dtype=np.int32)
        call("hh_hiccups_set_pixels", self._h, ptr(r32), ptr(c32), self.n, self.stream)

    def widen(self):
        """The widening loop over the current pixels (all pending); returns
        [(w, newly valid, ratio)] with the reference's stop rule."""
        B = self.B
        pending = self.n
        widths = []
        for w in range(B["ww"], B["maxww"] + 1):
            if pending == 0:
                break  # the reference divides by zero here
            nv = C.c_int64(0)
            call("hh_hiccups_width", self._h, int(w), C.byref(nv), self.stream)
            ratio = nv.value / float(pending)
            pending -= nv.value
            widths.append((w, int(nv.value), ratio))
            if ratio < 0.1:
                break
        return widths

    def reset(self):
        call("hh_hiccups_reset", self._h, self.stream)

    def run(self, xi, yi):
        """The widening loop; returns (S, E, valid, widths) like the oracle."""
        self.set_pixels(xi, yi)
        widths = self.widen()
        n = self.n
        sK, sY, eK, eY = (np.empty(n) for _ in range(4))
        wid = np.empty(n, np.uint8)
        call("hh_hiccups_results", self._h, ptr(sK), ptr(sY), ptr(eK), ptr(eY), ptr(wid), self.stream)
        return {"K": sK, "Y": sY}, {"K": eK, "Y": eY}, wid != 0, widths

    def close(self):
        if getattr(self, "_h", None):
            call("hh_hiccups_free", self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lambda_chunks(E):
    """lambdachunk (:1617-1629) as (lv, rv) edges."""
    numbin = int(np.ceil(np.log(E.max()) / np.log(2) * 3 + 1))
    edges = []
    for i in range(1, numbin + 1):
        if i == 1:
            edges.append((0, 1))
        else:
            edges.append((np.power(2, ((i - 2) / 3.)), np.power(2, ((i - 1) / 3.))))
    return edges


def _bh_by_value(p):
    """statsmodels fdr_bh corrected p-values computed per distinct p-value
    (ties share a rank block; the reversed running minimum of p / (rank / n)
    over a block is its last rank's value)."""
    n = p.size
    u, inv, cnt = np.unique(p, return_inverse=True, return_counts=True)
    last = np.cumsum(cnt)                              # 1-based rank of each block's end
    ecdf = np.arange(1, n + 1) / float(n)              # statsmodels' ecdf factors
    raw = u / ecdf[last - 1]
    corr = np.minimum.accumulate(raw[::-1])[::-1]
    corr[corr > 1] = 1
    return corr[inv]


def significance(B, xi, yi, S, E, valid):
    """:1832-1948 -> (Donuts, LL) {(x*res, y*res): (O, fold, p, q)}."""
    from scipy.stats import poisson
    N, res, sig = B["N"], B["res"], B["sig"]
    mask = (E["K"] != 0) & (E["Y"] != 0) & valid
    xi, yi = xi[mask], yi[mask]
    gapind = (B["Hb"].sum(axis=1) == 0).astype(np.int64)
    gcum = np.concatenate([[0], np.cumsum(gapind)])
    res_fl = {}
    for fl in "KY":
        ratio = S[fl][mask] / E[fl][mask]
        cem = B["Eall"][yi - xi] * ratio
        nz = cem != 0
        x, y, cem = xi[nz], yi[nz], cem[nz]
        Ev = cem * B["biases"][x] * B["biases"][y]
        m = Ev > 0
        Ev, x, y = Ev[m], x[m], y[m]
        Ov = B["Hb"][x, y - x]
        fold = Ov / Ev
        pv = np.ones(x.size)
        qv = np.ones(x.size)
        edges = lambda_chunks(Ev) if Ev.size else []
        # no chunk at all when every expected value is below 2**(-2/3)
        # (numbin <= 0): the reference's lambdachunk Pool is empty, so p and q
        # stay 1 and nothing is called (StructureFind.py:1617-1629, :1866-1880)
        if edges:
            rvs = np.array([e[1] for e in edges], dtype=np.float64)
            lvs = np.array([e[0] for e in edges], dtype=np.float64)
            ci = np.searchsorted(rvs, Ev, side="right")        # first rv > E
            inchunk = ci < rvs.size
            ci_c = np.minimum(ci, rvs.size - 1)
            inchunk &= (Ev > lvs[ci_c]) & (Ev < rvs[ci_c])
            for c in np.unique(ci_c[inchunk]):
                idx = np.nonzero(inchunk & (ci_c == c))[0]
                ko, kinv = np.unique(Ov[idx], return_inverse=True)
                cp = (1 - poisson(edges[c][1]).cdf(ko))[kinv]
                pv[idx] = cp
                qv[idx] = _bh_by_value(cp)
        rej = qv <= sig
        x, y, Ov, fold, pv, qv = x[rej], y[rej], Ov[rej], fold[rej], pv[rej], qv[rej]
        if gapind.any():
            def lo_up(v):
                lo = np.where(v > 5, v - 5, 0)
                up = np.where(v + 5 < N, v + 5, N - 1)
                return lo, up
            l1, u1 = lo_up(x)
            l2, u2 = lo_up(y)
            hit = ((gcum[np.maximum(u1, l1)] - gcum[l1]) > 0) | ((gcum[np.maximum(u2, l2)] - gcum[l2]) > 0)
            keep = ~hit
            x, y, Ov, fold, pv, qv = x[keep], y[keep], Ov[keep], fold[keep], pv[keep], qv[keep]
        res_fl[fl] = (x * N + y, Ov, fold, pv, qv)
    kk, kc = res_fl["K"], res_fl["Y"]
    common, ia, ib = np.intersect1d(kk[0], kc[0], assume_unique=True, return_indices=True)
    Donuts, LL = {}, {}
    for j, lin in enumerate(common):
        pos = (int(lin // N) * res, int(lin % N) * res)
        a, b = ia[j], ib[j]
        Donuts[pos] = (kk[1][a], kk[2][a], kk[3][a], kk[4][a])
        LL[pos] = (kc[1][b], kc[2][b], kc[3][b], kc[4][b])
    return Donuts, LL


def pcaller(H_raw, weights, res, allelic=False, gap=None, stream=None, return_widths=False):
    """One chromosome of StructureFind.CallPeaks: (Donuts, LL) as the reference."""
    return _pcaller_bands(bands(H_raw, weights, res, allelic), gap, stream, return_widths)


def _pcaller_bands(B, gap=None, stream=None, return_widths=False):
    xi, yi = candidates(B, gap)
    nb = Neighbourhood(B, stream)
    try:
        S, E, valid, widths = nb.run(xi, yi)
    finally:
        nb.close()
    out = significance(B, xi, yi, S, E, valid)
    return out + (widths,) if return_widths else out


LINE_FORMAT = "%s\t%d\t%d\t%.4g\t%.4g\t%.4g\t%.4g\t%.4g\t%.4g\t%.4g\n"
HEAD = "\t".join(["chromLabel", "loc_1", "loc_2", "IF", "D-Enrichment", "D-pvalue", "D-qvalue",
                  "LL-Enrichment", "LL-pvalue", "LL-qvalue"]) + "\n"


def call_peaks_cooler(cooler_uri, outfil, res, allelic=False, gaps=None):
    """CallPeaks (:1954-2043) reading the cooler itself, as the reference
    does (:2003-2015): per chromosome the raw band from the pixel table
    (``matrix(balance=False)``), the balanced band from the same pixels and
    ``bins/weight`` (``matrix(balance=True)`` + nan_to_num, biases
    ``1 / weight``), allelic data raw with its gap list; no N x N matrix.
    ``allelic``: False, 'Maternal' or 'Paternal' (chromosomes by prefix)."""
    from .coolio import Cooler
    out = {}
    with Cooler(cooler_uri) as c:
        chroms = allelic_chroms(allelic, c.chromnames)
        if allelic is not False and gaps is None:
            raise ValueError("Gap file needed for haplotype-resolved loop calling ...")
        w_all = c.weights() if allelic is False else None
        num = band_width(res)
        with open(outfil, "w") as f:
            f.write(HEAD)
            for chro in chroms:
                lo, hi = c.extent(chro)
                b1, b2, v = c.pixel_rows(lo, hi)
                raw = raw_band_from_pixels(b1, b2, v, lo, hi - lo, num)
                w = None if w_all is None else w_all[lo:hi]
                B = bands(None, w, res, allelic is not False, raw=raw)
                D, L = _pcaller_bands(B, None if allelic is False else gaps[chro])
                out[chro] = (D, L)
                label = chrom_label(allelic, chro)
                for pos in sorted(D):
                    f.write(LINE_FORMAT % ((label,) + pos + tuple(D[pos]) + tuple(L[pos][1:])))
    return out


def call_peaks(matrices, res, outfil, allelic=False, gaps=None):
    """CallPeaks (:1953-2043) over {chrom: (raw dense H, weights)}; writes the
    reference's tab-separated file (positions sorted; the reference's Python-2
    dict order is arbitrary).  Returns {chrom: (Donuts, LL)}."""
    out = {}
    with open(outfil, "w") as f:
        f.write(HEAD)
        for chro, (H, w) in matrices.items():
            D, L = pcaller(H, w, res, allelic, None if gaps is None else gaps[chro])
            out[chro] = (D, L)
            label = chro if not allelic else chro[1:]
            for pos in sorted(D):
                f.write(LINE_FORMAT % ((label,) + pos + tuple(D[pos]) + tuple(L[pos][1:])))
    return out


# ------------------------------------------------------------------------
# Loop_Selecting / LoopCluster (HiCHap/StructureFind.py:2063-2243)
#
# Loop_Selecting keeps a called pixel by the rank of its raw count within its
# own diagonal: bisect_left(sorted(M.diagonal(d)), M[r][c]).  Diagonal d has
# N - d entries and all but its stored pixels are zero, so for IF > 0
#     bisect_left = (N - d - nnz_d) + #{pixels on d with count < IF}
# and 0 for IF = 0 -- integer compares over cooler's pixel table
# (``hh_diag_rank_pixels``, csrc/select.hip), no dense matrix.
#
# Deviations from the reference, all stated in DESIGN.md:
# * positions are divided by ``Res`` (the reference hard-codes 40000 in
#   Loop_Selecting, :2078-2079, and uses self.Res in LoopCluster); identical
#   at 40 kb;
# * chromosome names are not truncated to 4 bytes (its 'S4' dtype);
# * chromosomes are clustered in order of first appearance in the file (its
#   ``list(set(...))`` order is arbitrary).

SELECT_HEAD = "\t".join(["chromLabel", "loc_1", "loc_2", "IF", "D-Enrichment", "D-pvalue", "LL-Enrichment",
                         "LL-pvalue", "LL-qvalue"]) + "\n"
CLUSTER_HEAD = "chr\tstart\tend\tIF\tweight_Q-value\taggregateNum\n"


def _int_counts(count):
    c = np.asarray(count)
    if c.dtype.kind == "f":
        if np.any(c != np.floor(c)):
            raise ValueError("raw counts must be integers")
    elif c.dtype.kind not in "iu":
        raise ValueError(f"raw counts must be integers, not {c.dtype}")
    return np.ascontiguousarray(c, dtype=np.int64)


def diag_rank(bin1, bin2, count, lo, N, rows, cols, stream=None):
    """(value, less) of the pixels (rows, cols) of chromosome bins
    [lo, lo + N) from cooler's pixel table (``bin1 <= bin2`` global ids of
    unique pixels; pixels reaching outside the chromosome are ignored):
    ``value`` the raw count (0 where no pixel is stored), ``less`` the number
    of entries of diagonal ``cols - rows`` of the symmetric dense matrix that
    are strictly smaller -- ``bisect_left(sorted(M.diagonal(d)), M[r][c])``.
    Exact int64, on the GPU (``hh_diag_rank_pixels``).  The pixel arrays may
    be int64 device tensors (no copy)."""
    _lib.require_gpu()
    r32 = np.ascontiguousarray(rows, dtype=np.int32)
    c32 = np.ascontiguousarray(cols, dtype=np.int32)
    if r32.shape != c32.shape or r32.ndim != 1:
        raise ValueError("rows and cols must be 1-D and of one length")
    if not (np.array_equal(r32, np.asarray(rows)) and np.array_equal(c32, np.asarray(cols))):
        raise ValueError("query bins do not fit int32")
    on_dev = bool(getattr(bin1, "is_cuda", False))
    if on_dev:
        import torch
        for t in (bin1, bin2, count):
            if not (getattr(t, "is_cuda", False) and t.dtype == torch.int64 and t.dim() == 1 and t.is_contiguous()):
                raise ValueError("device pixel arrays must be contiguous 1-D int64 tensors")
        b1, b2, c = bin1, bin2, count
        nnz = int(b1.numel())
        if not (int(b2.numel()) == int(c.numel()) == nnz):
            raise ValueError("bin1, bin2 and count must have the same length")
    else:
        b1 = np.ascontiguousarray(bin1, dtype=np.int64)
        b2 = np.ascontiguousarray(bin2, dtype=np.int64)
        c = _int_counts(count)
        if not (b1.shape == b2.shape == c.shape and b1.ndim == 1):
            raise ValueError("bin1, bin2 and count must be 1-D and of one length")
        nnz = int(b1.size)
    value = np.zeros(r32.size, np.int64)
    less = np.zeros(r32.size, np.int64)
    call("hh_diag_rank_pixels", ptr(b1), ptr(b2), ptr(c), nnz, int(lo), int(N), ptr(r32), ptr(c32), int(r32.size),
         ptr(value), ptr(less), 1 if on_dev else 0, None if stream is None else C.c_void_p(int(stream)))
    return value, less


def diag_rank_reference(bin1, bin2, count, lo, N, rows, cols):
    """NumPy restatement of ``diag_rank`` (``lexsort`` + ``searchsorted``
    over the same pixels) for the tests and tools/bench_loop_select.py; the
    library never calls it."""
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    b1 = np.asarray(bin1, dtype=np.int64) - lo
    b2 = np.asarray(bin2, dtype=np.int64) - lo
    c = _int_counts(count)
    k = (b1 >= 0) & (b1 < N) & (b2 >= 0) & (b2 < N)
    b1, b2, c = b1[k], b2[k], c[k]
    d = b2 - b1
    qd = cols - rows
    key = d * N + b1
    ko = np.argsort(key, kind="stable")
    ks = key[ko]
    qk = qd * N + rows
    pos = np.minimum(np.searchsorted(ks, qk), max(ks.size - 1, 0))
    found = (ks[pos] == qk) if ks.size else np.zeros(qk.shape, bool)
    value = np.where(found, c[ko][pos] if ks.size else 0, 0).astype(np.int64)
    order = np.lexsort((c, d))
    ds, cs = d[order], c[order]
    span = int(cs.max()) + 2 if cs.size else 2
    comb = ds * span + cs                              # sorted: by diagonal, then count
    start = np.searchsorted(ds, qd, side="left")
    nnz_d = np.searchsorted(ds, qd, side="right") - start
    smaller = np.searchsorted(comb, qd * span + np.minimum(value, span - 1), side="left") - start
    less = np.where(value > 0, (N - qd - nnz_d) + smaller, 0).astype(np.int64)
    return value, less


def loop_select(lines, rank_fn, res, ratio, strength):
    """Body of Loop_Selecting (:2063-2094) over the lines of a HICCUPS table
    (the first is its header and is skipped): the output lines -- the
    reference's nine-name header (:2070-2071; the data lines keep their ten
    columns), then verbatim every line that is not rejected by
    ``less / (N - d) < ratio or IF < strength``.

    ``rank_fn(chrom, rows, cols) -> (value, less, N)`` is called once per
    chromosome with that chromosome's pixels (``diag_rank`` on its cooler
    pixels and its bin count N).

    Deviation: positions are divided by ``res`` where the reference
    hard-codes 40000 (:2078-2079) although LoopCluster, a few lines later,
    uses ``self.Res``; identical at 40 kb."""
    body = [ln for ln in list(lines)[1:] if ln.strip()]
    per = {}
    for k, ln in enumerate(body):
        f = ln.strip().split()
        b1, b2 = int(f[1]) // res, int(f[2]) // res
        per.setdefault(f[0], []).append((k, min(b1, b2), max(b1, b2)))
    keep = np.zeros(len(body), dtype=bool)
    for chro, items in per.items():
        idx = np.array([t[0] for t in items])
        rows = np.array([t[1] for t in items], dtype=np.int64)
        cols = np.array([t[2] for t in items], dtype=np.int64)
        value, less, N = rank_fn(chro, rows, cols)
        for j in range(idx.size):
            IF = int(value[j])
            rank = int(less[j]) / (int(N) - int(cols[j] - rows[j]))
            keep[idx[j]] = not (rank < ratio or IF < strength)
    return [SELECT_HEAD] + [ln for ln, k in zip(body, keep) if k]


def _center_sites(lists):
    """center_sites (:2097-2104): the running mean of a class."""
    n = len(lists)
    return [float(sum(x[1] for x in lists)) / n, float(sum(x[2] for x in lists)) / n]


def _distance(center, loop):
    """distance (:2106-2107)."""
    import math
    return math.sqrt((center[0] - loop[1]) ** 2 + (center[1] - loop[2]) ** 2)


def peak_cluster(loop_sites, dis, chroms):
    """peakcluster (:2109-2127) over tuples (chr, S1, E1, Q[, sums]).

    The reference removes from ``c_loops`` inside ``for loop in c_loops``
    (:2118-2122): after each accepted loop the list iterator skips the
    element that slid into its place.  The iterator is emulated by index so
    that the classes are the reference's; this is not "fixed"."""
    classes = []
    for chro in chroms:
        c_loops = sorted((x for x in loop_sites if x[0] == chro), key=lambda x: x[1])
        while True:
            c_class = [c_loops[0]]
            c_loops.remove(c_loops[0])
            center = _center_sites(c_class)
            i = 0                                   # CPython's list iterator
            while i < len(c_loops):
                loop = c_loops[i]
                i += 1
                if _distance(center, loop) <= dis:
                    c_class.append(loop)
                    center = _center_sites(c_class)
                    c_loops.remove(loop)
            classes.append(c_class)
            if len(c_loops) == 0:
                break
    return classes


def filter_initial(cls):
    """filter_initial (:2129-2138): per class the member with the smallest Q
    (stable sort), ``sums`` = the class size."""
    out = []
    for outs in cls:
        best = sorted(outs, key=lambda x: x[3])[0]
        out.append((best[0], int(best[1]), int(best[2]), float(best[3]), float(len(outs))))
    return out


def filter_next(cls):
    """filter_next (:2140-2152): as filter_initial, ``sums`` = the sum of the
    members' ``sums``."""
    out = []
    for outs in cls:
        sums = 0
        for x in outs:
            sums += x[4]
        best = sorted(outs, key=lambda x: x[3])[0]
        out.append((best[0], int(best[1]), int(best[2]), float(best[3]), float(sums)))
    return out


def read_loop_table(rawfil):
    """``np.loadtxt(rawfil, usecols=[0, 1, 2, 9], skiprows=1)`` (:2169-2172)
    as tuples (chr, S1, E1, Q); names are kept whole."""
    loops = []
    with open(rawfil) as f:
        for k, ln in enumerate(f):
            if k == 0 or not ln.strip():
                continue
            p = ln.split()
            loops.append((p[0], int(p[1]), int(p[2]), float(p[9])))
    return loops


def cluster_rounds(loops, res):
    """The clustering rounds of LoopCluster (:2174-2186): one round at
    ``Res * sqrt(2) + 1000``, then rounds at twice that until the number of
    loops stops changing.  Returns (loop_final, rounds of the second kind)."""
    import math
    dis = res * math.sqrt(2) + 1000
    chroms = list(dict.fromkeys(x[0] for x in loops))
    loop_initial = filter_initial(peak_cluster(loops, dis, chroms))
    rounds = 0
    while True:
        loop_final = filter_next(peak_cluster(loop_initial, dis * 2, chroms))
        rounds += 1
        if len(loop_initial) == len(loop_final):
            break
        loop_initial = loop_final
    return loop_final, rounds


def loop_cluster(rawfil, res, allelic, value_fn, weight_q_value=1e-4):
    """LoopCluster (:2154-2243): cluster the loops of ``rawfil`` (a HICCUPS
    table or the Selected_ file) and write ``Cluster_<name>`` next to it;
    returns that path.

    ``value_fn(chrom, rows, cols) -> raw counts`` is called once per
    chromosome with the loops that pass ``q = Q / 10 ** sums <
    weight_q_value`` (``diag_rank``'s ``value``); for haplotype data
    (``allelic`` 'Maternal' / 'Paternal') ``chrom`` carries the 'M' / 'P'
    prefix (:2208-2211).  Traditional lines are ``chr, start, end, IF, q,
    sums``; haplotype data go through the reference's typed table (IF float,
    level int), ``w_q == 0 -> 1e-20`` and the per-chromosome 15th-percentile
    filter of ``IF * -log10(w_q)`` (:2218-2239).  Numbers are printed as
    Python 2's ``str`` prints them.

    A table without data lines gives a header-only file (the reference
    raises on fewer than two lines).  Chromosome names are not truncated and
    chromosomes are processed in order of first appearance (see above)."""
    import os
    from .StructureFind import py2_float_str
    loops = read_loop_table(rawfil)
    loop_final = cluster_rounds(loops, res)[0] if loops else []
    kept = []
    with np.errstate(over="ignore"):
        for outs in loop_final:
            q = np.float64(outs[3]) / (10 ** np.float64(outs[4]))
            if q < weight_q_value:
                kept.append(outs + (float(q),))
    prefix = "" if allelic is False else allelic[0]
    IF = [0] * len(kept)
    for chro in dict.fromkeys(x[0] for x in kept):
        idx = [k for k, x in enumerate(kept) if x[0] == chro]
        x = np.array([kept[k][1] // res for k in idx], dtype=np.int64)
        y = np.array([kept[k][2] // res for k in idx], dtype=np.int64)
        v = value_fn(prefix + chro, np.minimum(x, y), np.maximum(x, y))
        for k, val in zip(idx, v):
            IF[k] = int(val)
    path, fil = os.path.split(rawfil)
    cluster_fil = os.path.join(path or "./", "Cluster_" + fil)
    with open(cluster_fil, "w") as f:
        f.write(CLUSTER_HEAD)
        if allelic is False:
            for x, v in zip(kept, IF):
                f.write("\t".join([x[0], str(x[1]), str(x[2]), str(v), py2_float_str(x[5]),
                                   py2_float_str(x[4])]) + "\n")
        else:
            w_q = np.array([x[5] for x in kept], dtype=np.float64)
            w_q[w_q == 0] = 10.0 ** (-20)
            IFf = np.array(IF, dtype=np.float64)
            level = [int(x[4]) for x in kept]
            with np.errstate(divide="ignore"):
                score = IFf * -np.log10(w_q)
            names = np.array([x[0] for x in kept], dtype=object)
            thr = {chro: np.percentile(score[names == chro], 15) for chro in dict.fromkeys(names)}
            for k, x in enumerate(kept):
                if (IFf[k] * -np.log10(w_q[k])) < thr[x[0]]:       # per row, as :2233-2235
                    continue
                f.write("\t".join([x[0], str(x[1]), str(x[2]), py2_float_str(IFf[k]), py2_float_str(w_q[k]),
                                   str(level[k])]) + "\n")
    return cluster_fil


__all__ = ["peaks_parameter", "bands", "band_width", "raw_band_from_pixels", "call_peaks_cooler", "candidates", "Neighbourhood", "significance", "pcaller", "call_peaks",
           "lambda_chunks", "biases_from_weights", "diag_rank", "diag_rank_reference", "loop_select", "peak_cluster",
           "filter_initial", "filter_next", "cluster_rounds", "loop_cluster", "read_loop_table"]
