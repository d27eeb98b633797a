"""Allele-specific loops, TAD boundaries and compartments on MI355X --
``HiCHap/AllelicSpecificity.py``, same class names, constructor arguments and
methods.

What moves data runs on the GPU; what is arithmetic stays the reference's:

* ``pixel_windows`` (``hh_pixel_windows``, csrc/allelic.hip) gathers the cells
  the loop and boundary classes read -- one cell per loop, a ``2 * offset``
  square per boundary -- from cooler's pixel table, one call per ``M<chrom>`` /
  ``P<chrom>`` holding all of that chromosome's loops or boundaries.  The
  reference fetches two dense float64 N x N matrices per chromosome for this
  (:79-80, :291-292); no N x N matrix is built here.  The gathered tiles are
  bit-equal to the dense slices.
* ``pairdiff_rank`` (``hh_pairdiff_rank``) is ``bisect_left`` on the sorted
  list of all K_M x K_P differences of the compartment candidates (:477-481,
  :509), counted exactly without the list, one call for all candidates.
* Everything after that (background, samples, ``ttest_rel``, ``norm.sf``, the
  percentile, Benjamini-Hochberg) is host NumPy / SciPy, the reference's calls
  in the reference's order on equal inputs.  BH is ``loops._bh_by_value``;
  floats print as Python 2's ``str`` (``StructureFind.py2_float_str``).

Deviations from the reference ("Allelic specificity"):

1. the two boundary branches that append stale ``M_mean`` / ``P_mean`` /
   ``stats`` (:376, :383) write the means and statistic of the pair tested;
2. a boundary whose window leaves the chromosome is skipped with a message
   (the reference gives a NaN p-value that turns every q-value NaN);
3. so is one with fewer than 2 pairs after ``removeGap`` or a window without a
   nonzero cell;
4. chromosome names are kept whole (its 'S4' / 'S8' dtypes truncate them).
"""
from __future__ import annotations

import bisect
import ctypes as C
import math
import os

import numpy as np

from . import _lib
from ._lib import call, ptr
from .loops import _bh_by_value
from .StructureFind import py2_float_str


def _stream(stream):
    return None if stream is None else C.c_void_p(int(stream))


def pixel_windows(bin1, bin2, count, lo, N, wrow, wcol, h, w, stream=None):
    """Dense ``h x w`` windows of the symmetric raw matrix of chromosome bins
    ``[lo, lo + N)`` from cooler's pixel table (global ids, ``bin1 <= bin2``,
    sorted by (bin1, bin2); pixels reaching outside the chromosome are
    ignored): ``out[k]`` = rows ``wrow[k] ..``, columns ``wcol[k] ..`` of
    ``matrix(balance=False).fetch``, 0.0 where no pixel is stored.  Exact, on
    the GPU (``hh_pixel_windows``).  With int64 / int64 / float64 device
    tensors as the pixel arrays the result is a device tensor (no copy)."""
    _lib.require_gpu()
    r32 = np.ascontiguousarray(wrow, dtype=np.int32)
    c32 = np.ascontiguousarray(wcol, dtype=np.int32)
    if r32.shape != c32.shape or r32.ndim != 1:
        raise ValueError("wrow and wcol must be 1-D and of one length")
    if not (np.array_equal(r32, np.asarray(wrow)) and np.array_equal(c32, np.asarray(wcol))):
        raise ValueError("window bins do not fit int32")
    nw, h, w = int(r32.size), int(h), int(w)
    on_dev = bool(getattr(bin1, "is_cuda", False))
    if on_dev:
        import torch
        for t, dt in ((bin1, torch.int64), (bin2, torch.int64), (count, torch.float64)):
            if not (getattr(t, "is_cuda", False) and t.dtype == dt and t.dim() == 1 and t.is_contiguous()):
                raise ValueError("device pixel arrays must be contiguous 1-D int64 / int64 / float64 tensors")
        b1, b2, c = bin1, bin2, count
        nnz = int(b1.numel())
        if not (int(b2.numel()) == int(c.numel()) == nnz):
            raise ValueError("bin1, bin2 and count must have the same length")
        out = torch.zeros((nw, h, w), dtype=torch.float64, device=b1.device)
    else:
        b1 = np.ascontiguousarray(bin1, dtype=np.int64)
        b2 = np.ascontiguousarray(bin2, dtype=np.int64)
        c = np.ascontiguousarray(count, dtype=np.float64)
        if not (b1.shape == b2.shape == c.shape and b1.ndim == 1):
            raise ValueError("bin1, bin2 and count must be 1-D and of one length")
        nnz = int(b1.size)
        out = np.zeros((nw, h, w), dtype=np.float64)
    call("hh_pixel_windows", ptr(b1), ptr(b2), ptr(c), nnz, int(lo), int(N), ptr(r32), ptr(c32), nw, h, w,
         ptr(out), 1 if on_dev else 0, _stream(stream))
    return out


def pairdiff_rank(a, b, q, stream=None):
    """``less[k] = #{(i, j) : a[i] - b[j] < q[k]}`` (the fp64 subtract), i.e.
    ``bisect_left(sorted(a_i - b_j for all i, j), q[k])`` without the list.
    Exact int64, on the GPU (``hh_pairdiff_rank``)."""
    _lib.require_gpu()
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    q = np.ascontiguousarray(q, dtype=np.float64)
    if not (a.ndim == b.ndim == q.ndim == 1):
        raise ValueError("a, b and q must be 1-D")
    less = np.zeros(q.size, np.int64)
    call("hh_pairdiff_rank", ptr(a), int(a.size), ptr(b), int(b.size), ptr(q), int(q.size), ptr(less), 0,
         _stream(stream))
    return less


def _py2_str(v):
    """Python 2's ``str`` of what the three tables hold."""
    if isinstance(v, (float, np.floating)):
        return py2_float_str(v)
    if isinstance(v, (int, np.integer)):
        return "%d" % int(v)
    return "%s" % (v,)


def _read_columns(fil, kinds):
    """Whitespace-separated columns of a headerless table (``np.loadtxt``
    with a typed record, names kept whole): a list of tuples."""
    rows = []
    with open(fil) as f:
        for ln in f:
            p = ln.split()
            if not p or p[0].startswith("#"):
                continue
            rows.append(tuple(k(x) for k, x in zip(kinds, p)))
    return rows


def _gather(cooler, chrom, wrow, wcol, h, w, stream=None):
    """Windows of one chromosome of an open ``coolio.Cooler``."""
    lo, hi = cooler.extent(chrom)
    b1, b2, v = cooler.pixel_rows(lo, hi)
    return pixel_windows(b1, b2, v, lo, hi - lo, wrow, wcol, h, w, stream=stream), hi - lo


class LoopAllelicSpecificity(object):
    """Reliability of allelic specificity of candidate loops (:16-238).

    ``Loop_file``: one loop per line, ``chr  M_loc1  M_loc2  P_loc1  P_loc2``
    (no header).  ``Running()`` writes ``Allelic_Specificity_<Loop file
    name>`` next to it.  Attributes as the reference: ``Data`` (before and
    after the filter), ``Mean``, ``p``, ``sum_M``, ``sum_T``, ``outfile``.

    Reference behaviour kept as it is:

    * ``Mean = (M_IF + P_IF) // 2`` on floats, zeros dropped, sorted;
    * ``vmax = np.percentile(np.nonzero(Mean), 95)`` is a percentile of the
      INDICES of ``Mean`` (0.95 * (len - 1)), not of its values (:173-174);
    * ``calculate_single_stat``: 'NA' for an empty side or an expected count
      below 5, the plain z from 30 up, the continuity-corrected |z| between;
    * ``QR`` = ``bisect_left(Mean, (M_IF + P_IF) // 2) / len(Mean)``.

    The two cells of a loop come from one ``pixel_windows`` call (1 x 1
    windows) per ``M<chrom>`` / ``P<chrom>``; chromosome names are whole.
    """

    def __init__(self, cooler_uri, Loop_file, Res):
        self.cooler_fil = "{}::{}".format(cooler_uri, Res)
        self.Loop_file = Loop_file
        self.Res = Res
        self.stream = None

    def DataSetBuilding(self):
        from .coolio import Cooler
        loops = _read_columns(self.Loop_file, (str, int, int, int, int))
        Path, prefix = os.path.split(self.Loop_file)
        self.outfile = os.path.join(Path, "Allelic_Specificity_" + prefix)
        M_IF = np.zeros(len(loops))
        P_IF = np.zeros(len(loops))
        with Cooler(self.cooler_fil) as c:
            for chro in dict.fromkeys(lp[0] for lp in loops):
                idx = np.array([k for k, lp in enumerate(loops) if lp[0] == chro])
                pos = np.array([loops[k][1:] for k in idx], dtype=np.int64) // self.Res
                M_IF[idx] = np.asarray(_gather(c, "M" + chro, pos[:, 0], pos[:, 1], 1, 1, self.stream)[0]).ravel()
                P_IF[idx] = np.asarray(_gather(c, "P" + chro, pos[:, 2], pos[:, 3], 1, 1, self.stream)[0]).ravel()
        DataSet_type = np.dtype({"names": ["chr", "start1", "end1", "start2", "end2", "M_IF", "P_IF"],
                                 "formats": ["U64", np.int64, np.int64, np.int64, np.int64, np.float64,
                                             np.float64]})
        self.Data = np.array([lp + (m, p) for lp, m, p in zip(loops, M_IF, P_IF)], dtype=DataSet_type)

    def calculate_two_group_stat(self, count, nobs):
        """Return stats of two property group test (:106-116)."""
        p1 = count[0] / nobs[0]
        p2 = count[1] / nobs[1]
        p_ = (nobs[0] * p1 + nobs[1] * p2) / (nobs[0] + nobs[1])
        return (p1 - p2) / math.sqrt((p_ * (1 - p_)) * ((1 / nobs[0]) + (1 / nobs[1])))

    def calculate_single_stat(self, p, count, nobs):
        """Return stats of Single group property test (:118-136)."""
        if count == 0 or (nobs - count) == 0:
            return "NA"
        p_ = count / nobs
        if p * nobs < 5 or (1 - p) * nobs < 5:
            return "NA"
        elif p * nobs >= 30 and (1 - p) * nobs >= 30:
            t = (nobs * p_ - nobs * p) / math.sqrt(nobs * p * (1 - p))
        else:
            t = (abs(nobs * p_ - nobs * p) - 0.5) / math.sqrt(nobs * p * (1 - p))
        return t

    def calculate_Pvalue(self, stat):
        """Two-sided P-value of the z-test (:138-146)."""
        from scipy import stats
        if isinstance(stat, str):
            return "NA"
        return stats.norm.sf(abs(stat)) * 2

    def BH_adjust_pvalue(self, P_value, alpha=0.05):
        """Benjamini-Hochberg q-values (:148-154)."""
        return _bh_by_value(np.asarray(P_value, dtype=np.float64))

    def Distribution(self):
        Mean = (self.Data["M_IF"] + self.Data["P_IF"]) // 2
        Mean = Mean[Mean.nonzero()]
        Mean.sort()
        self.Mean = Mean

    def BackGround(self):
        print("Filtering the candidate loops ...")
        self.Distribution()
        nonzero = np.nonzero(self.Mean)
        vmax = np.percentile(nonzero, 95) if self.Mean.size else np.nan
        mask = ((self.Data["M_IF"] + self.Data["P_IF"]) / 2 <= vmax) & \
               (self.Data["M_IF"] != 0) & (self.Data["P_IF"] != 0)
        self.Data = self.Data[mask]
        self.sum_M = self.Data["M_IF"].sum()
        self.sum_T = self.Data["M_IF"].sum() + self.Data["P_IF"].sum()

    def Running(self):
        print("=================Allelic Specificity==============")
        print("DataSet preparing ...")
        self.DataSetBuilding()
        print("Background preparing ...")
        self.BackGround()
        with np.errstate(invalid="ignore"):
            self.p = self.sum_M / self.sum_T
        print("Maternal total ratio %s." % self.p)
        print("Modeling ...")
        head = ["chr", "startM", "endM", "startP", "endP", "M_IF", "P_IF", "QR", "Log2(FC)", "stat", "P_value"]
        with open(self.outfile, "w") as out:
            out.writelines("\t".join(head) + "\n")
            for loop in self.Data:
                loop_M = loop["M_IF"]
                loop_T = loop["P_IF"] + loop["M_IF"]
                stat = self.calculate_single_stat(self.p, loop_M, loop_T)
                pvalue = self.calculate_Pvalue(stat)
                if isinstance(stat, str):
                    Ratio_P = "NA"
                    FC = "NA"
                else:
                    loop_mean = loop_T // 2
                    Ratio_P = bisect.bisect_left(self.Mean, loop_mean) / len(self.Mean)
                    FC = np.log2((loop_M) / (loop_T - loop_M))
                Info = [loop["chr"], loop["start1"], loop["end1"], loop["start2"], loop["end2"],
                        loop["M_IF"], loop["P_IF"], Ratio_P, FC, stat, pvalue]
                out.writelines("\t".join(map(_py2_str, Info)) + "\n")
        print("Done!")


class BoundaryAllelicSpecificity(object):
    """Allelic specificity of TAD boundaries (:242-428).

    ``Boundary_fil``: ``chr  maternal_boundary  paternal_boundary`` per line
    (no header).  ``Running(Outfil)`` writes the table; ``results`` is the
    reference's record array.  Each chromosome's windows (the ``2 * offset``
    square around every position named for it) come from one
    ``pixel_windows`` call per haplotype.

    Reference behaviour kept as it is:

    * the diagonal is zeroed first (:341-342);
    * the sample is ``np.tril`` of the ``offset x offset`` block above the
      diagonal divided by BG, a length ``offset ** 2`` vector whose 45 of 100
      upper entries are always 0 and count in the 0.85 zero test;
    * BG is the mean over the nonzeros of the two symmetric flanking blocks
      plus the tril block (:304-308);
    * with ``M_pos == P_pos`` the two means are of the whole samples, taken
      before ``removeGap`` (:352-353);
    * with both positions valid the pair with the smaller p is written, its
      means taken after ``removeGap`` (:386-395).

    Deviations: (1) when exactly one position passes the zero test the
    reference appends ``M_mean`` / ``P_mean`` / ``stats`` left over from an
    earlier boundary (:376, :383); here the means (after ``removeGap``) and
    the statistic of the pair that was tested are written, with the same p.
    (2) A boundary with ``b - offset < 0`` or ``b + offset > N`` and (3) one
    with fewer than 2 pairs after ``removeGap`` or a window without a nonzero
    cell are skipped with a message (the reference's NaN p-value turns every
    q-value of the file NaN).  (4) Names are whole.
    """

    def __init__(self, cooler_fil, Boundary_fil, Res, offset=10):
        self.cooler_fil = "{}::{}".format(cooler_fil, Res)
        self.Res = Res
        self.offset = offset
        self.BoundaryFile = Boundary_fil
        self.stream = None

    def LoadingBoundary(self):
        dtype = np.dtype({"names": ["chr", "pos1", "pos2"], "formats": ["U64", np.int64, np.int64]})
        self.boundarys = np.array(_read_columns(self.BoundaryFile, (str, int, int)), dtype=dtype)

    def DataSetBuilding(self):
        """``M_Tiles`` / ``P_Tiles``: {chrom: {bin: 2 offset x 2 offset tile,
        diagonal zeroed}} for every position whose window fits; ``N``:
        {chrom: bins}."""
        from .coolio import Cooler
        print("Loading Boundaries")
        self.LoadingBoundary()
        print("Loading Matrix")
        o = self.offset
        self.M_Tiles, self.P_Tiles, self.N = {}, {}, {}
        with Cooler(self.cooler_fil) as c:
            for chro in dict.fromkeys(self.boundarys["chr"].tolist()):
                sel = self.boundarys[self.boundarys["chr"] == chro]
                pos = np.unique(np.concatenate([sel["pos1"], sel["pos2"]]) // self.Res)
                self.N[chro] = c.extent("M" + chro)[1] - c.extent("M" + chro)[0]
                fit = pos[(pos - o >= 0) & (pos + o <= self.N[chro])]
                for tiles, hap in ((self.M_Tiles, "M"), (self.P_Tiles, "P")):
                    T = np.array(_gather(c, hap + chro, fit - o, fit - o, 2 * o, 2 * o, self.stream)[0])
                    T[:, np.arange(2 * o), np.arange(2 * o)] = 0.0
                    tiles[chro] = dict(zip(fit.tolist(), T))

    def SampleGenerate(self, M, b):
        """The sample of position ``b`` (:294-315) from its tile ``M[b]``;
        None when no cell of the three blocks is nonzero."""
        o = self.offset
        T = M[b]
        upstream = T[:o, :o]
        downstream = T[o:, o:]
        middlestream = np.tril(T[:o, o:])
        up_non = upstream[np.nonzero(upstream)]
        down_non = downstream[np.nonzero(downstream)]
        middle_non = middlestream[np.nonzero(middlestream)]
        if len(up_non) + len(down_non) + len(middle_non) == 0:
            return None
        BG = (up_non.sum() + down_non.sum() + middle_non.sum()) / (len(up_non) + len(down_non) + len(middle_non))
        middlestream = middlestream / BG
        N = middlestream.shape[0] * middlestream.shape[1]
        return middlestream.reshape((N,))

    def removeGap(self, M_S, P_S):
        bool_mask = (M_S != 0) & (P_S != 0)
        return M_S[bool_mask], P_S[bool_mask]

    def Calculating(self):
        from scipy.stats import ttest_rel
        self.DataSetBuilding()
        print("Calculating ...")
        Info = []
        p_value = []
        o = self.offset

        def zeros(S):
            return (S == 0).sum() / len(S) >= 0.85

        def tested(M_S, P_S):
            """removeGap + ttest_rel; None with fewer than 2 pairs."""
            M_S, P_S = self.removeGap(M_S, P_S)
            if len(M_S) < 2:
                return None
            stat, p = ttest_rel(M_S, P_S)
            return M_S, P_S, stat, p

        for bound in self.boundarys:
            chro = str(bound["chr"])
            label = (chro, bound["pos1"], bound["pos2"])
            M_M, P_M, N = self.M_Tiles[chro], self.P_Tiles[chro], self.N[chro]
            M_pos = int(bound["pos1"] // self.Res)
            P_pos = int(bound["pos2"] // self.Res)
            if any(b - o < 0 or b + o > N for b in (M_pos, P_pos)):
                print("Chromosome %s Boundary M:%s -- P:%s too close to the chromosome end.. skip ..." % label)
                continue
            few = "Chromosome %s Boundary M:%s -- P:%s fewer than 2 nonzero pairs.. skip ..." % label
            many = "Chromosome %s Boundary M:%s -- P:%s surrounded by too much zero bins.. skip ..." % label
            if M_pos == P_pos:
                M_S = self.SampleGenerate(M_M, M_pos)
                P_S = self.SampleGenerate(P_M, P_pos)
                if M_S is None or P_S is None:
                    print("Chromosome %s Boundary M:%s -- P:%s without a nonzero cell.. skip ..." % label)
                    continue
                M_mean = M_S.mean()
                P_mean = P_S.mean()
                if zeros(M_S) or zeros(P_S):
                    print(many)
                    continue
                t = tested(M_S, P_S)
                if t is None:
                    print(few)
                    continue
                Info.append(label + (M_mean, P_mean, t[2], t[3]))
                p_value.append(t[3])
            else:
                M_S1 = self.SampleGenerate(M_M, M_pos)
                P_S1 = self.SampleGenerate(P_M, M_pos)
                M_S2 = self.SampleGenerate(M_M, P_pos)
                P_S2 = self.SampleGenerate(P_M, P_pos)
                if any(S is None for S in (M_S1, P_S1, M_S2, P_S2)):
                    print("Chromosome %s Boundary M:%s -- P:%s without a nonzero cell.. skip ..." % label)
                    continue
                valid1 = not (zeros(M_S1) or zeros(P_S1))
                valid2 = not (zeros(M_S2) or zeros(P_S2))
                if not valid1 and not valid2:
                    print(many)
                    continue
                t1 = tested(M_S1, P_S1) if valid1 else None
                t2 = tested(M_S2, P_S2) if valid2 else None
                if (valid1 and t1 is None) or (valid2 and t2 is None):
                    print(few)
                    continue
                if valid1 and valid2:
                    t = t1 if t1[3] < t2[3] else t2
                else:
                    t = t1 if valid1 else t2           # deviation 1: this pair's own means and statistic
                Info.append(label + (t[0].mean(), t[1].mean(), t[2], t[3]))
                p_value.append(t[3])

        print("BH fdr processing ...")
        Q_value = _bh_by_value(np.asarray(p_value, dtype=np.float64)) if p_value else []
        dtype = np.dtype({"names": ["chr", "boundary1", "boundary2", "M_mean", "P_mean", "stat", "p_value",
                                    "q_value"],
                          "formats": ["U64", np.int64, np.int64, np.float64, np.float64, np.float64, np.float64,
                                      np.float64]})
        self.results = np.array([tuple(Info[i]) + (Q_value[i],) for i in range(len(Info))], dtype=dtype)

    def OutputTXT(self, outfil):
        print("Output ...")
        head = ["chr", "boundaryM", "boundaryP", "M_mean", "P_mean", "stat", "p_value", "q_value"]
        with open(outfil, "w") as o:
            o.writelines("\t".join(head) + "\n")
            for line in self.results:
                o.writelines("\t".join(map(_py2_str, line.tolist())) + "\n")

    def Running(self, Outfil):
        self.Calculating()
        self.OutputTXT(Outfil)
        print("Done !!!")


class CompartmentAllelicSpecificity(object):
    """Allelic specificity of compartments (:432-551) from the maternal and
    paternal PC files (``chrom<TAB>value`` per bin, as ``OutPut_PC_To_txt``
    and ``run_Compartment`` write them).

    Reference behaviour kept as it is: per chromosome the maternal PC is
    negated when ``np.corrcoef(M_PC, P_PC)[0][1] < 0``; candidates are the
    bins whose product is ``< 0``; the background is every maternal candidate
    minus every paternal candidate, of all chromosomes together; ``p =
    min(fwd, n - fwd) / n`` with ``fwd = bisect_left(BG, M_PC[i] - P_PC[i])``.

    ``BG`` itself (K_M x K_P sorted differences) is not kept: ``BackGround``
    stores its length ``n_BG`` and the candidate arrays ``M_candidate`` /
    ``P_candidate``, and ``fwd`` comes from one ``pairdiff_rank`` call over
    all candidates of all chromosomes -- the same integers.  Chromosomes go in
    the maternal file's order (the reference's Python 2 dict order is
    arbitrary); names are whole.
    """

    def __init__(self, Maternal_PC, Paternal_PC, Res):
        self.M_PC_file = Maternal_PC
        self.P_PC_file = Paternal_PC
        self.Res = Res
        self.stream = None

    def Loading_PC(self, fil):
        PC = {}
        with open(fil, "r") as f:
            for line in f:
                line = line.strip().split()
                if not line:
                    continue
                PC.setdefault(line[0], []).append(float(line[1]))
        return {k: np.array(v) for k, v in PC.items()}

    def _flipped(self, chro):
        M_PC = self.M_PC[chro]
        P_PC = self.P_PC[chro]
        if np.corrcoef(M_PC, P_PC)[0][1] < 0:
            M_PC = -M_PC
        return M_PC, P_PC

    def BackGround(self):
        """The candidates of the background (:460-485): ``M_candidate``,
        ``P_candidate`` and ``n_BG = len(BG)``; returns ``n_BG``."""
        M_candidate = []
        P_candidate = []
        for chro in self.M_PC.keys():
            M_PC, P_PC = self._flipped(chro)
            cand = M_PC * P_PC < 0
            M_candidate.append(M_PC[cand])
            P_candidate.append(P_PC[cand])
        self.M_candidate = np.concatenate(M_candidate) if M_candidate else np.zeros(0)
        self.P_candidate = np.concatenate(P_candidate) if P_candidate else np.zeros(0)
        self.n_BG = int(self.M_candidate.size) * int(self.P_candidate.size)
        return self.n_BG

    def Calculating(self):
        print("Loading PC1 values ...")
        self.M_PC = self.Loading_PC(self.M_PC_file)
        self.P_PC = self.Loading_PC(self.P_PC_file)
        n_BG = self.BackGround()
        rows = []
        for chro in self.M_PC.keys():
            print("chroms %s start" % chro)
            M_PC, P_PC = self._flipped(chro)
            for i in range(len(M_PC)):
                if M_PC[i] * P_PC[i] >= 0:
                    continue
                rows.append((chro, i * self.Res, M_PC[i], P_PC[i], M_PC[i] - P_PC[i]))
        diff = np.array([r[4] for r in rows], dtype=np.float64)
        fwd = pairdiff_rank(self.M_candidate, self.P_candidate, diff, stream=self.stream) if rows else []
        P_Value = [min(int(f), n_BG - int(f)) / n_BG for f in fwd]
        print("BH fdr processing ...")
        Q_value = _bh_by_value(np.asarray(P_Value, dtype=np.float64)) if rows else []
        dtype = np.dtype({"names": ["chr", "pos", "pc-m", "pc-p", "diff", "p_value", "Q_value"],
                          "formats": ["U64", np.int64, np.float64, np.float64, np.float64, np.float64, np.float64]})
        self.results = np.array([rows[i] + (P_Value[i], Q_value[i]) for i in range(len(rows))], dtype=dtype)

    def OutputTXT(self, outfil):
        print("Output ...")
        head = ["chr", "position", "PC-M", "PC-P", "diff", "P_Value", "Q_Value"]
        with open(outfil, "w") as out:
            out.writelines("\t".join(head) + "\n")
            for line in self.results:
                out.writelines("\t".join(map(_py2_str, line.tolist())) + "\n")

    def Running(self, Outfil):
        self.Calculating()
        self.OutputTXT(Outfil)


__all__ = ["LoopAllelicSpecificity", "BoundaryAllelicSpecificity", "CompartmentAllelicSpecificity",
           "pixel_windows", "pairdiff_rank"]
