#!/usr/bin/env python3
"""Golden tables for allele-specific loops, boundaries and compartments from
the REFERENCE's own code (HiCHap/AllelicSpecificity.py, its three classes).

Run in the build container only (reads the reference checkout, absent on the
GPU box):

    python tests/golden/make_golden_allelic.py

As in make_golden_loopselect.py, the Python-2 source TEXT of the module is
converted with lib2to3 in memory and its three classes are executed; nothing
converted is written to disk.  What Python 3 forces on the converted text:

* the ``'S4'`` / ``'S8'`` dtypes become ``'U4'`` / ``'U8'`` (``'M' + chro``
  raises with bytes names);
* ``str`` resolves to a Python-2 ``str`` (floats as ``'%.12g'``, ``.0`` on
  integral values).

Injected: a stub ``cooler`` whose ``Cooler(uri).matrix(balance=False)
.fetch(name)`` serves the fixture's dense matrices, ``multipletests`` as
restated in make_golden_loops.py, SciPy's ``stats`` / ``ttest_rel``.

Data: chromosomes '1' (96 bins) and '2' (80 bins), maternal and paternal,
symmetric with power-law decay, counts that are multiples of 1/64 (stored as
the integer numerators of the upper triangle), a gap region in both
haplotypes of '1' and one in the paternal '2' only, planted allele-specific
loops and boundaries.

In the two boundary branches where the reference appends stale values (:376,
:383) only its p (and the q computed from the p-values) is kept: the three
stale fields are stored as ``STALE``.  ``boundary_edge_file`` (boundaries
near the chromosome ends) is not run through the reference.

The first 'NA' cause of ``calculate_single_stat`` (an empty side) cannot
occur through ``Running``: ``BackGround`` has dropped every loop with
``M_IF == 0`` or ``P_IF == 0`` by then.  All four branches are therefore also
recorded from direct calls (``stat_in`` -> ``stat_out``, NaN for 'NA'); the
other three are asserted on the table.
"""
from __future__ import annotations

import ast
import bisect
import math
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/HiCHap"
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

from make_golden import _py3_source  # noqa: E402
from make_golden_loops import multipletests  # noqa: E402
from make_golden_loopselect import py2_str  # noqa: E402

RES = 40000
OFFSET = 10
SIZES = {"1": 96, "2": 80}
GAPS = {"M1": range(40, 48), "P1": range(40, 48), "P2": range(30, 38)}
CLASSES = ["LoopAllelicSpecificity", "BoundaryAllelicSpecificity", "CompartmentAllelicSpecificity"]

# (chrom, maternal bin, paternal bin); an equal-position boundary comes first
BOUNDARIES = [("1", 20, 20), ("1", 42, 42), ("1", 20, 22), ("1", 60, 62), ("1", 70, 68), ("1", 25, 30),
              ("1", 80, 76), ("1", 30, 42), ("1", 43, 55), ("1", 42, 44), ("1", 66, 66),
              ("2", 15, 15), ("2", 32, 32), ("2", 50, 52), ("2", 58, 55), ("2", 20, 33), ("2", 33, 60),
              ("2", 64, 64)]
# near the chromosome ends (deviation 2), with boundaries that fit between them
EDGE_BOUNDARIES = [("1", 20, 20), ("1", 5, 5), ("1", 60, 62), ("1", 20, 90), ("2", 75, 75), ("2", 9, 15),
                   ("2", 50, 52), ("1", 86, 86), ("1", 10, 10)]
PLANTED_BOUNDARIES = {"M1": [60, 25], "P1": [68, 80], "M2": [50], "P2": [55]}


def load_reference(mats, log):
    from scipy import stats
    from scipy.stats import ttest_rel
    for name, val in (("int", int), ("float", float), ("bool", bool)):
        if not hasattr(np, name):
            setattr(np, name, val)

    class StubCooler:
        def __init__(self, uri):
            self.uri = uri

        def matrix(self, balance=True):
            assert balance is False
            return self

        def fetch(self, name):
            return mats[name].copy()

    ns = {"np": np, "os": os, "math": math, "bisect": bisect, "cooler": types.SimpleNamespace(Cooler=StubCooler),
          "stats": stats, "ttest_rel": ttest_rel, "multipletests": multipletests, "str": py2_str,
          "print": lambda *a: log.append(" ".join(map(py2_str, a)))}
    text = _py3_source(os.path.join(REF, "AllelicSpecificity.py"))
    assert "'S4'" in text and "'S8'" in text
    text = text.replace("'S4'", "'U4'").replace("'S8'", "'U8'")
    tree = ast.parse(text)
    classes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in CLASSES]
    assert [c.name for c in classes] == CLASSES
    exec(compile(ast.fix_missing_locations(ast.Module(body=classes, type_ignores=[])), "<AllelicSpecificity>",
                 "exec"), ns)
    return ns


def synth(rng):
    """{'M1': dense float64, ...}: per chromosome one shared expectation, the
    planted differences, independent Poisson draws, numerators of 1/64."""
    mats, numer = {}, {}
    for chro, N in SIZES.items():
        i = np.arange(N)
        d = np.abs(i[:, None] - i[None, :])
        vis = rng.lognormal(0, 0.15, N)
        lam = 150.0 * (d + 1.0) ** -1.0 * vis[:, None] * vis[None, :]
        for hap in "MP":
            L = lam.copy()
            for b in PLANTED_BOUNDARIES.get(hap + chro, []):
                L[b - OFFSET:b, b:b + OFFSET] *= 0.35
                L[b:b + OFFSET, b - OFFSET:b] *= 0.35
            base = rng.poisson(np.triu(L)).astype(np.int64)
            jitter = rng.integers(-31, 32, size=base.shape)
            num = np.triu(np.where(base > 0, base * 64 + jitter, 0))
            for g in GAPS.get(hap + chro, []):
                num[g, :] = 0
                num[:, g] = 0
            numer[hap + chro] = num
    return numer


def plant_loops(rng, numer):
    """Loop lines (chrom, M bins, P bins) and the cells changed for them."""
    loops = []
    for chro, N in SIZES.items():
        for k in range(42):
            a = int(rng.integers(0, N - 42))
            dd = int(rng.integers(1, 41)) if k >= 10 else 1 + k % 5
            b = a + dd
            pa, pb = (a, b) if k % 9 else (a + 1, b + 1)       # a few paternal loops one bin off
            f = (1.0, 1.0)
            if k % 7 == 3:
                f = (3.0, 1.0)
            elif k % 7 == 5:
                f = (1.0, 3.0)
            for hap, (r, c), ff in (("M", (a, b), f[0]), ("P", (pa, pb), f[1])):
                numer[hap + chro][r, c] = int(numer[hap + chro][r, c] * ff)
            loops.append((chro, a, b, pa, pb))
    # the zero filters: a maternal-only and a paternal-only loop
    numer["M1"][3, 9] = 0
    numer["P1"][3, 9] = 777
    loops.append(("1", 3, 9, 3, 9))
    numer["P2"][5, 12] = 0
    numer["M2"][5, 12] = 555
    loops.append(("2", 5, 12, 5, 12))
    loops.append(("1", 41, 60, 41, 60))                          # both zero: in the gap
    return loops


def dense(num):
    H = num.astype(np.float64) / 64.0
    return np.triu(H) + np.triu(H, 1).T


def pc_files(rng):
    m_lines, p_lines = [], []
    flips = {}
    for chro, N in SIZES.items():
        x = np.arange(N)
        base = 0.06 * np.sin(2 * np.pi * x / 31.0 + (0.4 if chro == "1" else 1.7))
        M = np.round(base + rng.normal(0, 0.02, N), 2)
        P = np.round(base + rng.normal(0, 0.02, N), 2)
        if chro == "2":
            M = -M                                               # needs the sign flip
        flips[chro] = bool(np.corrcoef(M, P)[0][1] < 0)
        m_lines += ["%s\t%s\n" % (chro, py2_str(float(v))) for v in M]
        p_lines += ["%s\t%s\n" % (chro, py2_str(float(v))) for v in P]
    assert flips == {"1": False, "2": True}, flips
    return "".join(m_lines), "".join(p_lines)


def boundary_text(items, rng):
    return "".join("%s\t%d\t%d\n" % (c, m * RES + int(rng.integers(0, RES)), p * RES + int(rng.integers(0, RES)))
                   for c, m, p in items)


def classify_boundaries(ref, mats):
    """Which branch of Calculating each boundary takes, by the reference's
    own SampleGenerate / removeGap on the same matrices."""
    out = []
    z = {h: {c: mats[h + c] - np.diag(mats[h + c].diagonal()) for c in SIZES} for h in "MP"}

    def valid(S):
        return not (S == 0).sum() / len(S) >= 0.85

    for chro, m, p in BOUNDARIES:
        S = {(h, b): ref.SampleGenerate(z[h][chro], b) for h in "MP" for b in (m, p)}
        pairs = []
        if m == p:
            ok = valid(S["M", m]) and valid(S["P", m])
            kind = "equal_tested" if ok else "equal_skipped"
            if ok:
                pairs.append((S["M", m], S["P", m]))
        else:
            v1 = valid(S["M", m]) and valid(S["P", m])
            v2 = valid(S["M", p]) and valid(S["P", p])
            kind = {(True, True): "both", (True, False): "first_only", (False, True): "second_only",
                    (False, False): "neither"}[v1, v2]
            if v1:
                pairs.append((S["M", m], S["P", m]))
            if v2:
                pairs.append((S["M", p], S["P", p]))
        for a, b in pairs:
            assert len(ref.removeGap(a, b)[0]) >= 2
        out.append(kind)
    return out


def main():
    rng = np.random.default_rng(20240911)
    numer = synth(rng)
    loops = plant_loops(rng, numer)
    mats = {k: dense(v) for k, v in numer.items()}
    log = []
    ns = load_reference(mats, log)
    store = {"res": np.int64(RES), "offset": np.int64(OFFSET),
             "chroms": np.array(list(SIZES)), "sizes": np.array(list(SIZES.values()), dtype=np.int64)}
    for k, num in numer.items():
        assert num.max() < 2 ** 31 and np.array_equal(dense(num), mats[k])
        store["numer/" + k] = num[np.triu_indices(num.shape[0])].astype(np.int32)

    def text(s):
        return np.frombuffer(s.encode(), dtype=np.uint8)

    with tempfile.TemporaryDirectory() as tmp:
        # ---------------------------------------------------------- loops
        loop_fil = os.path.join(tmp, "g_Loops_40K.txt")
        loop_text = "".join("%s\t%d\t%d\t%d\t%d\n" % (c, a * RES, b * RES + 17, pa * RES + 5, pb * RES)
                            for c, a, b, pa, pb in loops)
        with open(loop_fil, "w") as f:
            f.write(loop_text)
        L = ns["LoopAllelicSpecificity"]("stub.cool", loop_fil, RES)
        L.DataSetBuilding()
        raw = L.Data.copy()
        L.Running()
        table = open(L.outfile).read()
        half = (raw["M_IF"] + raw["P_IF"]) / 2
        vmax = 0.95 * (L.Mean.size - 1)
        by_vmax = int(((half > vmax) & (raw["M_IF"] != 0) & (raw["P_IF"] != 0)).sum())
        by_m0 = int(((raw["M_IF"] == 0) & (raw["P_IF"] != 0)).sum())
        by_p0 = int(((raw["P_IF"] == 0) & (raw["M_IF"] != 0)).sum())
        both0 = int(((raw["P_IF"] == 0) & (raw["M_IF"] == 0)).sum())
        assert by_vmax >= 1 and by_m0 >= 1 and by_p0 >= 1 and both0 >= 1, (by_vmax, by_m0, by_p0, both0)
        assert np.any(raw["M_IF"] != np.floor(raw["M_IF"])), "integer counts only"
        nobs = L.Data["M_IF"] + L.Data["P_IF"]
        small = (L.p * nobs < 5) | ((1 - L.p) * nobs < 5)
        plain = (L.p * nobs >= 30) & ((1 - L.p) * nobs >= 30)
        n_na = sum(ln.split("\t")[9] == "NA" for ln in table.splitlines()[1:])
        assert n_na == int(small.sum()) >= 1 and plain.sum() >= 1 and (~small & ~plain).sum() >= 1
        print("loops: %d lines, %d over vmax, %d/%d/%d zero (M/P/both), kept %d: %d NA, %d corrected z, %d plain z"
              % (raw.size, by_vmax, by_m0, by_p0, both0, L.Data.size, n_na, int((~small & ~plain).sum()),
                 int(plain.sum())))
        cases = [(0.5, 0.0, 40.0), (0.5, 40.0, 40.0), (0.5, 3.0, 8.0), (0.97, 60.0, 100.0), (0.5, 41.5, 70.25),
                 (0.5, 12.0, 31.5), (0.45, 20.0, 64.0), (0.52, 100.25, 150.0)]
        got = [L.calculate_single_stat(*c) for c in cases]
        assert [g == "NA" for g in got] == [True, True, True, True, False, False, False, False]
        store["stat_in"] = np.array(cases, dtype=np.float64)
        store["stat_out"] = np.array([np.nan if g == "NA" else g for g in got], dtype=np.float64)
        store["loop_file"], store["loop_table"] = text(loop_text), text(table)

        # ------------------------------------------------------ boundaries
        b_fil = os.path.join(tmp, "boundaries.txt")
        b_text = boundary_text(BOUNDARIES, rng)
        with open(b_fil, "w") as f:
            f.write(b_text)
        B = ns["BoundaryAllelicSpecificity"]("stub.cool", b_fil, RES)
        kinds = classify_boundaries(B, mats)
        assert kinds[0] == "equal_tested"
        assert set(kinds) == {"equal_tested", "equal_skipped", "both", "first_only", "second_only", "neither"}, kinds
        log.clear()
        out_b = os.path.join(tmp, "boundary_as.txt")
        B.Running(out_b)
        written = [k for k in kinds if k not in ("equal_skipped", "neither")]
        assert sum("skip" in ln for ln in log) == len(kinds) - len(written)
        lines = open(out_b).read().splitlines()
        assert len(lines) == 1 + len(written)
        assert np.all(np.isfinite(B.results["p_value"])) and np.all(np.isfinite(B.results["q_value"]))
        # both-valid lines: p1 < p2 once, and once not (the second pair's statistic is written)
        first = second = 0
        zz = {h: {c: mats[h + c] - np.diag(mats[h + c].diagonal()) for c in SIZES} for h in "MP"}
        from scipy.stats import ttest_rel
        for (chro, m, p), kind in zip(BOUNDARIES, kinds):
            if kind == "both":
                p1 = ttest_rel(*B.removeGap(B.SampleGenerate(zz["M"][chro], m), B.SampleGenerate(zz["P"][chro], m)))[1]
                p2 = ttest_rel(*B.removeGap(B.SampleGenerate(zz["M"][chro], p), B.SampleGenerate(zz["P"][chro], p)))[1]
                first += p1 < p2
                second += not p1 < p2
        assert first >= 1 and second >= 1, (first, second)
        for k, kind in enumerate(written):
            if kind in ("first_only", "second_only"):
                f = lines[1 + k].split("\t")
                f[3:6] = ["STALE"] * 3
                lines[1 + k] = "\t".join(f)
        print("boundaries: %s; both-valid %d first / %d second" % ({k: kinds.count(k) for k in sorted(set(kinds))},
                                                                  first, second))
        store["boundary_file"] = text(b_text)
        store["boundary_kinds"] = np.array(kinds)
        store["boundary_table"] = text("\n".join(lines) + "\n")
        store["boundary_edge_file"] = text(boundary_text(EDGE_BOUNDARIES, rng))

        # ---------------------------------------------------- compartments
        pc_m, pc_p = pc_files(rng)
        fm, fp = os.path.join(tmp, "M_PC.txt"), os.path.join(tmp, "P_PC.txt")
        open(fm, "w").write(pc_m)
        open(fp, "w").write(pc_p)
        Cm = ns["CompartmentAllelicSpecificity"](fm, fp, RES)
        out_c = os.path.join(tmp, "compartment_as.txt")
        Cm.Running(out_c)
        assert list(Cm.M_PC.keys()) == list(SIZES)
        n = Cm.results.size
        assert n >= 12 and len(Cm.BG) >= n * n and len(set(Cm.BG)) < len(Cm.BG)
        assert len(set(Cm.results["pc-m"].tolist())) < n, "no tied candidate values"
        assert set(Cm.results["chr"].tolist()) == set(SIZES)
        print("compartments: %d candidates, %d background differences, %d distinct" % (n, len(Cm.BG),
                                                                                      len(set(Cm.BG))))
        store["pc_m"], store["pc_p"] = text(pc_m), text(pc_p)
        store["compartment_table"] = text(open(out_c).read())

    path = os.path.join(HERE, "allelic_40k.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 100 * 1024


if __name__ == "__main__":
    main()
