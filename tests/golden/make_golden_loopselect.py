#!/usr/bin/env python3
"""Golden vectors for loop selection and loop clustering from the REFERENCE's
own code (StructureFind.Loop_Selecting / LoopCluster, :2063-2243).

Run in the build container only (reads the reference checkout, absent on the
GPU box):

    python tests/golden/make_golden_loopselect.py

As in make_golden_loops.py, the Python-2 source TEXT of
HiCHap/StructureFind.py is converted with lib2to3 in memory and the methods
``Loop_Selecting``, ``center_sites``, ``distance``, ``peakcluster``,
``filter_initial``, ``filter_next`` and ``LoopCluster`` are executed on
``self.Matrix`` = a dict of small dense integer matrices, ``Res`` = 40000,
once for traditional data and once for ``Allelic = 'Maternal'``.  Nothing
converted is written to disk.

Two things Python 3 forces on the converted text, both stated here because
they touch what is executed:

* the ``'S4'`` dtypes become ``'U4'``: with bytes names ``'M' + outs[0]``
  (:2209) raises in Python 3;
* ``str`` resolves to a Python-2 ``str``: floats print as ``'%.12g'`` (with
  ``.0`` on integral values), NumPy integers and names as themselves -- the
  text Python 2 writes with ``'\\t'.join(map(str, lst))``.

The HICCUPS tables are synthetic (CallPeaks runs on the GPU): blobs of called
pixels around planted loops plus scattered single pixels, in CallPeaks' line
format.  The assertions at the end keep the fixture from being vacuous.
"""
from __future__ import annotations

import ast
import bisect
import math
import os
import sys
import tempfile
from itertools import islice

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/HiCHap"
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

from make_golden import _py3_source  # noqa: E402

METHODS = ["Loop_Selecting", "center_sites", "distance", "peakcluster", "filter_initial", "filter_next",
           "LoopCluster"]
RES = 40000
RATIO, STRENGTH, WEIGHT_Q = 0.6, 16, 1e-4
LINE_FORMAT = "%s\t%d\t%d\t%.4g\t%.4g\t%.4g\t%.4g\t%.4g\t%.4g\t%.4g\n"
HEAD = "\t".join(["chromLabel", "loc_1", "loc_2", "IF", "D-Enrichment", "D-pvalue", "D-qvalue",
                  "LL-Enrichment", "LL-pvalue", "LL-qvalue"]) + "\n"


def py2_str(v):
    """Python 2's ``str`` of the values LoopCluster prints."""
    if isinstance(v, bytes):
        return v.decode()
    if isinstance(v, (float, np.floating)):
        t = "%.12g" % float(v)
        return t + ".0" if t.lstrip("-").isdigit() else t
    if isinstance(v, (int, np.integer)):
        return "%d" % int(v)
    return "%s" % (v,)


def load_reference():
    for name, val in (("int", int), ("float", float), ("bool", bool)):
        if not hasattr(np, name):
            setattr(np, name, val)
    ns = {"np": np, "math": math, "os": os, "bisect": bisect, "islice": islice, "str": py2_str}
    text = _py3_source(os.path.join(REF, "StructureFind.py"))
    assert "'S4'" in text
    text = text.replace("'<S4'", "'<U4'").replace("'S4'", "'U4'")
    tree = ast.parse(text)
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "StructureFind"][0]
    meths = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in METHODS]
    assert {m.name for m in meths} == set(METHODS)
    klass = ast.ClassDef(name="RefSF", bases=[], keywords=[], body=meths, decorator_list=[])
    exec(compile(ast.fix_missing_locations(ast.Module(body=[klass], type_ignores=[])), "<StructureFind>", "exec"),
         ns)
    return ns["RefSF"]


def synth_chrom(rng, N, n_loops, A=220.0):
    """Raw symmetric int counts (power-law decay, planted loop blobs) and the
    called pixels: the blobs plus scattered single pixels."""
    i = np.arange(N)
    d = np.abs(i[:, None] - i[None, :])
    lam = A * (d + 1.0) ** -1.0 * rng.lognormal(0, 0.2, N)[:, None] * rng.lognormal(0, 0.2, N)[None, :]
    called = set()
    for k in range(n_loops):
        a = int(rng.integers(6, N - 45))
        b = a + int(rng.integers(8, 36))
        wide = 2 if k % 3 == 0 else 1           # 5 x 5 blobs need a second clustering round
        for da in range(-2, 3):
            for db in range(-2, 3):
                f = 10.0 if (da, db) == (0, 0) else (5.0 if max(abs(da), abs(db)) == 1 else 2.5)
                lam[a + da, b + db] *= f
                lam[b + db, a + da] *= f
                if max(abs(da), abs(db)) <= wide and rng.random() < 0.85:
                    called.add((a + da, b + db))
    H = rng.poisson(np.triu(lam))
    H = np.triu(H) + np.triu(H, 1).T
    for _ in range(3 * n_loops):               # single pixels, near and far
        a = int(rng.integers(0, N - 50))
        b = a + int(rng.integers(3, 48))
        if H[a, b] > 0:
            called.add((a, b))
    return H.astype(np.int64), sorted(called)


def table(rng, label, pixels, H, zero_q=False):
    lines = []
    for k, (a, b) in enumerate(pixels):
        q = 10.0 ** rng.uniform(-6.5, -1.4)
        if zero_q and k == len(pixels) // 2:
            q = 0.0
        lines.append(LINE_FORMAT % (label, a * RES, b * RES, H[a, b], rng.uniform(1.5, 6), q / 20, q / 2,
                                    rng.uniform(1.5, 6), q / 10, q))
    return lines


def dense_rank(H, a, b):
    diag = np.sort(H.diagonal(b - a))
    return bisect.bisect_left(list(diag), H[a][b]) / len(diag)


def peakcluster_noskip(sf, loop_sites, dis, chrom):
    """peakcluster with the member loop over a snapshot (no iterator skip)."""
    classes = []
    for i in chrom:
        c_loops = sorted(loop_sites[loop_sites["chr"] == i], key=lambda x: x[1])
        while True:
            c_class = [c_loops.pop(0)]
            center = sf.center_sites(c_class)
            for loop in list(c_loops):
                if sf.distance(center, loop) <= dis:
                    c_class.append(loop)
                    center = sf.center_sites(c_class)
                    c_loops.remove(loop)
            classes.append(c_class)
            if len(c_loops) == 0:
                break
    return classes


def class_key(classes):
    return [[(str(x[0]), int(x[1]), int(x[2])) for x in c] for c in classes]


def run_case(RefSF, rng, allelic, tmp):
    probe = {"rounds": 0, "first": None, "noskip": None, "final": None}

    class Probe(RefSF):
        def peakcluster(self, loop_sites, dis, chrom):
            out = RefSF.peakcluster(self, loop_sites, dis, chrom)
            if probe["first"] is None:
                probe["first"] = class_key(out)
                probe["noskip"] = class_key(peakcluster_noskip(self, loop_sites, dis, chrom))
            return out

        def filter_next(self, cls):
            probe["rounds"] += 1
            probe["final"] = RefSF.filter_next(self, cls)
            return probe["final"]

    sf = Probe()
    sf.Res, sf.ratio, sf.LoopStrength, sf.Allelic = RES, RATIO, STRENGTH, allelic
    names = ["1", "2"]
    sizes = [96, 80]
    prefix = "" if allelic is False else allelic[0]
    sf.Matrix = {}
    lines = [HEAD]
    for nm, N in zip(names, sizes):
        H, pixels = synth_chrom(rng, N, n_loops=7)
        sf.Matrix[prefix + nm] = H
        lines += table(rng, nm, pixels, H, zero_q=allelic is not False and nm == "1")
    raw = os.path.join(tmp, "g_Loops_40K.txt")
    with open(raw, "w") as f:
        f.writelines(lines)
    out = {"raw": "".join(lines)}
    rawfil = raw
    if allelic is False:
        sel = os.path.join(tmp, "Selected_g_Loops_40K.txt")
        sf.Loop_Selecting(raw, sel)
        out["selected"] = open(sel).read()
        kept = set(out["selected"].splitlines()[1:])
        by_ratio = by_strength = passed = 0
        for ln in lines[1:]:
            p = ln.split()
            H = sf.Matrix[p[0]]
            a, b = int(p[1]) // RES, int(p[2]) // RES
            low_rank, weak = dense_rank(H, a, b) < RATIO, H[a][b] < STRENGTH
            assert (ln.rstrip("\n") in kept) == (not (low_rank or weak))
            by_ratio += low_rank and not weak
            by_strength += weak and not low_rank
            passed += not (low_rank or weak)
        assert by_ratio >= 1 and by_strength >= 1 and passed >= 1, (by_ratio, by_strength, passed)
        print("  selection: %d by ratio alone, %d by strength alone, %d pass" % (by_ratio, by_strength, passed))
        rawfil = sel
    sf.LoopCluster(rawfil)
    out["cluster"] = open(sf.out_fil).read()

    first, noskip, final = probe["first"], probe["noskip"], probe["final"]
    assert max(len(c) for c in first) >= 3, "no class with three members"
    assert first != noskip, "the iterator skip does not change the clustering"
    assert probe["rounds"] >= 2, "the while loop ran once"
    q = np.array([x[3] / 10 ** x[4] for x in final])
    assert (q < WEIGHT_Q).any() and (q >= WEIGHT_Q).any(), "loops on one side of weight_q_value only"
    n_out = len(out["cluster"].splitlines()) - 1
    print("  clustering: %d loops -> %d classes -> %d final (%d rounds), %d below weight_q, %d written"
          % (sum(len(c) for c in first), len(first), len(final), probe["rounds"], int((q < WEIGHT_Q).sum()), n_out))
    if allelic is False:
        assert n_out == int((q < WEIGHT_Q).sum())
    else:
        assert 1 <= n_out < int((q < WEIGHT_Q).sum()), "the percentile filter drops or keeps nothing"
        assert any(x[3] == 0 for x in final if x[3] / 10 ** x[4] < WEIGHT_Q), "no w_q == 0"
        assert "\t1e-20\t" in out["cluster"]
    return sf.Matrix, out


def main():
    RefSF = load_reference()
    rng = np.random.default_rng(20240607)
    store = {"res": np.int64(RES), "ratio": np.float64(RATIO), "strength": np.int64(STRENGTH),
             "weight_q": np.float64(WEIGHT_Q)}
    with tempfile.TemporaryDirectory() as tmp:
        for case, allelic in (("trad", False), ("maternal", "Maternal")):
            print(case)
            mats, texts = run_case(RefSF, rng, allelic, os.path.join(tmp))
            for nm, H in mats.items():
                assert H.max() < 32767
                store[f"{case}/M/{nm}"] = H.astype(np.int16)
            for k, t in texts.items():
                store[f"{case}/{k}"] = np.frombuffer(t.encode(), dtype=np.uint8)
    path = os.path.join(HERE, "loopselect_40k.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 100 * 1024


if __name__ == "__main__":
    main()
