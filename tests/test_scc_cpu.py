"""The host side of the reproducibility score (hichap_master_amd.reproducibility,
DESIGN.md §4q) and its dense restatement (tests/scc_ref.py): no GPU is needed."""
import math
import os

import numpy as np
import pytest

from hichap_master_amd import _lib, coolio, h5
from hichap_master_amd import reproducibility as rp
from hichap_master_amd.StructureFind import StructureFind, py2_float_str
from tests import knobs
from tests import scc_ref as ref

RES = 10000


# ------------------------------------------------------- the restatement itself
def test_restatement_on_a_hand_computed_pair():
    """N = 6, h = 1, ignore_diags = 1, bin 3 invalid (valid = 1 1 1 0 1 1, so nv =
    2 3 2 2 2 2).  A holds x(0,1) = 2, x(0,2) = 6, x(1,2) = 4, x(0,5) = 3, x(4,5)
    = 8, B y(0,1) = 1, y(1,2) = 3, y(4,5) = 2; the diagonal pixels and those at
    bin 3 must not count.  By hand:
      d = 1  (0,1): SX = 2+6+2+4 = 14 (window clipped at row -1), SY = 1+1+3 = 5,
                    nv nv = 6;  (1,2): SX = 2+6+4+4 = 16, SY = 1+3+3 = 7, 6;
             (4,5): SX = 8+8 = 16 (clipped at column 6), SY = 4, 4;
             (2,3), (3,4) have an invalid bin.
      d = 2  (0,2): SX = 2+6+4 = 12, SY = 1+3 = 4, 4;  (2,4): SX = SY = 0, dropped.
      d = 3  (1,4): SX = 3, SY = 0, 6;  (2,5): both 0, dropped;  (0,3) invalid.
      d = 4  (0,4): SX = 3, 4;  (1,5): SX = 3, 6.      d = 5  (0,5): SX = 3, 4."""
    A = (np.array([0, 0, 0, 0, 1, 2, 3, 3, 4]), np.array([0, 1, 2, 5, 2, 3, 3, 4, 5]),
         np.array([1.0, 2, 6, 3, 4, 5, 9, 7, 8]))
    B = (np.array([0, 1, 3, 4]), np.array([1, 2, 5, 5]), np.array([1.0, 3, 11, 2]))
    bad = [0, 0, 0, 1, 0, 0]
    valid = ref.validity(None, 0, 6, bad)
    assert valid == [True, True, True, False, True, True]
    strata = ref.smoothed(ref.dense(*A, None, 0, 6), ref.dense(*B, None, 0, 6), valid, 1, 1, 5)
    want = [([], []),
            ([14 / 6, 16 / 6, 16 / 4], [5 / 6, 7 / 6, 4 / 4]),
            ([12 / 4], [4 / 4]),
            ([3 / 6], [0.0]),
            ([3 / 4, 3 / 6], [0.0, 0.0]),
            ([3 / 4], [0.0])]
    assert strata == want
    n, S, T = ref.moments(strata)
    assert n.tolist() == [0, 3, 1, 1, 2, 1]
    np.testing.assert_allclose(S[:, 1], [9.0, 3.0, 49 / 9 + 64 / 9 + 16, 25 / 36 + 49 / 36 + 1,
                                         35 / 18 + 56 / 18 + 4], rtol=4e-16)
    assert S[:, 4].tolist() == [1.25, 0.0, 0.8125, 0.0, 0.0] and np.array_equal(S, T)
    rho, weight, usable, cond = ref.correlations(strata)
    assert usable.tolist() == [False, True, False, False, False, False] and weight[1] == 4 / 12
    X, Y = np.array(want[1][0]), np.array(want[1][1])
    assert abs(rho[1] - np.corrcoef(X, Y)[0, 1]) < 1e-15
    # the package's host rules on the same moments
    r = rp.scc_from_moments(n, S)
    assert r["usable"].tolist() == usable.tolist() and abs(r["rho"][1] - rho[1]) < 1e-13
    assert abs(r["scc"] - rho[1]) < 1e-13 and abs(ref.scc([rho], [weight], [usable]) - rho[1]) < 1e-15
    # a weighted table: (count * w[bin1]) * w[bin2], a NaN weight makes the bin invalid
    w = np.array([7.0, 0.5, 2.0, 1.0, np.nan, 1.0, 4.0, 1.0])       # global bins; the chromosome is [1, 7)
    M = ref.dense(A[0] + 1, A[1] + 1, A[2], w, 1, 6)
    assert M[0][1] == M[1][0] == 2 * 0.5 * 2.0 and M[0][2] == 6 * 0.5 and M[2][3] == 0.0 and M[4][5] == 32.0
    assert ref.validity(w, 1, 6, None) == valid


# ----------------------------------------------------------- scc_from_moments
def _moments_of(X, Y):
    X, Y = np.asarray(X, float), np.asarray(Y, float)
    return len(X), [X.sum(), Y.sum(), (X * X).sum(), (Y * Y).sum(), (X * Y).sum()]


def test_scc_from_moments_rules():
    cases = [([1, 2, 3, 4.0], [2, 4, 6, 9.0]),           # usable
             ([1, 2.0], [3, 5.0]),                       # n = 2: not usable
             ([1, 2, 3.0], [5, 5, 5.0]),                 # zero variance of Y: not usable
             ([1, 2, 3, 4, 5.0], [5, 3, 4, 1, 2.0]),     # usable, negative
             ([], [])]
    n = np.array([_moments_of(*c)[0] for c in cases])
    S = np.array([_moments_of(*c)[1] for c in cases]).T
    r = rp.scc_from_moments(n, S)
    assert r["usable"].tolist() == [True, False, False, True, False]
    assert r["weight"].tolist() == [5 / 12, 0.0, 0.0, 6 / 12, 0.0]
    rho0, rho3 = np.corrcoef(*cases[0])[0, 1], np.corrcoef(*cases[3])[0, 1]
    np.testing.assert_allclose(r["rho"][[0, 3]], [rho0, rho3], rtol=1e-13)
    assert np.isnan(r["rho"][[1, 2, 4]]).all()
    assert abs(r["scc"] - (5 * rho0 + 6 * rho3) / 11) < 1e-13
    # no usable stratum
    none = rp.scc_from_moments(n[[1, 2, 4]], S[:, [1, 2, 4]])
    assert math.isnan(none["scc"]) and not none["usable"].any()
    assert math.isnan(rp.scc_from_moments(np.zeros(0, np.int64), np.zeros((5, 0)))["scc"])
    # the genome pools the usable strata of all chromosomes in the same formula
    chroms = {"a": dict(n=n[:3], S=S[:, :3]), "b": dict(n=n[3:], S=S[:, 3:])}
    pooled = rp.pooled_scc(chroms)
    assert pooled["scc"] == r["scc"] and pooled["usable"].tolist() == r["usable"].tolist()
    assert math.isnan(rp.pooled_scc({})["scc"])


def test_default_h():
    assert [rp.default_h(r) for r in (1000, 5000, 10000, 20000, 40000, 100000, 200000, 500000, 1000000)] == \
        [20, 20, 20, 10, 5, 2, 1, 0, 0]
    assert rp.MAX_H == 20


# --------------------------------------------------------------------- files
def test_file_format(tmp_path):
    n = np.array([0, 7, 2])
    res = {"Mchr1": dict(h=3, max_dist=2, n=n, rho=np.array([np.nan, 0.5, np.nan]),
                         weight=np.array([0.0, 8 / 12, 0.0]), usable=np.array([False, True, False]), scc=0.5),
           "Mchr2": dict(h=3, max_dist=1, n=n[:2], rho=np.array([np.nan, -0.25]), weight=np.array([0.0, 1.0]),
                         usable=np.array([False, True]), scc=-0.25)}
    genome = dict(usable=np.array([False, True, False, False, True]), scc=0.05)
    a, b = str(tmp_path / "scc.txt"), str(tmp_path / "strata.txt")
    rp.write_scc(a, b, res, RES, genome, name=lambda chro: chro[1:])
    assert open(a).read().splitlines() == [
        "chrom\th\tmax_dist_bins\tn_usable\tscc", "chr1\t3\t2\t1\t0.5", "chr2\t3\t1\t1\t-0.25",
        "genome\t3\t2\t2\t0.05"]
    assert open(b).read().splitlines() == [
        "chrom\tdist_bins\tdist_bp\tn\trho\tweight",
        "chr1\t0\t0\t0\tnan\t0.0", f"chr1\t1\t10000\t7\t0.5\t{py2_float_str(8 / 12)}", "chr1\t2\t20000\t2\tnan\t0.0",
        "chr2\t0\t0\t0\tnan\t0.0", "chr2\t1\t10000\t7\t-0.25\t1.0"]


# ------------------------------------------------------------- ValueErrors
def _cooler(path, sizes, weight=False):
    nb = sum(-(-s // RES) for _, s in sizes)
    b = np.arange(nb, dtype=np.int64)
    coolio.create_cooler(path, {RES: (sizes, b, b, np.ones(nb, np.int32))})
    if weight:
        h5.append_dataset(path, f"{RES}/bins", "weight", np.ones(nb))
    return path


def test_run_reproducibility_value_errors(tmp_path):
    sizes = [("chr1", 50 * RES), ("chr2", 30 * RES)]
    mine = _cooler(str(tmp_path / "a.cool"), sizes, weight=True)
    out = str(tmp_path / "out")
    sf = StructureFind(mine, Res=RES)
    with pytest.raises(ValueError, match="chr2 has 300000 bp in one cooler and 310000"):
        sf.run_Reproducibility(out, other=_cooler(str(tmp_path / "b.cool"), [sizes[0], ("chr2", 31 * RES)], True))
    with pytest.raises(ValueError, match="chromosome 1 is chr2 in one cooler and chrX"):
        sf.run_Reproducibility(out, other=_cooler(str(tmp_path / "c.cool"), [sizes[0], ("chrX", 30 * RES)], True))
    with pytest.raises(ValueError, match="2 chromosomes in one cooler and 1 in the other"):
        sf.run_Reproducibility(out, other=_cooler(str(tmp_path / "d.cool"), sizes[:1], True))
    with pytest.raises(ValueError, match="run_Reproducibility: the cooler has no bins/weight"):   # an unbalanced other
        sf.run_Reproducibility(out, other=_cooler(str(tmp_path / "e.cool"), sizes))
    with pytest.raises(ValueError, match="needs other="):
        sf.run_Reproducibility(out)
    for h in (-1, rp.MAX_H + 1):
        with pytest.raises(ValueError, match="h must be 0..20"):
            sf.run_Reproducibility(out, other=mine, h=h)
    with pytest.raises(ValueError, match="ignore_diags"):
        sf.run_Reproducibility(out, other=mine, ignore_diags=-1)
    with pytest.raises(ValueError, match="Only Maternal, Paternal, False allowed"):
        StructureFind(mine, Res=RES, Allelic="Both").run_Reproducibility(out, other=mine)
    # haplotype data: a chromosome without its other copy, and copies of different lengths
    hap = _cooler(str(tmp_path / "h.cool"), [("Mchr1", 50 * RES), ("Pchr1", 50 * RES), ("Mchr2", 30 * RES)])
    with pytest.raises(ValueError, match="Mchr2 has no copy of the other haplotype"):
        StructureFind(hap, Res=RES, Allelic="Maternal").run_Reproducibility(out, max_dist=0, h=0, ignore_diags=9)
    hap = _cooler(str(tmp_path / "i.cool"), [("Pchr1", 50 * RES), ("Mchr1", 49 * RES)])
    with pytest.raises(ValueError, match="Pchr1 has 50 bins, Mchr1 49"):
        StructureFind(hap, Res=RES, Allelic="Paternal").run_Reproducibility(out)
    assert not os.path.exists(out)


# ---------------------------------------------------------------- the knob
@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libhichap_hip.so is not built")
def test_scc_rows_roundtrip_and_rejection():
    """hh_tune "scc_rows" as tests/test_tune_cpu.py holds every key: the default
    (0: from h), a legal value, illegal values rejected with the key named."""
    if "scc_rows" not in os.environ.get("HH_TUNE", ""):
        assert knobs.get("scc_rows") == 0
    before = knobs.get("scc_rows")
    with knobs.tuned(scc_rows=8):
        assert knobs.get("scc_rows") == 8
        for illegal in (36, 6, -4):
            with pytest.raises(_lib.HipLibraryError) as e:
                _lib.call("hh_tune", b"scc_rows", illegal)
            assert e.value.code == -1 and "scc_rows" in str(e.value)
        assert knobs.get("scc_rows") == 8
    assert knobs.get("scc_rows") == before
