"""Per-bin coverage and virtual 4C without a GPU (hichap_master_amd/coverage.py,
DESIGN.md §4v): the dense restatement (tests/coverage_ref.py) against
hand-written 6-bin examples, ``coverage_tracks``, the two text files written
and read back, and the Python-side argument checks."""
import numpy as np
import pytest

from hichap_master_amd import coverage as cov
from hichap_master_amd.StructureFind import py2_float_str
from tests import coverage_ref as ref

# Two chromosomes of 4 and 2 bins.  Upper-triangle pixels (bin1, bin2, count):
OFF = np.array([0, 4, 6], np.int64)
PIX = [(0, 0, 5.0), (0, 1, 2.0), (0, 3, 1.0), (0, 4, 7.0), (1, 1, 3.0), (1, 2, 4.0), (2, 3, 0.0), (2, 5, 6.0),
       (3, 3, 9.0), (4, 5, 8.0), (5, 5, 10.0)]
B1, B2, CNT = (np.array([p[k] for p in PIX], dtype=t) for k, t in ((0, np.int64), (1, np.int64), (2, np.float64)))


def _cov(ignore, near, weight=None, valid=None):
    valid = np.ones(6, bool) if valid is None else valid
    A, stored = ref.dense_A(B1, B2, CNT, weight, OFF, valid)
    return ref.coverage(A, stored, OFF, valid, ignore, near)


def test_restatement_on_a_hand_written_table():
    # no cell dropped, no near class: the diagonal enters its row ONCE (row 0: 5 + 2 + 1 cis, 7 trans)
    S, n = _cov(0, 0)
    assert S.tolist() == [[0, 8, 7], [0, 9, 0], [0, 4, 6], [0, 10, 0], [0, 8, 7], [0, 18, 6]]
    assert n.tolist() == [[0, 3, 1], [0, 3, 0], [0, 2, 1], [0, 3, 0], [0, 1, 1], [0, 2, 1]]    # the stored 0 counts
    # ignore_diags = 1 drops the diagonal alone; near_bins = 2 makes d = 1 near, d >= 2 far
    S, n = _cov(1, 2)
    assert S.tolist() == [[2, 1, 7], [6, 0, 0], [4, 0, 6], [0, 1, 0], [8, 0, 7], [8, 0, 6]]
    assert n.tolist() == [[1, 1, 1], [2, 0, 0], [2, 0, 1], [1, 1, 0], [1, 0, 1], [1, 0, 1]]
    # ignore_diags = 2 drops d = 0 and d = 1; trans is never dropped
    S, n = _cov(2, 3)
    assert S.tolist() == [[0, 1, 7], [0, 0, 0], [0, 0, 6], [0, 1, 0], [0, 0, 7], [0, 0, 6]]
    # near_bins <= ignore_diags simply leaves near empty
    for near in (0, 1, 2):
        S2, n2 = _cov(2, near)
        assert not S2[:, 0].any() and not n2[:, 0].any() and S2[:, 1:].tolist() == S[:, 1:].tolist()
    # near_bins beyond the chromosome: far is empty
    S, n = _cov(0, 200)
    assert not S[:, 1].any() and S[:, 0].tolist() == [8, 9, 4, 10, 8, 18]
    # the classes with the dropped cells partition the symmetric row sum
    A, _ = ref.dense_A(B1, B2, CNT, None, OFF, np.ones(6, bool))
    M = ref.class_masks(OFF, 2, 3)
    assert np.array_equal(sum(M[k].astype(int) for k in M), np.ones((6, 6), int))
    assert np.array_equal(A, A.T) and A[0, 0] == 5.0


def test_restatement_weights_validity_and_viewpoints():
    w = np.array([0.5, 2.0, np.nan, 1.0, 4.0, 0.25])
    valid = np.isfinite(w)
    S, n = _cov(0, 0, w, valid)
    # bin 2 is invalid: its row is 0 and it reaches no other row (rows 1, 3 and 5 lose its pixels)
    assert S.tolist() == [[0, 5 * 0.25 + 2 * 1.0 + 1 * 0.5, 7 * 2.0], [0, 2 * 1.0 + 3 * 4.0, 0], [0, 0, 0],
                          [0, 0.5 + 9.0, 0], [0, 8.0, 14.0], [0, 8.0 + 10 * 0.0625, 0]]
    assert n[2].tolist() == [0, 0, 0] and n[1].tolist() == [0, 2, 0]
    A, _ = ref.dense_A(B1, B2, CNT, None, OFF, np.ones(6, bool))
    # a one-bin viewpoint is the row; ignore_diags drops the cis cells next to the diagonal only
    assert ref.viewpoint(A, OFF, 0, 0, 1).tolist() == [5, 2, 0, 1, 7, 0]
    assert ref.viewpoint(A, OFF, 2, 0, 1).tolist() == [0, 0, 0, 1, 7, 0]
    assert ref.viewpoint(A, OFF, 1, 4, 6).tolist() == [7, 0, 6, 0, 8, 8]       # (4,4) none, (5,5) dropped, (4,5) twice
    t = ref.sym_tables(B1, B2, 6)
    assert t["rowptr_u"].tolist() == [0, 4, 6, 8, 9, 10, 11]
    assert t["rowptr_l"].tolist() == [0, 0, 1, 2, 4, 5, 7]
    assert t["partner_l"].tolist() == [0, 1, 0, 2, 0, 2, 4] and t["src_l"].tolist() == [1, 5, 2, 6, 3, 7, 9]


def test_coverage_tracks():
    S = np.array([[2.0, 6.0, 8.0],     # ICF 8 / 16, DLR log2 3
                  [0.0, 4.0, 4.0],     # near = 0: DLR NaN
                  [3.0, 0.0, 0.0],     # far = 0: DLR -inf, ICF 0
                  [0.0, 0.0, 0.0],     # nothing: both NaN
                  [1.0, 1.0, 2.0]])    # an invalid bin: both NaN
    valid = np.array([1, 1, 1, 1, 0], np.uint8)
    t = cov.coverage_tracks(S, valid)
    assert t["cov_cis"].tolist() == [8, 4, 3, 0, 2] and t["cov_tot"].tolist() == [16, 8, 3, 0, 4]
    assert t["ICF"][:3].tolist() == [0.5, 0.5, 0.0] and np.isnan(t["ICF"][3:]).all()
    assert t["DLR"][0] == np.log2(3.0) and np.isnan(t["DLR"][[1, 3, 4]]).all() and t["DLR"][2] == -np.inf
    want = ref.tracks(S, valid != 0)
    for k in want:
        assert np.array_equal(t[k], want[k], equal_nan=True), k
    assert cov.default_near_bins(40000) == 75 and cov.default_near_bins(1000000) == 3 and \
        cov.default_near_bins(7000000) == 1


def test_files_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    off = np.array([0, 4, 6, 9], np.int64)
    names, sel, res = ["a", "Pb", "c"], [0, 2], 5000
    valid = np.array([1, 1, 0, 1, 1, 1, 1, 0, 1], np.uint8)
    n = rng.integers(0, 50, (9, 3))
    S_raw = rng.integers(0, 90, (9, 3)).astype(np.float64)
    S = rng.uniform(0, 2, (9, 3))
    S[3] = 0.0
    fil = str(tmp_path / "cov.txt")
    cov.write_coverage(fil, names, off, sel, res, valid, n, S_raw, S)
    lines = open(fil).read().splitlines()
    assert lines[0].split("\t") == list(cov.COVERAGE_COLUMNS) and len(lines) == 1 + 4 + 3
    r = cov.read_coverage(fil)
    rows = [0, 1, 2, 3, 6, 7, 8]                                                   # chromosome Pb is not selected
    assert r["chrom"].tolist() == ["a"] * 4 + ["c"] * 3
    assert r["start"].tolist() == [0, 5000, 10000, 15000, 0, 5000, 10000] and np.array_equal(r["end"], r["start"] + res)
    assert np.array_equal(r["valid"], valid[rows]) and np.array_equal(r["n_cis"], (n[:, 0] + n[:, 1])[rows])
    assert np.array_equal(r["n_trans"], n[rows, 2])
    raw, bal = cov.coverage_tracks(S_raw, valid), cov.coverage_tracks(S, valid)
    for key, want in (("cov_cis_raw", raw["cov_cis"]), ("cov_tot_raw", raw["cov_tot"]), ("cov_cis", bal["cov_cis"]),
                      ("cov_tot", bal["cov_tot"]), ("ICF", bal["ICF"]), ("DLR", bal["DLR"])):
        assert np.array_equal(r[key], [float(py2_float_str(v)) for v in want[rows]], equal_nan=True), key
    assert np.isnan(r["ICF"][[2, 3, 5]]).all() and "\tnan\t" in lines[3]
    with pytest.raises(ValueError, match="not a coverage file"):
        cov.read_coverage(__file__)
    P = rng.uniform(0, 5, (2, 9))
    P[1, 8] = np.nan
    fil = str(tmp_path / "v4c.txt")
    cov.write_virtual4c(fil, names, off, sel, res, [("prom", "a", 5000, 15000), ("snp", "c", 0, 1)], P)
    chrom, start, end, views, Q = cov.read_virtual4c(fil)
    assert views == ["prom|a:5000-15000", "snp|c:0-1"] and chrom.tolist() == ["a"] * 4 + ["c"] * 3
    assert np.array_equal(end, start + res)
    assert np.array_equal(Q, [[float(py2_float_str(v)) for v in row[rows]] for row in P], equal_nan=True)


def test_viewpoint_bins_and_their_errors(tmp_path):
    names, off, res = ["Ma", "Mb", "Pa", "Pb"], np.array([0, 10, 14, 24, 28], np.int64), 1000
    v = cov.viewpoint_bins({"p": ("Mb", 1500, 2500), "q": ("Pa", 0, 10000)}, names, off, res)
    assert v == [("p", "Mb", 11, 13, 1500, 2500), ("q", "Pa", 14, 24, 0, 10000)]      # the bins that overlap
    # a bare name is the selected parent's copy; a full name stays what it is
    assert cov.viewpoint_bins({"p": ("b", 0, 1)}, names, off, res, "Paternal") == [("p", "Pb", 24, 25, 0, 1)]
    assert cov.viewpoint_bins({"p": ("Mb", 0, 1)}, names, off, res, "Paternal")[0][1:4] == ("Mb", 10, 11)
    fil = tmp_path / "views.txt"
    fil.write_text("# chrom start end name\nMa\t2000\t3000\tanchor\nMb\t0\t4000\n")
    assert cov.viewpoint_bins(str(fil), names, off, res) == [("anchor", "Ma", 2, 3, 2000, 3000),
                                                             ("Mb:0-4000", "Mb", 10, 14, 0, 4000)]
    with pytest.raises(ValueError, match="crosses the end"):
        cov.viewpoint_bins({"p": ("Mb", 3000, 4001)}, names, off, res)
    with pytest.raises(ValueError, match="unknown chromosome"):
        cov.viewpoint_bins({"p": ("chrZ", 0, 1000)}, names, off, res)
    with pytest.raises(ValueError, match="unknown chromosome"):
        cov.viewpoint_bins({"p": ("b", 0, 1000)}, names, off, res)                     # bare, but no parent chosen
    for start, end in ((2000, 2000), (3000, 2000), (-5, 10)):
        with pytest.raises(ValueError, match="start < end"):
            cov.viewpoint_bins({"p": ("Ma", start, end)}, names, off, res)
    fil.write_text("Ma\t5\n")
    with pytest.raises(ValueError, match="chrom start end"):
        cov.viewpoint_bins(str(fil), names, off, res)


def test_coverage_knob_in_the_one_table():
    """cov_rows in hh_tune's table: the documented default, a round trip, the rejection outside 1..16."""
    from hichap_master_amd import _lib
    from tests import knobs
    assert knobs.get("cov_rows") == 4
    with knobs.tuned(cov_rows=16):
        assert knobs.get("cov_rows") == 16
        for wrong in (0, 17, -1):
            with pytest.raises(_lib.HipLibraryError, match="cov_rows"):
                _lib.call("hh_tune", b"cov_rows", wrong)
        assert knobs.get("cov_rows") == 16
    assert knobs.get("cov_rows") == 4
