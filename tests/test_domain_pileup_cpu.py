"""The domain pileup's dense restatement (tests/domain_pileup_ref.py) against
the pileup's restatement, a hand-computed example and closed forms, and the
host functions of ``hichap_master_amd.domain_pileup``: no GPU
is needed."""
import math

import numpy as np
import pytest

from hichap_master_amd import domain_pileup as dp
from hichap_master_amd.StructureFind import StructureFind, py2_float_str
from tests import domain_pileup_data as data
from tests import domain_pileup_ref as ref
from tests import pileup_ref

N = data.N


def test_overlaps_by_hand():
    # L = 3 bins on R = 2 cells, one cell of flank: cells of 1.5 bins, in halves of a bin
    got = ref.overlaps(4, 3, 2, 1, 10)
    assert got == [[(2, 1), (3, 2)], [(4, 2), (5, 1)], [(5, 1), (6, 2)], [(7, 2), (8, 1)]]
    # L = 1 bin on R = 3 cells: three cells inside bin 5, the flank in bins 4 and 6
    assert ref.overlaps(5, 1, 3, 3, 10) == [[(4, 1)]] * 3 + [[(5, 1)]] * 3 + [[(6, 1)]] * 3
    # the flank leaves the chromosome on both sides: its bins are not listed
    assert ref.overlaps(0, 4, 2, 1, 4) == [[], [(0, 2), (1, 2)], [(2, 2), (3, 2)], []]
    for s, L, R, P in ((1000, 300, 63, 32), (17, 5, 8, 4), (290, 10, 7, 3), (3, 120, 5, 0)):
        o = ref.overlaps(s, L, R, P, 10 ** 9)                         # (nothing is clipped)
        assert len(o) == R + 2 * P and all(sum(x for _, x in c) == L for c in o)   # a cell is L / R bins long
        assert o[P][0][0] == s and o[P + R - 1][-1][0] == s + L - 1   # the body is the domain


def test_restatement_by_hand():
    """One domain [1, 3) of a 4-bin chromosome on R = 1, P = 1: cells of two
    bins; bins -1 and 4 do not exist."""
    a, b = np.indices((4, 4))
    M = (10.0 * np.minimum(a, b) + np.maximum(a, b) + 1.0)             # M[a][b] = 10 a + b + 1
    valid = np.ones(4, bool)
    S, Wn, m = ref.domain_pileup_sums(M, valid, [1], [3], 1, 1, None, 0, 64)
    # body: (1,1) + 2 (1,2) + (2,2) over 4; left flank: bin 0 only; right: bin 3 only
    assert S[1, 1] == (12.0 + 2 * 13.0 + 23.0) / 4 and Wn[1, 1] == 1.0 and m[1, 1] == 3
    assert S[0, 0] == 1.0 / 4 and Wn[0, 0] == 0.25 and S[2, 2] == 34.0 / 4 and Wn[2, 2] == 0.25
    assert S[0, 1] == (2.0 + 3.0) / 4 and Wn[0, 1] == 0.5 and S[1, 2] == (14.0 + 24.0) / 4 and S[0, 2] == 4.0 / 4
    assert np.array_equal(S, S.T) and np.array_equal(Wn, Wn.T) and np.array_equal(m, m.T)
    S, Wn, m = ref.domain_pileup_sums(M, valid, [1], [3], 1, 1, [2.0, math.nan], 0, 64)   # d = 1 unusable, d >= 2 cut
    assert S[1, 1] == (6.0 + 11.5) / 4 and Wn[1, 1] == 0.5 and m[1, 1] == 2 and Wn[0, 1] == 0.0 and S[0, 2] == 0.0
    valid[2] = False
    S, Wn, m = ref.domain_pileup_sums(M, valid, [1], [3], 1, 1, None, 1, 64)
    assert Wn[1, 1] == 0.0 and S[0, 1] == 2.0 / 4 and Wn[0, 1] == 0.25 and Wn[1, 2] == 0.25
    S, Wn, m = ref.domain_pileup_sums(M, valid, [], [], 2, 1, None, 0, 64)
    assert S.shape == Wn.shape == (4, 4) and not S.any() and not Wn.any()


@pytest.mark.parametrize("kind,use_e,min_dist", [("general_nan", True, 2), ("general_bad", False, 0)])
def test_restatement_reduces_to_the_pileup(kind, use_e, min_dist):
    """L == R and G odd: every output cell is one bin, phi is 1 or 0 -- the
    sums of ``pileup_ref.pileup_sums`` for on-diagonal features, bit for bit."""
    start, end = data.features("seven")
    S, Wn, m = data.want(kind, "seven", 7, 3, use_e, min_dist)
    M, valid = data.dense(kind)
    S0, Cn0 = pileup_ref.pileup_sums(M, valid, start + 3, start + 3, 6, data.expected_vector(kind, use_e), min_dist,
                                     data.CHUNK)
    assert S0.sum() > 0 and Cn0.max() > 50
    assert S.tobytes() == S0.tobytes()
    assert np.array_equal(Wn, Cn0.astype(np.float64))
    assert m.max() <= 150


@pytest.mark.parametrize("R,P", [(8, 4), (7, 3), (5, 0), (1, 0)])
def test_restatement_is_symmetric_and_counts_domains(R, P):
    S, Wn, m = data.want("general_nan", "general", R, P, True, 2)
    assert S.tobytes() == S.T.copy().tobytes() and Wn.tobytes() == Wn.T.copy().tobytes()
    assert (S >= 0).all() and S.sum() > 0 and m.sum() > 0
    # everything eligible: every domain weighs exactly 1 in every cell, whatever its length (1 .. 126: mostly no
    # powers of two); no flank here leaves the chromosome
    rng = np.random.default_rng(4)
    Nb = 700
    L = np.concatenate([rng.integers(1, 127, 60), [3, 7, 100, 126]])
    start = 250 + rng.integers(0, 150, L.size)
    _, Wn, _ = ref.domain_pileup_sums(np.zeros((Nb, Nb)), np.ones(Nb, bool), start, start + L, R, P, None, 0, 16)
    assert (Wn == float(L.size)).all()


def test_read_domain_file_and_rounding(tmp_path):
    fil = tmp_path / "x_Domain_10K.txt"
    fil.write_text("chr1\t40000\t120000\nchr2\t0\t35000\nchr1\t125000\t250001\n\nchr1\t300000.0\t310000\n")
    got = dp.read_domain_file(str(fil))
    assert list(got) == ["chr1", "chr2"]
    assert got["chr1"][0].tolist() == [40000, 125000, 300000] and got["chr1"][1].tolist() == [120000, 250001, 310000]
    assert got["chr2"][0].tolist() == [0] and got["chr2"][1].tolist() == [35000]
    s, e, dropped = dp.domain_bins(*got["chr1"], 10000)
    assert s.tolist() == [4, 12, 30] and e.tolist() == [12, 26, 31] and dropped == 0      # floor, ceiling
    assert s.dtype == e.dtype == np.int32
    s, e, dropped = dp.domain_bins(*got["chr2"], 10000)
    assert s.tolist() == [0] and e.tolist() == [4]


def test_size_filters():
    sb = np.array([0, 100000, 200000, 300000, 400000])
    eb = sb + np.array([10000, 50000, 80000, 80001, 500000])
    s, e, dropped = dp.domain_bins(sb, eb, 10000, 50000, 80000)                           # both ends inclusive
    assert s.tolist() == [10, 20] and e.tolist() == [15, 28] and dropped == 3
    s, e, dropped = dp.domain_bins(sb, eb, 10000, 50000)                                  # no upper limit
    assert s.tolist() == [10, 20, 30, 40] and e.tolist() == [15, 28, 39, 90] and dropped == 1
    s, e, dropped = dp.domain_bins(sb, eb, 10000, 0, 10000)
    assert s.tolist() == [0] and e.tolist() == [1] and dropped == 4
    s, e, dropped = dp.domain_bins(sb[:0], eb[:0], 10000)
    assert s.size == 0 and e.size == 0 and dropped == 0
    with pytest.raises(ValueError):
        dp.domain_bins(sb, eb[:2], 10000)


def test_domain_scores_and_pileup_from_sums():
    # body 2, pad 1: the body cells are the inner 2 x 2, the cross cells the 8 edge cells that are no corners
    Pm = np.array([[9.0, 1.0, 2.0, 9.0],
                   [1.0, 6.0, math.nan, 3.0],
                   [2.0, math.nan, 10.0, math.nan],
                   [9.0, 3.0, math.nan, 9.0]])
    sc = dp.domain_scores(Pm, 2, 1)
    assert sc["body"] == 8.0 and sc["cross"] == 2.0 and sc["strength"] == 4.0             # NaN cells are skipped
    assert list(sc) == list(dp.SCORE_NAMES)
    sc = dp.domain_scores(np.full((4, 4), math.nan), 2, 1)
    assert all(math.isnan(sc[k]) for k in dp.SCORE_NAMES)
    sc = dp.domain_scores(np.diag([0.0, 5.0, 5.0, 0.0]), 2, 1)                            # cross = 0
    assert sc["body"] == 2.5 and sc["cross"] == 0.0 and math.isnan(sc["strength"])
    sc = dp.domain_scores(np.ones((3, 3)), 3, 0)                                          # no flank: no cross cells
    assert sc["body"] == 1.0 and math.isnan(sc["cross"]) and math.isnan(sc["strength"])
    with pytest.raises(ValueError):
        dp.domain_scores(np.ones((4, 4)), 2, 2)
    got = dp.domain_pileup_from_sums([[1.0, 3.0], [0.0, 5.0]], [[0.5, 0.0], [0.0, 2.0]])
    assert got[0, 0] == 2.0 and got[1, 1] == 2.5 and math.isnan(got[0, 1]) and math.isnan(got[1, 0])


def test_write_domain_pileup(tmp_path):
    Pm = np.array([[1.0 / 3, math.nan], [math.nan, 2.5]])
    Wn = np.array([[3.0, 0.0], [0.0, 0.125]])
    files = [str(tmp_path / n) for n in ("p.txt", "w.txt", "s.txt")]
    scores = {"body": 0.1, "cross": math.nan, "strength": 2.0}
    dp.write_domain_pileup(*files, Pm, Wn, scores, 7, 2, {"body": 1.5, "cross": 1.0, "strength": 1.5})
    rows = [[ln.rstrip("\n").split("\t") for ln in open(f)] for f in files]
    assert rows[0] == [[py2_float_str(x) for x in r] for r in Pm] and rows[0][0][1] == "nan"
    assert rows[1] == [[py2_float_str(x) for x in r] for r in Wn]
    assert rows[2] == [["body", py2_float_str(0.1)], ["cross", "nan"], ["strength", py2_float_str(2.0)],
                       ["n_features", "7"], ["n_dropped", "2"], ["body_over_controls", py2_float_str(1.5)],
                       ["cross_over_controls", py2_float_str(1.0)], ["strength_over_controls", py2_float_str(1.5)]]


def test_run_domain_pileup_arguments():
    sf = StructureFind("no_such_file.cool", Res=10000)
    assert hasattr(sf, "run_DomainPileup")
    with pytest.raises(ValueError, match="exactly one"):
        sf.run_DomainPileup("out")
    with pytest.raises(ValueError, match="exactly one"):
        sf.run_DomainPileup("out", features={}, domain_file="x")
