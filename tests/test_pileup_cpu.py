"""The pileup's dense restatement (tests/pileup_ref.py) against a hand-computed
example and a closed form, and the host functions of
``hichap_master_amd.pileup``: no GPU is needed."""
import math

import numpy as np
import pytest

from hichap_master_amd import coolio, h5, loops
from hichap_master_amd import pileup as pu
from hichap_master_amd.StructureFind import StructureFind
from tests import pileup_ref as ref

RES = 10000


def _six():
    """M[a][b] = 10 a + b on the upper triangle of a 6-bin chromosome."""
    a, b = np.indices((6, 6))
    return (10 * np.minimum(a, b) + np.maximum(a, b)).astype(float)


# one loop, one on-diagonal feature, one window over the corner of the matrix
ROW, COL = [1, 2, 0], [4, 2, 5]


def test_restatement_by_hand():
    M, valid = _six(), np.ones(6, bool)
    S, Cn = ref.pileup_sums(M, valid, ROW, COL, 1, None, 0, 64)
    assert S.tolist() == [[14.0, 16.0, 18.0], [29.0, 41.0, 38.0], [50.0, 62.0, 58.0]]
    assert Cn.tolist() == [[2, 2, 2], [3, 3, 2], [3, 3, 2]]
    S, Cn = ref.pileup_sums(M, valid, ROW, COL, 1, None, 1, 2)            # the diagonal of the boundary goes
    assert S.tolist() == [[3.0, 16.0, 18.0], [29.0, 19.0, 38.0], [50.0, 62.0, 25.0]]
    assert Cn.tolist() == [[1, 2, 2], [3, 2, 2], [3, 3, 1]]
    e = [2.0, 1.0, math.nan, 4.0]                                         # d = 2 unusable, d >= 4 cut
    S, Cn = ref.pileup_sums(M, valid, ROW, COL, 1, e, 0, 1)
    assert S.tolist() == [[6.25, 12.0, 0.0], [12.0, 14.5, 23.0], [26.5, 23.0, 22.75]]
    assert Cn.tolist() == [[2, 1, 0], [1, 2, 1], [2, 1, 2]]
    valid[1] = False                                                      # bin 1 invalid: its rows and columns go
    S, Cn = ref.pileup_sums(M, valid, ROW, COL, 1, None, 0, 64)
    assert S.tolist() == [[3.0, 4.0, 5.0], [4.0, 27.0, 23.0], [23.0, 47.0, 58.0]]
    assert Cn.tolist() == [[1, 1, 1], [1, 2, 1], [1, 2, 2]]
    S, Cn = ref.pileup_sums(M, valid, [], [], 1, None, 0, 64)
    assert not S.any() and not Cn.any() and S.shape == Cn.shape == (3, 3)


def test_restatement_chunks_associate_as_stated():
    """Three terms whose sum depends on the association."""
    M = np.zeros((4, 4))
    M[0, 0], M[1, 1], M[2, 2] = 1.0, 2.0 ** -53, 2.0 ** -53
    valid = np.ones(4, bool)

    def cell(order, chunk):
        return ref.pileup_sums(M, valid, order, order, 0, None, 0, chunk)[0][0, 0]

    assert cell([0, 1, 2], 3) == 1.0                 # (1 + e) + e: each add rounds back to 1
    assert cell([0, 1, 2], 2) == 1.0                 # (1 + e) + (e)
    assert cell([0, 1, 2], 1) == 1.0
    assert cell([1, 2, 0], 2) == 1.0 + 2.0 ** -52    # (e + e) + (1)
    assert cell([1, 2, 0], 3) == 1.0 + 2.0 ** -52    # (e + e) + 1
    assert cell([1, 0, 2], 2) == 1.0                 # (e + 1) + (e)


@pytest.mark.parametrize("f,min_dist", [(0, 0), (2, 0), (3, 2)])
def test_count_closed_form(f, min_dist):
    N = 23
    rng = np.random.default_rng(3)
    row = rng.integers(0, N, 40)
    col = np.minimum(row + rng.integers(0, 9, 40), N - 1)
    S, Cn = ref.pileup_sums(np.ones((N, N)), np.ones(N, bool), row, col, f, None, min_dist, 16)
    u = np.arange(2 * f + 1)
    i = row[:, None, None] - f + u[None, :, None]
    j = col[:, None, None] - f + u[None, None, :]
    want = ((i >= 0) & (i < N) & (j >= 0) & (j < N) & (np.abs(i - j) >= min_dist)).sum(0)
    assert np.array_equal(Cn, want) and np.array_equal(S, want.astype(float))


def test_pileup_from_sums():
    P = pu.pileup_from_sums([[3.0, 0.0], [5.0, 1.0]], [[2, 0], [4, 1]])
    assert P[0, 0] == 1.5 and math.isnan(P[0, 1]) and P[1, 0] == 1.25 and P[1, 1] == 1.0


def test_apa_scores():
    P = np.ones((9, 9))
    P[4, 4] = 6.0
    P[7:, :2] = [[2.0, 4.0], [np.nan, 3.0]]          # the lower-left 2 x 2 corner (q = max(1, 4 // 2))
    s = pu.apa_scores(P)
    assert list(s) == list(pu.APA_NAMES)
    assert s["peak"] == 6.0 and s["P2UL"] == 6.0 and s["P2UR"] == 6.0 and s["P2LR"] == 6.0
    assert s["P2LL"] == 6.0 / 3.0                                         # NaN cells are skipped
    assert s["ZscoreLL"] == (6.0 - 3.0) / 1.0                             # std([2, 4, 3], ddof=1) = 1
    rest = np.delete(P.ravel(), 40)
    assert s["P2M"] == pytest.approx(6.0 / np.nanmean(rest), rel=1e-14)
    assert math.isnan(pu.apa_scores(P, corner=1)["P2LL"])                 # that corner is the NaN cell alone
    P[7:, :2] = np.nan                                                    # an empty corner
    s = pu.apa_scores(P)
    assert math.isnan(s["P2LL"]) and math.isnan(s["ZscoreLL"]) and s["P2UL"] == 6.0
    P[:2, :2] = 0.0                                                       # a zero denominator
    assert math.isnan(pu.apa_scores(P)["P2UL"])
    s = pu.apa_scores(np.ones((9, 9)), corner=3)                          # a flat corner: no deviation
    assert s["P2LL"] == 1.0 and math.isnan(s["ZscoreLL"])
    s = pu.apa_scores(np.array([[2.0]]))                                  # W = 1: no other cell
    assert s["peak"] == 2.0 and math.isnan(s["P2M"]) and math.isnan(s["ZscoreLL"])
    with pytest.raises(ValueError):
        pu.apa_scores(np.ones((4, 4)))


def test_shifted_controls():
    N, f, n = 5000, 3, 4
    rng = np.random.default_rng(1)
    row = rng.integers(0, N - 60, 200)
    col = row + rng.integers(0, 60, 200)
    rc, cc = pu.shifted_controls(row, col, N, f, n, seed=11)
    assert rc.dtype == cc.dtype == np.int32 and rc.shape == cc.shape and rc.size == 200 * n   # nothing dropped here
    assert np.array_equal(cc - rc, np.repeat(col - row, n))               # the distance is kept
    assert rc.min() >= 0 and cc.max() < N
    off = np.abs(rc - np.repeat(row, n))
    W = 2 * f + 1
    assert off.min() >= W and off.max() <= 100 * W and len(set(off.tolist())) > 50
    assert (rc < np.repeat(row, n)).any() and (rc > np.repeat(row, n)).any()
    again = pu.shifted_controls(row, col, N, f, n, seed=11)
    assert np.array_equal(again[0], rc) and np.array_equal(again[1], cc)  # reproducible by seed
    assert not np.array_equal(pu.shifted_controls(row, col, N, f, n, seed=12)[0], rc)
    # a chromosome shorter than the smallest offset: every copy is dropped
    rc, cc = pu.shifted_controls([2], [4], 6, f, 3, seed=0)
    assert rc.size == 0 and cc.size == 0
    rc, cc = pu.shifted_controls(row, col, N, f, 0, seed=0)
    assert rc.size == 0


def test_feature_files(tmp_path):
    """A loop file in ``loops.call_peaks``' format and in the cluster file's,
    and a boundary file as ``run_TADs`` writes it (``chrom<TAB>bin * Res``)."""
    lf = tmp_path / "loops.txt"
    with open(lf, "w") as f:
        f.write(loops.HEAD)
        for chrom, a, b in (("1", 120000, 450000), ("1", 30000, 90000), ("X", 700000, 1000000)):
            f.write(loops.LINE_FORMAT % ((chrom, a, b) + (1.5,) * 7))
    got = pu.read_loop_file(str(lf))
    assert list(got) == ["1", "X"]
    assert got["1"][0].tolist() == [120000, 30000] and got["1"][1].tolist() == [450000, 90000]
    assert got["X"][0].tolist() == [700000] and got["X"][1].tolist() == [1000000]
    cf = tmp_path / "clusters.txt"
    with open(cf, "w") as f:
        f.write(loops.CLUSTER_HEAD)
        f.write("\t".join(["2", "50000", "250000", "17.5", "0.001", "3"]) + "\n")
    got = pu.read_loop_file(str(cf))
    assert got["2"][0].tolist() == [50000] and got["2"][1].tolist() == [250000]
    bf = tmp_path / "b.txt"
    with open(bf, "w") as f:
        for chrom, b in (("1", 40000), ("1", 1200000), ("2", 0)):
            f.write(f"{chrom}\t{b}\n")
    got = pu.read_boundary_file(str(bf))
    assert got["1"][0].tolist() == got["1"][1].tolist() == [40000, 1200000] and got["2"][0].tolist() == [0]


def test_run_pileup_value_errors(tmp_path):
    path = str(tmp_path / "t.cool")
    b = np.arange(30, dtype=np.int64)
    coolio.create_cooler(path, {RES: ([("chr1", 20 * RES), ("chr2", 10 * RES)], b, b, np.ones(30, np.int64))})
    out = str(tmp_path / "out")
    sf = StructureFind(path, Res=RES)
    feats = {"chr1": ([50000], [120000])}
    with pytest.raises(ValueError, match="exactly one"):
        sf.run_Pileup(out)
    with pytest.raises(ValueError, match="exactly one"):
        sf.run_Pileup(out, features=feats, loop_file="x.txt")
    with pytest.raises(ValueError, match="exactly one"):
        sf.run_Pileup(out, loop_file="x.txt", boundary_file="y.txt")
    with pytest.raises(ValueError, match="flank"):
        sf.run_Pileup(out, features=feats, flank=64 * RES)
    with pytest.raises(ValueError, match=">= 0"):
        sf.run_Pileup(out, features=feats, flank=RES, min_dist=-RES)
    with pytest.raises(ValueError, match="no bins/weight"):
        sf.run_Pileup(out, features=feats, flank=RES)
    h5.append_dataset(path, f"{RES}/bins", "weight", np.ones(30))
    with pytest.raises(ValueError, match="chrX"):
        sf.run_Pileup(out, features={"chr1": ([50000], [120000]), "chrX": ([0], [0])}, flank=RES)
    with pytest.raises(ValueError, match="outside the chromosome"):
        sf.run_Pileup(out, features={"chr2": ([50000], [100000])}, flank=RES)
    hap = StructureFind(path, Res=RES, Allelic="Maternal")                # no chromosome starts with 'M'
    with pytest.raises(ValueError, match="hr1"):
        hap.run_Pileup(out, features={"hr1": ([0], [0])}, flank=RES)
    with pytest.raises(ValueError, match="Unkonwn"):
        StructureFind(path, Res=RES, Allelic="Both").run_Pileup(out, features=feats)
