"""The host side of the trans expected, the cis / trans totals and the trans
saddle (hichap_master_amd/trans.py) without a device: the cell
counts against the brute force of tests/trans_ref.py, the expected and the
totals on hand examples, the four files through a parse, ``run_Trans``'s
error on an unbalanced cooler and the ``trans_trips`` knob."""
import math
import os

import numpy as np
import pytest

from hichap_master_amd import _lib, coolio
from hichap_master_amd import trans as tr
from hichap_master_amd.StructureFind import StructureFind, py2_float_str
from tests import knobs
from tests import trans_ref as ref

RES = 10000


def _counts_case():
    """Five chromosomes of 7, 12, 1, 9 and 6 bins; chromosome 3 is not used,
    bins are invalid by weight and by bad, one bin in eight has class 255, and
    the blocks (0, 2) (NaN) and (2, 4) (zero) are unusable."""
    rng = np.random.default_rng(11)
    off = np.array([0, 7, 19, 20, 29, 35])
    n, K = int(off[-1]), 5
    use = np.array([1, 1, 1, 0, 1], np.uint8)
    w = rng.uniform(0.5, 2.0, n)
    w[[0, 8, 9, 34]] = np.nan
    bad = np.zeros(n, np.uint8)
    bad[[6, 7, 30]] = 1
    cls = rng.integers(0, K, n).astype(np.uint8)
    cls[rng.random(n) < 0.125] = 255
    cls[3], cls[12], cls[19] = K - 1, 255, 1
    e = np.full((5, 5), np.nan)
    e[np.triu_indices(5, 1)] = rng.uniform(0.5, 2.0, 10)
    e[0, 2], e[2, 4] = np.nan, 0.0
    return off, use, w, bad, cls, K, e


def test_saddle_counts_equal_the_brute_force():
    off, use, w, bad, cls, K, e = _counts_case()
    n = int(off[-1])
    valid, nvb = tr.valid_bins(off, w, use, bad)
    want_valid = ref.validity(off, w, use, bad)
    assert valid.tolist() == [int(x) for x in want_valid] and nvb.tolist() == ref.n_valid(off, want_valid)
    assert nvb[3] == 0 and 0 < nvb[1] < 12
    usable = tr.trans_usable(e)
    assert usable.tolist() == ref.usable(e) and not usable[0, 2] and not usable[2, 4] and usable[0, 1]
    M = [[0.0] * n for _ in range(n)]
    stored = [[False] * n for _ in range(n)]
    _, want, _ = ref.saddle_sums(M, stored, off, want_valid, e, cls, K)
    got = tr.trans_saddle_counts(off, valid, cls, K, usable)
    assert got.dtype == np.int64 and got.shape == (5, K, K)
    assert np.array_equal(got, want)
    assert want[0].sum() > 0 and want[1].sum() > 0 and not want[2].any() and not want[3].any() and not want[4].any()
    cls[5] = K                                           # a class in [K, 254] is an error here too
    with pytest.raises(ValueError, match="cls entry"):
        tr.trans_saddle_counts(off, valid, cls, K, usable)


def test_expected_is_nan_where_a_chromosome_has_no_valid_bin():
    s = np.array([[5.0, 6.0, 7.0], [0.0, 8.0, 9.0], [0.0, 0.0, 10.0]])
    e = tr.trans_expected_from_sums(s, [3, 0, 4])
    assert np.isnan(e[0, 1]) and np.isnan(e[1, 2]) and e[0, 2] == 7.0 / 12.0
    assert np.isnan(e[np.tril_indices(3)]).all()
    assert np.array_equal(np.isnan(e), np.isnan(ref.expected(s, [3, 0, 4])))
    big = tr.trans_expected_from_sums([[0.0, 3.0], [0.0, 0.0]], [94906267, 94906269])   # an exact int64 product > 2^53
    assert big[0, 1] == 3.0 / float(94906267 * 94906269)


def test_cis_trans_totals_by_hand():
    s = np.array([[10.0, 2.0, 3.0], [0.0, 20.0, 5.0], [0.0, 0.0, 0.0]])
    t = tr.cis_trans_totals(s)
    assert t["cis"].tolist() == [10.0, 20.0, 0.0]
    assert t["trans"].tolist() == [5.0, 7.0, 8.0]
    assert t["cis_fraction"].tolist() == [10.0 / 15.0, 20.0 / 27.0, 0.0]
    assert t["genome"] == (30.0, 10.0, 0.75)
    cis, trans, frac, genome = ref.totals(s)
    assert (cis, trans, frac, genome) == (t["cis"].tolist(), t["trans"].tolist(), t["cis_fraction"].tolist(),
                                          t["genome"])
    z = tr.cis_trans_totals(np.zeros((2, 2)))            # nothing at all: 0 / 0
    assert np.isnan(z["cis_fraction"]).all() and math.isnan(z["genome"][2])


def _parse(path):
    return [ln.rstrip("\n").split("\t") for ln in open(path)]


def test_write_trans_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    names, sel = ["a", "skipped", "b", "c"], [0, 2, 3]
    nvb = np.array([4, 0, 0, 7])
    s = np.triu(rng.uniform(1, 50, (4, 4)))
    npix = np.triu(rng.integers(1, 90, (4, 4)))
    e = tr.trans_expected_from_sums(s, nvb)
    t = tr.cis_trans_totals(s)
    K = 6
    edges = np.sort(rng.normal(size=K - 1))
    S = rng.uniform(1, 9, (K, K))
    S = S + S.T
    C = rng.integers(0, 5, (K, K))
    C = C + C.T
    f = [str(tmp_path / x) for x in ("e.txt", "c.txt", "s.txt", "k.txt")]
    tr.write_trans(f[0], f[1], names, sel, nvb, s, npix, e, t, f[2], f[3], edges, S, C)
    exp, ct, sad, st = (_parse(x) for x in f)
    assert exp[0] == ["chrom1", "chrom2", "n_valid1", "n_valid2", "n_pixels", "balanced_sum", "balanced_avg"]
    pairs = [(0, 2), (0, 3), (2, 3)]
    assert exp[1:] == [[names[p], names[q], str(nvb[p]), str(nvb[q]), str(npix[p, q]), py2_float_str(s[p, q]),
                        py2_float_str(e[p, q])] for p, q in pairs]
    assert exp[1][6] == "nan" and exp[2][6] != "nan"
    np.testing.assert_allclose(float(exp[2][6]), s[0, 3] / 28, rtol=5e-12)
    assert ct[0] == ["chrom", "cis_sum", "trans_sum", "cis_fraction"]
    assert ct[1:-1] == [[names[p], py2_float_str(t["cis"][p]), py2_float_str(t["trans"][p]),
                         py2_float_str(t["cis_fraction"][p])] for p in sel]
    assert ct[-1] == ["genome"] + [py2_float_str(x) for x in t["genome"]]
    np.testing.assert_allclose([float(x) for x in ct[-1][1:]], t["genome"], rtol=5e-12)
    assert sad[0] == [py2_float_str(x) for x in edges] and len(sad) == 1 + K
    want = np.where(C > 0, S / np.where(C > 0, C, 1), np.nan)
    np.testing.assert_allclose([[float(x) for x in row] for row in sad[1:]], want, rtol=5e-12, equal_nan=True)
    assert st == [["k", "strength"]] + [[str(k + 1), py2_float_str(x)]
                                        for k, x in enumerate(tr.saddle_strength(S, C))]
    # without a saddle only the first two files are written
    g = [str(tmp_path / x) for x in ("e2.txt", "c2.txt")]
    tr.write_trans(g[0], g[1], names, sel, nvb, s, npix, e, t)
    assert _parse(g[0]) == exp and _parse(g[1]) == ct


def test_run_trans_needs_weights_on_traditional_data(tmp_path):
    path = str(tmp_path / "raw.cool")
    b1, b2 = np.array([0, 0, 1, 2]), np.array([0, 3, 2, 3])
    coolio.create_cooler(path, {RES: ([("chr1", 2 * RES), ("chr2", 2 * RES)], b1, b2, np.array([3, 4, 5, 6]))})
    sf = StructureFind(path, Res=RES)
    with pytest.raises(ValueError, match="run_Trans: the cooler has no bins/weight"):
        sf.run_Trans(str(tmp_path / "out"))
    with pytest.raises(ValueError, match="ignore_diags"):
        sf.run_Trans(str(tmp_path / "out"), ignore_diags=-1)
    assert not os.path.exists(str(tmp_path / "out"))


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libhichap_hip.so is not built")
def test_trans_trips_roundtrip_and_rejection():
    """hh_tune "trans_trips" as tests/test_tune_cpu.py holds every key."""
    if "trans_trips" not in os.environ.get("HH_TUNE", ""):
        assert knobs.get("trans_trips") == 8
    before = knobs.get("trans_trips")
    with knobs.tuned(trans_trips=1):
        assert knobs.get("trans_trips") == 1
        for illegal in (0, 257, -1):
            with pytest.raises(_lib.HipLibraryError) as e:
                _lib.call("hh_tune", b"trans_trips", illegal)
            assert e.value.code == -1 and "trans_trips" in str(e.value)
        assert knobs.get("trans_trips") == 1
    assert knobs.get("trans_trips") == before
