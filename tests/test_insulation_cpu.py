"""Host half of the insulation score (hichap_master_amd/insulation.py): the
boundary rule against scipy, the track's rules, ``full(w, g)`` and the two
files' format.  No GPU."""
import numpy as np
import pytest
from scipy.signal import find_peaks, peak_prominences

from hichap_master_amd import insulation as ins
from tests import insulation_ref as ref


def test_boundaries_equal_scipy():
    """300 tracks of 3..80 quarter-integers (ties and plateaus), 15 % NaN:
    the same minima and bit-equal prominences as scipy's defaults."""
    rng = np.random.default_rng(11)
    n_peaks = n_plateau = 0
    for _ in range(300):
        m = int(rng.integers(3, 81))
        L = rng.integers(-8, 9, m) / 4.0
        L[rng.random(m) < 0.15] = np.nan
        where = np.nonzero(np.isfinite(L))[0]
        x = L[where]
        peaks, _ = find_peaks(-x)
        prom = peak_prominences(-x, peaks)[0] if peaks.size else np.empty(0)
        idx, strength, called = ins.insulation_boundaries(L, 0.5)
        assert idx.tolist() == where[peaks].tolist()
        assert strength.tobytes() == prom.astype(np.float64).tobytes()
        assert called.tolist() == (prom >= 0.5).tolist()
        n_peaks += peaks.size
        n_plateau += sum(1 for p in peaks if x[p + 1] == x[p] or x[p - 1] == x[p])
    assert n_peaks > 1000 and n_plateau > 50


def test_boundaries_small_cases():
    nan = np.nan
    idx, s, called = ins.insulation_boundaries([nan, 3.0, nan, 1.0, 1.0, nan, 1.0, 2.0, 0.5, nan, 4.0, nan])
    # finite entries 3 1 1 1 2 .5 4: plateau 1 1 1 (midpoint = its 2nd entry, L index 4), then .5 (index 8)
    assert idx.tolist() == [4, 8] and s.tolist() == [1.0, 2.5] and called.tolist() == [True, True]
    for L in ([], [1.0], [2.0, 1.0], [nan, nan, nan], [3.0, 1.0, nan], [1.0, 1.0, 1.0], [1.0, 2.0, 3.0]):
        idx, s, called = ins.insulation_boundaries(L)
        assert idx.size == 0 and s.size == 0 and called.size == 0 and idx.dtype == np.int64
    # the first and last entries never count, a plateau reaching an end neither
    assert ins.insulation_boundaries([0.0, 1.0, 1.0, 0.0])[0].size == 0
    assert ins.insulation_boundaries([2.0, 1.0, 1.0])[0].size == 0
    idx, s, called = ins.insulation_boundaries([1.0, 0.95, 1.0, 0.0, 1.0], min_strength=0.1)
    assert idx.tolist() == [1, 3] and called.tolist() == [False, True]


@pytest.mark.parametrize("w", [1, 2, 3, 5, 17, 64])
def test_full_cells(w):
    for g in range(0, 2 * w + 3):
        assert ins.full_cells(w, g) == ref.full(w, g)


def test_track_rules():
    w, g = 3, 1
    full = ins.full_cells(w, g)                  # 8 of 9 cells
    assert full == 8
    N = 12
    valid = np.ones(N, np.uint8)
    n = np.full(N, full, np.int32)
    n[0], n[1], n[-1], n[-2] = 2, 5, 2, 5        # clipped diamonds: 5 < 0.66 * 8 = 5.28 <= 6
    n[2] = 6
    n[5] = 0
    S = np.arange(1, N + 1, dtype=np.float64) * n
    S[5] = 0.0
    S[6] = 0.0                                   # a score of 0: log2 = -inf -> NaN
    valid[7] = 0                                 # an invalid bin with a full diamond
    L = ins.insulation_track(S, n, valid, w, g)
    score = np.array([np.nan, np.nan, 3.0, 4.0, 5.0, np.nan, 0.0, np.nan, 9.0, 10.0, np.nan, np.nan])
    want = np.log2(score[[2, 3, 4, 8, 9]] / 4.5)     # median of 3 4 5 0 9 10
    assert np.isnan(L[[0, 1, 5, 6, 7, 10, 11]]).all()
    np.testing.assert_allclose(L[[2, 3, 4, 8, 9]], want, rtol=1e-15, atol=0)
    assert np.array_equal(L, ref.track(S, n, valid, w, g), equal_nan=True)
    # min_frac_valid = 0: only n = 0, the invalid bin and the zero score stay NaN
    L0 = ins.insulation_track(S, n, valid, w, g, 0.0)
    assert np.isnan(L0).tolist() == [i in (5, 6, 7) for i in range(N)]
    # nothing finite
    for Sx, nx, vx in ((S, np.zeros(N, np.int32), valid), (S, n, np.zeros(N, np.uint8)),
                       (np.full(N, np.nan), n, valid)):
        assert np.isnan(ins.insulation_track(Sx, nx, vx, w, g)).all()
    # all scores 0: the median is 0, every ratio NaN
    assert np.isnan(ins.insulation_track(np.zeros(N), n, valid, w, g, 0.0)).all()


def test_files_format(tmp_path):
    nan = np.nan
    res = {
        "Ma": dict(size=35000, valid=np.array([1, 0, 1, 1], np.uint8),
                   L=np.array([[nan, nan, -0.5, 1.0], [0.25, nan, -1.25e-7, 2.0]]),
                   n=np.array([[1, 0, 4, 3], [7, 0, 16, 9]], np.int32),
                   strength=np.array([[nan, nan, 0.75, nan], [nan, nan, 0.05, nan]])),
        "Mb": dict(size=20000, valid=np.array([1, 1], np.uint8),
                   L=np.array([[0.0, 1 / 3.0], [nan, nan]]), n=np.array([[4, 4], [0, 0]], np.int32),
                   strength=np.array([[nan, 0.1], [2.0, nan]])),
    }
    t, b = tmp_path / "t.txt", tmp_path / "b.txt"
    ins.write_insulation(str(t), str(b), res, 10000, [2, 150], 0.1, name=lambda c: c[1:])
    assert t.read_text().splitlines() == [
        "chrom\tstart\tend\tvalid\tlog2_insulation_20K\tn_valid_20K\tboundary_strength_20K"
        "\tlog2_insulation_1M500K\tn_valid_1M500K\tboundary_strength_1M500K",
        "a\t0\t10000\t1\tnan\t1\tnan\t0.25\t7\tnan",
        "a\t10000\t20000\t0\tnan\t0\tnan\tnan\t0\tnan",
        "a\t20000\t30000\t1\t-0.5\t4\t0.75\t-1.25e-07\t16\t0.05",
        "a\t30000\t35000\t1\t1.0\t3\tnan\t2.0\t9\tnan",
        "b\t0\t10000\t1\t0.0\t4\tnan\tnan\t0\t2.0",
        "b\t10000\t20000\t1\t0.333333333333\t4\t0.1\tnan\t0\tnan",
    ]
    assert b.read_text().splitlines() == [
        "chrom\tpos\twindow\tstrength",
        "a\t20000\t20000\t0.75",
        "b\t10000\t20000\t0.1",
        "b\t0\t1500000\t2.0",
    ]


def test_run_insulation_argument_errors(tmp_path):
    from hichap_master_amd.StructureFind import StructureFind
    sf = StructureFind("unused.cool", Res=10000)
    for windows in ((), (5000,), (600000, 605000), tuple(range(10000, 100000, 10000)), (2570000,)):
        with pytest.raises(ValueError, match="run_Insulation"):
            sf.run_Insulation(str(tmp_path / "o"), windows=windows)
    with pytest.raises(ValueError, match="Unkonwn key word"):
        StructureFind("unused.cool", Res=10000, Allelic="Both").run_Insulation(str(tmp_path / "o"))
