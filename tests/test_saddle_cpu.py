"""Host half of the expected / saddle code (hichap_master_amd/saddle.py):
``digitize_track`` and ``saddle_strength`` against the dense restatement
(tests/saddle_ref.py), ``expected_from_sums``' NaN rules, the three files'
format, and the planted chromosome through the restatement alone.  No GPU."""
import numpy as np
import pytest

from hichap_master_amd import saddle as sd
from hichap_master_amd.StructureFind import py2_float_str
from tests import saddle_ref as ref


def _tracks(rng, sizes):
    tracks, valids = {}, {}
    for k, n in enumerate(sizes):
        t = rng.normal(size=n)
        t[rng.random(n) < 0.1] = 0.0                      # gap bins of a PC file
        t[rng.random(n) < 0.05] = np.nan
        t[rng.random(n) < 0.02] = np.inf
        tracks[f"c{k}"] = t
        valids[f"c{k}"] = (rng.random(n) < 0.9).astype(np.uint8)
    return tracks, valids


@pytest.mark.parametrize("n_bins,qrange", [(50, (0.025, 0.975)), (10, (0.0, 1.0)), (1, (0.2, 0.7)), (62, (0.1, 0.9))])
def test_digitize_track(n_bins, qrange):
    rng = np.random.default_rng(n_bins)
    tracks, valids = _tracks(rng, [300, 41, 120])
    cls, edges = sd.digitize_track(tracks, valids, n_bins, qrange)
    want, want_edges = ref.digitize(list(tracks.values()), list(valids.values()), n_bins, *qrange)
    assert np.array_equal(edges, want_edges) and edges.size == n_bins + 1
    for got, w, t, v in zip(cls.values(), want, tracks.values(), valids.values()):
        assert got.dtype == np.uint8 and np.array_equal(got, w)
        out = ~np.isfinite(t) | (t == 0) | (v == 0)
        assert np.all(got[out] == 255) and np.all(got[~out] <= n_bins + 1)
    seen = np.concatenate(list(cls.values()))
    if qrange[0] > 0:
        assert (seen == 0).any() and (seen == n_bins + 1).any()          # the two outlier classes
    # without valid: only the track decides
    cls2, _ = sd.digitize_track(tracks, None, n_bins, qrange)
    assert all(np.array_equal(a == 255, ~np.isfinite(t) | (t == 0)) for a, t in zip(cls2.values(), tracks.values()))


def test_digitize_track_errors():
    with pytest.raises(ValueError, match="n_bins"):
        sd.digitize_track({"a": np.ones(5)}, None, 63)
    with pytest.raises(ValueError, match="no finite non-zero"):
        sd.digitize_track({"a": np.array([0.0, np.nan])}, None, 4)


def test_saddle_strength():
    rng = np.random.default_rng(3)
    for K in (4, 7, 12, 52):
        U = rng.random((K, K)) * 50
        Cu = rng.integers(0, 40, (K, K))
        Cu[1, 1] = 0                                      # an empty cell inside a corner
        S, C = U + U.T, Cu + Cu.T
        got = sd.saddle_strength(S, C)
        want = ref.strength(S, C)
        assert got.shape == ((K - 2) // 2,)
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
    # corners without a single cell: NaN, not an exception
    assert np.isnan(sd.saddle_strength(np.zeros((6, 6)), np.zeros((6, 6), np.int64))).all()
    assert sd.saddle_strength(np.ones((3, 3)), np.ones((3, 3))).size == 0


def test_expected_from_sums():
    s = np.array([5.0, 4.0, 0.0, 3.0, 2.0])
    n = np.array([5, 2, 4, 0, 1])
    e = sd.expected_from_sums(s, n, 1)
    assert np.isnan(e[0]) and np.isnan(e[3])              # below ignore_diags; no valid cell
    assert e[1] == 2.0 and e[2] == 0.0 and e[4] == 2.0    # a diagonal of zeros is 0, not NaN
    assert np.array_equal(e, ref.expected(s, n, 1), equal_nan=True)
    assert sd.expected_from_sums(s, n, 0)[0] == 1.0
    assert np.isnan(sd.expected_from_sums(s, n, 9)).all()


def test_write_saddle(tmp_path):
    rng = np.random.default_rng(9)
    K, Res = 6, 10000
    results = {}
    for chro, D in (("Ma", 7), ("Mb", 3)):
        s = rng.random(D + 1) * 100
        n = rng.integers(0, 5, D + 1)
        results[chro] = dict(sum=s, nvalid=n, expected=sd.expected_from_sums(s, n, 1))
    U, Cu = rng.random((K, K)), rng.integers(0, 3, (K, K))
    S, C = U + U.T, Cu + Cu.T
    C[2, 3] = C[3, 2] = 0
    edges = np.sort(rng.normal(size=K - 1))
    f = [str(tmp_path / x) for x in ("e.txt", "s.txt", "k.txt")]
    sd.write_saddle(*f, results, Res, edges, S, C, name=lambda chro: chro[1:])
    rows = [ln.rstrip("\n").split("\t") for ln in open(f[0])]
    assert rows[0] == ["chrom", "dist_bins", "dist_bp", "n_valid", "balanced_sum", "balanced_avg"]
    want = [[chro[1:], str(d), str(d * Res), str(int(r["nvalid"][d])), py2_float_str(r["sum"][d]),
             py2_float_str(r["expected"][d])] for chro, r in results.items() for d in range(len(r["sum"]))]
    assert rows[1:] == want and any(w[5] == "nan" for w in want)
    rows = [ln.rstrip("\n").split("\t") for ln in open(f[1])]
    assert rows[0] == [py2_float_str(e) for e in edges] and len(rows) == 1 + K
    got = np.array([[float(x) for x in r] for r in rows[1:]])
    assert np.isnan(got[2, 3]) and np.isnan(got[3, 2])
    ok = C > 0
    np.testing.assert_allclose(got[ok], (S / np.where(ok, C, 1))[ok], rtol=1e-11)        # '%.12g'
    rows = [ln.rstrip("\n").split("\t") for ln in open(f[2])]
    assert rows[0] == ["k", "strength"]
    assert rows[1:] == [[str(k + 1), py2_float_str(x)] for k, x in enumerate(sd.saddle_strength(S, C))]
    assert len(rows) == 1 + (K - 2) // 2


def test_planted_strength_through_the_restatement():
    """The planted chromosome of the end-to-end GPU tests, dense restatement
    only: the AA BB / AB^2 contrast of the input is 3, and strength(2) of a
    10-class saddle keeps more than 2 of it."""
    b1, b2, count, weight, track = ref.planted()
    N = track.size
    M = ref.dense(b1, b2, count, weight, 0, N)
    valid = ref.validity(weight, 0, N, None)
    assert np.count_nonzero(~valid) == 5
    s, n = ref.expected_sums(M, valid, 2, N - 1)
    e = ref.expected(s, n, 2)
    (cls,), _ = ref.digitize([track], [valid], 10, 0.025, 0.975)
    U, Cu = ref.saddle_sums(M, valid, e, cls, 12, 2, N - 1)
    S, C, _ = ref.symmetric(U, Cu)
    k = ref.strength(S, C)
    print("planted: strength(k) =", k)
    assert k.size == 5 and k[1] > 2
    # the package's host functions on the same sums
    np.testing.assert_allclose(sd.saddle_strength(S, C), k, rtol=1e-13, atol=0)
