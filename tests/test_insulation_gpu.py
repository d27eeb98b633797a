"""Insulation score on the GPU (K11 ``k_insulation``):
``hh_insulation_scan`` and ``hh_insulation_pixels`` against the dense NumPy
restatement (tests/insulation_ref.py) -- exactly where every sum is exact in
fp64, within a derived bound otherwise -- then ``run_Insulation`` on planted
borders (raw haplotype path) and on a balanced synthetic cooler."""
import functools
import os

import numpy as np
import pytest

from hichap_master_amd import _lib, coolio, synth
from hichap_master_amd import insulation as ins
from hichap_master_amd._lib import HipLibraryError, ptr
from hichap_master_amd.StructureFind import StructureFind, column_band, py2_float_str
from tests import insulation_ref as ref

pytestmark = pytest.mark.gpu

RES = 10000
N = 200
LO, NB = 11, 11 + N + 9                      # 'a' 11 bins, 'b' N bins (queried), 'c' 9 bins
WINDOWS = (1, 2, 5, 17, 64, 65)              # a wave boundary, w > N / 3 (clipped diamonds), nesting
INVALID = [0, N - 1, 90, 91, 92, 93, 150]    # both ends, a run of 4, a single bin
EMPTY_ROW = 40                               # a bin with no pixels at all
HH_ERR_ARG = -1


@functools.lru_cache(maxsize=None)
def _table():
    """Sorted upper-triangle pixel table of the three chromosomes, counts in
    1/64: dense near the diagonal of 'b' (every diamond cell within 130 bins
    may be hit), trans pixels into 'b' (bin1 < LO) and out of it (bin2 >= hi)."""
    rng = np.random.default_rng(2024)
    i, j = np.indices((NB, NB))
    H = np.triu(rng.integers(1, 4000, (NB, NB)) * (rng.random((NB, NB)) < np.where(j - i < 140, 0.7, 0.05)))
    H[LO + EMPTY_ROW, :] = 0
    H[:, LO + EMPTY_ROW] = 0
    assert np.count_nonzero(H[:LO, LO:LO + N]) > 20 and np.count_nonzero(H[LO:LO + N, LO + N:]) > 20
    b1, b2 = np.nonzero(H)
    cnt = H[b1, b2] / 64.0
    for a in (b1, b2, cnt):
        a.setflags(write=False)
    return b1.astype(np.int64), b2.astype(np.int64), cnt


def _weights(kind):
    """Global weights and the 'bad' list of chromosome 'b'.  exact: powers of
    two, so every product and sum of the k/64 counts is exact in fp64."""
    rng = np.random.default_rng(5)
    if kind.startswith("exact"):
        w = 2.0 ** rng.integers(-3, 1, NB)
    else:
        w = rng.uniform(0.05, 3.0, NB)
    bad = None
    if kind.endswith("nan"):
        w[LO + np.array(INVALID)] = np.nan
        w[3] = np.nan                         # a masked bin of 'a': its trans pixels must not matter
    else:
        bad = np.zeros(N, np.uint8)
        bad[INVALID] = 1
    return w, bad


@functools.lru_cache(maxsize=None)
def _dense(kind):
    """The dense matrix of 'b' as cooler balances it (count * w[bin1] * w[bin2],
    NaN -> 0), and valid."""
    b1, b2, cnt = _table()
    w, bad = _weights(kind)
    keep = (b1 >= LO) & (b2 < LO + N)
    val = cnt[keep] * w[b1[keep]] * w[b2[keep]]
    M = np.zeros((N, N))
    M[b1[keep] - LO, b2[keep] - LO] = val
    M[b2[keep] - LO, b1[keep] - LO] = val
    valid = np.isfinite(w[LO:LO + N]).astype(np.uint8)
    if bad is not None:
        valid &= 1 - bad
    M = np.nan_to_num(M)
    M.setflags(write=False)
    valid.setflags(write=False)
    return M, valid


@functools.lru_cache(maxsize=None)
def _want(kind, g):
    M, valid = _dense(kind)
    S, n = ref.diamond_sums(M, valid, WINDOWS, g)
    S.setflags(write=False)
    n.setflags(write=False)
    return S, n


def _both(kind, g, device=False):
    """(S, n) of the pixel entry point and of the scan entry point."""
    b1, b2, cnt = _table()
    w, bad = _weights(kind)
    M, valid = _dense(kind)
    band = column_band(M, 2 * max(WINDOWS) - 2)
    if device:
        import torch
        b1, b2, cnt, band = (torch.from_numpy(np.array(a)).cuda() for a in (b1, b2, cnt, band))
    Sp, npx = ins.diamond_sums_pixels(b1, b2, cnt, w, LO, N, WINDOWS, g, bad)
    Sb, nb = ins.diamond_sums_band(band, valid, WINDOWS, g)
    if device:
        assert Sp.is_cuda and npx.is_cuda and Sb.is_cuda and nb.is_cuda
        Sp, npx, Sb, nb = (t.cpu().numpy() for t in (Sp, npx, Sb, nb))
    return (Sp, npx), (Sb, nb)


@pytest.mark.parametrize("kind", ["exact_nan", "exact_bad"])
@pytest.mark.parametrize("g", [0, 1, 2, 3])
def test_exact(kind, g):
    S, n = _want(kind, g)
    assert S[:, EMPTY_ROW].any() and n[3].max() == ref.full(17, g) and n[5].max() < ref.full(65, g)
    for device in (False, True):
        for got_S, got_n in _both(kind, g, device):
            assert got_S.dtype == np.float64 and got_n.dtype == np.int32
            assert np.array_equal(got_n, n)
            assert np.array_equal(got_S, S)


@pytest.mark.parametrize("g", [0, 1, 2, 3])
def test_small_chromosome(g):
    """N = 7 with w = 5: every diamond is clipped on at least one side."""
    rng = np.random.default_rng(g)
    U = np.triu(rng.integers(1, 500, (7, 7))) / 64.0
    M = U + np.triu(U, 1).T
    b1, b2 = np.nonzero(U)
    for bad in (None, np.array([0, 0, 1, 0, 0, 0, 0], np.uint8)):
        valid = None if bad is None else 1 - bad
        S, n = ref.diamond_sums(M, valid, (5,), g)
        got = ins.diamond_sums_pixels(b1, b2, U[b1, b2], None, 0, 7, (5,), g, bad)
        assert np.array_equal(got[0], S) and np.array_equal(got[1], n)
        got = ins.diamond_sums(M, (1, 5), g, valid)
        assert np.array_equal(got[0][1], S[0]) and np.array_equal(got[1][1], n[0])


@pytest.mark.parametrize("kind", ["general_nan", "general_bad"])
@pytest.mark.parametrize("g", [0, 1, 2, 3])
def test_general(kind, g):
    """Random positive double weights.  A sum of at most 65^2 = 4225
    non-negative terms has relative error below 4225 * 2^-53 = 4.7e-13 in any
    order, the restatement's as well: rtol 1e-12, derived, not measured."""
    S, n = _want(kind, g)
    for got_S, got_n in _both(kind, g):
        assert np.array_equal(got_n, n)
        err = np.abs(got_S - S) / np.where(S > 0, S, 1.0)
        print(f"{kind} g={g}: max relative error {err.max():.3g}")
        np.testing.assert_allclose(got_S, S, rtol=1e-12, atol=0)


def test_repeatable():
    for kind in ("general_nan", "exact_bad"):
        (S1, n1), (S2, n2) = _both(kind, 1)
        (S3, n3), (S4, n4) = _both(kind, 1)
        assert S1.tobytes() == S3.tobytes() and S2.tobytes() == S4.tobytes()      # two calls
        assert S1.tobytes() == S2.tobytes() and n1.tobytes() == n2.tobytes()      # the two entry points
        assert n1.tobytes() == n3.tobytes() and n2.tobytes() == n4.tobytes()


def _raw_pixels(windows, g=1, weight="default", n_weight=None, S=None, n=None):
    b1, b2, cnt = _table()
    w = _weights("exact_nan")[0] if isinstance(weight, str) else weight
    wa = np.asarray(windows, np.int32)
    return _lib.load().hh_insulation_pixels(
        ptr(b1), ptr(b2), ptr(cnt), b1.size, ptr(w), (0 if w is None else w.size) if n_weight is None else n_weight,
        LO, N, None, ptr(wa), wa.size, g, ptr(S), ptr(n), 0, None)


def test_argument_errors_leave_outputs_untouched():
    S = np.full((9, N), -7.5)
    n = np.full((9, N), -3, np.int32)
    M, valid = _dense("exact_nan")
    band = column_band(M, 126)                                # enough for w = 64, not for 65
    lib = _lib.load()

    def scan(windows, g=1, B=126):
        wa = np.asarray(windows, np.int32)
        return lib.hh_insulation_scan(ptr(band), N, B, ptr(valid), ptr(wa), wa.size, g, ptr(S), ptr(n), 0, None)

    bad_windows = ([], list(range(1, 10)), [0, 5], [5, 257], [5, 5], [17, 5], [-1])
    for windows in bad_windows:
        assert _raw_pixels(windows, S=S, n=n) == HH_ERR_ARG, windows
        assert scan(windows) == HH_ERR_ARG, windows
    assert _raw_pixels([5], g=-1, S=S, n=n) == HH_ERR_ARG and scan([5], g=-1) == HH_ERR_ARG
    assert scan([5, 65]) == HH_ERR_ARG                        # B = 126 < 2 * 65 - 2
    assert b"band narrower" in lib.hh_last_error()
    assert _raw_pixels([5], n_weight=LO + N - 1, S=S, n=n) == HH_ERR_ARG   # weights end inside the chromosome
    assert b"weights do not cover" in lib.hh_last_error()
    assert np.all(S == -7.5) and np.all(n == -3)
    with pytest.raises(HipLibraryError, match="ascending"):
        ins.diamond_sums_pixels(*_table(), None, LO, N, (17, 5))
    # the library is still usable, and B = 126 serves w = 64
    assert scan([5, 64]) == 0
    want = _want("exact_nan", 1)
    assert np.array_equal(S[:2], want[0][[2, 4]]) and np.array_equal(n[:2], want[1][[2, 4]])
    assert np.all(S[2:] == -7.5) and np.all(n[2:] == -3)


def test_no_pixels():
    e = np.empty(0, np.int64)
    w, bad = _weights("exact_nan")
    S, n = ins.diamond_sums_pixels(e, e, np.empty(0), w, LO, N, WINDOWS, 1)
    assert not S.any() and np.array_equal(n, _want("exact_nan", 1)[1])
    S, n = ins.diamond_sums_pixels(e, e, np.empty(0), None, 0, 7, (5,), 0)
    assert not S.any() and np.array_equal(n, ref.diamond_sums(np.zeros((7, 7)), None, (5,), 0)[1])


def _read_tables(out):
    prefix = os.path.basename(out)
    res = StructureFind.properU(RES)
    with open(os.path.join(out, f"{prefix}_Insulation_{res}.txt")) as f:
        track = [ln.rstrip("\n").split("\t") for ln in f]
    with open(os.path.join(out, f"{prefix}_InsulationBoundary_{res}.txt")) as f:
        bnd = [ln.rstrip("\n").split("\t") for ln in f]
    assert bnd[0] == ["chrom", "pos", "window", "strength"]
    return track, bnd[1:]


@pytest.mark.parametrize("g", [0, 1, 2])
def test_planted_borders_raw_path(tmp_path, g):
    """M[i][j] = 1000 / (|i - j| + 1), times 4 inside blocks of 25 bins, as a
    haplotype cooler ('Mb', raw counts): every border between bins 25k - 1 and
    25k (k = 1..7) gives exactly one boundary, on either side of it (the two
    bins have mirror-image diamonds), and nothing else is called."""
    i, j = np.indices((N, N))
    M = 1000.0 / (np.abs(i - j) + 1) * np.where(i // 25 == j // 25, 4.0, 1.0)
    b1, b2 = np.nonzero(np.triu(np.ones((N, N))))
    path = str(tmp_path / "hap.cool")
    coolio.create_cooler(path, {RES: ([("Mb", N * RES), ("Pb", 30 * RES)], b1, b2, M[b1, b2])})
    out = str(tmp_path / "planted")
    sf = StructureFind(path, Res=RES, Allelic="Maternal")
    r = sf.run_Insulation(out, windows=(5 * RES, 12 * RES), ignore_diags=g)
    assert list(r) == ["Mb"]
    track, bnd = _read_tables(out)
    assert len(track) == 1 + N and {t[0] for t in track[1:]} == {"b"}        # 'Mb' without its prefix
    for w in (5, 12):
        pos = sorted(int(p) // RES for c, p, win, s in bnd if int(win) == w * RES)
        print(f"g={g} w={w}: boundaries at {pos}, strengths "
              f"{[s for c, p, win, s in bnd if int(win) == w * RES]}")
        assert len(pos) == 7
        assert all(pos[k - 1] in (25 * k - 1, 25 * k) for k in range(1, 8))
    assert len(bnd) == 14 and all(c == "b" for c, _, _, _ in bnd)


@pytest.fixture(scope="module")
def balanced_cooler(tmp_path_factory):
    rng = np.random.default_rng(77)
    sizes = [260, 120, 60]
    b1, b2, c, off = synth.coo_genome(sizes, rng, A=40.0, trans_density=0.01)
    path = str(tmp_path_factory.mktemp("ins") / "bal.cool")
    coolio.create_cooler(path, {RES: ([(f"chr{k + 1}", s * RES) for k, s in enumerate(sizes)], b1, b2, c)})
    with pytest.raises(ValueError, match="no bins/weight"):
        StructureFind(path, Res=RES).run_Insulation(str(tmp_path_factory.mktemp("x") / "o"))
    coolio.balance_cooler(f"{path}::{RES}")
    return path


def test_end_to_end_balanced(balanced_cooler, tmp_path):
    """run_Insulation's files against the restatement on the dense balanced
    matrices.  Boundary lines: the same (chrom, pos, window).  Floats: the sums
    agree to the rtol of test_general (1e-12); one division and one log2 turn
    that relative error of the score into an absolute error of about
    1e-12 / ln 2 of the log2 track, so the track and the strengths (differences
    of track values) are compared with rtol = atol = 1e-11."""
    wbins, g = [4, 10], 1
    out = str(tmp_path / "e2e")
    sf = StructureFind(balanced_cooler, Res=RES)
    r = sf.run_Insulation(out, windows=(10 * RES, 4 * RES))                   # any order: sorted by the call
    mats = {}
    with coolio.Cooler(f"{balanced_cooler}::{RES}") as c:
        wt = c.weights()
        for chro in c.chromnames:
            lo, hi = c.extent(chro)
            mats[chro] = (np.nan_to_num(c.matrix(balance=True).fetch(chro)), np.isfinite(wt[lo:hi]))
    tr, bnd_want = ref.tables(mats, RES, wbins, g)
    assert list(r) == list(mats) and len(bnd_want) > 10
    track, bnd = _read_tables(out)
    units = [StructureFind.properU(w * RES) for w in wbins]
    assert track[0] == ["chrom", "start", "end", "valid"] + [
        f"{col}_{u}" for u in units for col in ("log2_insulation", "n_valid", "boundary_strength")]
    assert [(c, int(p), int(w)) for c, p, w, s in bnd] == [(c, p, w) for c, p, w, s in bnd_want]
    np.testing.assert_allclose([float(s) for *_, s in bnd], [s for *_, s in bnd_want], rtol=1e-11, atol=1e-11)
    row = 1
    for chro, (M, valid) in mats.items():
        L_want, n_want = tr[chro]
        assert np.array_equal(r[chro]["n"], n_want) and np.array_equal(r[chro]["valid"] != 0, valid)
        assert np.array_equal(np.isnan(r[chro]["L"]), np.isnan(L_want)) and np.isfinite(L_want).sum() > 50
        np.testing.assert_allclose(r[chro]["L"], L_want, rtol=1e-11, atol=1e-11)
        for i in range(len(valid)):                                          # the file is the text of these arrays
            t = track[row]
            row += 1
            assert t[:4] == [chro, str(i * RES), str((i + 1) * RES), str(int(valid[i]))]
            for k in range(2):
                assert t[4 + 3 * k:7 + 3 * k] == [py2_float_str(r[chro]["L"][k][i]), str(n_want[k][i]),
                                                  py2_float_str(r[chro]["strength"][k][i])]
    assert row == len(track)
    # Get_Insulation on the dense matrix gives the same track
    chro = list(mats)[1]
    with coolio.Cooler(f"{balanced_cooler}::{RES}") as c:
        L = sf.Get_Insulation(c.matrix(balance=True).fetch(chro), wbins)
    np.testing.assert_allclose(L, tr[chro][0], rtol=1e-11, atol=1e-11)
