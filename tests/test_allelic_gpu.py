"""Allelic specificity on the GPU: ``hh_pixel_windows`` against slices of the
dense ``fetch`` and ``hh_pairdiff_rank`` against the sorted outer difference
(csrc/allelic.hip), both with exact equality; then the three classes and
``run_Compartment`` end to end on the reference's golden fixture written as a
haplotype cooler."""
import functools

import numpy as np
import pytest

from hichap_master_amd import AllelicSpecificity as AS
from hichap_master_amd import coolio
from hichap_master_amd._lib import HipLibraryError
from tests.test_allelic_cpu import (assert_table, check_boundary_table, fixture_matrices, outer_rank,
                                    run_boundaries, run_compartments, run_loops, text_of, write_cooler)

pytestmark = pytest.mark.gpu

RES = 10000
N = 70
SIZES = [("a", 11), ("b", N), ("c", 9)]      # 'b' is queried: lo = 11, and 'c' lies behind it


@functools.lru_cache(maxsize=None)
def _table():
    """Pixel table (sorted, float counts in 1/64) of three chromosomes.  Row 0
    of 'b' stores all 70 cis pixels (> 64), row 5 none, row 6 one; 'a' and
    'b' carry trans pixels into 'b' (bin1 < lo) and out of it (bin2 >= hi)."""
    rng = np.random.default_rng(42)
    lo, hi, nb = 11, 11 + N, 11 + N + 9
    H = np.triu(rng.integers(1, 4000, (nb, nb)) * (rng.random((nb, nb)) < 0.45))
    H[lo, lo:hi] = rng.integers(1, 4000, N)
    H[lo + 5, :] = 0
    H[lo + 6, :] = 0
    H[lo + 6, lo + 31] = 77
    assert np.count_nonzero(H[lo, lo:hi]) > 64 and np.count_nonzero(H[:lo, lo:hi]) > 20
    assert np.count_nonzero(H[lo:hi, hi:]) > 20
    b1, b2 = np.nonzero(H)
    cnt = H[b1, b2] / 64.0
    for a in (b1, b2, cnt):
        a.setflags(write=False)
    return b1.astype(np.int64), b2.astype(np.int64), cnt, lo


@pytest.fixture(scope="module")
def cooler_b(tmp_path_factory):
    b1, b2, cnt, lo = _table()
    path = str(tmp_path_factory.mktemp("allelic") / "w.cool")
    coolio.create_cooler(path, {RES: ([(nm, n * RES) for nm, n in SIZES], b1, b2, cnt)})
    with coolio.Cooler(f"{path}::{RES}") as c:
        assert c.extent("b") == (lo, lo + N)
        dense = c.matrix(balance=False).fetch("b")
        rows = c.pixel_rows(lo, lo + N)
    assert dense.dtype == np.float64 and np.any(dense != np.floor(dense))
    dense.setflags(write=False)
    return dense, rows


def _slices(dense, wrow, wcol, h, w):
    return np.array([dense[r:r + h, c:c + w] for r, c in zip(wrow, wcol)]).reshape(len(wrow), h, w)


WINDOWS = [
    (1, 1, [0, 6, 31, 12, 40, 5, 69, 0, 69, 6], [0, 31, 6, 12, 3, 5, 69, 69, 0, 31]),   # on / above / below, repeats
    (20, 20, [25, 0, 50, 20, 33, 25], [25, 0, 50, 30, 28, 25]),     # straddling the diagonal; rows 0 and N - 1
    (3, 7, [0, 67, 5, 30, 67, 30], [63, 0, 2, 28, 63, 28]),
]


@pytest.mark.parametrize("h,w,wrow,wcol", WINDOWS)
def test_pixel_windows_equal_dense_slices(cooler_b, h, w, wrow, wcol):
    dense, (r1, r2, rc) = cooler_b
    b1, b2, cnt, lo = _table()
    want = _slices(dense, wrow, wcol, h, w)
    for t1, t2, tc in ((b1, b2, cnt), (r1, r2, rc)):     # the whole table; the chromosome's rows only
        got = AS.pixel_windows(t1, t2, tc, lo, N, wrow, wcol, h, w)
        assert got.dtype == np.float64 and got.shape == (len(wrow), h, w)
        assert got.tobytes() == want.tobytes()


def test_pixel_windows_many_none_and_device(cooler_b):
    import torch
    dense, _ = cooler_b
    b1, b2, cnt, lo = _table()
    rng = np.random.default_rng(3)
    wrow, wcol = rng.integers(0, N - 2, 257), rng.integers(0, N - 6, 257)
    want = _slices(dense, wrow, wcol, 3, 7)
    got = AS.pixel_windows(b1, b2, cnt, lo, N, wrow, wcol, 3, 7)
    assert got.tobytes() == want.tobytes()
    d1, d2, dc = (torch.from_numpy(np.array(a)).cuda() for a in (b1, b2, cnt))
    dev = AS.pixel_windows(d1, d2, dc, lo, N, wrow, wcol, 3, 7)
    assert dev.is_cuda and dev.cpu().numpy().tobytes() == got.tobytes()
    assert AS.pixel_windows(b1, b2, cnt, lo, N, [], [], 20, 20).shape == (0, 20, 20)
    assert tuple(AS.pixel_windows(d1, d2, dc, lo, N, [], [], 1, 1).shape) == (0, 1, 1)
    e = np.empty(0, np.int64)
    assert not AS.pixel_windows(e, e, np.empty(0), 0, 12, [0, 3], [2, 3], 2, 2).any()


def test_pixel_windows_errors(cooler_b):
    dense, _ = cooler_b
    b1, b2, cnt, lo = _table()
    for wrow, wcol, h, w in (([0, 51], [0, 0], 20, 20), ([0, 3], [0, 64], 3, 7), ([0, -1], [0, 0], 1, 1)):
        with pytest.raises(HipLibraryError, match=r"window 1 .*leaves \[0, 70\)"):
            AS.pixel_windows(b1, b2, cnt, lo, N, wrow, wcol, h, w)
    k = int(np.nonzero(b1 == lo + 20)[0][0])
    u1, u2, uc = b1.copy(), b2.copy(), cnt.copy()
    for a in (u1, u2, uc):
        a[[k, k + 1]] = a[[k + 1, k]]                   # still bin1 <= bin2 everywhere
    with pytest.raises(HipLibraryError, match="not sorted"):
        AS.pixel_windows(u1, u2, uc, lo, N, [0], [0], 1, 1)
    k = int(np.nonzero((b1 == lo + 20) & (b2 >= lo + 20))[0][0])
    l2 = b2.copy()
    l2[k] = lo + 3                                      # (lo + 20, lo + 3): below the diagonal, order kept
    assert np.all(np.diff(b1 * 1000 + l2) > 0)
    with pytest.raises(HipLibraryError, match="bin1 > bin2"):
        AS.pixel_windows(b1, l2, cnt, lo, N, [0], [0], 1, 1)
    bad = cnt.copy()
    bad[k] = np.inf
    with pytest.raises(HipLibraryError, match="non-finite count"):
        AS.pixel_windows(b1, b2, bad, lo, N, [0], [0], 1, 1)
    # the library is still usable
    got = AS.pixel_windows(b1, b2, cnt, lo, N, [0], [0], 20, 20)
    assert got.tobytes() == np.ascontiguousarray(dense[None, :20, :20]).tobytes()


def _pairdiff_case(na, nb):
    """Values m * 10 ** e (m in 1 .. 9, e in -8 .. 0, both signs): magnitudes
    from 1e-8 to 1 and ties everywhere; queries in the difference set, off
    it, below its minimum and above its maximum."""
    rng = np.random.default_rng(1000 * na + nb)

    def draw(n):
        return rng.choice([-1.0, 1.0], n) * rng.integers(1, 10, n) * 10.0 ** rng.integers(-8, 1, n)
    a, b = draw(na), draw(nb)
    inset = a[rng.integers(0, na, 40)] - b[rng.integers(0, nb, 40)]
    off = np.concatenate([inset[:20] * (1 + 1e-15), inset[:20] + 1e-9, rng.uniform(-3, 3, 20)])
    lo, hi = a.min() - b.max(), a.max() - b.min()
    q = np.concatenate([inset, off, [lo, hi, lo - 1.0, hi + 1.0]])
    return a, b, q


@pytest.mark.parametrize("na,nb", [(1, 1), (63, 65), (257, 257), (1000, 37), (3000, 3000)])
def test_pairdiff_rank_equals_sorted_outer_difference(na, nb):
    a, b, q = _pairdiff_case(na, nb)
    want = outer_rank(a, b, q)
    got = AS.pairdiff_rank(a, b, q)
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, want)
    # the minimum itself, the maximum itself, below the minimum, above the maximum
    assert got[-4] == 0 and got[-3] < na * nb and got[-2] == 0 and got[-1] == na * nb
    assert AS.pairdiff_rank(a, b, q).tobytes() == got.tobytes()
    assert AS.pairdiff_rank(a, b, []).size == 0


def test_pairdiff_rank_rejects_nan_and_takes_empty_sides():
    a, b, q = _pairdiff_case(63, 65)
    for k in range(3):
        args = [a.copy(), b.copy(), q.copy()]
        args[k][1] = np.nan
        with pytest.raises(HipLibraryError, match="non-finite"):
            AS.pairdiff_rank(*args)
    assert AS.pairdiff_rank([], b, q).tolist() == [0] * q.size
    assert AS.pairdiff_rank(a, [], q).tolist() == [0] * q.size
    np.testing.assert_array_equal(AS.pairdiff_rank(a, b, q), outer_rank(a, b, q))


# ------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def golden_cooler(golden, tmp_path_factory):
    g = golden("allelic_40k")
    path = str(tmp_path_factory.mktemp("allelic_golden") / "hap.cool")
    return g, write_cooler(path, int(g["res"]), fixture_matrices(g))


def test_three_tables_equal_reference(golden_cooler, tmp_path):
    g, cool = golden_cooler
    _, got = run_loops(g, tmp_path, cool)
    assert_table(got, text_of(g, "loop_table"), {5, 6, 7, 8, 9, 10})
    B, got = run_boundaries(g, tmp_path, cool)
    check_boundary_table(g, got)
    _, edge = run_boundaries(g, tmp_path, cool, key="boundary_edge_file")
    assert len(edge.splitlines()) == 1 + 5
    Cm, got = run_compartments(g, tmp_path)
    assert_table(got, text_of(g, "compartment_table"), {2, 3, 4, 5, 6})
    assert Cm.n_BG == Cm.results.size ** 2


def test_run_compartment_writes_the_pc_file(golden_cooler, tmp_path):
    from hichap_master_amd.StructureFind import StructureFind
    g, cool = golden_cooler
    res = int(g["res"])
    trad = tmp_path / "trad_PC.txt"
    trad.write_text(text_of(g, "pc_p"))
    files = {}
    for allelic in ("Maternal", "Paternal"):
        sf = StructureFind(cool, res, Allelic=allelic)
        out = tmp_path / allelic
        sf.run_Compartment(str(out), plot=False, Tranditional_PC_file=str(trad))
        assert [p.name for p in out.iterdir()] == [f"{allelic}_Compartment_40K.txt"]
        files[allelic] = out / f"{allelic}_Compartment_40K.txt"
        sf.Compartment(Tranditional_PC_file=str(trad))
        again = tmp_path / (allelic + "_again.txt")
        sf.OutPut_PC_To_txt(str(again))
        assert files[allelic].read_bytes() == again.read_bytes()
        names = [ln.split("\t")[0] for ln in files[allelic].read_text().splitlines()]
        assert names == ["1"] * 96 + ["2"] * 80
    Cm, got = run_compartments(g, tmp_path, files["Maternal"], files["Paternal"])
    want = outer_rank(Cm.M_candidate, Cm.P_candidate, Cm.results["diff"])
    p = np.minimum(want, Cm.n_BG - want) / max(Cm.n_BG, 1)
    np.testing.assert_array_equal(Cm.results["p_value"], p)
    assert len(got.splitlines()) == 1 + Cm.results.size
