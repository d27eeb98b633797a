"""The symmetric pixel table, the per-bin coverage and the virtual 4C on the GPU
(csrc/symtab.hip, csrc/coverage.hip, hichap_master_amd/coverage.py, DESIGN.md
§4v) against the dense restatement (tests/coverage_ref.py): the tables to the
entry, the sums exactly where every operation is exact in fp64 and within a
bound computed from the input otherwise, their bits across calls, forms, grids
and the number of viewpoints of a call, reciprocity and the partition of the
coverage by viewpoints, the argument errors, and ``run_Coverage`` /
``run_Virtual4C`` on a four-chromosome cooler through the traditional and the
haplotype path."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from hichap_master_amd import _lib, coolio, h5
from hichap_master_amd import coverage as cov
from hichap_master_amd._lib import ptr
from hichap_master_amd.StructureFind import StructureFind, py2_float_str
from tests import coverage_ref as ref
from tests import transeig_ref as tref
from tests.h5_listing import listing
from tests.knobs import tuned

pytestmark = pytest.mark.gpu

RES = 10000
HH_ERR_ARG = -1
U53 = 2.0 ** -53
PAIRS = [(0, 0), (2, 10), (1, 1), (3, 200)]      # (ignore_diags, near_bins)
ROWS = (1, 4, 5, 16)                             # hh_tune "cov_rows": the default, the ends, one that divides no genome
BIG = tref.BIG                                   # first bin of A's 130-bin chromosome
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _dev(*arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.array(a)).cuda() for a in arrays]


def _table(name, device=False, scale=1.0):
    off, b1, b2, cnt = ref.genome(name) if name in ("A", "B") else ref.degenerate(name)
    cnt = cnt * scale
    if device:
        b1, b2, cnt = _dev(b1, b2, cnt)
    return cov.SymTable(b1, b2, cnt, off)


@functools.lru_cache(maxsize=None)
def _dense(name, kind, scale=1.0):
    """(off, valid, A, stored, m): the restatement's dense A and the stored entries per row."""
    off, b1, b2, cnt = ref.genome(name)
    w, bad, use = ref.weights(name, kind)
    valid = ref.validity(off, w, use, bad)
    A, stored = ref.dense_A(b1, b2, cnt * scale, w, off, valid)
    m = stored.sum(axis=1)
    for a in (valid, A, stored, m):
        a.setflags(write=False)
    return off, valid, A, stored, m


def _bound(m, terms):
    """2 (m + 3) 2^-53 sum |terms|: a sum of m terms has m - 1 additions and every term two multiplications, on
    the GPU and as many on the dense side in another order (tests/test_transeig_gpu.py's _product_bound with the
    multiplications this value has)."""
    return 2.0 * (m + 3) * U53 * terms


# ------------------------------------------------------------------ 1. tables
@pytest.mark.parametrize("name", ["A", "B", "empty", "one_chrom", "no_diag", "all_diag"])
def test_tables_equal_the_lexsort_tables(name):
    off, b1, b2, cnt = ref.genome(name) if name in ("A", "B") else ref.degenerate(name)
    n = int(off[-1])
    want = ref.sym_tables(b1, b2, n)
    if name in ("A", "B"):
        assert b1.size % 256 and np.diff(want["rowptr_l"]).max() > 64 and np.diff(want["rowptr_u"]).max() > 64
        assert (np.diff(want["rowptr_l"]) + np.diff(want["rowptr_u"]) == 0).any()
    for device in (False, True, False, True):                              # either form, twice over
        with _table(name, device) as tab:
            assert tab.nnz == b1.size and tab.n_lower == want["src_l"].size and tab.n == n
            got = tab.tables()
        assert got["rowptr_u"].dtype == got["rowptr_l"].dtype == np.int64
        assert got["partner_l"].dtype == np.int32 and got["src_l"].dtype == np.uint32
        for key in want:
            assert np.array_equal(got[key], want[key]), key
    assert want["src_l"].size == int(np.count_nonzero(b1 < b2))
    if name == "all_diag":
        assert tab.n_lower == 0 and tab.nnz > 0


def test_a_malformed_table_returns():
    """Ids out of range and bin1 > bin2: wrong numbers are allowed, the calls must return, and whatever the lower
    table holds points inside the arrays."""
    off, b1, b2, cnt = ref.degenerate("malformed")
    n = int(off[-1])
    assert (b2 >= n).any() and (b2 < 0).any() and (b1 >= n).any() and (b1 > b2).any()
    w = ref.weights("A", "general_nan")[0]
    for device in (False, True):
        with _table("malformed", device) as tab:
            t = tab.tables()
            assert 0 <= tab.n_lower <= tab.nnz == b1.size
            assert np.all(np.diff(t["rowptr_l"]) >= 0) and t["rowptr_l"][-1] == tab.n_lower
            assert np.all((t["partner_l"] >= 0) & (t["partner_l"] < n)) and np.all(t["src_l"] < b1.size)
            S, cnt_ = tab.coverage(w, None, None, 2, 10)
            assert tuple(S.shape) == (n, 3) and tuple(cnt_.shape) == (n, 3)
            P = tab.viewpoints([(0, n), (BIG, BIG + 65), (5, 6)], w)
            assert tuple(P.shape) == (3, n)
    # the well-formed part of the lower table is what the restatement says
    want = ref.sym_tables(b1, b2, n)
    for key in ("rowptr_l", "partner_l", "src_l"):
        assert np.array_equal(t[key], want[key]), key


# ---------------------------------------------------------- 2. exact coverage
@pytest.mark.parametrize("name", ["A", "B"])
def test_exact_coverage(name):
    """Power-of-two weights, counts in 1/64: every product and sum is exact in fp64 (terms are multiples of 2^-12
    below 2^10, at most 260 of them), so S equals the dense sums whatever the order.  The weights are NaN on the
    invalid bins: they must reach nothing."""
    kind = "exact_nan"
    off, valid, A, stored, m = _dense(name, kind, 1 / 64)
    w = ref.weights(name, kind)[0]
    assert np.isnan(w[~valid]).all() and (~valid).sum() >= 5
    with _table(name, scale=1 / 64) as tab, _table(name, True, 1 / 64) as dtab:
        for ig, near in PAIRS:
            want_S, want_n = ref.coverage(A, stored, off, valid, ig, near)
            S, n = tab.coverage(w, None, None, ig, near)
            assert S.dtype == np.float64 and n.dtype == np.int64 and S.shape == n.shape == (valid.size, 3)
            assert np.array_equal(S, want_S) and np.array_equal(n, want_n), (ig, near)
            assert not S[~valid].any() and not np.signbit(S[~valid]).any() and not n[~valid].any()
            dS, dn = dtab.coverage(_dev(w)[0], None, None, ig, near)
            assert dS.is_cuda and dn.is_cuda
            assert np.array_equal(dS.cpu().numpy(), want_S) and np.array_equal(dn.cpu().numpy(), want_n)
            if (ig, near) == (2, 10) and name == "A":
                assert want_n[:, 0].any() and want_n[:, 1].any() and want_n[:, 2].any()


@pytest.mark.parametrize("name", ["A", "B"])
def test_raw_coverage_is_the_two_ended_bincount(name):
    """weight = None, integer counts, every bin valid: near + far + trans + the dropped pixels is the bincount of
    the counts over both ends (a diagonal pixel once), exactly."""
    off, b1, b2, cnt = ref.genome(name)
    n = int(off[-1])
    ch = ref.chrom_of(off)
    assert np.array_equal(cnt, np.floor(cnt))
    offd = b1 != b2
    total = np.bincount(b1, weights=cnt, minlength=n) + np.bincount(b2[offd], weights=cnt[offd], minlength=n)
    pixels = np.bincount(b1, minlength=n) + np.bincount(b2[offd], minlength=n)
    with _table(name) as tab:
        for ig, near in PAIRS:
            S, k = tab.coverage(None, None, None, ig, near)
            drop = (ch[b1] == ch[b2]) & (b2 - b1 < ig)
            d_sum = (np.bincount(b1[drop], weights=cnt[drop], minlength=n)
                     + np.bincount(b2[drop & offd], weights=cnt[drop & offd], minlength=n))
            d_pix = np.bincount(b1[drop], minlength=n) + np.bincount(b2[drop & offd], minlength=n)
            assert np.array_equal(S.sum(axis=1) + d_sum, total), (ig, near)
            assert np.array_equal(k.sum(axis=1) + d_pix, pixels), (ig, near)


# -------------------------------------------------------- 3. general weights
CASES = [("A", "nan"), ("A", "bad"), ("A", "nan_nouse"), ("B", "nan"), ("B", "bad")]


@pytest.mark.parametrize("name,kind", CASES)
def test_general_coverage(name, kind):
    kind = "general_" + kind
    off, valid, A, stored, m = _dense(name, kind)
    w, bad, use = ref.weights(name, kind)
    with _table(name) as tab:
        for ig, near in PAIRS:
            want_S, want_n = ref.coverage(A, stored, off, valid, ig, near)
            bound = _bound(m[:, None], ref.abs_terms(A, off, ig, near))
            S, n = tab.coverage(w, use, bad, ig, near)
            err = np.abs(S - want_S)
            print(f"{name} {kind} {(ig, near)}: worst error / bound "
                  f"{np.max(err[bound > 0] / bound[bound > 0]):.3g}, longest row {m.max()}")
            assert np.array_equal(n, want_n) and np.all(err <= bound)
    if kind.endswith("nouse"):
        assert not S[ref.chrom_of(off) == 3].any() and (use == 0).sum() == 1


# -------------------------------------------------------------------- 4. bits
@pytest.mark.parametrize("name", ["A", "B"])
def test_coverage_bits(name):
    w, _, _ = ref.weights(name, "general_nan")
    wb, bad, _ = ref.weights(name, "general_bad")
    assert np.array_equal(np.isnan(w), bad != 0) and np.array_equal(w[bad == 0], wb[bad == 0])
    C = len(ref.genome(name)[0]) - 1
    with _table(name) as tab, _table(name, True) as dtab:
        S, n = tab.coverage(w, None, None, 2, 10)
        ref_bits = (S.tobytes(), n.tobytes())

        def same(got):
            return (np.asarray(got[0]).tobytes(), np.asarray(got[1]).tobytes()) == ref_bits

        assert same(tab.coverage(w, None, None, 2, 10))                                # two calls
        dS, dn = dtab.coverage(_dev(w)[0], None, None, 2, 10)                          # the device form
        assert same((dS.cpu().numpy(), dn.cpu().numpy()))
        for rows in ROWS:                                                              # the grid regroups no sum
            with tuned(cov_rows=rows):
                assert same(tab.coverage(w, None, None, 2, 10)), rows
        assert same(tab.coverage(w, np.ones(C, np.uint8), None, 2, 10))                # use = None is all ones
        assert same(tab.coverage(wb, None, bad, 2, 10))                                # bad marks what NaN marked


# -------------------------------------------------------------- 5. viewpoints
def _views_A():
    n = int(ref.genome("A")[0][-1])
    return [(BIG + 7, BIG + 8), (BIG + 20, BIG + 83), (BIG + 20, BIG + 84), (BIG + 20, BIG + 85), (BIG, BIG + 130),
            (BIG + 130, BIG + 131),                 # the 1-bin chromosome
            (0, 5), (n - 11, n),                    # from bin 0, to n_bins
            (BIG + 90, BIG + 92),                   # invalid bins only
            (BIG + 125, BIG + 140)]                 # across two chromosome ends (C call only)


@pytest.mark.parametrize("ig", [0, 2])
def test_exact_viewpoints(ig):
    kind = "exact_nan"
    off, valid, A, stored, m = _dense("A", kind, 1 / 64)
    w = ref.weights("A", kind)[0]
    views = _views_A()
    assert [hi - lo for lo, hi in views[:5]] == [1, 63, 64, 65, 130] and not valid[BIG + 90:BIG + 92].any()
    want = np.stack([ref.viewpoint(A, off, ig, lo, hi) for lo, hi in views])
    with _table("A", scale=1 / 64) as tab, _table("A", True, 1 / 64) as dtab:
        P = tab.viewpoints(views, w, None, None, ig)
        assert P.dtype == np.float64 and P.shape == (len(views), valid.size)
        for c in range(len(views)):
            assert np.array_equal(P[c], want[c]), views[c]
        assert not P[8].any() and not P[:, ~valid].any() and not np.signbit(P).any()
        dP = dtab.viewpoints(views, _dev(w)[0], None, None, ig)
        assert dP.is_cuda and np.array_equal(dP.cpu().numpy(), want)
    assert want[4].any() and want[5].any() and want[9].any()


def test_viewpoint_bits_do_not_depend_on_the_call():
    """Column c of a K = 64 call has the bits of the K = 1 call; 70 viewpoints go in two calls."""
    w = ref.weights("A", "general_nan")[0]
    rng = np.random.default_rng(21)
    n = int(ref.genome("A")[0][-1])
    lo = rng.integers(0, n - 1, 70)
    views = [(int(a), int(min(n, a + 1 + rng.integers(0, 90)))) for a in lo]
    with _table("A") as tab, _table("A", True) as dtab:
        P = tab.viewpoints(views[:64], w)
        assert P.shape == (64, n)
        for c in (0, 1, 17, 63):
            assert tab.viewpoints([views[c]], w).tobytes() == P[c:c + 1].tobytes(), c
        assert tab.viewpoints(views[:64], w).tobytes() == P.tobytes()                  # two calls
        assert tab.viewpoints(views[5:9], w).tobytes() == P[5:9].tobytes()
        P70 = tab.viewpoints(views, w)
        assert P70.shape == (70, n) and P70[:64].tobytes() == P.tobytes()
        assert tab.viewpoints(views[64:], w).tobytes() == P70[64:].tobytes()
        assert dtab.viewpoints(views[:64], _dev(w)[0]).cpu().numpy().tobytes() == P.tobytes()   # the device form
        assert tab.viewpoints([], w).shape == (0, n)


def test_viewpoint_reciprocity():
    """P_{x}[y] and P_{y}[x] are the same bits: both are the one term v(min, max), general weights."""
    off = ref.genome("A")[0]
    w = ref.weights("A", "general_nan")[0]
    last = np.arange(int(off[5]), int(off[6]))                                         # the 40-bin chromosome
    other = np.arange(int(off[3]), int(off[4]))[::3][:24]                              # 24 bins of the 70-bin one
    bins = np.concatenate([last, other])
    assert bins.size == 64
    with _table("A") as tab:
        P = tab.viewpoints([(int(x), int(x) + 1) for x in bins], w, None, None, 0)
    sub = P[:, bins]
    assert sub.tobytes() == np.ascontiguousarray(sub.T).tobytes()
    assert np.count_nonzero(sub[:40, :40]) > 700 and np.count_nonzero(sub[:40, 40:]) > 300


def test_viewpoints_tile_the_coverage():
    """Exact case: the viewpoints that tile the genome bin by bin add up to S.sum(1) of a coverage call with
    near_bins = 0 (A is symmetric)."""
    kind = "exact_nan"
    for name in ("A", "B"):
        w = ref.weights(name, kind)[0]
        n = int(ref.genome(name)[0][-1])
        with _table(name, scale=1 / 64) as tab:
            for ig in (0, 2):
                P = tab.viewpoints([(x, x + 1) for x in range(n)], w, None, None, ig)
                S, _ = tab.coverage(w, None, None, ig, 0)
                assert P.shape == (n, n) and np.array_equal(P.sum(axis=0), S.sum(axis=1)), (name, ig)
                assert np.array_equal(P, P.T)


@pytest.mark.parametrize("name,kind", [("A", "nan"), ("A", "bad_nouse"), ("B", "bad")])
def test_general_viewpoints(name, kind):
    kind = "general_" + kind
    off, valid, A, stored, m = _dense(name, kind)
    w, bad, use = ref.weights(name, kind)
    n = valid.size
    views = _views_A() if name == "A" else [(0, 1), (3, 70), (100, n - 1), (0, n)]
    keep = ~ref.class_masks(off, 2, 0)["dropped"]
    with _table(name) as tab:
        P = tab.viewpoints(views, w, use, bad, 2)
    for c, (lo, hi) in enumerate(views):
        want = ref.viewpoint(A, off, 2, lo, hi)
        bound = _bound(hi - lo, (np.abs(A) * keep)[lo:hi].sum(axis=0))
        err = np.abs(P[c] - want)
        assert np.all(err <= bound), (lo, hi)


# ------------------------------------------------------------------ 6. errors
def test_argument_errors_leave_outputs_untouched():
    off, b1, b2, cnt = ref.genome("A")
    w = ref.weights("A", "exact_nan")[0]
    n, C = int(off[-1]), len(off) - 1
    lib = _lib.load()
    h = ctypes.c_void_p()

    def create(off_=off, C_=C, bin1=b1, nnz=b1.size):
        return lib.hh_symtab_create(ptr(bin1), ptr(b2), ptr(cnt), nnz, ptr(off_), C_, 0, None, ctypes.byref(h))

    assert create(C_=0) == HH_ERR_ARG and create(off_=np.arange(514, dtype=np.int64), C_=513) == HH_ERR_ARG
    assert b"C outside" in lib.hh_last_error()
    flat = off.copy()
    flat[3] = flat[2]
    assert create(off_=flat) == HH_ERR_ARG and b"ascending" in lib.hh_last_error()
    assert create(off_=off + 1) == HH_ERR_ARG and b"start at 0" in lib.hh_last_error()
    assert create(bin1=None) == HH_ERR_ARG and b"null pixel arrays" in lib.hh_last_error()
    assert create(off_=np.array([0, 2 ** 31], np.int64), C_=1, nnz=0) == HH_ERR_ARG and b"2^31" in lib.hh_last_error()
    assert create(nnz=2 ** 32) == HH_ERR_ARG and b"2^32" in lib.hh_last_error()
    assert create(nnz=-1) == HH_ERR_ARG
    assert h.value is None
    assert create() == 0 and h.value
    S, k = np.full((n, 3), -7.5), np.full((n, 3), -7, np.int64)

    def coverage(h_=h, n_weight=n, ig=2, near=10, S_=S, k_=k, w_=w, on_device=0):
        return lib.hh_symtab_coverage(h_, ptr(w_), n_weight, None, None, ig, near, ptr(S_), ptr(k_), on_device, None)

    assert coverage(h_=None) == HH_ERR_ARG and b"null handle" in lib.hh_last_error()
    assert coverage(ig=-1) == HH_ERR_ARG and b"ignore_diags" in lib.hh_last_error()
    assert coverage(near=-1) == HH_ERR_ARG and b"near_bins" in lib.hh_last_error()
    assert coverage(n_weight=n - 1) == HH_ERR_ARG and b"weights do not cover" in lib.hh_last_error()
    assert coverage(S_=None) == HH_ERR_ARG and coverage(k_=None) == HH_ERR_ARG and b"null outputs" in lib.hh_last_error()
    assert np.all(S == -7.5) and np.all(k == -7)
    import torch
    tS, tk = torch.full((n, 3), -7.5, dtype=torch.float64).cuda(), torch.full((n, 3), -7, dtype=torch.int64).cuda()
    assert coverage(ig=-3, S_=tS, k_=tk, w_=_dev(w)[0], on_device=1) == HH_ERR_ARG
    assert bool((tS == -7.5).all()) and bool((tk == -7).all())
    P = np.full((3, n), -7.5)

    def views(lo=(0, 5, 9), hi=(1, 9, 20), K=3, h_=h, n_weight=n, ig=2, P_=P):
        lo_, hi_ = (None if a is None else np.array(a, np.int64) for a in (lo, hi))
        return lib.hh_symtab_viewpoints(h_, ptr(w), n_weight, None, None, ig, ptr(lo_), ptr(hi_), K, ptr(P_), 0, None)

    assert views(h_=None) == HH_ERR_ARG and views(ig=-1) == HH_ERR_ARG and views(n_weight=3) == HH_ERR_ARG
    assert views(K=0) == HH_ERR_ARG and views(lo=[0] * 65, hi=[1] * 65, K=65) == HH_ERR_ARG
    assert b"K outside" in lib.hh_last_error()
    assert views(lo=None) == HH_ERR_ARG and views(hi=None) == HH_ERR_ARG and views(P_=None) == HH_ERR_ARG
    for lo, hi in (((0, -1, 9), (1, 9, 20)), ((0, 5, 9), (1, 9, n + 1)), ((0, 9, 9), (1, 9, 20)), ((0, 5, 20), (1, 9, 9))):
        assert views(lo=lo, hi=hi) == HH_ERR_ARG, (lo, hi)
        assert b"not an interval" in lib.hh_last_error()
    assert np.all(P == -7.5)
    assert views() == 0 and coverage() == 0 and np.isfinite(P).all() and np.all(k >= 0)
    assert lib.hh_symtab_free(h) == 0 and lib.hh_symtab_free(None) == 0
    # a closed table is refused before the library sees the pointer
    tab = _table("A")
    tab.close()
    for use_it in (lambda: tab.coverage(), lambda: tab.viewpoints([(0, 1)]), lambda: tab.tables()):
        with pytest.raises(ValueError, match="closed"):
            use_it()
    with _table("A") as tab:
        with pytest.raises(ValueError, match="one entry per bin"):
            tab.coverage(None, None, np.zeros(n - 1, np.uint8))
        with pytest.raises(ValueError, match="one entry per chromosome"):
            tab.coverage(None, np.ones(C + 1, np.uint8))
        with pytest.raises(_lib.HipLibraryError, match="not an interval"):
            tab.viewpoints([(3, 3)])


# ------------------------------------------------- 7. run_Coverage / run_Virtual4C
NAMES = ["chr1", "chr2", "chr3", "chr4"]
VIEWS = {"prom": ("chr2", 55000, 85000), "snp": ("chr4", 120000, 120001), "whole": ("chr3", 0, 64 * RES)}
VIEW_BINS = [(55, 59), (163, 164), (87, 151)]


def _parsed(fil):
    return [ln.rstrip("\n").split("\t") for ln in open(fil)]


def _check_coverage_file(r, shown, off, sel):
    """The file against the arrays returned, entry by entry as written; then read back."""
    rows = _parsed(r["file"])
    assert rows[0] == list(cov.COVERAGE_COLUMNS)
    want = []
    for p in sel:
        for x in range(int(off[p]), int(off[p + 1])):
            i = x - int(off[p])
            want.append([shown[p], str(i * RES), str((i + 1) * RES), str(int(r["valid"][x])), str(int(r["n_cis"][x])),
                         str(int(r["n_trans"][x]))] + [py2_float_str(r[k][x]) for k in cov.COVERAGE_COLUMNS[6:]])
    assert rows[1:] == want
    back = cov.read_coverage(r["file"])
    bins = np.concatenate([np.arange(int(off[p]), int(off[p + 1])) for p in sel])
    for k in cov.COVERAGE_COLUMNS[6:]:
        assert np.array_equal(back[k], [float(py2_float_str(v)) for v in r[k][bins]], equal_nan=True), k
    return back, bins


H5 = os.environ.get("HDF5_PREFIX", "/opt/conda")
HAVE_H5 = all(os.path.exists(os.path.join(H5, q)) for q in ("include/hdf5.h", "lib/libhdf5.so"))


@pytest.mark.skipif(not HAVE_H5 or shutil.which("gcc") is None, reason="libhdf5 or gcc absent")
def test_stored_coverage_columns_are_listed_by_libhdf5(tmp_path):
    """After run_Coverage(store=True), once and again, libhdf5 lists the cooler exactly as h5.py does (the listing
    tool of tests/golden/make_h5_fixtures.c, as tests/test_construction.py uses it)."""
    off, b1, b2, count = ref.planted()
    path = str(tmp_path / "stored.cool")
    coolio.create_cooler(path, {RES: ([(x, L * RES) for x, L in zip(NAMES, ref.PLANTED)], b1, b2, count)})
    h5.append_dataset(path, f"{RES}/bins", "weight", 2.0 ** -(np.arange(int(off[-1])) % 3), {"ignore_diags": 2})
    exe = str(tmp_path / "make_h5_fixtures")
    subprocess.run(["gcc", "-O2", "-I" + os.path.join(H5, "include"), "-o", exe,
                    os.path.join(GOLDEN, "make_h5_fixtures.c"), "-L" + os.path.join(H5, "lib"),
                    "-Wl,-rpath," + os.path.join(H5, "lib"), "-lhdf5"], check=True)
    sf = StructureFind(path, Res=RES)
    for ig in (2, 0):                                                             # the second run replaces the columns
        sf.run_Coverage(str(tmp_path / "cov"), ignore_diags=ig, store=True)
        r = subprocess.run([exe, "dump", path], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
        mine = listing(path)
        assert sorted(r.stdout.splitlines()) == mine
        assert sum(ln.startswith(f"D /{RES}/bins/cov_") for ln in mine) == 2


def test_run_coverage_and_virtual4c_traditional(tmp_path):
    off, b1, b2, count = ref.planted()
    n = int(off[-1])
    path = str(tmp_path / "trad.cool")
    coolio.create_cooler(path, {RES: ([(x, L * RES) for x, L in zip(NAMES, ref.PLANTED)], b1, b2, count)})
    uri = f"{path}::{RES}"
    out = str(tmp_path / "cov")
    with pytest.raises(ValueError, match="balance it first"):
        StructureFind(path, Res=RES).run_Coverage(out)
    w, st = coolio.balance_cooler(uri, ignore_diags=2, min_nnz=5, mad_max=0)
    assert np.array_equal(np.nonzero(~np.isfinite(w))[0], [7, 60, 150])           # the three empty bins
    sf = StructureFind(path, Res=RES)
    # how flat the balanced marginal is at the ICE's own ignore_diags: recorded, not asserted
    flat = sf.run_Coverage(str(tmp_path / "flat"), ignore_diags=2, near_bp=120000)
    print(f"balanced cooler (ICE ignore_diags = 2, tol 1e-5, {st['iters']} iterations, converged {st['converged']}): "
          f"max |cov_tot - 1| over the valid bins = {np.abs(flat['cov_tot'][np.isfinite(w)] - 1).max():.3g}")
    w = w.copy()
    w[[20, 99, 100, 171]] = np.nan                                                # invalid bins that hold pixels
    h5.append_dataset(path, f"{RES}/bins", "weight", w)
    valid = np.isfinite(w)
    sf = StructureFind(path, Res=RES)
    r = sf.run_Coverage(out, ignore_diags=2, near_bp=120000, store=True)
    assert r is sf.Coverage_dict and r["near_bins"] == 12 and r["selected"] == [0, 1, 2, 3]
    assert np.array_equal(r["valid"] != 0, valid) and r["nnz"] == b1.size and os.listdir(out) == [os.path.basename(r["file"])]
    back, bins = _check_coverage_file(r, NAMES, off, [0, 1, 2, 3])
    # the raw call masks nothing and is exact: integers
    every = np.ones(n, bool)
    A0, stored0 = ref.dense_A(b1, b2, count.astype(np.float64), None, off, every)
    S0, n0 = ref.coverage(A0, stored0, off, every, 2, 12)
    assert np.array_equal(r["S_raw"], S0) and np.array_equal(r["n"], n0)
    assert np.array_equal(back["n_cis"], n0[:, 0] + n0[:, 1]) and np.array_equal(back["n_trans"], n0[:, 2])
    assert np.array_equal(back["cov_cis_raw"], S0[:, 0] + S0[:, 1]) and np.array_equal(back["cov_tot_raw"], S0.sum(axis=1))
    # the balanced call against the restatement on the same table and weights: within the rounding bound of
    # test 3, not to the bit (general ICE weights, summed in another order than the dense side); the raw columns
    # above and the haplotype path, whose sums are exact, are compared exactly
    A, stored = ref.dense_A(b1, b2, count.astype(np.float64), w, off, valid)
    S, _ = ref.coverage(A, stored, off, valid, 2, 12)
    bound = _bound(stored.sum(axis=1)[:, None], ref.abs_terms(A, off, 2, 12))
    assert np.all(np.abs(r["S"] - S) <= bound) and not r["S"][~valid].any()
    t = ref.tracks(r["S"], valid)
    for k in ("cov_cis", "cov_tot", "ICF", "DLR"):
        assert np.array_equal(r[k], t[k], equal_nan=True), k
    assert np.isnan(r["ICF"][~valid]).all() and np.isfinite(r["ICF"][valid]).all()
    # store=True: the two int64 columns, cooltools' names; the file still lists cleanly (by libhdf5: the test above)
    with coolio.Cooler(uri) as c:
        for key, want in (("cov_cis_raw", S0[:, 0] + S0[:, 1]), ("cov_tot_raw", S0.sum(axis=1))):
            col = c._g("bins")[key].read()
            assert col.dtype == np.int64 and np.array_equal(col, want.astype(np.int64)), key
        np.testing.assert_array_equal(c.weights(), w)
    assert sum(ln.startswith(f"D /{RES}/bins/cov_") for ln in listing(path)) == 2
    # a second run replaces the columns (ignore_diags = 0: other numbers under the same names)
    r2 = sf.run_Coverage(out, ignore_diags=0, near_bp=120000, store=True)
    S00, _ = ref.coverage(A0, stored0, off, every, 0, 12)
    with coolio.Cooler(uri) as c:
        assert np.array_equal(c._g("bins")["cov_tot_raw"].read(), S00.sum(axis=1).astype(np.int64))
        assert sorted(c._g("bins").keys()).count("cov_tot_raw") == 1
    assert np.array_equal(r2["S_raw"], S00) and (S00.sum(axis=1) > S0.sum(axis=1)).any()
    assert sum(ln.startswith(f"D /{RES}/bins/cov_") for ln in listing(path)) == 2
    with pytest.raises(ValueError, match="integer counts"):
        fpath = str(tmp_path / "frac.cool")
        coolio.create_cooler(fpath, {RES: ([(x, L * RES) for x, L in zip(NAMES, ref.PLANTED)], b1, b2, count + 0.5)})
        h5.append_dataset(fpath, f"{RES}/bins", "weight", w)
        StructureFind(fpath, Res=RES).run_Coverage(str(tmp_path / "frac"), store=True)
    # virtual 4C of three viewpoints on the same cooler
    vout = str(tmp_path / "v4c")
    v = sf.run_Virtual4C(vout, VIEWS, ignore_diags=2)
    assert v is sf.Virtual4C_dict and [x[2:4] for x in v["viewpoints"]] == VIEW_BINS
    chrom, start, end, heads, P = cov.read_virtual4c(v["file"])
    assert heads == ["prom|chr2:55000-85000", "snp|chr4:120000-120001", f"whole|chr3:0-{64 * RES}"]
    assert chrom.tolist() == [NAMES[q] for q in ref.chrom_of(off)] and np.array_equal(end - start, np.full(n, RES))
    keep = ~ref.class_masks(off, 2, 0)["dropped"]
    for c, (lo, hi) in enumerate(VIEW_BINS):
        want = ref.viewpoint(A, off, 2, lo, hi)
        assert np.all(np.abs(v["P"][c] - want) <= _bound(hi - lo, (np.abs(A) * keep)[lo:hi].sum(axis=0))), c
        assert np.array_equal(P[c], [float(py2_float_str(x)) for x in v["P"][c]])
    fil = tmp_path / "views.bed"
    fil.write_text("".join(f"{ch}\t{s}\t{e}\t{nm}\n" for nm, (ch, s, e) in VIEWS.items()))
    v2 = sf.run_Virtual4C(vout, str(fil), ignore_diags=2)
    assert v2["P"].tobytes() == v["P"].tobytes()
    with pytest.raises(ValueError, match="crosses the end"):
        sf.run_Virtual4C(vout, {"x": ("chr2", 360000, 380000)})
    with pytest.raises(ValueError, match="unknown chromosome"):
        sf.run_Virtual4C(vout, {"x": ("chr9", 0, 10)})


def test_run_coverage_and_virtual4c_haplotype(tmp_path):
    """The same four chromosomes as the maternal haplotype (raw counts), gap lists as invalid bins, next to two
    paternal chromosomes whose pixels must not be read.  Integer counts and no weights: everything is exact."""
    off, b1, b2, count = ref.planted()
    n = int(off[-1])
    sizes = ref.PLANTED + (13, 8)
    off2 = ref.offsets(sizes)
    n2 = int(off2[-1])
    rng = np.random.default_rng(9)
    extra = np.array([(a, b) for a in range(n2) for b in range(max(a, n), n2) if rng.random() < 0.3])
    t1, t2 = np.concatenate([b1, extra[:, 0]]), np.concatenate([b2, extra[:, 1]])
    tc = np.concatenate([count, rng.integers(1, 9, len(extra))])
    o = np.lexsort((t2, t1))
    t1, t2, tc = t1[o], t2[o], tc[o]
    names = ["Ma", "Mb", "Mc", "Md", "Pa", "Pb"]
    path = str(tmp_path / "hap.cool")
    coolio.create_cooler(path, {RES: ([(x, L * RES) for x, L in zip(names, sizes)], t1, t2, tc)})
    gap = np.array([0, 49, 60, 61, 150, 171])
    gaps = {x: gap[(gap >= off2[q]) & (gap < off2[q + 1])] - off2[q] for q, x in enumerate(names)}
    sf = StructureFind(path, Res=RES, Allelic="Maternal", GapFile={str(RES): gaps})
    out = str(tmp_path / "hap")
    r = sf.run_Coverage(out, ignore_diags=1, near_bp=80000)
    valid = np.zeros(n2, bool)
    valid[:n] = True
    valid[gap] = False
    assert r["selected"] == [0, 1, 2, 3] and np.array_equal(r["valid"] != 0, valid) and r["near_bins"] == 8
    assert r["S"] is r["S_raw"]
    shown = [x[1:] for x in names]
    back, bins = _check_coverage_file(r, shown, off2, [0, 1, 2, 3])                # names without the prefix
    assert set(back["chrom"]) == {"a", "b", "c", "d"} and bins.size == n
    A, stored = ref.dense_A(t1, t2, tc.astype(np.float64), None, off2, valid)      # the paternal pixels dropped
    S, k = ref.coverage(A, stored, off2, valid, 1, 8)
    assert np.array_equal(r["S"], S) and np.array_equal(r["n"], k) and not r["S"][n:].any()
    t = ref.tracks(S, valid)
    for key, want in (("cov_cis_raw", t["cov_cis"]), ("cov_tot_raw", t["cov_tot"]), ("cov_cis", t["cov_cis"]),
                      ("cov_tot", t["cov_tot"]), ("ICF", t["ICF"]), ("DLR", t["DLR"])):
        assert np.array_equal(back[key], [float(py2_float_str(x)) for x in want[bins]], equal_nan=True), key
    assert np.array_equal(back["n_cis"], (k[:, 0] + k[:, 1])[bins]) and np.array_equal(back["n_trans"], k[bins, 2])
    with pytest.raises(ValueError, match="traditional data"):
        sf.run_Coverage(out, store=True)
    # a bare chromosome name is the maternal copy
    vout = str(tmp_path / "hv")
    v = sf.run_Virtual4C(vout, {"prom": ("b", 55000, 85000), "full": ("Md", 0, 21 * RES)}, ignore_diags=1)
    assert [x[1:4] for x in v["viewpoints"]] == [("Mb", 55, 59), ("Md", 151, 172)]
    chrom, start, end, heads, P = cov.read_virtual4c(v["file"])
    assert heads == ["prom|b:55000-85000", f"full|d:0-{21 * RES}"] and P.shape == (2, n)
    for c, (lo, hi) in enumerate([(55, 59), (151, 172)]):
        want = ref.viewpoint(A, off2, 1, lo, hi)
        assert np.array_equal(v["P"][c], want) and np.array_equal(P[c], [float(py2_float_str(x)) for x in want[:n]])
    assert not v["P"][:, n:].any()
    with pytest.raises(ValueError, match="does not read"):
        sf.run_Virtual4C(vout, {"x": ("Pa", 0, 10000)})
