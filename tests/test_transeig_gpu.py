"""The symmetric trans operator and the trans eigenvectors on the GPU
(csrc/transeig.hip, hichap_master_amd/transeig.py) against the
dense restatement (tests/transeig_ref.py): the two row-compressed tables to the
bit, the product exactly where every operation is exact in fp64 and within a
bound computed from the input otherwise, its bits across calls, forms and k,
the normalisation, the eigenpairs within residual / Davis-Kahan bounds, the
argument errors, and ``run_TransEig`` on a planted four-chromosome cooler
through the traditional and the haplotype path."""
import ctypes
import functools
import os

import numpy as np
import pytest

from hichap_master_amd import _lib, coolio, h5
from hichap_master_amd import transeig as te
from hichap_master_amd._lib import ptr
from hichap_master_amd.StructureFind import StructureFind, py2_float_str
from tests import saddle_ref
from tests import trans_ref
from tests import transeig_ref as ref
from tests.knobs import tuned
from tests.test_transeig_cpu import check_eigenpairs

pytestmark = pytest.mark.gpu

RES = 10000
HH_ERR_ARG = -1
U53 = 2.0 ** -53
CASES = [("A", "nan"), ("A", "bad"), ("A", "nan_nouse"), ("B", "nan"), ("B", "bad")]
ROWS = (1, 4, 5, 16)                 # hh_tune "teig_rows": the default, the ends, one that divides no genome


def _dev(*arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.array(a)).cuda() for a in arrays]


def _inputs(name, kind, junk_seed=0, scale=1.0):
    off, b1, b2, cnt = ref.genome(name, junk_seed)
    w, bad, use = ref.weights(name, kind)
    return off, b1, b2, cnt * scale, w, bad, use


def _op(name, kind, device=False, junk_seed=0, scale=1.0):
    off, b1, b2, cnt, w, bad, use = _inputs(name, kind, junk_seed, scale)
    if device:
        b1, b2, cnt, w, bad = _dev(b1, b2, cnt, w, bad)
    return te.TransOperator(b1, b2, cnt, w, off, use, bad)


@functools.lru_cache(maxsize=None)
def _dense(name, kind, scale=1.0):
    """(valid, T, m): the restatement's dense T and the stored entries per row."""
    off, b1, b2, cnt, w, bad, use = _inputs(name, kind, 0, scale)
    valid = ref.validity(off, w, use, bad)
    T = ref.dense_T(b1, b2, cnt, w, off, valid)
    k = ref.kept(b1, b2, off, valid)
    m = np.bincount(b1[k], minlength=valid.size) + np.bincount(b2[k], minlength=valid.size)
    for a in (valid, T, m):
        a.setflags(write=False)
    return valid, T, m


def _product_bound(T, m, d, X):
    """2 (m_i + 3) 2^-53 sum_j |d_i T_ij d_j x_j|: m_i - 1 additions and three multiplications per term on
    the GPU, as many on the dense side, in another order (§4m's bound with the two extra multiplications)."""
    return 2.0 * (m[:, None] + 3) * U53 * (np.abs(T * np.outer(d, d)) @ np.abs(X))


# ------------------------------------------------------------------ 1. tables
@pytest.mark.parametrize("name,kind", CASES)
def test_tables_equal_the_lexsort_tables(name, kind):
    off, b1, b2, cnt, w, bad, use = _inputs(name, kind)
    valid = ref.validity(off, w, use, bad)
    want = ref.tables(b1, b2, cnt, w, off, valid)
    assert want["upper"][1].size > 2000 and np.diff(want["lower"][0]).max() > (64 if name == "A" else 100)
    for device in (False, True, False, True):                              # either form, twice over
        with _op(name, kind, device) as op:
            assert np.array_equal(op.valid != 0, valid) and op.nnz == want["upper"][1].size
            got = op.tables()
        for which in ("upper", "lower"):
            rp, p, v = got[which]
            assert rp.dtype == np.int64 and p.dtype == np.int32 and v.dtype == np.float64
            assert np.array_equal(rp, want[which][0]), which
            assert np.array_equal(p, want[which][1]), which
            assert v.tobytes() == want[which][2].tobytes(), which
    if kind.endswith("nouse"):
        ch = ref.chrom_of(off)
        assert not np.diff(got["upper"][0])[ch == 3].any() and not np.isin(got["upper"][1], np.nonzero(ch == 3)[0]).any()


# ----------------------------------------------------------- 2. exact product
@pytest.mark.parametrize("name", ["A", "B"])
def test_exact_product(name):
    """Power-of-two weights and d, counts in 1/64, integer X in [-7, 7]: every product and sum is exact in fp64
    (terms are multiples of 2^-16 below 2^13, at most 260 of them), so the product equals the dense one.  d and X
    hold NaN on the invalid bins: nothing may read them there."""
    kind = "exact_nan"
    valid, T, m = _dense(name, kind, 1 / 64)
    n = valid.size
    rng = np.random.default_rng(11)
    d0 = np.where(valid, 2.0 ** rng.integers(-2, 2, n), 0.0)
    X0 = np.where(valid[:, None], rng.integers(-7, 8, (n, 8)).astype(np.float64), 0.0)
    want = (T * np.outer(d0, d0)) @ X0
    want_plain = T @ X0
    d, X = np.where(valid, d0, np.nan), np.where(valid[:, None], X0, np.nan)
    with _op(name, kind, scale=1 / 64) as op:
        for rows in ROWS:
            with tuned(teig_rows=rows):
                for k in (1, 3, 8):
                    got = op.apply(np.ascontiguousarray(X[:, :k]), d)
                    assert got.shape == (n, k) and np.array_equal(got, want[:, :k]), (rows, k)
                assert np.array_equal(op.apply(X[:, 0].copy(), d), want[:, 0])          # a 1-D X
                assert np.array_equal(op.apply(X), want_plain)                          # d = None: all ones
        tX, td = _dev(X, d)
        got = op.apply(tX, td)
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
        wide = np.concatenate([X, X[:, :3]], axis=1)                                    # 11 columns: two calls
        assert np.array_equal(op.apply(wide, d), np.concatenate([want, want[:, :3]], axis=1))


# --------------------------------------------------------- 3. general product
@pytest.mark.parametrize("name,kind", CASES)
def test_general_product(name, kind):
    kind = "general_" + kind
    valid, T, m = _dense(name, kind)
    n = valid.size
    rng = np.random.default_rng(12)
    d = np.where(valid, rng.uniform(0.5, 2.0, n), 0.0)
    X = rng.standard_normal((n, 8))
    want = (T * np.outer(d, d)) @ np.where(valid[:, None], X, 0.0)
    bound = _product_bound(T, m, d, np.where(valid[:, None], X, 0.0))
    with _op(name, kind) as op:
        got = op.apply(X, d)
    err = np.abs(got - want)
    print(f"{name} {kind}: worst error / bound {np.max(err[bound > 0] / bound[bound > 0]):.3g}, longest row {m.max()}")
    assert np.all(err <= bound)


# -------------------------------------------------------------------- 4. bits
@pytest.mark.parametrize("name", ["A", "B"])
def test_bits(name):
    kind = "general_nan"
    valid, T, m = _dense(name, kind)
    n = valid.size
    rng = np.random.default_rng(13)
    d = rng.uniform(0.5, 2.0, n)
    X = rng.standard_normal((n, 8))
    with _op(name, kind) as op, _op(name, kind, device=True) as dop, _op(name, kind, junk_seed=1) as jop:
        Y = op.apply(X, d)
        assert op.apply(X, d).tobytes() == Y.tobytes()                                 # two calls
        assert dop.apply(X, d).tobytes() == Y.tobytes()                                # tables built on the device
        tX, td = _dev(X, d)
        assert dop.apply(tX, td).cpu().numpy().tobytes() == Y.tobytes()                # the device form of the call
        assert jop.apply(X, d).tobytes() == Y.tobytes()                                # other cis junk: no bit moves
        for c in range(8):                                                             # column c alone = one of 8
            assert op.apply(np.ascontiguousarray(X[:, c:c + 1]), d).tobytes() == Y[:, c:c + 1].tobytes(), c
        assert op.apply(np.ascontiguousarray(X[:, 2:5]), d).tobytes() == np.ascontiguousarray(Y[:, 2:5]).tobytes()
        for rows in ROWS:                                                              # the grid regroups no sum
            with tuned(teig_rows=rows):
                assert op.apply(X, d).tobytes() == Y.tobytes()
    assert (~valid).sum() >= 5 and not Y[~valid].any() and not np.signbit(Y[~valid]).any()   # +0.0


# ----------------------------------------------------------- 5. normalisation
@pytest.mark.parametrize("name,kind", CASES)
@pytest.mark.parametrize("tol", [1e-6, 1e-9])
def test_normalisation(name, kind, tol):
    R = ref.solved(name, kind, tol)
    with _op(name, kind) as op:
        nrm = te.trans_normalise(op, tol)
        assert op.d is nrm["d"] or np.array_equal(op.d, nrm["d"])
    d, T = nrm["d"], R["T"]
    assert nrm["converged"] and nrm["deviation"] < tol
    dropped = [ref.EMPTY_ROW[name], ref.NO_TRANS[name]]
    assert R["valid0"][dropped].all() and not nrm["valid"][dropped].any() and not d[dropped].any()
    assert np.array_equal(nrm["valid"], R["valid"]) and np.all(d[R["valid"]] > 0) and not d[~R["valid"]].any()
    # ntp was recomputed: a partner's target is one lower per dropped bin outside its chromosome
    ch = ref.chrom_of(R["off"])
    before = ref.partners(R["off"], R["valid0"])
    lower = np.array([sum(1 for x in dropped if ch[x] != ch[i]) for i in range(d.size)])
    assert np.array_equal(nrm["ntp"], np.where(R["valid"], before - lower, 0)) and lower.max() == 2
    r = (d * (T @ d))[R["valid"]] / nrm["ntp"][R["valid"]]                 # the restatement's dense row means
    print(f"{name} {kind} tol {tol}: {nrm['iterations']} iterations (restatement {R['iterations']}), deviation "
          f"{nrm['deviation']:.3g}, dense {np.abs(r - 1).max():.3g}")
    assert np.abs(r - 1).max() < tol
    assert abs(nrm["iterations"] - R["iterations"]) <= 1
    # d itself against the restatement's.  Both have |r - 1| < tol, and to first order d log r = (I + P) d log d
    # with P_ij = d_i T_ij d_j / ntp(i) on the valid bins, so |log d - log d_ref|_2 <= 2 tol sqrt(nv) /
    # sigma_min(I + P); twice that for the terms beyond the first order.  sigma_min comes from the restatement.
    v = R["valid"]
    P = (T * np.outer(R["d"], R["d"]))[np.ix_(v, v)] / R["ntp"][v][:, None]
    smin = np.linalg.svd(np.eye(int(v.sum())) + P, compute_uv=False)[-1]
    rtol = 4 * tol * np.sqrt(v.sum()) / smin
    print(f"  d against the restatement's: worst relative difference {np.abs(d[v] / R['d'][v] - 1).max():.3g}, bound "
          f"{rtol:.3g} (sigma_min {smin:.3g})")
    assert rtol < 0.1
    np.testing.assert_allclose(d[v], R["d"][v], rtol=rtol, atol=0)


# -------------------------------------------------------------- 6. eigenpairs
@pytest.mark.parametrize("name,kind", [("A", "nan"), ("B", "bad")])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_eigenpairs(name, kind, k):
    """The dense E is the restatement's T with the d under test (test_normalisation holds that d to the
    restatement's own d, entry by entry), so eps counts only the difference between the GPU product and the dense
    one: the bound of test 3 summed over the rows."""
    tol_eig = 1e-8
    valid0, T, m = _dense(name, kind)
    s, _ = ref.planted(valid0.size)
    with _op(name, kind) as op:
        r = te.trans_eigs(op, k, phasing=-s, tol=1e-8, tol_eig=tol_eig, seed=0)
        r0 = te.trans_eigs(op, k, tol=1e-8, tol_eig=tol_eig, seed=0)
    valid = r["valid"] != 0
    assert r["normalised"] and r["converged"] and np.isnan(r["vectors"][~valid]).all()
    E = ref.operator(T, r["d"], ref.genome(name)[0], valid)
    lam, V = ref.eigh_desc(E, valid)
    X = np.where(valid[:, None], r["vectors"], 0.0)
    eps = _product_bound(T, m, r["d"], X).sum(axis=0)
    res = check_eigenpairs(E, valid, r["eigenvalues"], r["vectors"], tol_eig, eps, lam, V, with_vectors=k < 3)
    print(f"{name} k={k}: eigenvalues {r['eigenvalues']}, residuals {res} (bound {tol_eig * abs(r['eigenvalues'][0]):.3g}"
          f" + {eps}), {r['cycles']} cycles, {r['columns']} operator columns, {r['iterations']} iterations")
    np.testing.assert_array_equal(r["E"], r["vectors"] * np.sqrt(np.maximum(r["eigenvalues"], 0)))
    # E1 is the planted track; the phasing track fixes its sign, and without one the largest entry is positive
    assert abs(ref.pearson(r["vectors"][:, 0], s, valid)) >= 0.9
    for c in range(k):
        assert ref.pearson(r["vectors"][:, c], -s, valid) >= 0
        x = np.nan_to_num(r0["vectors"][:, c])
        assert x[int(np.argmax(np.abs(x)))] > 0
        assert np.array_equal(np.abs(r0["vectors"][:, c]), np.abs(r["vectors"][:, c]), equal_nan=True)


# ------------------------------------------------------------------ 7. errors
def test_argument_errors_leave_outputs_untouched():
    off, b1, b2, cnt, w, bad, use = _inputs("A", "exact_nan")
    n, C = int(off[-1]), len(off) - 1
    lib = _lib.load()
    h = ctypes.c_void_p()

    def create(off_=off, C_=C, n_weight=n, bin1=b1, nnz=b1.size):
        return lib.hh_teig_create(ptr(bin1), ptr(b2), ptr(cnt), nnz, ptr(w), n_weight, ptr(off_), C_, None, None, 0,
                                  None, ctypes.byref(h))

    assert create(C_=0) == HH_ERR_ARG and create(off_=np.arange(514, dtype=np.int64), C_=513) == HH_ERR_ARG
    assert b"C outside" in lib.hh_last_error()
    flat = off.copy()
    flat[3] = flat[2]
    assert create(off_=flat) == HH_ERR_ARG and b"ascending" in lib.hh_last_error()
    assert create(off_=off + 1) == HH_ERR_ARG and b"start at 0" in lib.hh_last_error()
    assert create(n_weight=n - 1) == HH_ERR_ARG and b"weights do not cover" in lib.hh_last_error()
    assert create(bin1=None) == HH_ERR_ARG and b"null pixel arrays" in lib.hh_last_error()
    assert create(off_=np.array([0, 2 ** 31], np.int64), C_=1, nnz=0) == HH_ERR_ARG and b"2^31" in lib.hh_last_error()
    assert h.value is None
    assert create() == 0 and h.value
    valid = ref.validity(off, w, use, bad)
    X, Y = np.ones((n, 8)), np.full((n, 8), -7.5)
    d = np.ones(n)

    def apply(k=3, d_=d, Y_=Y, X_=X, on_device=0):
        return lib.hh_teig_apply(h, ptr(d_), ptr(X_), k, ptr(Y_), on_device, None)

    assert apply(k=0) == HH_ERR_ARG and apply(k=9) == HH_ERR_ARG and b"k outside" in lib.hh_last_error()
    i = int(np.nonzero(valid)[0][7])
    for wrong in (-1.0, -0.5, np.nan, np.inf):
        dd = d.copy()
        dd[i] = wrong
        assert apply(d_=dd) == HH_ERR_ARG, wrong
        assert b"negative or non-finite" in lib.hh_last_error()
    assert apply(X_=None) == HH_ERR_ARG
    assert np.all(Y == -7.5)
    import torch
    dd = d.copy()
    dd[i] = -2.0
    tX, td = _dev(X, dd)
    tY = torch.full((n, 8), -7.5, dtype=torch.float64).cuda()
    assert apply(d_=td, Y_=tY, X_=tX, on_device=1) == HH_ERR_ARG and bool((tY == -7.5).all())
    # a negative or NaN d on an invalid bin is nobody's business, and only the head of Y is written
    dd = d.copy()
    dd[~valid] = [-1.0, np.nan] * ((~valid).sum() // 2) + [-3.0] * ((~valid).sum() % 2)
    assert apply(d_=dd) == 0
    assert np.all(Y.ravel()[3 * n:] == -7.5) and np.isfinite(Y.ravel()[:3 * n]).all()
    assert lib.hh_teig_free(h) == 0 and lib.hh_teig_free(None) == 0
    with pytest.raises(_lib.HipLibraryError, match="negative or non-finite"):
        with _op("A", "exact_nan") as op:
            op.apply(X, -d)
    with pytest.raises(ValueError, match="one row per bin"):
        with _op("A", "exact_nan") as op:
            op.apply(X[:-1])


def test_degenerate_genomes_give_nan_without_raising():
    off, b1, b2, cnt = ref.genome("A")
    n = int(off[-1])
    ch = ref.chrom_of(off)
    cis = ch[b1] == ch[b2]
    for device in (False, True):
        for args in ((b1, b2, cnt, None, np.array([0, n])),                                      # C = 1
                     (b1[:0], b2[:0], cnt[:0], None, off),                                       # nnz = 0
                     (b1, b2, cnt, np.full(n, np.nan), off),                                     # no valid bin
                     (b1[cis], b2[cis], cnt[cis], None, off)):                                   # no trans pixel
            t = _dev(*args[:4]) if device else args[:4]
            with te.TransOperator(*t, args[4]) as op:
                assert op.nnz == 0
                tb = op.tables()
                assert not tb["upper"][0].any() and not tb["lower"][0].any() and tb["upper"][1].size == 0
                Y = op.apply(np.ones((n, 2)))
                assert Y.shape == (n, 2) and not Y.any()
                r = te.trans_eigs(op, 3)
            assert not r["d"].any() and r["iterations"] == 0 and not r["valid"].any()
            assert np.isnan(r["eigenvalues"]).all() and np.isnan(r["vectors"]).all() and np.isnan(r["E"]).all()


# ------------------------------------------------------------ 8. run_TransEig
PLANTED = (50, 37, 64, 21)


@functools.lru_cache(maxsize=None)
def _planted():
    """Four chromosomes with a +-1 track in runs of 5-11 bins.  Cis counts decay with the distance; every trans
    cell is stored, 8 between bins of the same sign and 2 between bins of opposite signs.  Weights are powers of
    two with five NaN.  Returns (off, bin1, bin2, count, weight, track)."""
    rng = np.random.default_rng(7)
    off = ref.offsets(PLANTED)
    n = int(off[-1])
    sign = np.empty(n)
    at, s = 0, 1.0
    while at < n:
        L = int(rng.integers(5, 12))
        sign[at:at + L] = s
        at, s = at + L, -s
    chrom = np.repeat(np.arange(4), PLANTED)
    a, b = np.nonzero(np.triu(np.ones((n, n))))
    cis = chrom[a] == chrom[b]
    keep = ~cis | (b - a < 25)
    a, b, cis = a[keep], b[keep], cis[keep]
    count = np.where(cis, 100 // (b - a + 1) + 1, np.where(sign[a] == sign[b], 8, 2)).astype(np.int64)
    weight = 2.0 ** rng.integers(-2, 2, n)
    weight[[0, 49, 60, 61, 171]] = np.nan
    track = sign * (1 + rng.random(n))
    return off, a.astype(np.int64), b.astype(np.int64), count, weight, track


def _read(out, kind):
    prefix = os.path.basename(out)
    fil = os.path.join(out, f"{prefix}_{kind}_{StructureFind.properU(RES)}.txt")
    return [ln.rstrip("\n").split("\t") for ln in open(fil)]


def _check_files(r, out, shown, off, sel):
    k = r["E"].shape[1]
    assert sorted(os.listdir(out)) == sorted(os.path.basename(f) for f in r["files"]) and len(r["files"]) == 3
    rows = _read(out, "TransEig")
    assert rows[0] == ["chrom", "start", "end", "valid", "d"] + [f"E{c + 1}" for c in range(k)]
    want = []
    for p in sel:
        for x in range(int(off[p]), int(off[p + 1])):
            i = x - int(off[p])
            want.append([shown[p], str(i * RES), str((i + 1) * RES), str(int(r["valid"][x])), py2_float_str(r["d"][x])]
                        + [py2_float_str(v) for v in r["E"][x]])
    assert rows[1:] == want
    vals = _read(out, "TransEigValues")
    assert vals == [["index", "eigenvalue", "residual"]] + \
        [[str(c + 1), py2_float_str(r["eigenvalues"][c]), py2_float_str(r["residuals"][c])] for c in range(k)] + \
        [["iterations", str(r["iterations"])], ["deviation", py2_float_str(r["deviation"])]]
    pc = _read(out, "TransEigPC")
    assert pc == [[row[0], row[5]] for row in rows[1:]]


def _dense_strength(off, table, weight, use, bad, track, n_bins):
    """The restatement's trans saddle strength of a track (tests/trans_ref.py), and its tolerance as
    tests/test_trans_gpu.py derives it."""
    n, C, Kc = int(off[-1]), len(off) - 1, n_bins + 2
    sel = [q for q in range(C) if use is None or use[q]]
    valid = trans_ref.validity(off, weight, use, bad)
    M, stored = trans_ref.dense_upper(*table, weight, n)
    s, npx = trans_ref.block_sums(M, stored, off, valid, 2)
    e = trans_ref.expected(s, trans_ref.n_valid(off, valid))
    cls_sel, edges = saddle_ref.digitize([track[off[q]:off[q + 1]] for q in sel],
                                         [valid[off[q]:off[q + 1]] for q in sel], n_bins, 0.025, 0.975)
    cls = np.full(n, 255, np.uint8)
    for q, c in zip(sel, cls_sel):
        cls[off[q]:off[q + 1]] = c
    U, Cu, Un = trans_ref.saddle_sums(M, stored, off, valid, e, cls, Kc)
    S, Cn, _ = trans_ref.symmetric(U, Cu)
    bound = 2.0 * (int(Un.max()) + 2) * U53
    bound_k = 2 * (2 * (2 * (n_bins // 2) ** 2 + 1) + 1) * U53
    return np.array(saddle_ref.strength(S, Cn)), 2 * bound + bound_k


def test_run_transeig_traditional(tmp_path):
    off, b1, b2, count, weight, track = _planted()
    names = ["chr1", "chr2", "chr3", "chr4"]
    path = str(tmp_path / "trad.cool")
    coolio.create_cooler(path, {RES: ([(x, L * RES) for x, L in zip(names, PLANTED)], b1, b2, count)})
    sf = StructureFind(path, Res=RES)
    out = str(tmp_path / "planted")
    with pytest.raises(ValueError, match="balance it first"):
        sf.run_TransEig(out)
    h5.append_dataset(path, f"{RES}/bins", "weight", weight)
    sf = StructureFind(path, Res=RES)
    phasing = {x: -track[off[q]:off[q + 1]] for q, x in enumerate(names)}
    with pytest.raises(ValueError, match="36 values"):
        sf.run_TransEig(out, phasing=dict(phasing, chr2=phasing["chr2"][:-1]))
    r = sf.run_TransEig(out, n_eigs=2, phasing=phasing)
    assert r is sf.TransEig_dict and r["normalised"] and r["converged"] and r["E"].shape == (int(off[-1]), 2)
    valid = np.isfinite(weight)
    assert np.array_equal(r["valid"] != 0, valid) and r["selected"] == [0, 1, 2, 3]
    _check_files(r, out, names, off, [0, 1, 2, 3])
    # the operator's own numbers against the restatement
    T = ref.dense_T(b1, b2, count.astype(np.float64), weight, off, valid)
    rm = (r["d"] * (T @ r["d"]))[valid] / ref.partners(off, valid)[valid]
    assert np.abs(rm - 1).max() < 1e-6
    E = ref.operator(T, r["d"], off, valid)
    lam, V = ref.eigh_desc(E, valid)
    # |theta - lambda| <= residual <= tol_eig theta_1 + eps, eps (rounding of the product, about 1e-13 theta_1)
    # far below the second tol_eig theta_1 that stands in for it
    np.testing.assert_allclose(r["eigenvalues"], lam[:2], rtol=0, atol=2 * 1e-8 * lam[0])
    e1 = r["E"][:, 0]
    assert ref.pearson(e1, -track, valid) >= 0.9                              # oriented by the phasing given
    r_plain = sf.run_TransEig(str(tmp_path / "plain"), n_eigs=1)              # no track: largest entry positive
    x = np.nan_to_num(r_plain["E"][:, 0])
    assert x[int(np.argmax(np.abs(x)))] > 0
    # the PC file goes into run_Trans unchanged: a saddle of strength above 1, the restatement's value
    rt = sf.run_Trans(str(tmp_path / "saddle"), PC_file=r["files"][2], n_bins=10, ignore_diags=2)
    written = np.array([float(py2_float_str(v)) for v in e1])
    want, rtol = _dense_strength(off, (b1, b2, count), weight, None, None, written, 10)
    print(f"trans saddle strength of the written E1: {rt['strength']}, restatement {want}; eigenvalues "
          f"{r['eigenvalues']}, {r['iterations']} iterations, {r['cycles']} cycles")
    np.testing.assert_allclose(rt["strength"], want, rtol=rtol, atol=0)
    assert want[1] > 1 and rt["strength"][1] > 1


def test_run_transeig_haplotype(tmp_path):
    """The same four chromosomes as the maternal haplotype (raw counts), the NaN-weight bins as their gap lists,
    next to two paternal chromosomes whose pixels must not be read."""
    off, b1, b2, count, weight, track = _planted()
    n = int(off[-1])
    sizes = PLANTED + (13, 8)
    off2 = ref.offsets(sizes)
    rng = np.random.default_rng(9)
    extra = np.array([(a, b) for a in range(int(off2[-1])) for b in range(max(a, n), int(off2[-1]))
                      if rng.random() < 0.3])
    t1, t2 = np.concatenate([b1, extra[:, 0]]), np.concatenate([b2, extra[:, 1]])
    tc = np.concatenate([count, rng.integers(1, 9, len(extra))])
    o = np.lexsort((t2, t1))
    t1, t2, tc = t1[o], t2[o], tc[o]
    names = ["Ma", "Mb", "Mc", "Md", "Pa", "Pb"]
    path = str(tmp_path / "hap.cool")
    coolio.create_cooler(path, {RES: ([(x, L * RES) for x, L in zip(names, sizes)], t1, t2, tc)})
    gap = np.nonzero(~np.isfinite(weight))[0]
    gaps = {x: gap[(gap >= off2[q]) & (gap < off2[q + 1])] - off2[q] for q, x in enumerate(names)}
    pc = str(tmp_path / "pc.txt")
    with open(pc, "w") as f:
        for q, x in enumerate(names[:4]):
            for v in track[off[q]:off[q + 1]]:
                f.write(f"{x[1:]}\t{float(v)!r}\n")
    out = str(tmp_path / "hap")
    sf = StructureFind(path, Res=RES, Allelic="Maternal", GapFile={str(RES): gaps})
    r = sf.run_TransEig(out, n_eigs=2, PC_file=pc)
    valid = np.concatenate([np.isfinite(weight), np.zeros(21, bool)])
    assert r["selected"] == [0, 1, 2, 3] and np.array_equal(r["valid"] != 0, valid)
    assert np.isnan(r["E"][n:]).all() and not r["d"][n:].any()
    _check_files(r, out, [x[1:] for x in names], off2, [0, 1, 2, 3])             # names without the prefix
    assert {row[0] for row in _read(out, "TransEig")[1:]} == {"a", "b", "c", "d"}
    T = ref.dense_T(t1, t2, tc.astype(np.float64), None, off2, valid)            # the paternal pixels dropped
    lam, _ = ref.eigh_desc(ref.operator(T, r["d"], off2, valid), valid)
    np.testing.assert_allclose(r["eigenvalues"], lam[:2], rtol=0, atol=2 * 1e-8 * lam[0])
    full = np.concatenate([track, np.full(21, np.nan)])
    assert ref.pearson(r["E"][:, 0], full, valid) >= 0.9
