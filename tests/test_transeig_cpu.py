"""Trans eigenvectors without a GPU: the dense restatement's
own properties (tests/transeig_ref.py), and the host side of
hichap_master_amd/transeig.py -- the solver over a NumPy operator, the
orientation, ``M x``, the normalisation loop over the bincount operator, the
files and the degenerate genomes."""
import os

import numpy as np
import pytest

from hichap_master_amd import _lib
from hichap_master_amd import transeig as te
from hichap_master_amd.StructureFind import StructureFind, py2_float_str
from tests import knobs
from tests import transeig_ref as ref

U53 = 2.0 ** -53
CASES = [("A", "nan"), ("A", "bad"), ("A", "nan_nouse"), ("B", "nan"), ("B", "bad")]
TOL = 1e-9


def _host_op(name, kind, junk_seed=0):
    off, b1, b2, cnt = ref.genome(name, junk_seed)
    w, bad, use = ref.weights(name, kind)
    return te.HostTransOperator(b1, b2, cnt, w, off, use, bad)


@pytest.mark.parametrize("name,kind", CASES)
def test_reference_is_symmetric_with_empty_cis_blocks(name, kind):
    R = ref.solved(name, kind, TOL)
    ch = ref.chrom_of(R["off"])
    cis = ch[:, None] == ch[None, :]
    for M in (R["T"], R["E"]):
        assert np.array_equal(M, M.T)
        assert not M[cis].any()
        assert not M[~R["valid"]].any() and not M[:, ~R["valid"]].any()
    assert R["T"][R["valid0"]].any(axis=1).sum() == R["valid"].sum()      # the dropped bins are the rows without a pixel
    dropped = np.nonzero(R["valid0"] & ~R["valid"])[0].tolist()
    assert dropped == sorted([ref.EMPTY_ROW[name], ref.NO_TRANS[name]])
    assert not R["d"][~R["valid"]].any() and np.all(R["d"][R["valid"]] > 0)
    if kind.endswith("nouse"):
        assert not R["valid"][ch == 3].any()


@pytest.mark.parametrize("name,kind", CASES)
def test_reference_rows_of_E_sum_to_zero(name, kind):
    R = ref.solved(name, kind, TOL)
    assert R["converged"] and R["deviation"] < TOL
    one = R["valid"].astype(np.float64)
    # (E 1)_i = ntp(i) (r_i - 1) and |r_i - 1| < tol; the sum of n terms adds n 2^-53 of their magnitudes
    slack = R["E"].shape[0] * U53 * (np.abs(R["E"]) @ one)
    assert np.all(np.abs(R["E"] @ one) <= TOL * R["ntp"] + slack)
    print(f"{name} {kind}: {R['iterations']} iterations to {R['deviation']:.3g}; top eigenvalues "
          f"{R['values'][:4]}, lowest {R['values'][-2:]}")


@pytest.mark.parametrize("name", ["A", "B"])
def test_cis_junk_changes_nothing(name):
    off, b1, b2, cnt = ref.genome(name)
    off2, c1, c2, cnt2 = ref.genome(name, 1)
    assert np.array_equal(b1, c1) and np.array_equal(b2, c2) and not np.array_equal(cnt, cnt2)
    w, bad, use = ref.weights(name, "nan")
    valid = ref.validity(off, w, use, bad)
    T1, T2 = ref.dense_T(b1, b2, cnt, w, off, valid), ref.dense_T(c1, c2, cnt2, w, off, valid)
    assert T1.tobytes() == T2.tobytes()
    t1, t2 = ref.tables(b1, b2, cnt, w, off, valid), ref.tables(c1, c2, cnt2, w, off, valid)
    assert all(x.tobytes() == y.tobytes() for k in t1 for x, y in zip(t1[k], t2[k]))
    a, b = _host_op(name, "nan"), _host_op(name, "nan", 1)
    x = np.random.default_rng(0).standard_normal((a.n, 3))
    assert a.apply(x).tobytes() == b.apply(x).tobytes()


def test_reference_E1_follows_the_planted_track():
    """The figure the GPU test's 0.9 rests on: the restatement alone."""
    for name, want in (("A", 0.98), ("B", 0.99)):
        R = ref.solved(name, "nan", TOL)
        s, t = ref.planted(R["E"].shape[0])
        r1, r2 = abs(ref.pearson(R["vectors"][:, 0], s, R["valid"])), abs(ref.pearson(R["vectors"][:, 1], t, R["valid"]))
        print(f"{name}: |r(E1, s)| = {r1:.4f}, |r(E2, t)| = {r2:.4f}; gaps {-np.diff(R['values'][:4])}")
        assert r1 >= want and r2 >= 0.85
        assert R["values"][1] - R["values"][2] > 15 and R["values"][-1] < -20   # a gap behind k = 2; big negative ones


def check_eigenpairs(E, valid, values, vectors, tol_eig, eps, lam, V, with_vectors=True):
    """The three bounds: (a) ||E x - theta x|| <= tol_eig |theta_1| + eps_c; (b) |theta_c - lambda_c| <= that
    residual (a symmetric matrix has an eigenvalue within the residual norm of any Ritz value); (c) the sine of the
    angle to the reference eigenvector <= residual / gap_c, gap_c the distance from lambda_c to the rest of the
    reference spectrum (Davis-Kahan).  Returns the residuals."""
    k = len(values)
    X = np.where(valid[:, None], vectors, 0.0)
    np.testing.assert_allclose(np.linalg.norm(X, axis=0), 1.0, rtol=0, atol=64 * U53)
    res = np.linalg.norm(E @ X - X * values, axis=0)
    for c in range(k):
        bound = tol_eig * abs(values[0]) + eps[c]
        assert res[c] <= bound, (c, res[c], bound)
        assert abs(values[c] - lam[c]) <= bound, (c, values[c], lam[c], bound)
        if with_vectors:
            gap = min(abs(lam[c] - lam[j]) for j in range(len(lam)) if j != c)
            v, x = V[:, c], X[:, c]
            sine = float(np.linalg.norm(x - v * float(v @ x)))       # the part of x outside span(v): no cancellation
            # the inner product and the norm of n terms carry n 2^-53 of rounding each, the unit norms 64 2^-53
            assert sine <= bound / gap + (2 * X.shape[0] + 64) * U53, (c, sine, bound / gap)
    return res


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_top_eigs_over_a_numpy_operator(name, k):
    R = ref.solved(name, "nan", TOL)
    E, valid = R["E"], R["valid"]
    tol_eig = 1e-9
    S = te.top_eigs(lambda X: E @ X, E.shape[0], k, valid, tol_eig, 200, 0)
    assert S["converged"] and S["residuals"].max() <= tol_eig * abs(S["values"][0])       # its own stopping rule
    assert not S["vectors"][~valid].any()
    # eps: the dense product's own rounding, n 2^-53 sum |E_ij x_j| per row, twice (the solver's and the check's)
    eps = [2 * np.linalg.norm(E.shape[0] * U53 * (np.abs(E) @ np.abs(S["vectors"][:, c]))) for c in range(k)]
    check_eigenpairs(E, valid, S["values"], S["vectors"], tol_eig, eps, R["values"], R["vectors"], with_vectors=k < 3)
    print(f"{name} k={k}: {S['cycles']} cycles, {S['columns']} operator columns, residuals {S['residuals']}")
    if k == 2:
        assert S["cycles"] <= 12
    # a second run: the same start, the same result
    S2 = te.top_eigs(lambda X: E @ X, E.shape[0], k, valid, tol_eig, 200, 0)
    assert S2["vectors"].tobytes() == S["vectors"].tobytes()


def test_top_eigs_takes_the_algebraically_largest_and_tiny_subspaces():
    rng = np.random.default_rng(3)
    Q, _ = np.linalg.qr(rng.standard_normal((60, 60)))
    lam = np.concatenate([[-50.0, 30.0, 12.0], rng.uniform(-5, 5, 57)])
    A = (Q * lam) @ Q.T
    S = te.top_eigs(lambda X: A @ X, 60, 2, None, 1e-10, 300, 1)
    np.testing.assert_allclose(S["values"], [30.0, 12.0], rtol=1e-9)          # not -50, the largest in magnitude
    # stopped at max_cycles: reported, and the values and residuals returned are those of the vectors returned
    for cycles in (1, 2):
        S = te.top_eigs(lambda X: A @ X, 60, 2, None, 1e-14, cycles, 1)
        assert not S["converged"] and S["cycles"] == cycles
        X = S["vectors"]
        np.testing.assert_allclose(np.einsum("ic,ic->c", X, A @ X), S["values"], rtol=1e-12)
        np.testing.assert_allclose(np.linalg.norm(A @ X - X * S["values"], axis=0), S["residuals"], rtol=1e-6)
    valid = np.zeros(60, bool)
    valid[[3, 10, 11, 40, 59]] = True                                        # fewer bins than one basis: dense
    B = np.where(np.outer(valid, valid), A, 0.0)
    S = te.top_eigs(lambda X: B @ X, 60, 3, valid, 1e-10, 300, 1)
    want = np.linalg.eigvalsh(B[np.ix_(valid, valid)])[::-1][:3]
    np.testing.assert_allclose(S["values"], want, rtol=1e-12)
    assert S["converged"] and not S["vectors"][~valid].any()
    S = te.top_eigs(lambda X: B @ X, 60, 2, np.zeros(60, bool))              # no valid bin
    assert np.isnan(S["values"]).all() and not S["converged"]
    with pytest.raises(ValueError, match="1..8"):
        te.top_eigs(lambda X: B @ X, 60, 9)


def test_orient_follows_both_sign_rules():
    valid = np.ones(12, bool)
    valid[[0, 7]] = False
    x = np.array([9.0, 1, -2, 3, -5, 5, 0.5, -9, 1, 2, -1, 0.25])
    x[~valid] = np.nan
    V = np.stack([x, -x], axis=1)
    out = te.orient(V, valid)
    # the largest magnitude among the valid bins is 5, at bins 4 (-5) and 5 (+5): the lowest bin decides
    assert out[4, 0] > 0 and out[4, 1] > 0 and np.array_equal(out[:, 0], out[:, 1], equal_nan=True)
    assert np.array_equal(out[:, 0], -x, equal_nan=True)
    ph = np.where(np.isnan(x), 1.0, x) + 0.1
    ph[3] = np.nan                                                            # NaN allowed in the track
    out = te.orient(V, valid, ph)
    assert np.array_equal(out[:, 0], x, equal_nan=True) and np.array_equal(out[:, 1], x, equal_nan=True)
    for c in range(2):
        assert ref.pearson(out[:, c], ph, valid) > 0
        assert ref.sign_of(V[:, c], valid, ph) * V[4, c] == out[4, c]
        assert ref.sign_of(V[:, c], valid) * V[4, c] == te.orient(V, valid)[4, c]
    # a track that is constant where the vector is finite gives no correlation: the second rule
    out = te.orient(V, valid, np.ones(12))
    assert np.array_equal(out[:, 0], -x, equal_nan=True)
    assert V[4, 0] == -5.0                                                    # the input is not changed


@pytest.mark.parametrize("name", ["A", "B"])
def test_mask_product_matches_the_formula(name):
    R = ref.solved(name, "nan", TOL)
    off, valid = R["off"], R["valid"]
    n = valid.size
    X = np.random.default_rng(1).integers(-7, 8, (n, 5)).astype(np.float64)   # exact sums: equality
    M = ref.mask_matrix(off, valid)
    assert np.array_equal(te.mask_product(X, valid, off), M @ X)
    assert np.array_equal(te.mask_product(X[:, 2], valid, off), M @ X[:, 2])
    Y = np.random.default_rng(2).standard_normal((n, 3))
    got = te.mask_product(Y, valid, off)
    bound = (n + 2) * U53 * np.abs(Y).sum(axis=0)                             # two orders of at most n terms
    assert np.all(np.abs(got - M @ Y) <= bound)
    assert not got[~valid].any()
    assert np.array_equal(te.trans_partners(off, valid), ref.partners(off, valid))
    assert np.array_equal(te.trans_partners(off, valid), (M @ valid.astype(float)).astype(np.int64))


@pytest.mark.parametrize("name,kind", CASES)
def test_host_operator_and_normalisation_against_the_restatement(name, kind):
    R = ref.solved(name, kind, TOL)
    op = _host_op(name, kind)
    assert np.array_equal(op.valid != 0, R["valid0"]) and op.nnz == np.count_nonzero(np.triu(R["T"]) != 0) + \
        np.count_nonzero(ref.kept(*ref.genome(name)[1:3], R["off"], R["valid0"]) & (ref.genome(name)[3] == 0))
    X = np.random.default_rng(4).standard_normal((op.n, 3))
    want = R["T"] @ X
    m = (R["T"] != 0).sum(axis=1)
    assert np.all(np.abs(op.apply(X) - want) <= 2 * (m[:, None] + 3) * U53 * (np.abs(R["T"]) @ np.abs(X)))
    nrm = te.trans_normalise(op, TOL)
    assert nrm["converged"] and abs(nrm["iterations"] - R["iterations"]) <= 1
    assert np.array_equal(nrm["valid"], R["valid"]) and np.array_equal(nrm["ntp"], R["ntp"])
    r = (nrm["d"] * (R["T"] @ nrm["d"]))[R["valid"]] / R["ntp"][R["valid"]]
    assert np.abs(r - 1).max() < TOL * (1 + 1e-6)
    assert op.d is nrm["d"] or np.array_equal(op.d, nrm["d"])
    E = op.apply_E(X)
    np.testing.assert_allclose(E, ref.operator(R["T"], nrm["d"], R["off"], R["valid"]) @ X, rtol=0, atol=1e-10)
    # not converging is reported, not raised
    short = te.trans_normalise(op, 1e-12, max_iter=3)
    assert short["iterations"] == 3 and not short["converged"] and short["deviation"] > 1e-12


def test_degenerate_genomes_give_nan_without_raising():
    off, b1, b2, cnt = ref.genome("A")
    n = int(off[-1])
    cases = [te.HostTransOperator(b1, b2, cnt, None, np.array([0, n])),                       # C = 1
             te.HostTransOperator(b1[:0], b2[:0], cnt[:0], None, off),                        # nnz = 0
             te.HostTransOperator(b1, b2, cnt, np.full(n, np.nan), off)]                      # no valid bin
    ch = ref.chrom_of(off)
    cis = ch[b1] == ch[b2]
    cases.append(te.HostTransOperator(b1[cis], b2[cis], cnt[cis], None, off))                 # no trans pixel
    for op in cases:
        assert op.nnz == 0
        r = te.trans_eigs(op, 3)
        assert not r["d"].any() and r["iterations"] == 0 and np.isnan(r["deviation"]) and not r["valid"].any()
        assert np.isnan(r["eigenvalues"]).all() and np.isnan(r["vectors"]).all() and np.isnan(r["E"]).all()
        assert np.isnan(r["residuals"]).all() and r["vectors"].shape == (n, 3) and not r["converged"]
    with pytest.raises(ValueError, match="1..8"):
        te.trans_eigs(cases[0], 0)


def test_trans_eigs_end_to_end_on_the_host_operator():
    R = ref.solved("A", "nan", 1e-8)
    op = _host_op("A", "nan")
    s, _ = ref.planted(op.n)
    r = te.trans_eigs(op, 2, phasing=-s, tol=1e-8, tol_eig=1e-8)
    assert r["normalised"] and r["converged"]
    assert np.isnan(r["vectors"][~R["valid"]]).all() and np.array_equal(r["valid"] != 0, R["valid"])
    assert ref.pearson(r["vectors"][:, 0], -s, R["valid"]) >= 0.9
    np.testing.assert_allclose(r["E"], r["vectors"] * np.sqrt(r["eigenvalues"]), rtol=0, atol=0, equal_nan=True)
    np.testing.assert_allclose(r["eigenvalues"], R["values"][:2], rtol=1e-7)
    r2 = te.trans_eigs(op, 2, tol=1e-8, tol_eig=1e-8)                          # no track: the largest entry positive
    x = np.nan_to_num(r2["vectors"][:, 0])
    assert x[np.argmax(np.abs(x))] > 0


def test_files_are_read_back(tmp_path):
    R = ref.solved("A", "nan", 1e-8)
    off, valid = R["off"], R["valid"]
    n = valid.size
    names = [f"chr{q + 1}" for q in range(len(off) - 1)]
    sel = [0, 1, 3, 5]
    lam = R["values"][:2]
    V = np.where(valid[:, None], R["vectors"][:, :2], np.nan)
    E = V * np.sqrt(lam)
    files = [str(tmp_path / x) for x in ("eig.txt", "val.txt", "pc.txt")]
    te.write_transeig(*files, names, off, sel, 40000, valid.astype(np.uint8), R["d"], E, lam, [1e-9, 2e-9], 62, 8.5e-9)
    rows = [ln.rstrip("\n").split("\t") for ln in open(files[0])]
    assert rows[0] == ["chrom", "start", "end", "valid", "d", "E1", "E2"]
    bins = [x for p in sel for x in range(off[p], off[p + 1])]
    assert rows[1:] == [[names[ref.chrom_of(off)[x]], str((x - off[ref.chrom_of(off)[x]]) * 40000),
                         str((x - off[ref.chrom_of(off)[x]] + 1) * 40000), str(int(valid[x])), py2_float_str(R["d"][x]),
                         py2_float_str(E[x, 0]), py2_float_str(E[x, 1])] for x in bins]
    assert "nan" in {r[5] for r in rows[1:]}
    vals = [ln.rstrip("\n").split("\t") for ln in open(files[1])]
    assert vals == [["index", "eigenvalue", "residual"], ["1", py2_float_str(lam[0]), "1e-09"],
                    ["2", py2_float_str(lam[1]), "2e-09"], ["iterations", "62"], ["deviation", "8.5e-09"]]
    # the PC file in the layout _saddle_track reads from PC_file
    sf = StructureFind(Res=40000)
    chroms = [names[p] for p in sel]
    tracks = sf._saddle_track(None, files[2], chroms, sf._name)
    for p in sel:
        want = np.array([float(py2_float_str(v)) for v in E[off[p]:off[p + 1], 0]])
        assert np.array_equal(tracks[names[p]], want, equal_nan=True)


def test_run_transeig_refuses_before_any_gpu_work(tmp_path):
    """An unbalanced cooler and a genome of more than 512 chromosomes raise as in run_Trans, before a device is
    asked for."""
    from hichap_master_amd import coolio, h5
    res = 10000
    path = str(tmp_path / "two.cool")
    coolio.create_cooler(path, {res: ([("chr1", 3 * res), ("chr2", 2 * res)], np.array([0, 1]), np.array([3, 4]),
                                      np.array([5, 6]))})
    with pytest.raises(ValueError, match="run_TransEig: the cooler has no bins/weight column; balance it first"):
        StructureFind(path, Res=res).run_TransEig(str(tmp_path / "out"))
    with pytest.raises(ValueError, match="Unkonwn key word"):
        StructureFind(path, Res=res, Allelic="Both").run_TransEig(str(tmp_path / "out"))
    many = str(tmp_path / "many.cool")
    coolio.create_cooler(many, {res: ([(f"s{i}", res) for i in range(513)], np.array([0]), np.array([1]),
                                      np.array([1]))})
    h5.append_dataset(many, f"{res}/bins", "weight", np.ones(513))
    with pytest.raises(ValueError, match="run_TransEig: 513 chromosomes, at most 512"):
        StructureFind(many, Res=res).run_TransEig(str(tmp_path / "out"))
    assert not os.path.exists(str(tmp_path / "out"))


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libhichap_hip.so is not built")
def test_tuning_key():
    """teig_rows in hh_tune's one table: the documented default, a round trip, the rejection outside 1..16."""
    assert knobs.get("teig_rows") == 4
    with knobs.tuned(teig_rows=16):
        assert knobs.get("teig_rows") == 16
        for wrong in (0, 17, -1):
            with pytest.raises(_lib.HipLibraryError, match="teig_rows") as e:
                _lib.call("hh_tune", b"teig_rows", wrong)
            assert e.value.code == -1
        assert knobs.get("teig_rows") == 16
    assert knobs.get("teig_rows") == 4
