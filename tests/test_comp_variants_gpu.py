"""The compartment kernels (comp.hip) at the instances and sizes the tests at
the workload's own size never choose: every case forces one template instance
or one branch through a tuning knob (tests.knobs.tuned) or through n, at the
smallest size at which that instance can still go wrong, and compares with a
plain reference (tests/comp_ref.py: extended-precision correlation, a planted
spectrum with exactly known eigenvectors; the oracle's SVD for whole runs).

Which instance a case runs follows from the host code alone, not from the
device: the rule is quoted in the case's docstring or parametrize id.  Two
rules take the device's k_ortho grid cap into account (pca_krylov):
cap(tpb) = min(CUs x blocks per CU / hardware queues, 64) -- 64 at 256 CUs
and the 4 hardware queues HIP opens by default -- and a forced "ortho_tpb" is
taken when nap = ceil(n / 64) <= tpb x cap(tpb).  The largest nap here is 9
(n = 513), so any cap >= 9 (36 CUs at 4 queues) takes every forced value.

Worst errors measured on an MI355X (tolerance in brackets):
  correlation vs corr_ld         n <= 260: 1.6e-15 (1e-12); n = 385: 1.7e-15 (1e-11)
  variants: components vs U      2.4e-14 (1e-11); eigenvalues rel. 1.1e-14 (1e-11)
  tiny n: components vs oracle   1.7e-14 (1e-11); planted 1.0e-15 (1e-11)
"""
import functools

import numpy as np
import pytest

from oracle import structure_ref
from tests.comp_ref import corr_ld, planted
from tests.knobs import tuned

pytestmark = pytest.mark.gpu

S = [9.0, 6.0, 4.0, 2.0, 1.5]


def _match_sign(a, b):
    return a * np.sign(np.dot(a, b))


# ------------------------------------------------------------ a. correlation
CORR_SHAPES = [(17, 16), (130, 129), (129, 128), (257, 250), (303, 300), (400, 385)]


def _gaps(N, n):
    """N - n gap bins: the first bin, the last bin and a run in the middle, as
    many of them as N - n allows (one gap: first for N = 17, last for 130,
    middle for 129)."""
    g = N - n
    if g == 1:
        return np.array([{17: 0, 130: N - 1}.get(N, N // 2)])
    mid = N // 2 + np.arange(g - 2)
    return np.concatenate([[0], mid, [N - 1]])


@functools.lru_cache(maxsize=None)
def _corr_case(N, n, kind):
    """(M, decline, NG, reference correlation) of one shape; ``kind``:
    'ones' (unit decline), 'const' (unit decline and a constant O/E column),
    'decay' (the decline Distance_Decay gives for M with these gaps)."""
    rng = np.random.default_rng(1000 * N + n)
    U = np.triu(rng.gamma(2.0, 1.0, (N, N)) * (rng.random((N, N)) < 0.6))
    M = U + np.triu(U, 1).T
    NG = np.setdiff1d(np.arange(N), _gaps(N, n))
    assert NG.size == n
    dec = np.ones(N)
    if kind == "const":
        M[:, NG[n // 3]] = 2.0  # O/E = 2 in every row: mean 2 exactly, Z = 0, sd = 0
    if kind == "decay":
        from hichap_master_amd.StructureFind import StructureFind
        M = M * (1.0 + 40.0 / (1.0 + np.abs(np.subtract.outer(np.arange(N), np.arange(N)))))
        dec, _, NG2 = StructureFind(Res=100000).Distance_Decay(M=M, G_array=_gaps(N, n))
        np.testing.assert_array_equal(NG2, NG)
        dec[dec == 0] = dec[np.nonzero(dec)].min()  # Get_PCA's zero fix
    d = np.abs(np.subtract.outer(np.arange(N), NG))
    X = np.where(M[:, NG] != 0, M[:, NG] / dec[d], 0.0)
    ref = corr_ld(X)
    for a in (M, dec, NG, ref):
        a.setflags(write=False)
    return M, dec, NG, ref


def _cor(M, dec, NG, split):
    from hichap_master_amd.StructureFind import _Comp
    with tuned(syrk_split=split):
        comp = _Comp(M)
        comp.correlation(dec, NG)
        return comp.cor()


def _check_cor(N, n, kind, split):
    M, dec, NG, ref = _corr_case(N, n, kind)
    C = _cor(M, dec, NG, split)
    err = np.abs(C - ref).max()
    print(f"correlation N={N} n={n} {kind} syrk_split={split}: worst |Cor - corr_ld| = {err:.2e}")
    np.testing.assert_allclose(C, ref, rtol=0, atol=1e-12 if n <= 260 else 1e-11)
    live = np.diagonal(ref) != 0  # (a constant column's diagonal is 0)
    np.testing.assert_array_equal(np.diagonal(C)[live], 1.0)
    np.testing.assert_allclose(C, C.T, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(_cor(M, dec, NG, split), C)  # the same knob: bitwise
    return C, ref, NG


@pytest.mark.parametrize("split", [0, 2, 3, 8, -1])
@pytest.mark.parametrize("N,n", CORR_SHAPES)
def test_correlation_syrk_split(N, n, split):
    """hh_comp_correlation against corr_ld.  ld = n rounded up to 128: 128
    (n = 16, 128) / 256 (129, 250) / 384 (300) / 512 (385), so 1, 3, 6 and 10
    Cov tiles; n = 129 has a second tile row with one live column.  Npad = N
    rounded up to 16: N mod 16 = 1 (17, 129, 257), 2 (130), 15 (303), 0 (400).
    syrk_splits(): split 0 ->
    k_syrk<false>; split s > 0 -> k_syrk<true> + k_syrk_reduce with
    min(s, Npad / 16) splits of kc = ceil(Npad / 16 / s) x 16 rows -- N = 130
    (Npad = 144, 9 steps), s = 8: kc = 32, the splits from row 160 on are
    empty and must add exact zeros; N = 17 (Npad = 32), s = 3 or 8: clamped to
    2; -1: the cost model (any outcome: asserted for correctness only)."""
    _check_cor(N, n, "ones", split)


@pytest.mark.parametrize("split", [0, 3])
def test_correlation_constant_column(split):
    """A constant O/E column has sd 0: its row and column of Cor are 0 / 0 =
    NaN -> 0 as pearson_columns gives (k_corr_norm_oop's x != x branch)."""
    N, n = 130, 129
    C, ref, NG = _check_cor(N, n, "const", split)
    j = n // 3
    assert not ref[j].any() and not ref[:, j].any()
    assert not C[j].any() and not C[:, j].any()


@pytest.mark.parametrize("split", [0, 2])
def test_correlation_distance_decay_decline(split):
    """The same with the decline of Distance_Decay (a decaying matrix, its
    zero distances filled as Get_PCA does): O/E = M / decline[|i - j|]."""
    _check_cor(257, 250, "decay", split)


# -------------------------------------------------- b. eigensolver variants
@functools.lru_cache(maxsize=None)
def _planted(n):
    Cor, U = planted(n, S, seed=n)
    Cor.setflags(write=False)
    U.setflags(write=False)
    return Cor, U


def _comp_with_cor(Cor):
    """An hh_comp whose device correlation is ``Cor`` (n x n)."""
    from hichap_master_amd.StructureFind import _Comp
    from hichap_master_amd._lib import call, ptr
    n = Cor.shape[0]
    comp = _Comp(np.eye(n))
    comp.correlation(np.ones(n), np.arange(n))
    call("hh_comp_set_cor", comp.h, ptr(np.ascontiguousarray(Cor)), None)
    return comp


def _solve(n, **knobs):
    """Top-3 PCA of planted(n) under ``knobs``, twice: (pcs, eigvals, status)
    of the first run; the second must be bitwise the same."""
    Cor, _ = _planted(n)
    with tuned(**knobs):
        comp = _comp_with_cor(Cor)
        pcs, ev, _ = comp.pca(3)
        st = dict(comp.pca_status)
        pcs2, ev2, _ = comp.pca(3)
    np.testing.assert_array_equal(pcs2, pcs)
    np.testing.assert_array_equal(ev2, ev)
    return pcs, ev, st


def _check_planted(n, method, **knobs):
    pcs, ev, st = _solve(n, **knobs)
    assert st["converged"], st
    assert st["method"] == method, st
    assert not st["ortho_fallback"], st
    _, U = _planted(n)
    k = U.shape[1]
    # n = 3: two planted directions; the third component is the null
    # direction of the centred matrix, 1 / sqrt(3), eigenvalue 0
    want = [U[:, q] if q < k else np.ones(n) / np.sqrt(n) for q in range(3)]
    lam = np.array([S[q] ** 2 if q < k else 0.0 for q in range(3)])
    err = max(np.abs(_match_sign(pcs[q], want[q]) - want[q]).max() for q in range(3))
    rel = np.abs(ev[lam > 0] / lam[lam > 0] - 1).max()
    print(f"planted n={n} {knobs}: {st['method']} products={st['products']} worst |pc - U| = {err:.2e} "
          f"eigenvalues rel {rel:.2e}")
    for q in range(3):
        np.testing.assert_allclose(_match_sign(pcs[q], want[q]), want[q], rtol=0, atol=1e-11)
    np.testing.assert_allclose(ev[lam > 0], lam[lam > 0], rtol=1e-11, atol=0)
    # a zero eigenvalue comes out at the rounding of the largest: eps x lambda_1 scale
    np.testing.assert_allclose(ev[lam == 0], 0.0, rtol=0, atol=1e-11 * lam[0])
    return pcs, ev, st


@pytest.mark.parametrize("n", [150, 300, 513])
@pytest.mark.parametrize("tpb", [1, 2, 4, 8])
def test_krylov_forced_ortho_tpb(tpb, n):
    """k_ortho<*, tpb> in its low-synch modes (FullLS, Last, Start, Ritz).
    nap = ceil(n / 64) = 3, 5, 9 <= tpb x cap(tpb) (module docstring), so the
    forced tpb is taken and the grid is ceil(nap / tpb) = 1 .. 9 blocks <=
    cap: one launch per product (pca_coop).  tpb 8, n 150: one block, 362 of
    its 512 row slots empty; tpb 1, n 513: the ninth block owns one row."""
    _check_planted(n, "krylov", ortho_tpb=tpb)


@pytest.mark.parametrize("n", [150, 300, 513])
@pytest.mark.parametrize("tpb", [1, 2])
def test_krylov_ortho_full_not_lowsync(tpb, n):
    """ortho_lowsync 0: k_ortho<kOrthoFull, tpb> (two CGS passes, each with
    its own projection reduction and shifted CholeskyQR3) in place of
    kOrthoFullLS; tpb forced as above."""
    _check_planted(n, "krylov", ortho_lowsync=0, ortho_tpb=tpb)


def test_krylov_auto_tpb_one():
    """ortho_tpb 0, ortho_min_tpb 1: the automatic loop tries t = 1 first and
    takes it when nap = 5 <= 1 x cap(1): k_ortho<*, 1> by the automatic rule."""
    _check_planted(300, "krylov", ortho_tpb=0, ortho_min_tpb=1)


def test_krylov_grid_cap_one_block():
    """ortho_grid_cap 1 caps every cap(t) at 1.  n = 150: nap = 3 fits t = 4
    only (3 <= 4 x 1): k_ortho<*, 4> with a single block."""
    _check_planted(150, "krylov", ortho_tpb=0, ortho_grid_cap=1)


def test_krylov_grid_cap_declines_one_launch():
    """ortho_grid_cap 1, n = 600: nap = 10 fits no t in {2, 4}, the choice
    falls to 8, ceil(10 / 8) = 2 blocks > cap 1: the solver takes the
    multi-launch orthogonalisation by its own decision -- method krylov, and
    not the abort's fallback flag."""
    _check_planted(600, "krylov", ortho_tpb=0, ortho_grid_cap=1)


@pytest.mark.parametrize("n,p,method", [
    (150, 2, "krylov"), (150, 3, "krylov"), (150, 4, "krylov"), (150, 8, "krylov"),
    (300, 2, "krylov"), (300, 3, "krylov"), (300, 4, "krylov"), (300, 8, "krylov"),
    (47, 2, "subspace"), (48, 2, "krylov"),
    (143, 8, "subspace"), (144, 8, "krylov"), (145, 8, "krylov")])
def test_pca_p_and_krylov_threshold(n, p, method):
    """pca_p products per Krylov cycle; Krylov runs when its basis and the
    last product's residual block fit, (pca_p + 1) x 16 <= n, else block
    subspace iteration: 3 x 16 = 48 (pca_p 2: 47 subspace, 48 krylov, its
    basis exactly n columns), 9 x 16 = 144 (143 / 144 / 145).  pca_p 2 leaves
    two basis blocks: the convergence bound then takes the residual block's
    part of A x as well."""
    _check_planted(n, method, pca_p=p, pca_method=1)


@pytest.mark.parametrize("coop", [0, 1])
@pytest.mark.parametrize("n", [150, 300])
def test_cor_sym_variants_small(n, coop):
    """Cor V from the upper triangle where the whole matrix is one 256-row
    rectangle (n = 150, ld = 256: one block, the diagonal rectangle only) or
    one and a ragged second (n = 300, ld = 384: rectangles (0,0), (0,1), (1,1),
    the last two with 2 of 4 column tiles): cor_sym 1 k_cor_sym, 2
    k_cor_sym_pf<false>, 3 k_cor_sym_pf<true> bitwise equal; 0 (k_cor_mul_part,
    the full matrix) to the tolerance; with the one-launch (pca_coop 1) and
    the multi-launch orthogonalisation."""
    out = {sym: _check_planted(n, "krylov", cor_sym=sym, pca_coop=coop, pca_method=1) for sym in (0, 1, 2, 3)}
    for sym in (2, 3):
        np.testing.assert_array_equal(out[sym][0], out[1][0])
        np.testing.assert_array_equal(out[sym][1], out[1][1])
        assert out[sym][2]["products"] == out[1][2]["products"]
    for q in range(3):
        np.testing.assert_allclose(_match_sign(out[0][0][q], out[1][0][q]), out[1][0][q], rtol=0, atol=1e-11)
    np.testing.assert_allclose(out[0][1], out[1][1], rtol=1e-11)


@pytest.mark.parametrize("n", [17, 64, 150])
def test_subspace_iteration_forced(n):
    """pca_method 0: block subspace iteration with 16 columns.  n = 17: the
    smallest n it runs at (the centred matrix has rank 16 = the block); 64:
    one block of the Gram kernels exactly; 150: where Krylov would run."""
    _check_planted(n, "subspace", pca_method=0)


# ------------------------------------------------------ c. tiny chromosomes
TINY = [3, 4, 8, 15, 16, 17]


def _tiny_method(n):
    # hh_comp_pca: n <= 16 -> the host eigensolver ("dense"); 17 < 144 -> subspace
    return "dense" if n <= 16 else "subspace"


@pytest.mark.parametrize("n", TINY)
def test_tiny_planted(n):
    """hh_comp_set_cor + pca(3) at the small end: planted(n) with s cut to
    n - 1 values (n = 3: the third component is the null direction)."""
    _check_planted(n, _tiny_method(n))


def _tiny_matrix(n):
    """Dense symmetric positive N = n + 2 matrix with a compartment-like sign
    pattern and two empty (gap) bins: the second and the last."""
    N = n + 2
    rng = np.random.default_rng(n)
    lab = np.where(np.arange(N) % 4 < 2, 1.0, -1.0)
    d = np.abs(np.subtract.outer(np.arange(N), np.arange(N)))
    U = np.triu(rng.gamma(4.0, 1.0, (N, N)) * 30.0 / (1.0 + d) * (1.0 + 0.5 * np.outer(lab, lab)))
    M = U + np.triu(U, 1).T
    for g in (1, N - 1):
        M[g, :] = 0
        M[:, g] = 0
    return M


@pytest.mark.parametrize("n", TINY)
def test_tiny_chromosome_vs_oracle(n):
    """The whole StructureFind.compartment(M) at n valid bins against the
    oracle (corrcoef + exact SVD + Select_PC_new): every component whose
    eigenvalue is separated from its neighbours by >= 1e-3 lambda_1 (rounding
    eps lambda_1 / gap <= 1e-13, far inside 1e-11) up to sign -- at n = 3 the
    third is the null direction of the centred matrix, determined as well --
    and the selected PC with its A/B signs."""
    from hichap_master_amd.StructureFind import StructureFind
    M = _tiny_matrix(n)
    sf = StructureFind(Res=1000000)
    dec, G, NG = sf.Distance_Decay(M=M, G_array=None)
    d_ref, G_ref, NG_ref = structure_ref.distance_decay(M)
    np.testing.assert_array_equal(NG, NG_ref)
    assert NG.size == n
    pcs, Cor, OE = sf.Get_PCA(distance_bin=dec.copy(), M=M, NG_array=NG)
    st = sf.pca_status
    assert st["converged"] and st["method"] == _tiny_method(n) and not st["ortho_fallback"], st
    p_ref, C_ref, _ = structure_ref.get_pca(d_ref, M, NG_ref)
    np.testing.assert_allclose(np.asarray(Cor), C_ref, rtol=0, atol=1e-12)
    lam = np.zeros(5)
    sv = np.linalg.svd(C_ref - C_ref.mean(axis=0), compute_uv=False) ** 2
    lam[: min(5, n)] = sv[:5]
    compared = 0
    for q in range(3):
        gap = min(lam[q - 1] - lam[q] if q else np.inf, lam[q] - lam[q + 1] if q + 1 < n else np.inf)
        if gap < 1e-3 * lam[0]:
            continue
        err = np.abs(_match_sign(pcs[q], p_ref[q]) - p_ref[q]).max()
        print(f"tiny n={n} PC{q + 1}: relative gap {gap / lam[0]:.2e} worst |pc - oracle| = {err:.2e}")
        np.testing.assert_allclose(_match_sign(pcs[q], p_ref[q]), p_ref[q], rtol=0, atol=1e-11)
        compared += 1
    assert compared >= 2, lam
    np.testing.assert_allclose(st["eigvals"], lam[:3], rtol=1e-11, atol=1e-11 * lam[0])
    full = sf.compartment(M)
    ref_full, k_ref, _, _ = structure_ref.compartment(M)
    np.testing.assert_allclose(full, ref_full, rtol=0, atol=1e-11)
    big = np.abs(ref_full) > 1e-8
    np.testing.assert_array_equal(np.sign(full[big]), np.sign(ref_full[big]))
    assert not full[[1, n + 1]].any()  # the gap bins


@pytest.mark.parametrize("n", [1, 2])
def test_too_few_valid_bins_raise(n):
    """n < 3 valid bins: the reference's PCA(n_components=3) raises; here a
    ValueError that says how many valid bins there were, and from
    Compartment() one that names the chromosome."""
    from hichap_master_amd._lib import HipLibraryError
    from hichap_master_amd.StructureFind import StructureFind
    M = _tiny_matrix(n)
    with pytest.raises((ValueError, HipLibraryError), match=rf"\b{n} valid bin"):
        StructureFind(Res=1000000).compartment(M)
    with pytest.raises((ValueError, HipLibraryError), match=rf"\b{n} valid bin") as ei:
        StructureFind(Res=1000000).Compartment(Matrix_Dict={"chr1": _tiny_matrix(8), "chrTiny": M})
    assert "chrTiny" in str(ei.value)
    # the C entry point itself: k = 3 components of an n x n correlation
    comp = _comp_with_cor(np.eye(n))
    with pytest.raises(HipLibraryError, match=rf"has {n}\b"):
        comp.pca(3)
