"""tests/comp_ref.py against LAPACK / np.corrcoef: the references alone hold
1e-13, two orders below the tightest tolerance the GPU tests put on the
kernels (1e-11 components, 1e-12 correlation at n <= 260).  Measured: planted
eigenvectors vs the SVD worst entry 9.3e-16, column means <= 3e-15; corr_ld vs
corrcoef <= 4.8e-16."""
import numpy as np
import pytest

from oracle import structure_ref
from tests.comp_ref import corr_ld, planted

S = [9.0, 6.0, 4.0, 2.0, 1.5]
TOL = 1e-13


def _match_sign(a, b):
    return a * np.sign(np.dot(a, b))


def sparse_gamma(N, n, seed, density=0.6):
    """Sparse non-negative columns (gamma-distributed nonzeros)."""
    rng = np.random.default_rng(seed)
    return rng.gamma(2.0, 1.0, (N, n)) * (rng.random((N, n)) < density)


@pytest.mark.parametrize("n", [3, 4, 15, 16, 17, 47, 48, 64, 65, 143, 144, 145, 150, 300, 513])
def test_planted_vs_lapack(n):
    Cor, U = planted(n, S, seed=n)
    k = min(len(S), n - 1)
    assert U.shape == (n, k)
    np.testing.assert_allclose(Cor, Cor.T, atol=1e-15)  # (U diag) U^T by BLAS: symmetric to rounding
    assert np.abs(Cor.mean(axis=0)).max() <= TOL
    assert np.abs(U.sum(axis=0)).max() <= TOL
    np.testing.assert_allclose(U.T @ U, np.eye(k), atol=TOL)
    # eigenvalues: s, then rest, then the 0 of the direction 1
    want = np.sort(np.concatenate([S[:k], np.full(n - 1 - k, 0.01), [0.0]]))
    np.testing.assert_allclose(np.linalg.eigvalsh(Cor), want, atol=TOL)
    # the PCA the oracle computes (SVD of the centred matrix): its top 3 are
    # U's first columns; at n = 3 the third is the null direction 1 / sqrt(3)
    V = structure_ref.top_components(Cor, 3)
    want_v = [U[:, q] if q < k else np.ones(n) / np.sqrt(n) for q in range(3)]
    worst = max(np.abs(_match_sign(V[q], want_v[q]) - want_v[q]).max() for q in range(3))
    print(f"n={n}: worst entry difference {worst:.2e}")
    assert worst <= TOL


@pytest.mark.parametrize("N,n", [(17, 16), (130, 129), (257, 250), (400, 385)])
def test_corr_ld_vs_corrcoef(N, n):
    X = sparse_gamma(N, n, seed=N)
    X[:, n // 2] = 1.25  # a constant column: sd 0, its row and column 0
    C = corr_ld(X)
    R = structure_ref.pearson_columns(X)
    worst = np.abs(C - R).max()
    print(f"N={N} n={n}: worst difference {worst:.2e}")
    assert worst <= TOL
    assert not C[n // 2].any() and not C[:, n // 2].any()
    np.testing.assert_allclose(C, C.T, atol=1e-15)  # the two divisions in either order
