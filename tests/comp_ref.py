"""Plain high-precision references for the compartment kernels (comp.hip):
the column Pearson correlation in extended precision and a matrix whose PCA
components are known exactly.  NumPy only; nothing here imports the package
under test (tests/test_comp_ref_cpu.py pins both against LAPACK / corrcoef).
"""
import numpy as np


def corr_ld(X):
    """np.corrcoef(X, rowvar=False) with NaN -> 0 (Get_PCA, StructureFind.py
    :335-337) in ``np.longdouble``: centre, X^T X / (N - 1), divide by both
    standard deviations, clip to [-1, 1]; float64 at the end.  A constant
    column has sd 0: its row and column are 0 / 0 = NaN -> 0."""
    X = np.asarray(X, dtype=np.longdouble)
    N = X.shape[0]
    Z = X - X.sum(axis=0) / np.longdouble(N)
    cov = (Z.T @ Z) / np.longdouble(N - 1)
    sd = np.sqrt(np.diagonal(cov))
    with np.errstate(invalid="ignore", divide="ignore"):
        C = cov / sd[:, None] / sd[None, :]
    C = np.clip(C, -1, 1)  # (NaN stays NaN)
    C[np.isnan(C)] = 0
    return np.asarray(C, dtype=np.float64)


def planted(n, s, seed, rest=0.01):
    """Symmetric n x n matrix with zero column means and eigenvalues ``s``
    then ``rest`` (n - 1 of them; the last is 0, eigenvector 1): Xc = Cor, so
    the PCA components are its top eigenvectors and the PCA eigenvalues the
    squares.  Returns (Cor, U): U's columns are the eigenvectors of ``s``,
    exactly orthonormal up to the rounding of one QR.  Only n - 1 directions
    are orthogonal to 1, so for tiny n ``s`` is cut to its first n - 1."""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, n))
    Z -= Z.mean(axis=0)
    U, _ = np.linalg.qr(Z)
    U = U[:, : n - 1]  # orthonormal, orthogonal to 1
    s = np.asarray(s, dtype=np.float64)[: n - 1]
    vals = np.full(n - 1, rest)
    vals[: len(s)] = s
    return (U * vals) @ U.T, U[:, : len(s)]
