"""Trans-contact compartment eigenvectors.

HiCHap has no such function and cooltools is absent: the definition is this
project's.  The genome, the pixels, ``v(a, b) = count * weight[a] * weight[b]``
(NaN -> 0), ``use``, ``bad`` and ``valid`` are ``trans.py``'s.  ``T[i][j] =
v(min, max)`` for valid i, j on different chromosomes (0 elsewhere, the cis
blocks empty) is symmetric; ``TransOperator`` owns the handle of its two
row-compressed tables on the GPU (``hh_teig_*``, csrc/transeig.hip) and
``apply`` computes ``D T (D X)``, the one hot path.  Around it, on the host:

* ``trans_normalise``: ``d >= 0`` with every valid row's mean over its valid
  trans partners equal to 1, ``d_i * sum_j T_ij d_j = ntp(i)`` (``ntp(i)`` the
  valid bins outside the chromosome of i); one ``k = 1`` product per iteration;
* ``mask_product``: ``M X`` with ``M[i][j] = 1`` for valid i, j on different
  chromosomes, from per-chromosome column sums (no pixel);
* ``apply_E``: ``E X = D T D X - M X``; the cis blocks of E are 0, the
  expectation of cooltools' random cis fill;
* ``top_eigs``: the k algebraically largest eigenpairs of a symmetric operator
  given as a callable, by explicitly restarted block Krylov with Rayleigh-Ritz
  (block k + 4, 3 products per cycle; QR and the small ``eigh`` in NumPy);
* ``orient``, ``write_transeig`` and ``TransEigCalling.run_TransEig``, mixed
  into ``StructureFind``.

The product and ``d`` are reproducible to the bit; the eigenvectors go through
LAPACK on the host and are reproducible to the tolerance.
"""
from __future__ import annotations

import ctypes
import time

import numpy as np

from ._lib import call, ptr, require_gpu
from ._pixels import empty, host_or_dev, is_dev
from .trans import MAX_CHROMS, _genome_table, valid_bins

MAX_K = 8          # HH_TEIG_MAX_K
BLOCK_EXTRA = 4    # block b = k + 4
PRODUCTS = 3       # operator products per cycle


def _host(a, dtype=None):
    if a is None:
        return None
    if is_dev(a):
        a = a.cpu().numpy()
    return np.asarray(a) if dtype is None else np.asarray(a, dtype=dtype)


def trans_partners(chrom_offset, valid):
    """``ntp`` (int64[n_bins]): for a valid bin the number of valid bins on
    the other chromosomes, 0 for an invalid one.  Host integer arithmetic."""
    off = np.asarray(chrom_offset, dtype=np.int64)
    v = np.asarray(valid) != 0
    csum = np.concatenate([[0], np.cumsum(v, dtype=np.int64)])
    per = csum[off[1:]] - csum[off[:-1]]
    return np.where(v, int(per.sum()) - np.repeat(per, np.diff(off)), 0).astype(np.int64)


def mask_product(X, valid, chrom_offset):
    """``M X`` for ``M[i][j] = 1`` where i and j are valid and on different
    chromosomes: ``(M X)_i = valid_i * (S - S_c(i))``, ``S_q`` the sum of X
    over the valid bins of chromosome q added in ascending bin order from the
    first (``np.cumsum``: a sequential sum), S the ``S_q`` added in ascending
    q.  X: float64[n] or [n, k]."""
    off = np.asarray(chrom_offset, dtype=np.int64)
    X = np.asarray(X, dtype=np.float64)
    flat = X.ndim == 1
    X2 = X.reshape(X.shape[0], -1)
    v = np.asarray(valid) != 0
    C = off.size - 1
    Sq = np.zeros((C, X2.shape[1]))
    for q in range(C):
        rows = X2[off[q]:off[q + 1]][v[off[q]:off[q + 1]]]
        if rows.shape[0]:
            Sq[q] = np.cumsum(rows, axis=0)[-1]
    S = np.cumsum(Sq, axis=0)[-1]
    out = np.where(v[:, None], S[None, :] - np.repeat(Sq, np.diff(off), axis=0), 0.0)
    return out[:, 0] if flat else out


class _Scaled:
    """What the two operators share: the genome, ``valid`` (uint8[n_bins],
    the validity the tables were built with), and ``d`` / ``valid_now`` as
    ``trans_normalise`` set them (before it: all ones on the valid bins)."""

    def _genome(self, off, C, wt, use, bad):
        self.chrom_offset, self.C, self.n = off, C, int(off[-1])
        self.valid, self.n_valid = valid_bins(off, _host(wt), use, _host(bad))
        self.valid_now = self.valid != 0
        self.d = self.valid.astype(np.float64)
        self._d_dev = None
        self.products = 0          # operator columns applied

    def set_scaling(self, d, valid_now=None):
        self.d = np.ascontiguousarray(d, dtype=np.float64)
        self.valid_now = (self.valid != 0) if valid_now is None else np.asarray(valid_now, bool)
        self._d_dev = None

    def apply_E(self, X):
        """``E X = D T D X - M X`` with the scaling and the validity of the
        last ``trans_normalise``; rows of bins that are not valid are 0.  The
        ``M X`` term is host arithmetic (``mask_product``)."""
        X = np.asarray(X, dtype=np.float64)
        Y = self.apply(X, self.d) - mask_product(X, self.valid_now, self.chrom_offset)
        Y[~self.valid_now] = 0.0
        return Y


class HostTransOperator(_Scaled):
    """The same operator in NumPy from the pixel table itself: two weighted
    ``np.bincount`` passes per column (the row half and the column half).  The
    host baseline of ``tools/bench_transeig.py`` and the operator of the tests
    that run without a GPU; ``run_TransEig`` never uses it."""

    def __init__(self, bin1, bin2, count, weight, chrom_offset, use=None, bad=None):
        off = np.ascontiguousarray(chrom_offset, dtype=np.int64)
        self._genome(off, off.size - 1, weight, use, bad)
        b1, b2 = np.asarray(bin1, dtype=np.int64), np.asarray(bin2, dtype=np.int64)
        v = np.asarray(count, dtype=np.float64)
        if weight is not None:
            w = np.asarray(weight, dtype=np.float64)
            with np.errstate(invalid="ignore"):
                v = np.nan_to_num(v * w[b1] * w[b2], nan=0.0, posinf=np.inf, neginf=-np.inf)
        chrom = np.repeat(np.arange(self.C), np.diff(off))
        keep = (self.valid[b1] != 0) & (self.valid[b2] != 0) & (chrom[b1] != chrom[b2])
        self.a, self.b, self.v = b1[keep], b2[keep], v[keep]
        self.nnz = int(self.a.size)

    def apply(self, X, d=None):
        X = np.asarray(X, dtype=np.float64)
        X2 = X.reshape(X.shape[0], -1)
        dd = np.ones(self.n) if d is None else np.asarray(d, dtype=np.float64)
        Y = np.zeros(X2.shape)
        for c in range(X2.shape[1]):
            z = np.where(self.valid != 0, dd * X2[:, c], 0.0)
            Y[:, c] = (np.bincount(self.a, weights=self.v * z[self.b], minlength=self.n)
                       + np.bincount(self.b, weights=self.v * z[self.a], minlength=self.n))
            Y[:, c] = np.where(self.valid != 0, dd * Y[:, c], 0.0)
        self.products += X2.shape[1]
        return Y[:, 0] if X.ndim == 1 else Y


class TransOperator(_Scaled):
    """The symmetric trans matrix T of one pixel table on the GPU (a context
    manager over an ``hh_teig`` handle)."""

    def __init__(self, bin1, bin2, count, weight, chrom_offset, use=None, bad=None, stream=None):
        require_gpu()
        dev, b1, b2, c, wt, off, C, use, bad = _genome_table(bin1, bin2, count, weight, chrom_offset, use, bad)
        self.stream = stream
        self._h = None
        self._genome(off, C, wt, use, bad)
        h = ctypes.c_void_p()
        call("hh_teig_create", ptr(b1), ptr(b2), ptr(c), int(b1.shape[0]), ptr(wt),
             0 if wt is None else int(wt.shape[0]), ptr(off), C, ptr(use), ptr(bad), 0 if dev is None else 1, stream,
             ctypes.byref(h))
        self._h = h
        u, lo = ctypes.c_int64(), ctypes.c_int64()
        call("hh_teig_nnz", self._h, ctypes.byref(u), ctypes.byref(lo))
        self.nnz = int(u.value)

    def close(self):
        if self._h is not None:
            call("hh_teig_free", self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def tables(self):
        """``{'upper': (rowptr, partner, value), 'lower': ...}`` as host
        arrays (int64[n + 1], int32[nnz], float64[nnz])."""
        out = {}
        for which, name in enumerate(("upper", "lower")):
            rp = np.zeros(self.n + 1, np.int64)
            p, v = np.zeros(self.nnz, np.int32), np.zeros(self.nnz, np.float64)
            call("hh_teig_export", self._h, which, ptr(rp), ptr(p) if self.nnz else None,
                 ptr(v) if self.nnz else None)
            out[name] = (rp, p, v)
        return out

    def _apply8(self, d, X, dev):
        Y = empty(tuple(X.shape), np.float64, dev)
        call("hh_teig_apply", self._h, ptr(d), ptr(X), int(X.shape[1]), ptr(Y), 0 if dev is None else 1, self.stream)
        self.products += int(X.shape[1])
        return Y

    def apply(self, X, d=None):
        """``D T (D X)`` for X float64[n] or [n, k] (any k: the columns go to
        the GPU in groups of 8); ``d`` float64[n] or None for all ones.  A
        torch tensor on the GPU is used in place and the result stays there."""
        dev = X.device if is_dev(X) else None
        flat = X.ndim == 1
        X2 = host_or_dev(X.reshape(X.shape[0], -1), np.float64, dev)
        if tuple(X2.shape)[0] != self.n:
            raise ValueError("X must have one row per bin of the genome")
        d = host_or_dev(d, np.float64, dev)
        if d is not None and tuple(d.shape) != (self.n,):
            raise ValueError("d must have one entry per bin of the genome")
        k = int(X2.shape[1])
        if k <= MAX_K:
            Y = self._apply8(d, X2, dev)
        else:
            parts = []
            for c0 in range(0, k, MAX_K):
                part = X2[:, c0:c0 + MAX_K]
                part = part.contiguous() if dev is not None else np.ascontiguousarray(part)
                parts.append(self._apply8(d, part, dev))
            if dev is None:
                Y = np.concatenate(parts, axis=1)
            else:
                import torch
                Y = torch.cat(parts, dim=1)
        return Y[:, 0] if flat else Y

    def apply_E(self, X):
        """``E X = D T D X - M X`` with the scaling and the validity of the
        last ``trans_normalise``; rows of bins that are not valid are 0.  The
        ``M X`` term is host arithmetic (``mask_product``); for a torch tensor
        on the GPU it is computed from a host copy and the result stays on
        the device."""
        if not is_dev(X):
            return _Scaled.apply_E(self, X)
        import torch
        if self._d_dev is None or self._d_dev.device != X.device:
            self._d_dev = torch.from_numpy(self.d).to(X.device)
        Y = self.apply(X, self._d_dev)
        MX = torch.from_numpy(mask_product(X.cpu().numpy(), self.valid_now, self.chrom_offset)).to(X.device)
        keep = torch.from_numpy(self.valid_now).to(X.device)
        Y = Y - MX
        return torch.where(keep if Y.ndim == 1 else keep[:, None], Y, torch.zeros_like(Y))


def trans_normalise(op, tol=1e-6, max_iter=500):
    """The trans normalisation of ``op``: start from ``d = valid``; every
    iteration ``s = d * (T d)`` (one k = 1 product); a valid bin with ``s_i ==
    0`` becomes invalid (``d_i = 0``), ``ntp`` is recomputed and the iteration
    is not counted; otherwise ``r = s / ntp``, stop when ``max |r - 1| < tol``,
    else ``d /= sqrt(r)``.  Sets ``op.d`` / ``op.valid_now`` and returns
    ``dict(d, valid, ntp, iterations, deviation, converged)``; not converging
    is reported, not raised.  Without a trans pixel or a valid bin: d all 0,
    0 iterations, deviation NaN."""
    return normalise_with(lambda d: op.apply(np.ones(op.n), d), op.valid, op.chrom_offset, tol, max_iter,
                          setter=op.set_scaling, empty_table=op.nnz == 0)


def normalise_with(product, valid, chrom_offset, tol=1e-6, max_iter=500, setter=None, empty_table=False):
    """``trans_normalise`` over a callable ``product(d) -> d * (T d)``."""
    valid_now = np.asarray(valid) != 0
    n = valid_now.size
    d = valid_now.astype(np.float64)
    ntp = trans_partners(chrom_offset, valid_now)
    iters, dev_, conv = 0, np.nan, False
    if empty_table:
        valid_now = np.zeros(n, bool)
    while valid_now.any() and iters < max_iter:
        s = np.asarray(product(d), dtype=np.float64)
        dead = valid_now & (s == 0)
        if dead.any():
            valid_now = valid_now & ~dead
            d[dead] = 0.0
            ntp = trans_partners(chrom_offset, valid_now)
            continue
        iters += 1
        r = s[valid_now] / ntp[valid_now]
        dev_ = float(np.max(np.abs(r - 1.0)))
        if dev_ < tol:
            conv = True
            break
        d[valid_now] = d[valid_now] / np.sqrt(r)
    if not valid_now.any():
        d = np.zeros(n)
        ntp = np.zeros(n, np.int64)
        dev_, conv = np.nan, False
    if setter is not None:
        setter(d, valid_now)
    return dict(d=d, valid=valid_now, ntp=ntp, iterations=iters, deviation=dev_, converged=conv)


def _dense_of(apply, n, idx):
    """The operator on the rows / columns idx as a dense matrix (tiny cases)."""
    m = idx.size
    A = np.zeros((m, m))
    for c0 in range(0, m, MAX_K):
        X = np.zeros((n, min(MAX_K, m - c0)))
        X[idx[c0:c0 + X.shape[1]], np.arange(X.shape[1])] = 1.0
        A[:, c0:c0 + X.shape[1]] = np.asarray(apply(X))[idx]
    return 0.5 * (A + A.T)


def top_eigs(apply, n, k, valid=None, tol=1e-8, max_cycles=200, seed=0):
    """The k algebraically largest eigenpairs of the symmetric operator
    ``apply(X) -> E X`` (X float64[n, m]) on the subspace of the valid bins.

    Explicitly restarted block Krylov with Rayleigh-Ritz: block b = k + 4; a
    cycle orthonormalises [V0, E V0, E V1, E V2] block by block (two passes of
    block Gram-Schmidt and a QR), 3 products of b columns (``E V0`` of a
    restarted cycle is the Ritz combination of products already made), takes
    the Ritz pairs of the 4 b-dimensional basis and keeps the b with the
    largest theta.  Stops when ``max_c ||E x_c - theta_c x_c|| <= tol *
    |theta_1|`` over the first k.  A subspace of fewer than 4 b + 1 valid bins
    is solved densely.  Returns ``dict(values[k], vectors[n, k] (unit 2-norm,
    0 on the invalid bins), residuals[k], cycles, converged, columns,
    t_product, t_host)``."""
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("top_eigs: k must be in 1..8")
    idx = np.arange(n) if valid is None else np.nonzero(np.asarray(valid) != 0)[0]
    nv = idx.size
    out = dict(values=np.full(k, np.nan), vectors=np.zeros((n, k)), residuals=np.full(k, np.nan), cycles=0,
               converged=False, columns=0, t_product=0.0, t_host=0.0)
    if nv == 0:
        return out
    b, t_prod, cols = k + BLOCK_EXTRA, 0.0, 0
    t_start = time.perf_counter()

    def product(Vc):
        nonlocal t_prod, cols
        X = np.zeros((n, Vc.shape[1]))
        X[idx] = Vc
        t0 = time.perf_counter()
        Y = np.asarray(apply(X), dtype=np.float64)
        t_prod += time.perf_counter() - t0
        cols += Vc.shape[1]
        return Y[idx]

    if nv <= (PRODUCTS + 1) * b:
        t0 = time.perf_counter()
        A = _dense_of(apply, n, idx)
        t_prod += time.perf_counter() - t0
        cols += nv
        lam, V = np.linalg.eigh(A)
        lam, V = lam[::-1], V[:, ::-1]
        kk = min(k, nv)
        out["values"][:kk] = lam[:kk]
        out["vectors"][idx, :kk] = V[:, :kk]
        out["residuals"][:kk] = np.linalg.norm(A @ V[:, :kk] - V[:, :kk] * lam[:kk], axis=0)
        out.update(cycles=0, converged=True, columns=cols, t_product=t_prod,
                   t_host=time.perf_counter() - t_start - t_prod)
        return out

    rng = np.random.default_rng(seed)
    V0, _ = np.linalg.qr(rng.standard_normal((nv, b)))
    AV0 = None
    theta = res = None
    for cycle in range(1, int(max_cycles) + 1):
        if AV0 is not None:     # a restart: the Ritz block orthonormal to working precision again
            V0, R = np.linalg.qr(V0)
            AV0 = np.linalg.solve(R.T, AV0.T).T
        Q, AQ = [V0], []
        for j in range(PRODUCTS + 1):
            AVj = product(Q[j]) if (j > 0 or AV0 is None) else AV0
            AQ.append(AVj)
            if j == PRODUCTS:
                break
            W = AVj.copy()
            for _ in range(2):      # the second pass also cleans the columns a rank-deficient QR made up
                for Vp in Q:
                    W -= Vp @ (Vp.T @ W)
                W, _ = np.linalg.qr(W)
            Q.append(W)
        Qm, AQm = np.hstack(Q), np.hstack(AQ)
        H = Qm.T @ AQm
        th, y = np.linalg.eigh(0.5 * (H + H.T))
        th, y = th[::-1][:b], y[:, ::-1][:, :b]
        V0, AV0 = Qm @ y, AQm @ y
        theta = th[:k]
        res = np.linalg.norm(AV0[:, :k] - V0[:, :k] * theta, axis=0)
        out["cycles"] = cycle
        if res.max() <= tol * abs(theta[0]):
            out["converged"] = True
            break
    X = V0[:, :k] / np.linalg.norm(V0[:, :k], axis=0)
    out["values"], out["residuals"] = theta.copy(), res
    out["vectors"][idx] = X
    out.update(columns=cols, t_product=t_prod, t_host=time.perf_counter() - t_start - t_prod)
    return out


def orient(vecs, valid, phasing=None):
    """The sign of every column of ``vecs`` (float64[n, k]; a copy is
    returned): with ``phasing`` (float64[n], NaN allowed) the Pearson
    correlation with it over the valid bins where both are finite is made >=
    0; without one, or where that correlation is undefined, the entry of
    largest magnitude (the lowest bin on ties) is made positive."""
    V = np.array(vecs, dtype=np.float64, copy=True)
    ok = np.asarray(valid) != 0
    ph = None if phasing is None else np.asarray(phasing, dtype=np.float64)
    for c in range(V.shape[1]):
        x = V[:, c]
        fin = ok & np.isfinite(x)
        if not fin.any():
            continue
        sign = 0.0
        if ph is not None:
            both = fin & np.isfinite(ph)
            if both.sum() >= 2:
                a, p = x[both] - x[both].mean(), ph[both] - ph[both].mean()
                den = np.sqrt((a * a).sum() * (p * p).sum())
                if den > 0:
                    sign = np.sign((a * p).sum() / den)
        if sign == 0.0:
            mag = np.where(fin, np.abs(x), -1.0)
            sign = 1.0 if x[int(np.argmax(mag))] >= 0 else -1.0
        if sign < 0:
            V[:, c] = -x
    return V


def write_transeig(eig_fil, values_fil, pc_fil, names, chrom_offset, sel, res, valid, d, E, values, residuals,
                   iterations, deviation):
    """The three text files of ``run_TransEig`` (tab-separated, floats as
    Python 2 printed them, NaN as 'nan').  ``names``: the chromosomes' names as
    shown, ``sel`` the indices of the selected ones in file order, ``E``
    float64[n, k] the scaled eigenvectors.  ``eig_fil``: chrom, start, end,
    valid, d, E1..Ek per bin; ``values_fil``: index, eigenvalue, residual per
    eigenpair, then the normalisation's iterations and final deviation;
    ``pc_fil``: 'chrom value' lines of E1 (``Loading_Tranditional_PC``'s
    layout)."""
    from .StructureFind import py2_float_str
    off = np.asarray(chrom_offset, dtype=np.int64)
    k = E.shape[1]
    with open(eig_fil, "w") as f, open(pc_fil, "w") as g:
        f.write("\t".join(["chrom", "start", "end", "valid", "d"] + [f"E{c + 1}" for c in range(k)]) + "\n")
        for p in sel:
            for x in range(int(off[p]), int(off[p + 1])):
                r = x - int(off[p])
                f.write("\t".join([names[p], str(r * res), str((r + 1) * res), str(int(valid[x])), py2_float_str(d[x])]
                                  + [py2_float_str(E[x, c]) for c in range(k)]) + "\n")
                g.write(f"{names[p]}\t{py2_float_str(E[x, 0])}\n")
    with open(values_fil, "w") as f:
        f.write("index\teigenvalue\tresidual\n")
        for c in range(k):
            f.write(f"{c + 1}\t{py2_float_str(values[c])}\t{py2_float_str(residuals[c])}\n")
        f.write(f"iterations\t{int(iterations)}\n")
        f.write(f"deviation\t{py2_float_str(deviation)}\n")


def trans_eigs(op, n_eigs=3, phasing=None, tol=1e-6, max_iter=500, tol_eig=1e-8, max_cycles=200, seed=0):
    """Normalisation, solver and orientation on one ``TransOperator``:
    ``dict(valid, d, ntp, iterations, deviation, normalised, eigenvalues[k],
    residuals[k], vectors[n, k] (unit 2-norm over the valid bins, NaN on the
    others), E[n, k] = vectors * sqrt(max(eigenvalue, 0)), cycles, converged,
    columns, t_product, t_host)``.  Without a valid trans pixel every float
    output is NaN and d is all 0."""
    k = int(n_eigs)
    if not 1 <= k <= MAX_K:
        raise ValueError("n_eigs must be in 1..8")
    nrm = trans_normalise(op, tol, max_iter)
    n = op.n
    r = dict(valid=nrm["valid"].astype(np.uint8), d=nrm["d"], ntp=nrm["ntp"], iterations=nrm["iterations"],
             deviation=nrm["deviation"], normalised=nrm["converged"])
    if not nrm["valid"].any():
        r.update(eigenvalues=np.full(k, np.nan), residuals=np.full(k, np.nan), vectors=np.full((n, k), np.nan),
                 E=np.full((n, k), np.nan), cycles=0, converged=False, columns=0, t_product=0.0, t_host=0.0)
        return r
    s = top_eigs(op.apply_E, n, k, nrm["valid"], tol_eig, max_cycles, seed)
    V = s["vectors"].copy()
    V[~nrm["valid"]] = np.nan
    V[:, ~np.isfinite(s["values"])] = np.nan
    V = orient(V, nrm["valid"], phasing)
    with np.errstate(invalid="ignore"):
        E = V * np.sqrt(np.maximum(s["values"], 0.0))
    r.update(eigenvalues=s["values"], residuals=s["residuals"], vectors=V, E=E, cycles=s["cycles"],
             converged=s["converged"], columns=s["columns"], t_product=s["t_product"], t_host=s["t_host"])
    return r


class TransEigCalling:
    """The trans eigenvector method of ``StructureFind``."""

    def run_TransEig(self, OutPath, n_eigs=3, phasing=None, PC_file=None, tol=1e-6, tol_eig=1e-8, seed=0):
        """Compartment eigenvectors from the contacts between chromosomes
        (DESIGN.md §4t): one walk over the cooler, the whole pixel table read
        once, one ``TransOperator``, the trans normalisation, the ``n_eigs``
        algebraically largest eigenpairs of ``E = D T D - M`` and their
        orientation.  Geometry, weights and invalid bins are ``run_Trans``'s:
        traditional data uses ``bins/weight``; haplotype data ('Maternal' /
        'Paternal') the chromosomes with that prefix, the raw counts and the
        gap lists as invalid bins when a ``GapFile`` was given.  The phasing
        track that fixes the signs is ``phasing`` ({chrom: array}, NaN
        allowed), else ``Compartment_Dict`` of an earlier ``Compartment`` run,
        else ``PC_file``; without any of them the entry of largest magnitude
        of every vector is positive.  Writes ``<prefix>_TransEig_<res>.txt``
        (chrom, start, end, valid, d, E1..Ek; E = unit vector * sqrt(max(
        eigenvalue, 0))), ``<prefix>_TransEigValues_<res>.txt`` (index,
        eigenvalue, residual; then the normalisation's iterations and final
        deviation) and ``<prefix>_TransEigPC_<res>.txt`` ('chrom value' lines
        of E1, which ``run_Trans(PC_file=...)`` and ``run_Saddle(PC_file=...)``
        read), haplotype chromosomes without their M/P prefix.  Returns (and
        keeps as ``TransEig_dict``) the arrays."""
        from .coolio import Cooler
        self._chroms()
        stream = getattr(self, "stream", None)
        with_track = phasing is not None or bool(getattr(self, "Compartment_Dict", None)) or PC_file is not None
        with Cooler(self.cooler_fil) as c:
            geom = list(self._cooler_walk(c, "run_TransEig"))
            chroms = list(c.chromnames)
            off = c.chrom_offsets()
            C = len(chroms)
            if C > MAX_CHROMS:
                raise ValueError(f"run_TransEig: {C} chromosomes, at most {MAX_CHROMS}")
            sel = [chroms.index(row[0]) for row in geom]
            use = None
            if len(sel) < C:
                use = np.zeros(C, np.uint8)
                use[sel] = 1
            wt = geom[0][3] if geom else None
            bad = None
            if any(row[4] is not None for row in geom):
                bad = np.zeros(int(off[-1]), np.uint8)
                for _, lo, N, _, b, _ in geom:
                    if b is not None:
                        bad[lo:lo + N] = b
            n = int(off[-1])
            track = None
            if with_track:
                tracks = self._saddle_track(phasing, PC_file, [row[0] for row in geom], self._name)
                track = np.full(n, np.nan)
                for chro, lo, N, *_ in geom:
                    if tracks[chro].shape != (N,):
                        raise ValueError(f"run_TransEig: the track of {chro} has {tracks[chro].size} values, "
                                         f"the chromosome {N} bins")
                    track[lo:lo + N] = tracks[chro]
            b1, b2, cnt = c.pixels_table()
            with TransOperator(b1, b2, cnt, wt, off, use, bad, stream) as op:
                r = trans_eigs(op, n_eigs, track, tol=tol, tol_eig=tol_eig, seed=seed)
                r.update(nnz=op.nnz, valid_input=op.valid)
        names = [self._name(x) if k in sel else x for k, x in enumerate(chroms)]
        r.update(chroms=chroms, selected=sel, chrom_offset=off)
        r["files"] = (self._out_path(OutPath, "TransEig"), self._out_path(OutPath, "TransEigValues"),
                      self._out_path(OutPath, "TransEigPC"))
        write_transeig(*r["files"], names, off, sel, int(self.Res), r["valid"], r["d"], r["E"], r["eigenvalues"],
                       r["residuals"], r["iterations"], r["deviation"])
        self.TransEig_dict = r
        return r
