"""Measure the stratum moments of the reproducibility score (hh_scc_pixels;
csrc/scc.hip) at their largest default shape: one synthetic
chromosome at chr1's 10 kb size with C2's generator parameters, h = 20 bins,
max_dist = 5 Mb (500 bins), ignore_diags 1.  The two tables differ by their
Poisson draw alone: the generator's counts c (Poisson of intensity lambda) are
split into Binomial(c, 1/2) and the rest, two independent Poisson draws of
lambda / 2.  Both use the ICE weights of the unsplit table; tables and
weights are in HBM.

It prints one line each for
  * the input and the bytes the call has to move,
  * the host-clock time of one on-device call (median over enough repeats to
    fill --seconds, after a warm-up) and the per-kernel split (hh_ktime: HIP
    events around every launch), with the compulsory bytes / time next to the
    measured linear-read rate of 6.2 TB/s and the cells per second,
  * with --rows, the call again at other rows per work item (hh_tune
    "scc_rows"; n stays the same, the sums within the rounding bound),
  * a vectorised NumPy computation of the same definition on the host (the
    band of diagonals -2h .. max_dist + 2h as an N x W array, the box sums as
    2 (2h + 1) shifted additions): the host baseline, its time, and the
    agreement of n (exactly), of the five sums and of the SCC.

A run without a GPU fails; there is no fallback.

    python tools/bench_scc.py [--nnz 5e7] [--seconds 1.0] [--h 20] [--rows 16,24]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RES = 10000
LINEAR_READ = 6.2e12        # B/s, profiles/r6d/probe.log
KERNELS = ("k_sd_rowptr", "k_scc_moments", "k_scc_sum")


def timed(run, seconds):
    import torch
    out = run()                                                      # warm-up (allocations)
    torch.cuda.synchronize()
    ts = []
    t_end = time.perf_counter() + seconds
    while time.perf_counter() < t_end or len(ts) < 5:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        again = run()
        ts.append(time.perf_counter() - t0)                          # the call synchronises its stream
    assert all(torch.equal(a, b) for a, b in zip(out, again))        # fixed order: the same bits
    return out, ts


def kernel_times(run, names, reps=5):
    from hichap_master_amd import _lib
    _lib.call("hh_ktime_reset")
    _lib.call("hh_ktime_enable", 1)
    for _ in range(reps):
        run()
    _lib.call("hh_synchronize", None)
    _lib.call("hh_ktime_enable", 0)
    return {k: _lib.ktime(k)[0] / reps * 1e-3 for k in names}        # seconds per call


def host_moments(tables, w, valid, N, h, g, D):
    """(n, S) by the definition, vectorised: band[a, k + 2h] = x(a, a + k) for k
    in [-2h, D + 2h]; H = the sums over 2h + 1 neighbouring k (the window's
    columns), SX[a, k] = sum over p of H[a + p, k - p] (the window's rows)."""
    W = D + 4 * h + 1
    nv = np.convolve(valid.astype(np.int64), np.ones(2 * h + 1, np.int64))[h:h + N]
    SXY = []
    for b1, b2, c in tables:
        d = b2 - b1
        ok = (d <= D + 2 * h) & (d >= g) & valid[b1] & valid[b2]
        i, j, d = b1[ok], b2[ok], d[ok]
        v = np.nan_to_num(c[ok] * w[i] * w[j])
        band = np.zeros((N + 2 * h, W))                              # rows [-h, N + h)
        band[i + h, d + 2 * h] = v
        lower = (d > 0) & (d <= 2 * h)
        band[j[lower] + h, 2 * h - d[lower]] = v[lower]
        H = np.zeros((N + 2 * h, D + 2 * h + 1))                     # k in [-h, D + h]
        for q in range(2 * h + 1):
            H += band[:, q:q + D + 2 * h + 1]
        SX = np.zeros((N, D + 1))                                    # k in [0, D]
        for p in range(-h, h + 1):
            SX += H[h + p:h + p + N, h - p:h - p + D + 1]
        SXY.append(SX)
    a = np.arange(N)[:, None]
    k = np.arange(D + 1)[None, :]
    b = np.minimum(a + k, N - 1)
    cell = (a + k < N) & (k >= g) & valid[a] & valid[b] & ((SXY[0] != 0) | (SXY[1] != 0))
    den = (nv[a] * nv[b]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):       # (a bin whose whole window is masked is no cell)
        X, Y = np.where(cell, SXY[0] / den, 0.0), np.where(cell, SXY[1] / den, 0.0)
    return cell.sum(axis=0), np.stack([X.sum(0), Y.sum(0), (X * X).sum(0), (Y * Y).sum(0), (X * Y).sum(0)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nnz", type=float, default=5e7)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--h", type=int, default=20)
    ap.add_argument("--max-dist", type=int, default=5000000)
    ap.add_argument("--ignore-diags", type=int, default=1)
    ap.add_argument("--rows", default="", help="also time the call at these scc_rows values")
    a = ap.parse_args()

    import torch
    from hichap_master_amd import _lib, ice, synth
    from hichap_master_amd import reproducibility as rp

    _lib.require_gpu()
    sizes = [synth.chrom_bins([synth.HG19["1"]], RES)[0]]
    A, td = synth.calibrate(sizes, a.nnz, 0.0)
    m = ice.ContactMatrix.synthetic(sizes, A=A, trans_density=td, comp_block=200, seed=20201015)
    w, st = ice.balance_matrix(m)
    b1, b2, c = m.export_upper()
    m.close()
    N = int(sizes[0])
    key = b1 * N + b2                                                # cooler's order: sorted by (bin1, bin2)
    if np.any(np.diff(key) <= 0):
        o = np.argsort(key, kind="stable")
        b1, b2, c = b1[o], b2[o], c[o]
    del key
    ca = np.random.default_rng(1).binomial(c.astype(np.int64), 0.5)  # Poisson splitting: two independent draws
    tables = []
    for cnt in (ca, c.astype(np.int64) - ca):
        keep = cnt > 0
        tables.append((b1[keep], b2[keep], cnt[keep].astype(np.float64)))
    del b1, b2, c, ca
    h, g, D = a.h, a.ignore_diags, min(N - 1, a.max_dist // RES)
    valid = np.isfinite(w)
    R = max(32, min(64, (72 - 2 * h) // 8 * 8))
    near = [int(np.count_nonzero(t[1] - t[0] <= D + 2 * h)) for t in tables]
    must = 16 * sum(near)
    cells = int((N - np.arange(g, D + 1)).sum())
    print(f"input: N = {N} bins, {tables[0][0].size} and {tables[1][0].size} pixels ({near[0]} and {near[1]} within "
          f"max_dist + 2h), {int((~valid).sum())} masked bins; h = {h}, ignore_diags {g}, max_dist {D} bins, "
          f"{cells} cells, {R} rows x 32 strata per work item, patches of {R + 2 * h} x {R + 31 + 2 * h} cells "
          f"= {16 * (R + 2 * h) * (R + 31 + 2 * h) / 1024:.0f} KiB of LDS.  Bytes from HBM per call, compulsory: "
          f"bin2 and count of the pixels within max_dist + 2h of both tables, 16 B/pixel = {must * 1e-6:.0f} MB "
          f"(a work item reads its patch's pixels again: {(R + 2 * h) * (R + 31 + 2 * h) / (R * 32):.1f} x as "
          f"many cells as it owns, from the caches)")

    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dw = dev(w)
    (a1, a2, ac), (e1, e2, ec) = [[dev(x) for x in t] for t in tables]
    run = lambda: rp.scc_pixels((a1, a2, ac, dw, 0), (e1, e2, ec, dw, 0), N, h, g, D)
    (n, S), ts = timed(run, a.seconds)
    kt = kernel_times(run, KERNELS)
    t_dev = float(np.median(ts))
    print(f"hh_scc_pixels on device: {t_dev * 1e3:.2f} ms per call (median of {len(ts)}, min {min(ts) * 1e3:.2f}); "
          f"kernels: " + ", ".join(f"{k} {t * 1e6:.0f} us" for k, t in kt.items())
          + f"; k_scc_moments: {must / kt['k_scc_moments'] * 1e-12:.3f} TB/s of compulsory bytes = "
          f"{100 * must / kt['k_scc_moments'] / LINEAR_READ:.1f} % of 6.2 TB/s, "
          f"{cells / kt['k_scc_moments'] * 1e-9:.2f} G cells/s, "
          f"{cells * (4 * h + 2) * 8 / kt['k_scc_moments'] * 1e-12:.2f} TB/s of LDS reads in the column pass")
    nh, Sh = n.cpu().numpy(), S.cpu().numpy()
    u53 = 2.0 ** -53
    rtol = 2 * (int(nh.max()) + 2 * (2 * h + 1) ** 2 + 4) * u53
    for rows in [int(x) for x in a.rows.split(",") if x]:
        _lib.call("hh_tune", b"scc_rows", rows)
        (n2, S2), ts2 = timed(run, a.seconds / 2)
        _lib.call("hh_tune", b"scc_rows", 0)
        assert torch.equal(n, n2)
        np.testing.assert_allclose(S2.cpu().numpy(), Sh, rtol=rtol, atol=0)
        print(f"  scc_rows {rows}: {np.median(ts2) * 1e3:.2f} ms per call (n the same, sums within the bound)")

    # host baseline: the same definition, vectorised NumPy on the band
    t0 = time.perf_counter()
    n_np, S_np = host_moments(tables, w, valid, N, h, g, D)
    t_np = time.perf_counter() - t0
    assert np.array_equal(nh[g:], n_np[g:]) and not nh[:g].any() and not Sh[:, :g].any()
    np.testing.assert_allclose(Sh[:, g:], S_np[:, g:], rtol=rtol, atol=0)
    dev_scc, np_scc = rp.scc_from_moments(nh, Sh), rp.scc_from_moments(n_np * (np.arange(D + 1) >= g), S_np)
    err = np.nanmax(np.abs(dev_scc["rho"] - np_scc["rho"]))
    assert abs(dev_scc["scc"] - np_scc["scc"]) < 1e-9 and err < 1e-9
    print(f"agreement: n equals NumPy's exactly, the five sums within 2 (m + 2 (2h + 1)^2 + 4) 2^-53 (largest "
          f"relative difference {np.max(np.abs(Sh[:, g:] - S_np[:, g:]) / S_np[:, g:]):.3g}), SCC "
          f"{dev_scc['scc']:.9f} on the device and {np_scc['scc']:.9f} on the host over "
          f"{int(dev_scc['usable'].sum())} usable strata (largest rho difference {err:.3g}).  Vectorised NumPy on the "
          f"host: {t_np:.2f} s = {t_np / t_dev:.0f} x the device call")


if __name__ == "__main__":
    main()
