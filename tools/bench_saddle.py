"""Measure the cis expected and the compartment saddle (hh_expected_pixels,
hh_saddle_pixels; csrc/saddle.hip) on the input of bench.py's TAD scan line:
one synthetic chromosome at chr1's 10 kb size with C2's generator parameters
(5e7 pixels), its ICE weights, the pixel table and the weights in HBM.  Full
distance (max_dist = N - 1), ignore_diags 2, K = 52 classes (50 quantile bins
of a synthetic track plus the two outlier classes).

It prints one line each for
  * the input and the bytes the two calls move,
  * the host-clock time of one on-device call of either entry point (median
    over enough repeats to fill --seconds, after a warm-up) and the per-kernel
    split (hh_ktime: HIP events around every launch), with each pass's bytes /
    time next to the measured linear-read rate of 6.2 TB/s,
  * with --tiles, hh_expected_pixels again at other sub-tile widths
    (hh_tune "saddle_diag_tile"; the results are bitwise the same),
  * the agreement of the results with a vectorised NumPy computation on the
    whole table (np.bincount; counts exactly, sums within 2 (m + 2) 2^-53),
  * the NumPy restatement of the definitions, row by row, on every 64th row,
    scaled by 64, as the host baseline, and the vectorised computation's time.

A run without a GPU fails; there is no fallback.

    python tools/bench_saddle.py [--nnz 5e7] [--seconds 1.0] [--tiles 64,128]
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
EXPECTED_KERNELS = ("k_sd_rowptr", "k_sd_seg", "k_sd_expected", "k_sd_exp_sum", "k_sd_nvalid")
SADDLE_KERNELS = ("k_sd_rowptr", "k_sd_rows", "k_sd_u_part", "k_sd_u_sum", "k_sd_cu")


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nnz", type=float, default=5e7)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--ignore-diags", type=int, default=2)
    ap.add_argument("--n-bins", type=int, default=50)
    ap.add_argument("--row-step", type=int, default=64)
    ap.add_argument("--tiles", default="", help="also time hh_expected_pixels at these saddle_diag_tile values")
    a = ap.parse_args()

    import torch
    from hichap_master_amd import _lib, ice, synth
    from hichap_master_amd import saddle as sd

    _lib.require_gpu()
    sizes = [synth.chrom_bins([synth.HG19["1"]], RES)[0]]
    A, td = synth.calibrate(sizes, a.nnz, 0.0)
    m = ice.ContactMatrix.synthetic(sizes, A=A, trans_density=td, comp_block=200, seed=20201015)
    w, st = ice.balance_matrix(m)
    b1, b2, c = m.export_upper()
    m.close()
    c = c.astype(np.float64)
    N, nnz = int(sizes[0]), int(b1.size)
    key = b1 * N + b2                                                # cooler's order: sorted by (bin1, bin2)
    if np.any(np.diff(key) <= 0):
        o = np.argsort(key, kind="stable")
        b1, b2, c = b1[o], b2[o], c[o]
    del key
    g, D, K = a.ignore_diags, N - 1, a.n_bins + 2
    dmin = max(1, g)
    valid = np.isfinite(w)
    rng = np.random.default_rng(1)
    track = np.sin(np.arange(N) / 200.0 * np.pi) + 0.3 * rng.normal(size=N)   # blocks of 200 bins, as comp_block
    cls, _ = sd.digitize_track({"1": track}, {"1": valid.astype(np.uint8)}, a.n_bins)
    cls = cls["1"]

    tile = 256                                                       # HH_SADDLE_DIAG_TILE; 128 rows per chunk
    nJ, chunks = D // tile + 1, (N + 127) // 128
    seg_b, part_b = 8 * N * (nJ + 1), 8 * chunks * (D + 1)
    exp_bytes = dict(k_sd_rowptr=8 * (N + 1), k_sd_seg=seg_b, k_sd_expected=16 * nnz + 2 * seg_b + part_b,
                     k_sd_exp_sum=part_b + 8 * (D + 1), k_sd_nvalid=8 * (D + 1))
    sad_bytes = dict(k_sd_rowptr=8 * (N + 1), k_sd_rows=16 * nnz + 8 * 64 * N, k_sd_u_part=8 * 64 * N,
                     k_sd_u_sum=8 * 64 * K * ((N + 511) // 512), k_sd_cu=N + D + 1)
    print(f"input: N = {N} bins, {nnz} pixels, {int((~valid).sum())} masked bins, ICE {st['iters']} iterations; "
          f"ignore_diags {g}, max_dist {D}, K = {K}.  Bytes from HBM per call, compulsory: the table's bin2 and "
          f"count, 16 B/pixel = {16e-6 * nnz:.0f} MB in either call (bin1 is read by the row-pointer bisections "
          f"only; weight, valid, class and expected gathers of 1-8 B per pixel come from {9e-3 * N:.0f} kB of "
          f"cache-resident vectors); expected: + {seg_b * 1e-6:.1f} MB of segment bounds written and read, "
          f"{part_b * 1e-6:.1f} MB of chunk partials written and read; saddle: + {8e-6 * 64 * N:.1f} MB of row "
          f"sums written and read; Cu: {N * (N - 1) / 2:.3g} pair visits on {N + D + 1} bytes of classes and flags")

    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d1, d2, dc, dw, dcls = dev(b1), dev(b2), dev(c), dev(w), dev(cls)
    run_e = lambda: sd.expected_pixels(d1, d2, dc, dw, 0, N, g, D)
    (s, n), ts = timed(run_e, a.seconds)
    kt = kernel_times(run_e, EXPECTED_KERNELS)
    print(f"hh_expected_pixels on device: {np.median(ts) * 1e3:.2f} ms per call (median of {len(ts)}, min "
          f"{min(ts) * 1e3:.2f}); kernels: " + ", ".join(
              f"{k} {t * 1e6:.0f} us ({exp_bytes[k] / t * 1e-12:.3f} TB/s = "
              f"{100 * exp_bytes[k] / t / LINEAR_READ:.1f} % of 6.2 TB/s)" for k, t in kt.items()))
    for t in [int(x) for x in a.tiles.split(",") if x]:              # the sub-tile width (hh_tune): same bits
        _lib.call("hh_tune", b"saddle_diag_tile", t)
        (s2, n2), ts = timed(run_e, a.seconds / 2)
        kt = kernel_times(run_e, EXPECTED_KERNELS)
        _lib.call("hh_tune", b"saddle_diag_tile", tile)
        assert torch.equal(s, s2) and torch.equal(n, n2)
        print(f"  saddle_diag_tile {t}: {np.median(ts) * 1e3:.2f} ms per call; k_sd_seg {kt['k_sd_seg'] * 1e6:.0f} us, "
              f"k_sd_expected {kt['k_sd_expected'] * 1e6:.0f} us (same bits as the default tile)")
    sh, nh = s.cpu().numpy(), n.cpu().numpy()
    e = sd.expected_from_sums(sh, nh, g)
    de = dev(e)
    run_s = lambda: sd.saddle_pixels(d1, d2, dc, dw, 0, N, de, dcls, K, dmin, D)
    (U, Cu), ts = timed(run_s, a.seconds)
    kt = kernel_times(run_s, SADDLE_KERNELS)
    pairs = N * (N - 1) / 2
    print(f"hh_saddle_pixels on device: {np.median(ts) * 1e3:.2f} ms per call (median of {len(ts)}, min "
          f"{min(ts) * 1e3:.2f}); kernels: " + ", ".join(
              f"{k} {t * 1e6:.0f} us ({sad_bytes[k] / t * 1e-12:.3f} TB/s = "
              f"{100 * sad_bytes[k] / t / LINEAR_READ:.1f} % of 6.2 TB/s)" for k, t in kt.items())
          + f"; k_sd_cu visits {pairs / kt['k_sd_cu'] * 1e-9:.1f} G pairs/s")
    Uh, Cuh = U.cpu().numpy(), Cu.cpu().numpy()

    # agreement: the same sums with np.bincount over the whole table (another order of the same terms)
    t0 = time.perf_counter()
    v = np.nan_to_num(c * w[b1] * w[b2])
    d = b2 - b1
    ok = valid[b1] & valid[b2] & (d >= g)
    s_np = np.bincount(d[ok], weights=v[ok], minlength=D + 1)
    usable = np.isfinite(e) & (e > 0) & (np.arange(D + 1) >= dmin)
    ok = valid[b1] & valid[b2] & usable[d] & (cls[b1] != 255) & (cls[b2] != 255)
    U_np = np.bincount(cls[b1[ok]].astype(np.int64) * K + cls[b2[ok]], weights=v[ok] / e[d[ok]],
                       minlength=K * K).reshape(K, K)
    t_vec = time.perf_counter() - t0
    vi = valid.astype(np.int64)
    n_np = np.array([np.dot(vi[:N - k], vi[k:]) if k >= g else 0 for k in range(D + 1)])
    assert np.array_equal(nh, n_np)
    u53 = 2.0 ** -53
    np.testing.assert_allclose(sh, s_np, rtol=2 * (n_np.max() + 2) * u53, atol=0)
    np.testing.assert_allclose(Uh, U_np, rtol=2 * (Cuh.max() + 2) * u53, atol=0)

    # host baseline: the definitions row by row on every row_step-th row (pixels of the row, then its cells)
    ec = np.where(valid, cls, 255)
    rows = list(range(0, N, a.row_step))
    rp = np.searchsorted(b1, np.arange(N + 1))
    t0 = time.perf_counter()
    s_r, n_r = np.zeros(D + 1), np.zeros(D + 1, np.int64)
    U_r, Cu_r = np.zeros((K, K)), np.zeros((K, K), np.int64)
    for r in rows:
        if not valid[r]:
            continue
        q, x = b2[rp[r]:rp[r + 1]], c[rp[r]:rp[r + 1]]
        vr = np.nan_to_num(x * w[r] * w[q])
        dr = q - r
        keep = valid[q] & (dr >= g)
        np.add.at(s_r, dr[keep], vr[keep])
        n_r[g:N - r] += valid[r + g:]
        if ec[r] != 255:
            keep = usable[dr] & (ec[q] != 255)
            np.add.at(U_r[ec[r]], ec[q[keep]], vr[keep] / e[dr[keep]])
            cells = ec[r + dmin:][usable[dmin:N - r]]
            Cu_r[ec[r]] += np.bincount(cells[cells != 255], minlength=K)[:K]
    t_ref = time.perf_counter() - t0
    Cu_full = np.zeros((K, K), np.int64)                             # every row once: the check of Cu
    for r in range(N):
        if ec[r] != 255:
            cells = ec[r + dmin:][usable[dmin:N - r]]
            Cu_full[ec[r]] += np.bincount(cells[cells != 255], minlength=K)[:K]
    assert np.array_equal(Cuh, Cu_full)
    print(f"agreement: nvalid and Cu equal NumPy's exactly, sum and U within 2 (m + 2) 2^-53 of np.bincount over the "
          f"whole table ({t_vec:.2f} s on the host, expected sums and U only).  NumPy restatement row by row on "
          f"{len(rows)} rows (every {a.row_step}th): {t_ref:.2f} s = {t_ref * a.row_step:.1f} s scaled to {N} rows "
          f"(host baseline only; sub-sampled and scaled)")


if __name__ == "__main__":
    main()
