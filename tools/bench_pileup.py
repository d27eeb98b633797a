"""Measure the pileup (hh_pileup_pixels; csrc/pileup.hip) on the input of
tools/bench_saddle.py: one synthetic chromosome at chr1's 10 kb size with C2's
generator parameters (5e7 pixels), its ICE weights and its cis expected, the
pixel table, the weights, the expected and the features in HBM.  Two feature
sets with a fixed seed:
  (a) 20 000 loops, col - row uniform in 20..200 bins, flank 10 (W = 21);
  (b) 5 000 on-diagonal features, flank 50 (W = 101).

Per set it prints
  * the host-clock time of one on-device call (median over enough repeats to
    fill --seconds, after a warm-up), balanced over expected and raw observed,
    and the per-kernel split (hh_ktime: HIP events around every launch) with
    the bytes each kernel must move;
  * the path the library offered before for the same raw observed pileup:
    ``AllelicSpecificity.pixel_windows`` (hh_pixel_windows) on the same
    device-resident table followed by a torch sum over the window axis, on the
    features whose windows stay inside the chromosome (hh_pixel_windows
    refuses the others), next to the new call on the same subset, the ratio,
    and the agreement of the two (raw counts are integers: exact);
  * a host NumPy baseline: the restatement vectorised per feature (a dense
    window gathered from the rows' pixel runs) on every --feature-step-th
    feature, scaled.

A run without a GPU fails; there is no fallback.

    python tools/bench_pileup.py [--nnz 5e7] [--seconds 1.0]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RES = 10000
KERNELS = ("k_sd_rowptr", "k_pu_count", "k_pu_sum", "k_pu_reduce")


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
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    if isinstance(out, tuple):
        assert all(torch.equal(a, b) for a, b in zip(out, again))    # fixed order: the same bits
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


def host_window_sum(b2, c, rp, N, row, col, f, step):
    """The observed raw pileup of every step-th feature on the host: the dense
    window of a feature from the pixel runs of its rows (and, below the
    diagonal, of its columns), added up.  Returns (S, seconds, features)."""
    W = 2 * f + 1
    S = np.zeros((W, W))
    ks = range(0, row.size, step)
    t0 = time.perf_counter()
    for k in ks:
        win = np.zeros((W, W))
        for tr in (False, True):                                     # upper cells, then the mirrored ones
            r0, c0 = (col[k], row[k]) if tr else (row[k], col[k])
            for u in range(W):
                i = r0 - f + u
                if i < 0 or i >= N:
                    continue
                q, x = b2[rp[i]:rp[i + 1]], c[rp[i]:rp[i + 1]]
                a, b = np.searchsorted(q, [max(c0 - f, i + (1 if tr else 0)), c0 + f + 1])
                v = q[a:b] - (c0 - f)
                keep = v < W
                if tr:
                    win[v[keep], u] += x[a:b][keep]
                else:
                    win[u, v[keep]] += x[a:b][keep]
        S += win
    return S, time.perf_counter() - t0, len(ks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nnz", type=float, default=5e7)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--ignore-diags", type=int, default=2)
    ap.add_argument("--feature-step", type=int, default=50)
    a = ap.parse_args()

    import torch
    from hichap_master_amd import _lib, ice, synth
    from hichap_master_amd import pileup as pu
    from hichap_master_amd import saddle as sd
    from hichap_master_amd.AllelicSpecificity import pixel_windows

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
    g = a.ignore_diags
    rp = np.searchsorted(b1, np.arange(N + 1))
    print(f"input: N = {N} bins, {nnz} pixels ({24e-6 * nnz:.0f} MB of table), mean row {nnz / N:.0f} pixels, "
          f"{int((~np.isfinite(w)).sum())} masked bins, ICE {st['iters']} iterations; ignore_diags {g}")

    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d1, d2, dc, dw = dev(b1), dev(b2), dev(c), dev(w)
    s, n = sd.expected_pixels(d1, d2, dc, dw, 0, N, g, N - 1)
    de = dev(sd.expected_from_sums(s.cpu().numpy(), n.cpu().numpy(), g))

    rng = np.random.default_rng(20240229)
    ra = rng.integers(0, N - 200, 20000)
    sets = [("a: 20000 loops, col - row in 20..200, flank 10", ra, ra + rng.integers(20, 201, 20000), 10)]
    rb = rng.integers(0, N, 5000)
    sets.append(("b: 5000 on-diagonal features, flank 50", rb, rb.copy(), 50))
    for label, row, col, f in sets:
        W, M = 2 * f + 1, int(row.size)
        row, col = row.astype(np.int32), col.astype(np.int32)
        drow, dcol = dev(row), dev(col)
        # compulsory traffic: per (feature, window row) two row pointers, the search probes (two rounds of 64
        # bin2) and the run's pixels (bin2 + count); the mirrored part: per (feature, column) two row pointers,
        # a bisection and 4 x 4 candidate pixels per wave; weights, valid and expected gathers hit the caches
        run_len = np.minimum(rp[np.clip(row, 0, N - 1) + 1] - rp[np.clip(row, 0, N - 1)], W).mean()
        bytes_sum = M * W * (16 + 2 * 64 * 8 + 16 * run_len) + 8 * W * W * ((M + 63) // 64)
        run_oe = lambda: pu.pileup_pixels(d1, d2, dc, dw, 0, N, drow, dcol, f, de, g)
        run_raw = lambda: pu.pileup_pixels(d1, d2, dc, None, 0, N, drow, dcol, f)
        (S, Cn), ts = timed(run_oe, a.seconds)
        kt = kernel_times(run_oe, KERNELS)
        (Sr, Cr), tr = timed(run_raw, a.seconds)
        print(f"set {label} (W = {W}): hh_pileup_pixels on device, balanced over expected "
              f"{np.median(ts) * 1e3:.3f} ms per call (median of {len(ts)}, min {min(ts) * 1e3:.3f}), raw observed "
              f"{np.median(tr) * 1e3:.3f} ms; kernels: " + ", ".join(f"{k} {t * 1e6:.0f} us" for k, t in kt.items())
              + f"; k_pu_sum touches about {bytes_sum * 1e-6:.1f} MB (probes, runs of <= {run_len:.0f} pixels and "
              f"partials) = {bytes_sum / kt['k_pu_sum'] * 1e-9:.1f} GB/s: latency-bound, far below any bandwidth")
        # the parent's path for the raw observed pileup, on the windows inside the chromosome
        inside = (row - f >= 0) & (col - f >= 0) & (row + f < N) & (col + f < N)
        ri, ci = row[inside], col[inside]
        dri, dci = dev(ri), dev(ci)
        run_new = lambda: pu.pileup_pixels(d1, d2, dc, None, 0, N, dri, dci, f)
        run_old = lambda: pixel_windows(d1, d2, dc, 0, N, ri - f, ci - f, W, W).sum(0)
        (S_new, _), t_new = timed(run_new, a.seconds)
        S_old, t_old = timed(run_old, a.seconds)
        assert torch.equal(S_new, S_old)                             # integer counts: exact in any order
        ratio = np.median(t_new) / np.median(t_old)
        print(f"  raw observed pileup of the {int(inside.sum())} features inside the chromosome: hh_pileup_pixels "
              f"{np.median(t_new) * 1e3:.3f} ms, hh_pixel_windows + torch sum over a {int(inside.sum())} x {W} x {W} "
              f"stack ({8e-6 * inside.sum() * W * W:.0f} MB) {np.median(t_old) * 1e3:.3f} ms: new / old = "
              f"{ratio:.3f} (the same bits)")
        S_h, t_h, n_h = host_window_sum(b2, c, rp, N, row, col, f, a.feature_step)
        sub = pu.pileup_pixels(d1, d2, dc, None, 0, N, dev(row[::a.feature_step]), dev(col[::a.feature_step]), f)[0]
        assert np.array_equal(sub.cpu().numpy(), S_h)
        print(f"  NumPy restatement per feature on {n_h} features (every {a.feature_step}th), raw observed: "
              f"{t_h:.2f} s = {t_h * a.feature_step:.1f} s scaled to {M} (host baseline only; sub-sampled and "
              f"scaled; equal to the GPU sums of the same features)")


if __name__ == "__main__":
    main()
