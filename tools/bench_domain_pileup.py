"""Measure the domain pileup (hh_domain_pileup_pixels; csrc/pileup.hip, DESIGN.md
§4u) on the input of tools/bench_pileup.py: one synthetic chromosome at chr1's
10 kb size with C2's generator parameters (5e7 pixels), its ICE weights and
its cis expected, the pixel table, the weights, the expected and the features
in HBM.  Two feature sets with a fixed seed:
  (a) the reduction case: 5 000 domains of L = R = 33 bins, P = 34 (G = 101):
      tools/bench_pileup.py's set (b) as domains.  The new call next to
      hh_pileup_pixels on the same features (row = col = start + 16, flank 50),
      the ratio, and the agreement of the two (the same bits);
  (b) the realistic case: 5 000 domains, L uniform in 20..400 bins, R = 40, P =
      20 (G = 80), balanced over expected.

Per set it prints the host-clock time of one on-device call (median over
enough repeats to fill --seconds, after a warm-up) and the per-kernel split
(hh_ktime: HIP events around every launch); for (b) also the pixels the walk
touches per second, and a host NumPy baseline: the definition vectorised per
feature (the dense window of a feature from the pixel runs of its rows, two
overlap matrices around it) on every --feature-step-th feature, scaled.

A run without a GPU fails; there is no fallback.

    python tools/bench_domain_pileup.py [--nnz 5e7] [--seconds 1.0]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RES = 10000
KERNELS_NEW = ("k_sd_rowptr", "k_dp_weight", "k_dp_sum", "k_dp_reduce")
KERNELS_OLD = ("k_sd_rowptr", "k_pu_count", "k_pu_sum", "k_pu_reduce")
LINEAR_READ = 6.2e12                                                 # bytes / s, DESIGN.md §4m


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


def overlap_matrix(start, L, R, P, w0, nb):
    """O[u][i - w0] = the length, in 1/R bin, of output cell u on bin i."""
    u = np.arange(R + 2 * P, dtype=np.int64)[:, None]
    i = (w0 + np.arange(nb, dtype=np.int64))[None, :]
    x0 = start * R + (u - P) * L
    return np.maximum(np.minimum(x0 + L, (i + 1) * R) - np.maximum(x0, i * R), 0).astype(np.float64)


def host_domain_sums(b2, c, rp, w, e, N, start, end, R, P, min_dist, step):
    """S and Wn of every step-th feature on the host: the dense window of a
    feature from the pixel runs of its rows, masked, between the two overlap
    matrices.  (The full double loop: symmetric to rounding only.)  Returns
    (S, Wn, seconds, features, pixels read)."""
    G = R + 2 * P
    S, Wn = np.zeros((G, G)), np.zeros((G, G))
    valid = np.isfinite(w)
    ok_d = np.zeros(N, bool)
    ok_d[:e.size] = np.isfinite(e) & (e > 0)
    ok_d[:min_dist] = False
    e_safe = np.where(ok_d[:e.size], e, 1.0)
    ks = range(0, start.size, step)
    touched = 0
    t0 = time.perf_counter()
    for k in ks:
        s, L = int(start[k]), int(end[k] - start[k])
        w0 = max((s * R - P * L) // R, 0)
        w1 = min(-((-(s * R + (R + P) * L)) // R), N)
        nb = w1 - w0
        win = np.zeros((nb, nb))
        for a in range(w0, w1):
            q = b2[rp[a]:rp[a + 1]]
            hi = np.searchsorted(q, w1)
            touched += hi
            b = q[:hi]
            v = c[rp[a]:rp[a] + hi] * w[a] * w[b]
            v[np.isnan(v)] = 0.0
            win[a - w0, b - w0] = v / e_safe[np.minimum(b - a, e.size - 1)]
        win = win + np.triu(win, 1).T
        d = np.abs(np.subtract.outer(np.arange(nb), np.arange(nb)))
        E = (valid[w0:w1, None] & valid[None, w0:w1] & ok_d[d]).astype(np.float64)
        O = overlap_matrix(s, L, R, P, w0, nb)
        S += O @ (win * E) @ O.T / float(L * L)
        Wn += O @ E @ O.T / float(L * L)
    return S, Wn, time.perf_counter() - t0, len(ks), touched


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nnz", type=float, default=5e7)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--ignore-diags", type=int, default=2)
    ap.add_argument("--feature-step", type=int, default=50)
    a = ap.parse_args()

    import torch
    from hichap_master_amd import _lib, ice, synth
    from hichap_master_amd import domain_pileup as dp
    from hichap_master_amd import pileup as pu
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
    g = a.ignore_diags
    rp = np.searchsorted(b1, np.arange(N + 1))
    print(f"input: N = {N} bins, {nnz} pixels ({24e-6 * nnz:.0f} MB of table), mean row {nnz / N:.0f} pixels, "
          f"{int((~np.isfinite(w)).sum())} masked bins, ICE {st['iters']} iterations; ignore_diags {g}")

    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d1, d2, dc, dw = dev(b1), dev(b2), dev(c), dev(w)
    s, n = sd.expected_pixels(d1, d2, dc, dw, 0, N, g, N - 1)
    e = sd.expected_from_sums(s.cpu().numpy(), n.cpu().numpy(), g)
    de = dev(e)

    def report(label, ts, kt):
        print(f"{label}: {np.median(ts) * 1e3:.3f} ms per call (median of {len(ts)}, min {min(ts) * 1e3:.3f}); "
              f"kernels: " + ", ".join(f"{k} {t * 1e6:.0f} us" for k, t in kt.items()))

    # ---- (a) the reduction case
    rng = np.random.default_rng(20240229)
    R, P = 33, 34
    start = rng.integers(0, N - R + 1, 5000).astype(np.int32)
    end = (start + R).astype(np.int32)
    mid = (start + R // 2).astype(np.int32)                          # = start - P + (G - 1) / 2
    ds, dn, dm = dev(start), dev(end), dev(mid)
    run_new = lambda: dp.domain_pileup_pixels(d1, d2, dc, dw, 0, N, ds, dn, R, P, de, g)
    run_old = lambda: pu.pileup_pixels(d1, d2, dc, dw, 0, N, dm, dm, 50, de, g)
    (S, Wn), t_new = timed(run_new, a.seconds)
    (S0, Cn0), t_old = timed(run_old, a.seconds)
    assert torch.equal(S, S0) and torch.equal(Wn, Cn0.double())      # the same bits
    print(f"set a: 5000 domains, L = R = {R}, P = {P} (G = {R + 2 * P}), balanced over expected")
    report("  hh_domain_pileup_pixels", t_new, kernel_times(run_new, KERNELS_NEW))
    report("  hh_pileup_pixels (row = col = start + 16, flank 50)", t_old, kernel_times(run_old, KERNELS_OLD))
    print(f"  new / old = {np.median(t_new) / np.median(t_old):.3f} (the same bits: S = S, Wn = Cn)")

    # ---- (b) the realistic case
    R, P = 40, 20
    L = rng.integers(20, 401, 5000)
    start = (rng.random(5000) * (N - L)).astype(np.int32)
    end = (start + L).astype(np.int32)
    ds, dn = dev(start), dev(end)
    run_new = lambda: dp.domain_pileup_pixels(d1, d2, dc, dw, 0, N, ds, dn, R, P, de, g)
    (S, Wn), t_new = timed(run_new, a.seconds)
    kt = kernel_times(run_new, KERNELS_NEW)
    print(f"set b: 5000 domains, L uniform in 20..400, R = {R}, P = {P} (G = {R + 2 * P}), balanced over expected")
    report("  hh_domain_pileup_pixels", t_new, kt)
    assert torch.equal(S, S.T) and torch.equal(Wn, Wn.T)
    S_h, W_h, t_h, n_h, touched = host_domain_sums(b2, c, rp, w, e, N, start, end, R, P, g, a.feature_step)
    touched_all = touched * start.size / n_h
    print(f"  the windows' upper triangles hold about {touched_all:.3g} pixels (from every {a.feature_step}th "
          f"feature, scaled): {touched_all / kt['k_dp_sum']:.3g} pixels/s through k_dp_sum = "
          f"{16 * touched_all / kt['k_dp_sum'] * 1e-12:.3f} TB/s of bin2 + count, "
          f"{16 * touched_all / kt['k_dp_sum'] / LINEAR_READ:.3f} of the {LINEAR_READ * 1e-12:.1f} TB/s linear-read rate")
    sub = dp.domain_pileup_pixels(d1, d2, dc, dw, 0, N, dev(start[::a.feature_step]), dev(end[::a.feature_step]),
                                  R, P, de, g)
    np.testing.assert_allclose(sub[0].cpu().numpy(), S_h, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(sub[1].cpu().numpy(), W_h, rtol=1e-9, atol=1e-9)
    print(f"  NumPy restatement per feature on {n_h} features (every {a.feature_step}th), balanced over expected: "
          f"{t_h:.2f} s = {t_h * a.feature_step:.1f} s scaled to {start.size} (host baseline only; sub-sampled and "
          f"scaled; within 1e-9 of the GPU sums of the same features)")


if __name__ == "__main__":
    main()
