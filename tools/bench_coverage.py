"""Measure the symmetric pixel table, the per-bin coverage and the virtual 4C
(hh_symtab_*, csrc/symtab.hip and csrc/coverage.hip; hichap_master_amd/
coverage.py) on a synthetic whole genome: tools/bench_trans.py's genome (hg19's
23 chromosome sizes from synth.coo_genome, its ICE weights), the pixel table
and the weights in HBM.

It prints one line each for
  * the input and the bytes one coverage call moves,
  * hh_symtab_create: the host clock per call and the per-kernel split
    (hh_ktime: HIP events around every launch),
  * hh_symtab_coverage, raw and balanced, on device tensors: the host clock per
    call and the HIP-event time of k_cv_coverage, with bytes / time next to the
    measured linear-read rate of 6.2 TB/s; with --rows, the balanced call again
    at other hh_tune "cov_rows" values (the same bits),
  * hh_symtab_viewpoints with K = 1 and K = 64, narrow (1 bin) and wide (200
    bins) intervals: the host clock and the HIP-event time of k_cv_viewpoints,
  * the NumPy baseline: weighted np.bincount on both ends per class for the
    coverage, the same over the pixels that touch the interval for a viewpoint,
    and the agreement of the two sides.

A run without a GPU fails; there is no fallback.

    python tools/bench_coverage.py [--res 250000] [--trans-density 0.3] [--seconds 1.0] [--rows 1,8,16]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINEAR_READ = 6.2e12        # B/s, profiles/r6d/probe.log
CREATE_KERNELS = ("k_st_chrom", "k_sd_rowptr", "k_st_upper", "k_rs_hist", "k_rs_scatter", "k_st_rowptr_l", "k_st_lower")


def timed(run, seconds):
    import torch
    out = run()                                                      # warm-up (allocations)
    torch.cuda.synchronize()
    ts = []
    t_end = time.perf_counter() + seconds
    while time.perf_counter() < t_end or len(ts) < 5:
        t0 = time.perf_counter()
        out = run()
        ts.append(time.perf_counter() - t0)                          # every call synchronises its stream
    return out, ts


def kernel_times(run, names, reps=3):
    from hichap_master_amd import _lib
    _lib.call("hh_ktime_reset")
    _lib.call("hh_ktime_enable", 1)
    for _ in range(reps):
        run()
    _lib.call("hh_synchronize", None)
    _lib.call("hh_ktime_enable", 0)
    return {k: _lib.ktime(k)[0] / reps * 1e-3 for k in names}        # seconds per run


def host_coverage(b1, b2, v, chrom, valid, n, ignore, near):
    """Weighted np.bincount on both ends per class: (S[n, 3], seconds)."""
    t0 = time.perf_counter()
    ok = valid[b1] & valid[b2]
    cis = chrom[b1] == chrom[b2]
    d = b2 - b1
    S = np.zeros((n, 3))
    offd = d > 0
    for k, m in enumerate((ok & cis & (d >= ignore) & (d < near), ok & cis & (d >= max(ignore, near)), ok & ~cis)):
        S[:, k] = (np.bincount(b1[m], weights=v[m], minlength=n)
                   + np.bincount(b2[m & offd], weights=v[m & offd], minlength=n))
    return S, time.perf_counter() - t0


def host_viewpoint(b1, b2, v, chrom, valid, n, ignore, lo, hi):
    t0 = time.perf_counter()
    keep = valid[b1] & valid[b2] & ((chrom[b1] != chrom[b2]) | (b2 - b1 >= ignore))
    ina, inb = keep & (b1 >= lo) & (b1 < hi), keep & (b2 >= lo) & (b2 < hi) & (b1 != b2)
    P = np.bincount(b2[ina], weights=v[ina], minlength=n) + np.bincount(b1[inb], weights=v[inb], minlength=n)
    return P, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=250000, help="bin size")
    ap.add_argument("--trans-density", type=float, default=0.3)
    ap.add_argument("--A", type=float, default=30.0)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--ignore-diags", type=int, default=2)
    ap.add_argument("--rows", default="", help="also time k_cv_coverage at these cov_rows values")
    ap.add_argument("--no-host", action="store_true", help="skip the NumPy baseline")
    a = ap.parse_args()

    import torch
    from hichap_master_amd import _lib, ice, synth
    from hichap_master_amd import coverage as cov

    _lib.require_gpu()
    sizes = synth.genome_bins(a.res)
    t0 = time.perf_counter()
    rng = np.random.default_rng(20201015)
    b1, b2, c, off = synth.coo_genome(sizes, rng, A=a.A, trans_density=a.trans_density)
    t_gen = time.perf_counter() - t0
    n, C, nnz = int(off[-1]), len(sizes), int(b1.size)
    chrom = np.repeat(np.arange(C), sizes)
    w, st = ice.balance(b1, b2, c, n, off, max_iters=300)
    c = c.astype(np.float64)
    valid = np.isfinite(w)
    near = cov.default_near_bins(a.res)
    ig = a.ignore_diags

    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d1, d2, dc, dw = dev(b1), dev(b2), dev(c), dev(w)

    def create():
        cov.SymTable(d1, d2, dc, off).close()
        return ()

    _, ts = timed(create, a.seconds)
    kt = kernel_times(create, CREATE_KERNELS)
    tab = cov.SymTable(d1, d2, dc, off)
    m = tab.n_lower
    walk_bytes = 12 * nnz + 12 * m + 16 * n + 4 * n + 48 * n     # partner + count of both halves, row pointers, info, S and n
    print(f"input: hg19 at {a.res // 1000} kb, {C} chromosomes, {n} bins, {nnz} pixels of which "
          f"{int(np.count_nonzero(chrom[b1] != chrom[b2]))} trans and {nnz - m} diagonal, {int((~valid).sum())} masked "
          f"bins, ICE {st['iters']} iterations (synth.coo_genome A = {a.A}, trans_density = {a.trans_density}: "
          f"{t_gen:.0f} s on the host).  The handle holds {28e-6 * nnz:.0f} MB (upper: int32 partner + fp64 count; "
          f"lower: int32 partner + uint32 index + fp64 count); one coverage call reads 12 B per entry of either half "
          f"once, {walk_bytes * 1e-6:.0f} MB with the row pointers and the outputs; the gathers of info and weight come "
          f"from {12e-3 * n:.0f} kB that stay in cache")
    print(f"hh_symtab_create on device: {np.median(ts) * 1e3:.2f} ms (median of {len(ts)}, min {min(ts) * 1e3:.2f}); "
          f"kernels: " + ", ".join(f"{k} {t * 1e6:.0f} us" for k, t in kt.items())
          + f" (k_rs_*: the stable radix sort of the {nnz} keys on the bin2 bits)")

    def coverage_line(weight, label):
        (S, k), ts = timed(lambda: tab.coverage(weight, None, None, ig, near), a.seconds / 2)
        S2, k2 = tab.coverage(weight, None, None, ig, near)
        assert torch.equal(S, S2) and torch.equal(k, k2)              # fixed order: the same bits
        kt = kernel_times(lambda: tab.coverage(weight, None, None, ig, near), ("k_cv_coverage", "k_cv_bininfo"), reps=10)
        t = kt["k_cv_coverage"]
        print(f"hh_symtab_coverage {label}: {np.median(ts) * 1e6:.0f} us per call on the host clock (median of "
              f"{len(ts)}, min {min(ts) * 1e6:.0f}), k_cv_bininfo {kt['k_cv_bininfo'] * 1e6:.0f} us, k_cv_coverage "
              f"{t * 1e6:.0f} us by HIP events = {walk_bytes / t * 1e-12:.3f} TB/s = "
              f"{100 * walk_bytes / t / LINEAR_READ:.1f} % of 6.2 TB/s over {walk_bytes * 1e-6:.0f} MB")
        return S, k, t

    S_raw, k_raw, _ = coverage_line(None, "raw")
    S_bal, k_bal, t_copy = coverage_line(dw, "balanced")
    for rows in [int(x) for x in a.rows.split(",") if x]:
        _lib.call("hh_tune", b"cov_rows", rows)
        S_r, _, _ = coverage_line(dw, f"balanced, cov_rows {rows}")
        assert torch.equal(S_r, S_bal)
        _lib.call("hh_tune", b"cov_rows", 4)

    big = int(np.argmax(sizes))
    mid = int(off[big]) + int(sizes[big]) // 2
    picks = np.linspace(0, n - 201, 64).astype(np.int64)

    def view_line(K, width):
        iv = [(mid, mid + width)] if K == 1 else [(int(x), int(x) + width) for x in picks]
        P, ts = timed(lambda: tab.viewpoints(iv, dw, None, None, ig), a.seconds / 4)
        assert torch.equal(P, tab.viewpoints(iv, dw, None, None, ig))
        t = kernel_times(lambda: tab.viewpoints(iv, dw, None, None, ig), ("k_cv_viewpoints",), reps=10)["k_cv_viewpoints"]
        print(f"hh_symtab_viewpoints K = {K}, {width} bin{'s' if width > 1 else ''} wide: {np.median(ts) * 1e6:.0f} us "
              f"per call on the host clock (median of {len(ts)}, min {min(ts) * 1e6:.0f}), k_cv_viewpoints "
              f"{t * 1e6:.0f} us by HIP events, {t / K * 1e6:.1f} us per viewpoint")
        return iv, P

    view_line(1, 1)
    iv_wide, P_wide = view_line(1, 200)
    view_line(64, 1)
    view_line(64, 200)

    if not a.no_host:
        v = np.nan_to_num(c * w[b1] * w[b2], nan=0.0)
        Sh, t_host = host_coverage(b1, b2, v, chrom, valid, n, ig, near)
        Sg = S_bal.cpu().numpy()
        np.testing.assert_allclose(Sg, Sh, rtol=1e-11, atol=0)
        Sr, t_host_raw = host_coverage(b1, b2, c, chrom, np.ones(n, bool), n, ig, near)
        assert np.array_equal(S_raw.cpu().numpy(), Sr)                # integer counts: exact on both sides
        lo, hi = iv_wide[0]
        Ph, t_view = host_viewpoint(b1, b2, v, chrom, valid, n, ig, lo, hi)
        np.testing.assert_allclose(P_wide.cpu().numpy()[0], Ph, rtol=1e-11, atol=0)
        print(f"host baseline, weighted np.bincount on both ends per class (the values c w w given): balanced "
              f"{t_host * 1e3:.0f} ms, raw {t_host_raw * 1e3:.0f} ms (equal to the GPU's raw sums exactly, to its "
              f"balanced ones to 1e-11); k_cv_coverage {t_host / t_copy:.0f} x faster; a 200-bin viewpoint "
              f"{t_view * 1e3:.0f} ms on the host")
    tab.close()


if __name__ == "__main__":
    main()
