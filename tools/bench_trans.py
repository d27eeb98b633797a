"""Measure the trans block sums and the trans saddle (hh_trans_blocks,
hh_trans_saddle; csrc/trans.hip) on a synthetic whole genome: hg19's chromosome
sizes at 40 kb from synth.coo_genome with a trans density that makes trans
pixels dominate, its ICE weights, the pixel table and the weights in HBM.  One
call per row chromosome, 23 calls per quantity; ignore_diags 2, K = 52 classes
(50 quantile bins of a synthetic track plus the two outlier classes).

It prints one line each for
  * the input and the bytes the calls move,
  * the host-clock time of the 23 on-device calls of either entry point
    (median over enough repeats to fill --seconds, after a warm-up) and of the
    largest single call (chromosome 1), and the per-kernel split (hh_ktime: HIP
    events around every launch, summed over the 23 calls), with each pass's
    bytes / time next to the measured linear-read rate of 6.2 TB/s,
  * with --trips, hh_trans_blocks again at other span lengths (hh_tune
    "trans_trips"; npix stays the same, the sums within the rounding bound),
  * the agreement of the results with a vectorised NumPy computation on the
    whole table (np.bincount over block and class-pair ids; npix exactly, the
    sums within 2 (m + 2) 2^-53), whose time is the host baseline.

A run without a GPU fails; there is no fallback.

    python tools/bench_trans.py [--trans-density 0.06] [--seconds 1.0] [--trips 16,64]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RES = 40000
LINEAR_READ = 6.2e12        # B/s, profiles/r6d/probe.log
BLOCK_KERNELS = ("k_tr_bininfo", "k_sd_rowptr", "k_tr_blocks", "k_tr_fold")
SADDLE_KERNELS = ("k_tr_bininfo", "k_sd_rowptr", "k_tr_rows", "k_tr_u_part", "k_tr_u_sum")
U53 = 2.0 ** -53


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
        ts.append(time.perf_counter() - t0)                          # every call synchronises its stream
    assert all(torch.equal(a, b) for a, b in zip(out, again))        # fixed order: the same bits
    return out, ts


def kernel_times(run, names, reps=3):
    from hichap_master_amd import _lib
    _lib.call("hh_ktime_reset")
    _lib.call("hh_ktime_enable", 1)
    for _ in range(reps):
        run()
    _lib.call("hh_synchronize", None)
    _lib.call("hh_ktime_enable", 0)
    return {k: _lib.ktime(k)[0] / reps * 1e-3 for k in names}        # seconds per genome


def rates(kt, nbytes):
    return ", ".join(f"{k} {t * 1e6:.0f} us ({nbytes[k] / t * 1e-12:.3f} TB/s = "
                     f"{100 * nbytes[k] / t / LINEAR_READ:.1f} % of 6.2 TB/s)" for k, t in kt.items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trans-density", type=float, default=0.06)
    ap.add_argument("--A", type=float, default=30.0)
    ap.add_argument("--res", type=int, default=RES, help="bin size (a coarser one makes a quick trial run)")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--ignore-diags", type=int, default=2)
    ap.add_argument("--n-bins", type=int, default=50)
    ap.add_argument("--trips", default="", help="also time hh_trans_blocks at these trans_trips values")
    a = ap.parse_args()

    import torch
    from hichap_master_amd import _lib, ice, synth
    from hichap_master_amd import trans as tr
    from hichap_master_amd.saddle import digitize_track

    _lib.require_gpu()
    sizes = synth.genome_bins(a.res)
    t0 = time.perf_counter()
    b1, b2, c, off = synth.coo_genome(sizes, np.random.default_rng(20201015), A=a.A, trans_density=a.trans_density)
    t_gen = time.perf_counter() - t0
    n, C, nnz = int(off[-1]), len(sizes), int(b1.size)
    w, st = ice.balance(b1, b2, c, n, off, max_iters=300)
    c = c.astype(np.float64)
    chrom = np.repeat(np.arange(C), sizes)
    p1, p2 = chrom[b1], chrom[b2]
    n_trans = int(np.count_nonzero(p1 != p2))
    g, K = a.ignore_diags, a.n_bins + 2
    valid, nvb = tr.valid_bins(off, w)
    rows_of = np.searchsorted(b1, off)                               # the pixel range of every row chromosome
    per_p = np.diff(rows_of)
    rng = np.random.default_rng(1)
    track = np.sin(np.arange(n) / 50.0 * np.pi) + 0.3 * rng.normal(size=n)
    cls_by, _ = digitize_track({q: track[off[q]:off[q + 1]] for q in range(C)},
                               {q: valid[off[q]:off[q + 1]] for q in range(C)}, a.n_bins)
    cls = np.concatenate([cls_by[q] for q in range(C)])

    v = ctypes.c_int64()
    _lib.call("hh_tune_get", b"trans_trips", ctypes.byref(v))
    trips = int(v.value)                                             # the default span length
    spans = int(np.sum((per_p + 64 * trips - 1) // (64 * trips)))
    tail = int(np.count_nonzero(p1 != p2))                           # the saddle walks the trans tails only
    blk_bytes = dict(k_tr_bininfo=C * (8 * n + 4 * n), k_sd_rowptr=8 * (n + C), k_tr_blocks=24 * nnz + 16 * spans * C,
                     k_tr_fold=16 * spans * C * 65 // 64)
    sad_bytes = dict(k_tr_bininfo=C * (8 * n + n + 4 * n), k_sd_rowptr=8 * (n + C), k_tr_rows=16 * tail + 8 * 64 * n,
                     k_tr_u_part=8 * 64 * n, k_tr_u_sum=8 * 64 * K * int(np.sum((np.asarray(sizes) + 511) // 512)))
    print(f"input: hg19 at {a.res // 1000} kb, {C} chromosomes, {n} bins, {nnz} pixels of which {n_trans} trans "
          f"({100 * n_trans / nnz:.1f} %), {int((valid == 0).sum())} masked bins, ICE {st['iters']} iterations "
          f"(synth.coo_genome A = {a.A}, trans_density = {a.trans_density}: {t_gen:.0f} s on the host); ignore_diags "
          f"{g}, K = {K}.  Bytes from HBM over the {C} calls, compulsory: bin1, bin2 and count of every pixel once for "
          f"the block sums, 24 B/pixel = {24e-6 * nnz:.0f} MB (16 B/pixel of bin2 + count and the bin1 that tells the "
          f"rows of a span apart), and bin2 and count of the trans pixels for the saddle, {16e-6 * tail:.0f} MB; the "
          f"gathers (4 B of bin info and 8 B of weight per end) come from {12e-3 * n:.0f} kB of vectors that stay in "
          f"cache; + {16e-6 * spans * C:.2f} MB of span partials written and read ({spans} spans of {64 * trips} "
          f"pixels), + {8e-6 * 64 * n:.1f} MB of row sums written and read")

    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d1, d2, dc, dw, dcls = dev(b1), dev(b2), dev(c), dev(w), dev(cls)

    def run_blocks(ps=range(C)):
        out = []
        for p in ps:
            out += tr.trans_blocks_pixels(d1, d2, dc, dw, off, p, g)
        return out

    res, ts = timed(run_blocks, a.seconds)
    _, ts1 = timed(lambda: run_blocks([0]), a.seconds / 2)
    kt = kernel_times(run_blocks, BLOCK_KERNELS)
    print(f"hh_trans_blocks on device, {C} calls: {np.median(ts) * 1e3:.2f} ms (median of {len(ts)}, min "
          f"{min(ts) * 1e3:.2f}); chromosome 1 alone ({int(per_p[0])} pixels): {np.median(ts1) * 1e3:.2f} ms; kernels "
          f"over the {C} calls: " + rates(kt, blk_bytes))
    sums = np.stack([x.cpu().numpy() for x in res[0::2]])
    npix = np.stack([x.cpu().numpy() for x in res[1::2]])
    for t in [int(x) for x in a.trips.split(",") if x]:              # the span length (hh_tune): last bits only
        _lib.call("hh_tune", b"trans_trips", t)
        res2, ts2 = timed(run_blocks, a.seconds / 2)
        kt2 = kernel_times(run_blocks, BLOCK_KERNELS)
        _lib.call("hh_tune", b"trans_trips", trips)
        assert np.array_equal(np.stack([x.cpu().numpy() for x in res2[1::2]]), npix)
        np.testing.assert_allclose(np.stack([x.cpu().numpy() for x in res2[0::2]]), sums,
                                   rtol=2 * (npix.max() + 2) * U53, atol=0)
        print(f"  trans_trips {t}: {np.median(ts2) * 1e3:.2f} ms for the {C} calls; k_tr_blocks "
              f"{kt2['k_tr_blocks'] * 1e6:.0f} us, k_tr_fold {kt2['k_tr_fold'] * 1e6:.0f} us (npix the same, sums within "
              f"the bound)")

    e = tr.trans_expected_from_sums(sums, nvb)
    de = [dev(e[p]) for p in range(C)]

    def run_saddle(ps=range(C)):
        return [tr.trans_saddle_pixels(d1, d2, dc, dw, off, p, de[p], dcls, K) for p in ps]

    Us, ts = timed(run_saddle, a.seconds)
    _, ts1 = timed(lambda: run_saddle([0]), a.seconds / 2)
    kt = kernel_times(run_saddle, SADDLE_KERNELS)
    print(f"hh_trans_saddle on device, {C} calls: {np.median(ts) * 1e3:.2f} ms (median of {len(ts)}, min "
          f"{min(ts) * 1e3:.2f}); chromosome 1 alone: {np.median(ts1) * 1e3:.2f} ms; kernels over the {C} calls: "
          + rates(kt, sad_bytes))
    U = np.stack([x.cpu().numpy() for x in Us])

    # agreement and host baseline: the same sums with np.bincount over the whole table
    t0 = time.perf_counter()
    v = np.nan_to_num(c * w[b1] * w[b2])
    ok = (valid[b1] != 0) & (valid[b2] != 0) & ((p1 != p2) | (b2 - b1 >= g))
    blk = p1[ok] * C + p2[ok]
    s_np = np.bincount(blk, weights=v[ok], minlength=C * C).reshape(C, C)
    n_np = np.bincount(blk, minlength=C * C).reshape(C, C)
    t_blk = time.perf_counter() - t0
    t0 = time.perf_counter()
    usable = tr.trans_usable(e)
    ok = (valid[b1] != 0) & (valid[b2] != 0) & usable[p1, p2] & (cls[b1] != 255) & (cls[b2] != 255)
    cell = (p1[ok] * K + cls[b1[ok]]) * K + cls[b2[ok]]
    U_np = np.bincount(cell, weights=v[ok] / e[p1[ok], p2[ok]], minlength=C * K * K).reshape(C, K, K)
    m_np = np.bincount(cell, minlength=C * K * K)
    t_sad = time.perf_counter() - t0
    assert np.array_equal(npix, n_np)
    np.testing.assert_allclose(sums, s_np, rtol=2 * (n_np.max() + 2) * U53, atol=0)
    np.testing.assert_allclose(U, U_np, rtol=2 * (m_np.max() + 2) * U53, atol=0)
    tot = tr.cis_trans_totals(sums)
    print(f"agreement: npix equals NumPy's exactly, sum and U within 2 (m + 2) 2^-53 (m = {n_np.max()}, "
          f"{m_np.max()}) of np.bincount over the whole table; host baseline, the same sums by np.bincount over "
          f"block ids: {t_blk:.2f} s for the block sums, {t_sad:.2f} s for U.  Genome cis fraction "
          f"{tot['genome'][2]:.4f}")


if __name__ == "__main__":
    main()
