"""Measure the two kernels of the allelic-specificity module (csrc/allelic.hip).

hh_pairdiff_rank at K = 1 000, 3 000 and 10 000 compartment candidates (K
maternal x K paternal values, K queries) against the reference's form restated
in NumPy: the sorted outer difference + searchsorted (skipped where the K^2
float64 list does not fit in a quarter of the free memory).

hh_pixel_windows for 5 000 boundary windows (20 x 20) on one synthetic
chromosome at 10 kb (24 896 bins) written as a float-count cooler, against
``Cooler.matrix(balance=False).fetch`` + slicing, which is what
BoundaryAllelicSpecificity.DataSetBuilding does per haplotype chromosome.

Every timed pair is checked for exact agreement; what is printed is also
written to profiles/allelic_bench.log.  No target ratio is set: the log is the
record.

    python tools/bench_allelic.py [--pixels 10000000] [--windows 5000] [--reps 5]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_BINS = 24896  # hg38 chr1 (248 956 422 bp) at 10 kb
RES = 10000


def free_bytes():
    try:
        return os.sysconf("SC_AVPHYS_PAGES") * os.sysconf("SC_PAGE_SIZE")
    except (ValueError, OSError):
        return 8 << 30


def make_pixels(n_pix, seed):
    """Unique upper-triangle pixels, density falling as d^-1/2, float counts
    in 1/64 like the two-step-corrected haplotype coolers."""
    rng = np.random.default_rng(seed)
    N = N_BINS
    want = int(n_pix * 1.25)
    d = np.minimum((N * rng.random(want) ** 2).astype(np.int64), N - 1)
    i = (rng.random(want) * (N - d)).astype(np.int64)
    key = np.unique(i * N + (i + d))
    if key.size > n_pix:
        key = np.sort(rng.choice(key, n_pix, replace=False))
    b1, b2 = key // N, key % N
    cnt = (64 * (1 + rng.poisson(60.0 / (b2 - b1 + 1.0) ** 0.8)) + rng.integers(-31, 32, b1.size)) / 64.0
    return b1, b2, cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=10_000_000)
    ap.add_argument("--windows", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "allelic_bench.log"))
    a = ap.parse_args()

    import torch
    from hichap_master_amd import AllelicSpecificity as AS
    from hichap_master_amd import _lib, coolio

    _lib.require_gpu()
    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)

    def timed(fn, reps):
        ts = []
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = fn()
            ts.append(time.perf_counter() - t)
        return r, 1e3 * float(np.median(ts[1:])), 1e3 * min(ts[1:])

    def kernel_ms(fn, *names):
        _lib.call("hh_ktime_reset")
        _lib.call("hh_ktime_enable", 1)
        fn()
        _lib.call("hh_synchronize", None)
        _lib.call("hh_ktime_enable", 0)
        return [_lib.ktime(n)[0] for n in names]

    # ------------------------------------------------------ hh_pairdiff_rank
    rng = np.random.default_rng(a.seed)
    for K in (1000, 3000, 10000):
        m = np.round(rng.normal(0, 0.03, K), 4)
        p = np.round(-np.sign(m) * np.abs(rng.normal(0, 0.03, K)), 4)
        q = m - p
        less, ms, mn = timed(lambda: AS.pairdiff_rank(m, p, q), a.reps)
        (k_ms,) = kernel_ms(lambda: AS.pairdiff_rank(m, p, q), "k_pairdiff_rank")
        line = (f"pairdiff_rank K = {K}: GPU {ms:.2f} ms median per call (min {mn:.2f}; kernel {k_ms * 1e3:.0f} us, "
                f"{K * K * 1e-6 / max(k_ms, 1e-9):.1f} G binary searches/s)")
        if K * K * 8 * 2 < free_bytes() // 4:
            t = time.perf_counter()
            want = np.searchsorted(np.sort(np.subtract.outer(m, p).ravel()), q, "left")
            t_ref = 1e3 * (time.perf_counter() - t)
            assert np.array_equal(less, want), "GPU and NumPy differ"
            line += f"; NumPy sorted outer difference + searchsorted {t_ref:.0f} ms ({t_ref / ms:.0f} x), identical"
        else:
            line += "; NumPy form skipped (the K^2 list does not fit)"
        say(line)

    # ------------------------------------------------------ hh_pixel_windows
    t0 = time.perf_counter()
    b1, b2, cnt = make_pixels(a.pixels, a.seed)
    wb = np.sort(rng.integers(10, N_BINS - 10, a.windows)) - 10
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.cool")
        coolio.create_cooler(path, {RES: ([("M1", N_BINS * RES)], b1, b2, cnt)})
        say(f"input: {N_BINS} bins, {b1.size} pixels ({b1.size * 24 / 1e6:.0f} MB as three 8-byte columns), "
            f"{wb.size} windows of 20 x 20; made and written in {time.perf_counter() - t0:.1f} s")
        with coolio.Cooler(f"{path}::{RES}") as c:
            def gpu_from_file():
                lo, hi = c.extent("M1")
                r1, r2, rc = c.pixel_rows(lo, hi)
                return AS.pixel_windows(r1, r2, rc, lo, hi - lo, wb, wb, 20, 20)
            tiles, ms_file, mn_file = timed(gpu_from_file, a.reps)
            say(f"pixel_windows, from the cooler file (read pixels + upload + gather + download): {ms_file:.1f} ms "
                f"median (min {mn_file:.1f})")
            _, ms_host, mn_host = timed(lambda: AS.pixel_windows(b1, b2, cnt, 0, N_BINS, wb, wb, 20, 20), a.reps)
            say(f"pixel_windows, host pixel arrays (upload + gather + download): {ms_host:.1f} ms median "
                f"(min {mn_host:.1f})")
            d1, d2, dc = torch.from_numpy(b1).cuda(), torch.from_numpy(b2).cuda(), torch.from_numpy(cnt).cuda()
            dev, ms_dev, mn_dev = timed(lambda: AS.pixel_windows(d1, d2, dc, 0, N_BINS, wb, wb, 20, 20), a.reps)
            kc, kg = kernel_ms(lambda: AS.pixel_windows(d1, d2, dc, 0, N_BINS, wb, wb, 20, 20), "k_win_check",
                               "k_win_gather")
            say(f"pixel_windows, pixels in HBM: {ms_dev:.2f} ms median per call (min {mn_dev:.2f}); kernels: "
                f"k_win_check {kc * 1e3:.0f} us ({b1.size * 24 / max(kc, 1e-9) / 1e9:.1f} TB/s of pixel columns), "
                f"k_win_gather {kg * 1e3:.0f} us ({wb.size * 400 / max(kg, 1e-9) / 1e6:.2f} G cells/s)")
            assert dev.cpu().numpy().tobytes() == tiles.tobytes(), "device-pointer form differs"
            if N_BINS * N_BINS * 8 * 2 < free_bytes():
                t = time.perf_counter()
                M = c.matrix(balance=False).fetch("M1")
                t_fetch = time.perf_counter() - t
                t = time.perf_counter()
                want = np.array([M[r:r + 20, r:r + 20] for r in wb])
                t_slice = time.perf_counter() - t
                assert want.tobytes() == tiles.tobytes(), "GPU and dense slices differ"
                say(f"Cooler.matrix(balance=False).fetch ({M.nbytes / 1e9:.1f} GB dense) {t_fetch * 1e3:.0f} ms + "
                    f"slicing {t_slice * 1e3:.1f} ms, one run: {(t_fetch + t_slice) * 1e3 / ms_file:.0f} x the "
                    f"from-file GPU form; identical tiles")
            else:
                say("dense fetch skipped (the N x N matrix does not fit)")
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
