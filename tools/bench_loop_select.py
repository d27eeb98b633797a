"""Measure the diagonal rank of loop selection (hh_diag_rank_pixels,
StructureFind.Loop_Selecting's numeric core) on one synthetic chromosome at
C2 size: chr1 at 10 kb, 24 896 bins, 5e7 unique upper-triangle pixels (near
diagonals full, density falling with distance), and a few thousand queries on
stored pixels within 2 Mb of the diagonal (where CallPeaks calls loops).

It times
  * the GPU call with host pixel arrays (the three int64 columns cross PCIe),
  * the GPU call with the pixel table already in HBM (on_device), with the
    buckets in LDS (default) and forced to global memory, and the per-kernel
    split (hh_ktime),
  * the NumPy restatement (loops.diag_rank_reference: lexsort + searchsorted
    over the same pixels),
checks that all of them agree exactly, and writes what it printed to
profiles/loop_select_bench.log.  No target ratio is set: the log is the record.

    python tools/bench_loop_select.py [--pixels 50000000] [--queries 4000] [--reps 5]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_BINS = 24896  # hg38 chr1 (248 956 422 bp) at 10 kb


def make_pixels(n_pix, seed):
    """Unique upper-triangle pixels of one chromosome: pixel density falling
    as d^-1/2 (the near diagonals full), counts 1 + Poisson(60 / (d + 1)^0.8)."""
    rng = np.random.default_rng(seed)
    N = N_BINS
    want = int(n_pix * 1.25)
    d = np.minimum((N * rng.random(want) ** 2).astype(np.int64), N - 1)
    i = (rng.random(want) * (N - d)).astype(np.int64)
    key = np.unique(i * N + (i + d))
    if key.size > n_pix:
        key = np.sort(rng.choice(key, n_pix, replace=False))
    b1, b2 = key // N, key % N
    cnt = 1 + rng.poisson(60.0 / (b2 - b1 + 1.0) ** 0.8)
    return b1, b2, cnt.astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=50_000_000)
    ap.add_argument("--queries", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "loop_select_bench.log"))
    a = ap.parse_args()

    import torch
    from hichap_master_amd import _lib, loops

    _lib.require_gpu()
    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)

    t0 = time.perf_counter()
    b1, b2, cnt = make_pixels(a.pixels, a.seed)
    rng = np.random.default_rng(a.seed + 1)
    near = np.nonzero((b2 - b1 >= 5) & (b2 - b1 <= 200))[0]
    q = rng.choice(near, min(a.queries, near.size), replace=False)
    rows, cols = b1[q], b2[q]
    say(f"input: {N_BINS} bins, {b1.size} pixels ({b1.size * 24 / 1e6:.0f} MB as three int64 columns), "
        f"{rows.size} queries on {np.unique(cols - rows).size} diagonals (5 <= d <= 200); made in "
        f"{time.perf_counter() - t0:.1f} s")

    def timed(fn, reps):
        ts = []
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = fn()
            ts.append(time.perf_counter() - t)
        return r, 1e3 * float(np.median(ts[1:])), 1e3 * min(ts[1:])

    (v, less), ms, mn = timed(lambda: loops.diag_rank(b1, b2, cnt, 0, N_BINS, rows, cols), a.reps)
    say(f"GPU, host pixel arrays (upload + two passes + download): {ms:.1f} ms median (min {mn:.1f}, {a.reps} reps)")
    d1, d2, dc = (torch.from_numpy(x).cuda() for x in (b1, b2, cnt))
    for knob, name in ((8192, "LDS buckets (default)"), (0, "global buckets (rank_lds_buckets 0)")):
        _lib.call("hh_tune", b"rank_lds_buckets", knob)
        (vd, ld), ms, mn = timed(lambda: loops.diag_rank(d1, d2, dc, 0, N_BINS, rows, cols), a.reps)
        _lib.call("hh_ktime_reset")
        _lib.call("hh_ktime_enable", 1)
        loops.diag_rank(d1, d2, dc, 0, N_BINS, rows, cols)
        _lib.call("hh_synchronize", None)
        _lib.call("hh_ktime_enable", 0)
        ka, kb = _lib.ktime("k_rank_lookup")[0], _lib.ktime("k_rank_count")[0]       # ms
        tbs = [b1.size * 24 / (max(k, 1e-9) * 1e-3) / 1e12 for k in (ka, kb)]       # pixel columns read once each
        say(f"GPU, pixels in HBM, {name}: {ms:.2f} ms median per call (min {mn:.2f}); kernels: k_rank_lookup "
            f"{ka * 1e3:.0f} us ({tbs[0]:.1f} TB/s of pixel columns), k_rank_count {kb * 1e3:.0f} us "
            f"({tbs[1]:.1f} TB/s)")
        assert np.array_equal(vd, v) and np.array_equal(ld, less), "device-pointer form differs"
    _lib.call("hh_tune", b"rank_lds_buckets", 8192)
    t = time.perf_counter()
    rv, rl = loops.diag_rank_reference(b1, b2, cnt, 0, N_BINS, rows, cols)
    t_ref = time.perf_counter() - t
    say(f"NumPy restatement (lexsort + searchsorted), one run: {t_ref * 1e3:.0f} ms")
    assert np.array_equal(rv, v) and np.array_equal(rl, less), "GPU and NumPy differ"
    say(f"agreement: value and less identical on all {rows.size} queries "
        f"(less / (N - d) median {np.median(less / (N_BINS - (cols - rows))):.3f})")
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    with open(a.log, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
