"""Measure merging and down-sampling of pixel tables (hh_merge_*, hh_sample_*;
csrc/merge.hip, csrc/sample.hip) on device-resident tables from
the synthetic generator (hh_synth_pixels, one seed per replicate):

  * chr1: one chromosome of 24 926 bins (chr1 at 10 kb), ~5e7 pixels a table;
  * 40k:  hg19 at 40 kb, ~8e8 pixels a table (bench.py's C3 parameters).

Per size it prints, under HIP events (median of --reps after a warm-up),
``merge_pixels`` of two and of four tables (pixels/s over the input pixels) and
``downsample_pixels`` at frac 1/2 (pixels/s and contacts/s, one mix64 per
contact), with the per-kernel split (hh_ktime).  With --host (chr1 only by
default) it also times the host baselines on the same tables and checks the
merge against them: ``np.unique`` + ``np.bincount`` over the concatenation, and
``numpy.random.Generator.binomial`` over the count column.

A run without a GPU fails; there is no fallback.  The tool sets no time limit
of its own: run it under ``timeout`` (both sizes take a few minutes, most of
it the generator and the host baselines).

    python tools/bench_merge_sample.py [--sizes chr1,40k] [--reps 5] [--host chr1]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MERGE_KERNELS = ("k_mg_rowptr", "k_mg_seg", "k_mg_count", "k_mg_write")
SAMPLE_KERNELS = ("k_sa_count", "k_sa_write")


def timed(torch, _lib, run, reps, kernels):
    out = run()                                                          # warm-up (pool allocations)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        o = run()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    assert all(torch.equal(x, y) for x, y in zip(o, out))               # the same bits on every run
    del o
    _lib.call("hh_ktime_reset")
    _lib.call("hh_ktime_enable", 1)
    run()
    _lib.call("hh_synchronize", None)
    _lib.call("hh_ktime_enable", 0)
    split = ", ".join(f"{kn} {_lib.ktime(kn)[0]:.2f}" for kn in kernels)
    return out, float(np.median(ms)), min(ms), split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="chr1,40k")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host", default="chr1", help="sizes whose host baselines are timed too")
    a = ap.parse_args()

    import torch
    from hichap_master_amd import _lib, ice, synth
    from hichap_master_amd import coarsen as co
    from hichap_master_amd.merge import merge_pixels
    from hichap_master_amd.sample import downsample_pixels
    from tests.merge_ref import merge_ref

    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    arch = torch.cuda.get_device_properties(dev).gcnArchName.split(":")[0]
    print(f"# tools/bench_merge_sample.py {' '.join(sys.argv[1:])}".rstrip() +
          f" on one {torch.cuda.get_device_name(dev)} ({arch})", flush=True)
    print(f"column tile {co.tile_width()} bins", flush=True)
    for size in a.sizes.split(","):
        if size == "chr1":
            sizes, target, tf = [24926], 5e7, 0.0
        elif size == "40k":
            sizes, target, tf = synth.genome_bins(40000), 8e8, 0.85
        else:
            raise SystemExit(f"unknown size {size}")
        A, td = synth.calibrate(sizes, target, tf)
        n_bins = int(np.sum(sizes))
        tabs = []
        for rep in range(4):
            P = ice.SynthPixels(list(sizes), ordered=False, A=A, trans_density=td, comp_block=200, ignore_diags=0,
                                seed=20201015 + rep)
            t = []
            for p in (P.bin1, P.bin2, P.count):
                x = torch.empty(P.nnz, dtype=torch.int32, device=dev)
                _lib.call("hh_device_copy", _lib.ptr(x), _lib.ptr(p), 4 * P.nnz, None)
                t.append(x)
            _lib.call("hh_synchronize", None)
            P.close()
            tabs.append(tuple(t))
        contacts = [int(t[2].sum(dtype=torch.int64)) for t in tabs]
        print(f"{size}: {n_bins} bins, 4 tables of {[int(t[0].numel()) for t in tabs]} pixels, {contacts} contacts, "
              f"largest count {max(int(t[2].max()) for t in tabs)}", flush=True)
        for K in (2, 4):
            nin = sum(int(t[0].numel()) for t in tabs[:K])
            out, med, mn, split = timed(torch, _lib, lambda: merge_pixels(tabs[:K], n_bins), a.reps, MERGE_KERNELS)
            print(f"{size}: merge_pixels of {K} tables: {nin} -> {int(out[0].numel())} pixels, counts "
                  f"{str(out[2].dtype).split('.')[-1]}: {med:.2f} ms (median of {a.reps}, min {mn:.2f}), "
                  f"{nin / med * 1e-6:.2f} G pixels/s; kernels (ms): {split}", flush=True)
            if size in a.host.split(",") and K == 2:
                h = [tuple(x.cpu().numpy() for x in t) for t in tabs[:K]]
                t0 = time.perf_counter()
                r = merge_ref(h, n_bins)
                dt = time.perf_counter() - t0
                ok = all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(out, r))
                print(f"{size}: np.unique + bincount over the concatenation of {K} tables on the host: {dt:.2f} s "
                      f"({'agrees exactly' if ok else 'DIFFERS'})", flush=True)
                assert ok
                del h, r
            del out
        t = tabs[0]
        nnz = int(t[0].numel())
        out, med, mn, split = timed(torch, _lib, lambda: downsample_pixels(*t, frac=0.5, seed=1), a.reps,
                                    SAMPLE_KERNELS)
        kept = int(out[2].sum(dtype=torch.int64))
        print(f"{size}: downsample_pixels at 1/2: {nnz} -> {int(out[0].numel())} pixels, {contacts[0]} -> {kept} "
              f"contacts: {med:.2f} ms (median of {a.reps}, min {mn:.2f}), {nnz / med * 1e-6:.2f} G pixels/s, "
              f"{contacts[0] / med * 1e-6:.2f} G contacts/s; kernels (ms): {split}", flush=True)
        if size in a.host.split(","):
            c = t[2].cpu().numpy()
            t0 = time.perf_counter()
            k = np.random.default_rng(1).binomial(c, 0.5)
            keep = k > 0
            dt = time.perf_counter() - t0
            print(f"{size}: numpy Generator.binomial over the count column on the host: {dt:.2f} s "
                  f"({int(keep.sum())} pixels, {int(k.sum())} contacts kept; another stream of random numbers, so "
                  f"only the totals compare)", flush=True)
        del out, tabs


if __name__ == "__main__":
    main()
