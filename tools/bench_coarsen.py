"""Measure the coarsening levels (hh_coarsen_count + hh_coarsen_write,
csrc/coarsen.hip) on device-resident pixel tables from the
synthetic generator (hh_synth_pixels):

  * 40k:  hg19 at 40 kb (~8e8 pixels, bench.py's C3 parameters), the chain
          40 kb -> 200 kb -> 1 Mb, every level taken from the one before;
  * 10k:  the diploid whole genome at 10 kb (~5e9 pixels, C4's parameters),
          10 kb -> 40 kb, if it fits.

Per level it prints the time under HIP events (median of --reps after a
warm-up), pixels/s, the bytes moved over that time as a fraction of 8 TB/s --
bytes = ids and counts read by the count pass (12 B per pixel: the count pass
needs the counts for the largest sum and the sign check), the column ids and
counts read by the write pass (8 B), the output written (12 B per coarse pixel)
-- and the per-kernel split (hh_ktime).  For the 40k chain it also prints the
time NumPy takes for the same levels on the host (the restatement of
tests/coarsen_ref.py) and checks that the tables agree.

A run without a GPU fails; there is no fallback.

    python tools/bench_coarsen.py [--sizes 40k,10k] [--reps 5] [--no-numpy]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8e12
KERNELS = ("k_co_map", "k_co_rowptr", "k_co_seg", "k_co_count", "k_co_write")


def level(co, _lib, torch, src, off, k, reps, name):
    """Time one level; returns its device table."""
    p1, p2, pc, c64, nnz, dev = src
    run = lambda: co.coarsen_device(p1, p2, pc, c64, nnz, off, k, dev)
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
    assert torch.equal(o[0], out[0]) and torch.equal(o[1], out[1]) and torch.equal(o[2], out[2])
    _lib.call("hh_ktime_reset")
    _lib.call("hh_ktime_enable", 1)
    run()
    _lib.call("hh_synchronize", None)
    _lib.call("hh_ktime_enable", 0)
    split = ", ".join(f"{kn} {_lib.ktime(kn)[0]:.2f}" for kn in KERNELS)
    t = float(np.median(ms)) * 1e-3
    onnz = int(out[0].numel())
    cw = 8 if c64 else 4
    moved = nnz * (8 + cw) + nnz * (4 + cw) + onnz * (8 + out[2].element_size())
    print(f"{name} (x{k}): {nnz} -> {onnz} pixels, {int(off[-1])} -> {int(out[3][-1])} bins, counts "
          f"{str(out[2].dtype).split('.')[-1]}: {t * 1e3:.2f} ms (median of {reps}, min {min(ms):.2f}), "
          f"{nnz / t * 1e-9:.2f} G pixels/s, {moved * 1e-9:.2f} GB moved = {moved / t * 1e-12:.2f} TB/s = "
          f"{moved / t / HBM:.3f} of 8 TB/s; kernels (ms): {split}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="40k,10k")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()

    import torch
    from hichap_master_amd import _lib, ice, synth
    from hichap_master_amd import coarsen as co
    from tests.coarsen_ref import coarsen_ref

    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    print(f"column tile {co.tile_width()} coarse bins; the project's measured linear-read rate is 6.2 TB/s "
          f"(profiles/r6d/probe.log): what both passes could reach at best", flush=True)
    for size in a.sizes.split(","):
        if size == "40k":
            sizes, target, tf, chain = synth.genome_bins(40000), 8e8, 0.85, ((5, "40 kb -> 200 kb"), (5, "200 kb -> 1 Mb"))
        elif size == "10k":
            sizes, target, tf, chain = synth.genome_bins(10000, diploid=True), 5e9, 0.2, ((4, "10 kb -> 40 kb"),)
        else:
            raise SystemExit(f"unknown size {size}")
        A, td = synth.calibrate(sizes, target, tf)
        try:
            P = ice.SynthPixels(list(sizes), ordered=False, A=A, trans_density=td, comp_block=200, ignore_diags=0,
                                seed=20201015)
        except _lib.HipLibraryError as e:
            print(f"{size}: the table does not fit ({e})", flush=True)
            continue
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        print(f"{size}: {len(sizes)} chromosomes, {int(off[-1])} bins, {P.nnz} pixels "
              f"({12e-9 * P.nnz:.1f} GB of int32 ids and counts in HBM)", flush=True)
        src = (P.bin1.data_ptr(), P.bin2.data_ptr(), P.count.data_ptr(), False, P.nnz, dev)
        levels, o = [], off
        try:
            for k, name in chain:
                out = level(co, _lib, torch, src, o, k, a.reps, name)
                levels.append((src, o, k, name, out))
                src, o = (out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[2].dtype == torch.int64,
                          int(out[0].numel()), dev), out[3]
        except _lib.HipLibraryError as e:
            print(f"{size}: {e}", flush=True)
        if size == "40k" and not a.no_numpy:
            h = []                                                       # the base table on the host
            for p in (P.bin1, P.bin2, P.count):
                t = torch.empty(P.nnz, dtype=torch.int32, device=dev)
                _lib.call("hh_device_copy", _lib.ptr(t), _lib.ptr(p), 4 * P.nnz, None)
                _lib.call("hh_synchronize", None)
                h.append(t.cpu().numpy())
                del t
            for (s, so, k, name, out) in levels:
                n = s[4]
                t0 = time.perf_counter()
                r = coarsen_ref(h[0], h[1], h[2], so, k)
                t_ref = time.perf_counter() - t0
                g = [x.cpu().numpy() for x in out[:3]]
                ok = np.array_equal(g[0], r[0]) and np.array_equal(g[1], r[1]) and np.array_equal(g[2], r[2])
                print(f"{name}: NumPy restatement on the host {t_ref:.1f} s for {n} pixels "
                      f"({'agrees exactly' if ok else 'DIFFERS'})", flush=True)
                assert ok
                h = g                                                    # the next level's source
        del levels
        P.close()


if __name__ == "__main__":
    main()
