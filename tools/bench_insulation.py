"""Measure the insulation-score scan (hh_insulation_pixels, K11 k_insulation)
on the input of bench.py's TAD scan line: one synthetic chromosome at chr1's
10 kb size with C2's generator parameters (5e7 pixels), its ICE weights, the
pixel table and the weights in HBM.  Windows of 100 kb, 250 kb, 500 kb and
1 Mb in one call.

It prints one line each for
  * the input, and the cells, bytes and additions the shapes imply,
  * the host-clock time of one on-device call (median over enough repeats to
    fill --seconds, after a warm-up) and the per-kernel split (hh_ktime) of
    k_band_from_pixels and k_insulation,
  * the NumPy restatement (tests/insulation_ref.py) on every 16th bin of the
    dense band-limited matrix, scaled by 16, as the CPU baseline.

A run without a GPU fails; there is no fallback.

    python tools/bench_insulation.py [--nnz 5e7] [--seconds 1.0]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RES = 10000
WINDOWS_BP = (100000, 250000, 500000, 1000000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nnz", type=float, default=5e7)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--ignore-diags", type=int, default=1)
    a = ap.parse_args()

    import torch
    from hichap_master_amd import _lib, ice, synth
    from hichap_master_amd import insulation as ins
    from tests import insulation_ref as ref

    _lib.require_gpu()
    sizes = [synth.chrom_bins([synth.HG19["1"]], RES)[0]]
    A, td = synth.calibrate(sizes, a.nnz, 0.0)
    m = ice.ContactMatrix.synthetic(sizes, A=A, trans_density=td, comp_block=200, seed=20201015)
    w, st = ice.balance_matrix(m)
    b1, b2, c = m.export_upper()
    m.close()
    N = int(sizes[0])
    wbins = [x // RES for x in WINDOWS_BP]
    g = a.ignore_diags
    B = 2 * wbins[-1] - 2
    valid = np.isfinite(w)
    cells = ins.full_cells(wbins[-1], g) * N                         # nested: the largest window's cells, once
    print(f"input: N = {N} bins, {b1.size} pixels, {int((~valid).sum())} masked bins, ICE {st['iters']} iterations; "
          f"windows {wbins} bins, ignore_diags {g}: band {2 * B + 1} x {N} doubles = {8e-6 * (2 * B + 1) * N:.0f} MB "
          f"written once (memset + {24e-6 * b1.size:.0f} MB of pixels read), {cells:.3g} diamond cells = additions "
          f"= {8e-9 * cells:.2f} GB of 8-byte band reads from cache (each band cell is read by up to "
          f"{wbins[-1]} bins), {12e-6 * len(wbins) * N:.1f} MB of results")

    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d1, d2, dc, dw = dev(b1), dev(b2), dev(c.astype(np.float64)), dev(w)
    run = lambda: ins.diamond_sums_pixels(d1, d2, dc, dw, 0, N, wbins, g)
    S, n = run()                                                     # warm-up (allocations)
    torch.cuda.synchronize()
    ts = []
    t_end = time.perf_counter() + a.seconds
    while time.perf_counter() < t_end or len(ts) < 5:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S2, n2 = run()
        ts.append(time.perf_counter() - t0)                          # the call synchronises its stream
    assert torch.equal(S, S2) and torch.equal(n, n2)
    _lib.call("hh_ktime_reset")
    _lib.call("hh_ktime_enable", 1)
    reps = 5
    for _ in range(reps):
        run()
    _lib.call("hh_synchronize", None)
    _lib.call("hh_ktime_enable", 0)
    kb, ki = (_lib.ktime(k)[0] / reps for k in ("k_band_from_pixels", "k_insulation"))
    print(f"hh_insulation_pixels on device: {np.median(ts) * 1e3:.2f} ms per call (median of {len(ts)}, min "
          f"{min(ts) * 1e3:.2f}); kernels: k_band_from_pixels {kb * 1e3:.0f} us, k_insulation {ki * 1e3:.0f} us "
          f"({cells / ki * 1e-6:.1f} G cells/s, {8e-9 * cells / ki:.2f} TB/s of band reads)")

    # CPU baseline: the restatement on every 16th bin of the dense matrix (band-limited: 5 GB dense otherwise)
    keep = b2 - b1 <= B
    r, q, v = b1[keep], b2[keep], c[keep] * w[b1[keep]] * w[b2[keep]]
    bins = list(range(0, N, 16))
    t0 = time.perf_counter()
    Sr = np.zeros((len(wbins), N))
    nr = np.zeros((len(wbins), N), np.int32)
    span = 4096                                                      # dense pieces of 4096 + 2 w_max bins
    for s in range(0, N, span):
        lo, hi = max(0, s - wbins[-1]), min(N, s + span + wbins[-1])
        k = (r >= lo) & (q < hi)
        M = np.zeros((hi - lo, hi - lo))
        M[r[k] - lo, q[k] - lo] = np.nan_to_num(v[k])
        M[q[k] - lo, r[k] - lo] = np.nan_to_num(v[k])
        sub = [i - lo for i in bins if s <= i < min(N, s + span)]
        Sp, npc = ref.diamond_sums(M, valid[lo:hi], wbins, g, bins=sub)
        # the piece reaches w_max bins past its bins, so only the chromosome's ends clip a diamond
        for i in sub:
            Sr[:, i + lo], nr[:, i + lo] = Sp[:, i], npc[:, i]
    t_ref = time.perf_counter() - t0
    Sh, nh = S.cpu().numpy(), n.cpu().numpy()
    assert np.array_equal(nh[:, bins], nr[:, bins])
    # two sums of up to 10^4 non-negative terms: 2 * 10^4 * 2^-53 = 2.2e-12
    np.testing.assert_allclose(Sh[:, bins], Sr[:, bins], rtol=3e-12, atol=0)
    print(f"NumPy restatement on {len(bins)} bins (every 16th; agrees, n exactly and S to 3e-12): {t_ref:.2f} s = "
          f"{t_ref * 16:.1f} s scaled to {N} bins (host baseline only)")


if __name__ == "__main__":
    main()
