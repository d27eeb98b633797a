"""Measure the Baum-Welch training of the TAD HMM (hh_hmm_bw_*) on a seeded
genome-scale input: 3.0e5 DI-like observations in 1 500 segments of lengths
8..3 000 (hg19 at 10 kb), M = 3 components, S = 3 and 5 states.

Per S it prints one line each for
  * the input and the operation / byte counts of one EM iteration, computed
    from the shapes, with the time each would take alone at the chip's rates
    and the serial chain of the longest sequence,
  * the device time of one EM iteration (HIP events around its kernels, after
    a warm-up; median of --reps) and the per-kernel split (hh_ktime),
  * the three-pass training (TADCalling.updateParameter x 3) on a host clock
    ending in a synchronise,
  * one NumPy reference iteration (tests/hmm_train_ref.py) on every 16th
    segment, scaled by the observation count, as the CPU baseline.

    python tools/bench_hmm_train.py [--obs 300000] [--segments 1500] [--reps 5]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# rates for the "alone" times: fp64 vector FMA peak 78.6 TFLOP/s (2 flop), an
# fp64 exp taken as 40 flop, HBM 6.0 TB/s achievable; one step of the serial
# chain taken as 64 dependent fp64 instructions of 8 cycles at 2.4 GHz
FP64_FLOPS, EXP_FLOP, HBM_BPS, CHAIN_STEP_S = 78.6e12, 40.0, 6.0e12, 64 * 8 / 2.4e9


def make_input(n_obs, n_seg, seed):
    """Segment lengths 8..3000 (log-uniform, rescaled to n_obs in all) of a
    regime-switching signal: means 6, 0, -6 in blocks of 5..40 bins, sd 1.6,
    6 % exact zeros (unmappable bins)."""
    rng = np.random.default_rng(seed)
    L = np.exp(rng.uniform(np.log(8), np.log(3000), n_seg))
    for _ in range(20):
        L = np.clip(L * n_obs / L.sum(), 8, 3000)
    L = np.maximum(8, L.astype(np.int64))
    L[0] = 3000
    seqs = []
    for n in L:
        reg = np.repeat(rng.integers(0, 3, n // 5 + 1), rng.integers(5, 41, n // 5 + 1))[:n]
        x = np.array([6.0, 0.0, -6.0])[reg] + rng.normal(0, 1.6, n)
        x[rng.random(n) < 0.06] = 0.0
        seqs.append(x)
    return seqs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", type=int, default=300000)
    ap.add_argument("--segments", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    from hichap_master_amd import _lib
    from hichap_master_amd.StructureFind import StructureFind
    from hichap_master_amd.tads import BaumWelchTrainer, GaussianMixtureHMM
    from tests import hmm_train_ref as ref

    _lib.require_gpu()
    seqs = make_input(a.obs, a.segments, a.seed)
    T, K, nmax, M = sum(s.size for s in seqs), len(seqs), max(s.size for s in seqs), 3
    for S in (3, 5):
        sf = StructureFind(Res=10000)
        A, B, pi = getattr(sf, f"init_parameter_state{S}")()
        n_exp, n_fma = S * M * T, 4 * S * S * T
        # doubles per observation: obs read twice; the S*M emissions written and
        # read once; b (written, read twice), alpha, gamma and b / c (written,
        # read once each): 9 S; c and the shift written and read once
        byt = 8 * T * (2 + 2 * S * M + 9 * S + 4)
        t_exp, t_fma, t_b = n_exp * EXP_FLOP / FP64_FLOPS, 2 * n_fma / FP64_FLOPS, byt / HBM_BPS
        t_chain = 2 * nmax * CHAIN_STEP_S
        bound = max((t_exp, "exp"), (t_fma, "recursion FMAs"), (t_b, "bytes"), (t_chain, "serial chain"))[1]
        print(f"S={S} M={M}: {T} observations, {K} segments (longest {nmax}); one iteration: {n_exp} exp "
              f"({t_exp * 1e6:.1f} us alone), {n_fma} recursion FMAs ({t_fma * 1e6:.1f} us), {byt / 1e6:.1f} MB "
              f"({t_b * 1e6:.1f} us), serial chain 2 x {nmax} steps (~{t_chain * 1e6:.0f} us): bound by the {bound}")
        with BaumWelchTrainer(seqs, S, M) as tr:
            m = GaussianMixtureHMM(A, B, pi)
            tr.step(m)  # warm-up
            ms = []
            for _ in range(a.reps):
                tr.step(GaussianMixtureHMM(A, B, pi))
                ms.append(tr.last_step_ms())
            _lib.call("hh_ktime_reset")
            _lib.call("hh_ktime_enable", 1)
            tr.step(GaussianMixtureHMM(A, B, pi))
            _lib.call("hh_synchronize", None)
            _lib.call("hh_ktime_enable", 0)
            split = ", ".join(f"{k} {_lib.ktime(k)[0] * 1e3:.0f} us"
                              for k in ("k_bw_emit", "k_bw_fb", "k_bw_stats", "k_bw_reduce"))
            t0 = time.perf_counter()
            tr.step(GaussianMixtureHMM(A, B, pi))
            wall = time.perf_counter() - t0
        print(f"S={S} one EM iteration: {np.median(ms) * 1e3:.0f} us on the device (min {min(ms) * 1e3:.0f}, "
              f"{a.reps} reps), {wall * 1e3:.2f} ms per host call; kernels: {split}")
        DI_train = {"1": {(i, i + s.size): s for i, s in enumerate(seqs)}}
        sf.updateParameter(DI_train, A, B, pi)  # warm-up (allocations)
        iters = []
        t0 = time.perf_counter()
        AA, BB, p = A, B, pi
        for _ in range(3):
            AA, BB, p, model = sf.updateParameter(DI_train, AA, BB, p)
            iters.append(model.bw_iters)
        _lib.call("hh_synchronize", None)
        t_train = time.perf_counter() - t0
        print(f"S={S} three-pass training: {t_train * 1e3:.1f} ms, iterations {iters} "
              f"({t_train * 1e3 / sum(iters):.2f} ms per iteration with uploads and the host M-step)")
        sub = seqs[::16]
        Bm = np.array(B, float)
        model = (np.array(A, float), np.array(pi, float), Bm[:, 0].copy(), Bm[:, 1].copy(), Bm[:, 2].copy())
        t0 = time.perf_counter()
        ref.step(sub, model)
        t_ref = time.perf_counter() - t0
        Ts = sum(s.size for s in sub)
        print(f"S={S} NumPy reference, one iteration on {Ts} observations ({len(sub)} segments): "
              f"{t_ref * 1e3:.0f} ms = {t_ref * T / Ts * 1e3:.0f} ms scaled to {T} observations")


if __name__ == "__main__":
    main()
