"""Measure the symmetric trans operator and the trans eigenvectors
(hh_teig_*, csrc/transeig.hip; hichap_master_amd/transeig.py) on a synthetic
whole genome: tools/bench_trans.py's genome (hg19's 23 chromosome sizes from
synth.coo_genome, its ICE weights) at a resolution a trans eigenvector is taken
at, the pixel table and the weights in HBM.  synth.coo_genome's trans pixels
are uniform; three +-1 tracks (runs of 8, 21 and 55 bins) are planted by
keeping a trans pixel with probability proportional to 1 + 0.45 s_i s_j + 0.3
t_i t_j + 0.2 u_i u_j, so the solver has three eigenvectors above the noise to
find.  --uniform leaves the genome as tools/bench_trans.py has it (the table and
product figures on that input; its solve has nothing to converge to).

It prints one line each for
  * the input and the bytes one product moves,
  * hh_teig_create: the host clock per call and the per-kernel split (hh_ktime:
    HIP events around every launch),
  * hh_teig_apply at k = 1 and k = 8 on device tensors: the host clock per call
    and the HIP-event time of k_te_apply, with bytes / time next to the
    measured linear-read rate of 6.2 TB/s,
  * with --rows, k_te_apply again at other hh_tune "teig_rows" values (the same
    bits),
  * the trans normalisation (iterations, host clock),
  * a k = 3 solve: cycles, operator columns, product time and host-algebra time,
  * the same solve over the NumPy operator (two weighted np.bincount passes per
    column), the host baseline, and the agreement of the two.

A run without a GPU fails; there is no fallback.

    python tools/bench_transeig.py [--res 250000] [--trans-density 0.3] [--seconds 1.0] [--rows 1,8,16] [--uniform]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINEAR_READ = 6.2e12        # B/s, profiles/r6d/probe.log
CREATE_KERNELS = ("k_te_bininfo", "k_sd_rowptr", "k_te_keep", "k_te_upper", "k_rs_hist", "k_rs_scatter", "k_te_lower",
                  "k_te_rowptr")
PLANTED = (0.45, 0.3, 0.2)  # contrast of the three planted tracks: a trans pixel is kept with p ~ 1 + sum g t_i t_j


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=250000, help="bin size")
    ap.add_argument("--trans-density", type=float, default=0.3)
    ap.add_argument("--A", type=float, default=30.0)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--tol-eig", type=float, default=1e-8)
    ap.add_argument("--max-cycles", type=int, default=40)
    ap.add_argument("--rows", default="", help="also time k_te_apply at these teig_rows values")
    ap.add_argument("--no-host", action="store_true", help="skip the NumPy baseline")
    ap.add_argument("--uniform", action="store_true",
                    help="tools/bench_trans.py's genome as it is, nothing planted: the table and product figures on "
                         "that input (its trans part has no eigenvector above the noise: the solve stops at "
                         "--max-cycles)")
    a = ap.parse_args()

    import torch
    from hichap_master_amd import _lib, ice, synth
    from hichap_master_amd import transeig as te

    _lib.require_gpu()
    sizes = synth.genome_bins(a.res)
    t0 = time.perf_counter()
    rng = np.random.default_rng(20201015)
    b1, b2, c, off = synth.coo_genome(sizes, rng, A=a.A, trans_density=a.trans_density)
    n, C = int(off[-1]), len(sizes)
    chrom = np.repeat(np.arange(C), sizes)
    x = np.arange(n)
    tracks = [np.where((x // 8) % 2 == 0, 1.0, -1.0), np.where(((x + 5) // 21) % 2 == 0, 1.0, -1.0),
              np.where(((x + 11) // 55) % 2 == 0, 1.0, -1.0)]
    track = tracks[0]
    if not a.uniform:
        keep_p = 1.0 + sum(g * t[b1] * t[b2] for g, t in zip(PLANTED, tracks))
        drop = (chrom[b1] != chrom[b2]) & (rng.random(b1.size) * (1.0 + sum(PLANTED)) >= keep_p)
        b1, b2, c = b1[~drop], b2[~drop], c[~drop]
    t_gen = time.perf_counter() - t0
    nnz = int(b1.size)
    w, st = ice.balance(b1, b2, c, n, off, max_iters=300)
    c = c.astype(np.float64)
    n_trans = int(np.count_nonzero(chrom[b1] != chrom[b2]))

    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d1, d2, dc, dw = dev(b1), dev(b2), dev(c), dev(w)

    def create():
        te.TransOperator(d1, d2, dc, dw, off).close()
        return ()

    _, ts = timed(create, a.seconds)
    kt = kernel_times(create, CREATE_KERNELS)
    op = te.TransOperator(d1, d2, dc, dw, off)
    m = op.nnz
    print(f"input: hg19 at {a.res // 1000} kb, {C} chromosomes, {n} bins, {nnz} pixels of which {n_trans} trans, "
          f"{int((op.valid == 0).sum())} masked bins, ICE {st['iters']} iterations (synth.coo_genome A = {a.A}, "
          f"trans_density = {a.trans_density}, "
          + ("its uniform trans pixels as they are: " if a.uniform else
             f"trans pixels thinned by three planted tracks of contrast {PLANTED}: ") +
          f"{t_gen:.0f} s on the host).  The two tables hold {m} entries each, {24e-6 * m:.0f} MB together "
          f"(int32 partner + fp64 value); one product reads them once, + 16 B of row pointers, 8 k B of X and 8 k B "
          f"of Y per bin; the gathers of X come from {8e-3 * n:.0f} k kB that stay in cache")
    print(f"hh_teig_create on device: {np.median(ts) * 1e3:.2f} ms (median of {len(ts)}, min {min(ts) * 1e3:.2f}); "
          f"kernels: " + ", ".join(f"{k} {t * 1e6:.0f} us" for k, t in kt.items())
          + f" (k_rs_*: the stable radix sort of the {m} keys on the bin2 bits)")

    def apply_line(k, label=""):
        X = torch.from_numpy(np.random.default_rng(k).standard_normal((n, k))).cuda()
        dd = torch.from_numpy(np.where(op.valid != 0, 1.0, 0.0)).cuda()
        Y, ts = timed(lambda: op.apply(X, dd), a.seconds / 2)
        again = op.apply(X, dd)
        assert torch.equal(Y, again)                                 # fixed order: the same bits
        kt = kernel_times(lambda: op.apply(X, dd), ("k_te_apply",), reps=10)["k_te_apply"]
        nbytes = 24 * m + 16 * n + 16 * k * n + 8 * n
        print(f"hh_teig_apply k = {k}{label}: {np.median(ts) * 1e6:.0f} us per call on the host clock (median of "
              f"{len(ts)}, min {min(ts) * 1e6:.0f}; it includes the check of d and its synchronisation), k_te_apply "
              f"{kt * 1e6:.0f} us by HIP events = {nbytes / kt * 1e-12:.3f} TB/s = "
              f"{100 * nbytes / kt / LINEAR_READ:.1f} % of 6.2 TB/s over {nbytes * 1e-6:.0f} MB; "
              f"{kt / k * 1e6:.0f} us per column")
        return Y

    apply_line(1)
    Y8 = apply_line(8)
    for rows in [int(x) for x in a.rows.split(",") if x]:
        _lib.call("hh_tune", b"teig_rows", rows)
        assert torch.equal(apply_line(8, f", teig_rows {rows}"), Y8)
        _lib.call("hh_tune", b"teig_rows", 4)

    t0 = time.perf_counter()
    nrm = te.trans_normalise(op, a.tol)
    t_nrm = time.perf_counter() - t0
    print(f"trans normalisation to {a.tol:g}: {nrm['iterations']} iterations, deviation {nrm['deviation']:.3g}, "
          f"converged {nrm['converged']}, {int((op.valid != 0).sum() - nrm['valid'].sum())} bins dropped, "
          f"{t_nrm * 1e3:.1f} ms on the host clock ({t_nrm / max(1, nrm['iterations']) * 1e6:.0f} us per iteration: "
          f"one k = 1 product from host arrays and the host update)")

    t0 = time.perf_counter()
    S = te.top_eigs(op.apply_E, n, a.k, nrm["valid"], a.tol_eig, a.max_cycles, 0)
    t_solve = time.perf_counter() - t0
    V = te.orient(np.where(nrm["valid"][:, None], S["vectors"], np.nan), nrm["valid"], track)
    ok = nrm["valid"]
    r1 = np.corrcoef(V[ok, 0], track[ok])[0, 1]
    print(f"k = {a.k} solve to {a.tol_eig:g}: eigenvalues {S['values']}, residuals {S['residuals']}, converged "
          f"{S['converged']} in {S['cycles']} cycles, {S['columns']} operator columns; {t_solve * 1e3:.0f} ms, of "
          f"which products {S['t_product'] * 1e3:.0f} ms (host arrays in, host arrays out, the M X term on the host) "
          f"and host algebra {S['t_host'] * 1e3:.0f} ms; r(E1, planted track) = {r1:.3f}")

    if not a.no_host:
        t0 = time.perf_counter()
        hop = te.HostTransOperator(b1, b2, c, w, off)
        hop.set_scaling(nrm["d"], nrm["valid"])
        t_make = time.perf_counter() - t0
        t0 = time.perf_counter()
        Sh = te.top_eigs(hop.apply_E, n, a.k, nrm["valid"], a.tol_eig, a.max_cycles, 0)
        t_host = time.perf_counter() - t0
        if S["converged"] and Sh["converged"]:
            np.testing.assert_allclose(Sh["values"], S["values"], rtol=0, atol=2 * a.tol_eig * abs(S["values"][0]))
        print(f"host baseline, the same solve over the NumPy operator: {t_host:.1f} s ({Sh['columns']} columns, "
              f"converged {Sh['converged']} in {Sh['cycles']} cycles, "
              f"products {Sh['t_product']:.1f} s, host algebra {Sh['t_host']:.2f} s; + {t_make:.1f} s to value and "
              f"filter the table); eigenvalues {Sh['values']} (held to 2 tol_eig |theta_1| of the GPU's when both "
              f"converged); GPU solve "
              f"{t_host / t_solve:.1f} x faster, its products {Sh['t_product'] / max(S['t_product'], 1e-9):.0f} x")
    op.close()


if __name__ == "__main__":
    main()
