// The symmetric trans operator on cooler's own pixel table (DESIGN.md §4t;
// HiCHap has no trans eigenvectors and cooltools is absent: the definitions
// are this project's).
//
// The genome, the pixels, v(a, b) = count * w[a] * w[b] (in that order, NaN ->
// 0), `use`, `bad` and valid[x] are §4s's (trans.hip).  T[i][j] = v(min, max)
// for valid i, j on different chromosomes, 0 elsewhere: symmetric, its cis
// blocks empty.  hh_teig_create turns the upper-triangle table into two
// trans-only row-compressed tables and hh_teig_apply computes Y = D T (D X)
// from them by row gathers alone:
//
//   k_te_bininfo  info[x] = chromosome of x, bit 15 set where the bin is invalid
//                 (k_tr_bininfo restated without the classes).
//   k_te_keep     a pixel is kept where both bins are in range and valid and on
//                 different chromosomes; nb[j] = the kept pixels of the block of
//                 256 pixels j (a ballot per wave, four counts in LDS): 8 B per
//                 256 pixels, no flag per pixel.
//   (dev_excl_scan_i64 of nb: base[j], and the number of kept pixels.)
//   k_te_upper    decides "kept" again, kept pixel i -> upper entry e = base[block]
//                 + its rank among the block's kept pixels: row[e] = bin1, partner[e]
//                 = bin2, value[e] = v, key[e] = bin2 << 33 | e.  The table is
//                 sorted by (bin1, bin2) and the compaction keeps its order, so
//                 the upper rows are contiguous with ascending partners.
//   (dev_sort_u64: the stable radix sort of pairs.hip, unchanged, on the bin2
//   bits of the keys.  e is ascending in table order, so after the sort the
//   entries of one bin2 follow each other in ascending bin1.)
//   k_te_lower    lower entry j = (partner row[e], value[e]) of the j-th key: the
//                 transpose, a pure function of the input (no cursor, no timing).
//   k_te_rowptr_u rpU[f] = the kept pixels before rp[f], the first pixel of row f
//                 (k_sd_rowptr's bisection in bin1): base of its block + the kept
//                 pixels of the block before it, counted again (at most 255);
//                 k_te_rowptr_l: rpL[f] = the first sorted key with bin2 >= f (a
//                 bisection).  No floating-point atomic, and no atomic on a
//                 position or a count of the tables: a histogram of bin1 by
//                 integer atomics met 64 lanes on one address and took 2.7 ms of a
//                 3.5 ms build.
//   k_te_dcheck   a d entry on a valid bin that is negative or not finite.
//   k_te_apply    one wave per row i: lane l takes the entries l, l + 64, ... of
//                 the row's lower segment, then of its upper segment, and keeps K
//                 running sums acc[c] += value * (d[j] * X[j][c]) in registers;
//                 the next trip's partner and value are loaded before the current
//                 trip's gather of X[j][0 .. K).  The 64 lane sums are added by
//                 a fixed xor butterfly (32, 16, ..., 1) and lane 0 stores d[i] *
//                 sum; an invalid row stores +0.0.
//
// Every fp64 sum has an order fixed by the two tables alone (not by the grid,
// hh_tune "teig_rows", K or the timing); no floating-point atomic is used and
// no product is contracted into an addition, so column c of a K = 8 call has
// the bits of the K = 1 call on that column.
// Range checks: a pixel's bin1 and bin2 are compared with n_bins before either
// indexes info, the weights or a table; a slot e < the number of kept pixels and
// e < that number by construction (the keys are written here, the sort
// permutes them) and both are compared with it again; the row pointers are
// clamped to [0, that number] (rpU) or bisections bounded by it (rpL), and a
// row whose pointers are out of order is empty; a partner read back in
// k_te_apply is compared with n_bins once more.
// A malformed table (unsorted, bin1 > bin2) gives wrong numbers, never an
// access outside the arrays.
#include "table_walk.hpp"   // DeviceScope, dev_excl_scan_i64, dev_sort_u64
#include "pixel_table.hpp"  // PixStage, grid_of

namespace hh {

constexpr int kTeMaxC = HH_TRANS_MAX_CHROMS;
constexpr unsigned kTeInvalid = 0x8000u, kTeChromMask = 0x7FFFu;
constexpr int kTeSlotBits = 33;  // key = bin2 << 33 | slot: n_bins < 2^31, kept pixels < 2^33

// count * w[a] * w[b] (NaN -> 0): single IEEE operations, §4s's order
__device__ __forceinline__ double te_value(double c, const double* __restrict__ w, long long a, long long b) {
#pragma clang fp contract(off)
    double v = c;
    if (w) {
        v = v * w[a] * w[b];
        if (v != v) v = 0.0;
    }
    return v;
}

__global__ __launch_bounds__(256) void k_te_bininfo(const long long* __restrict__ off, int C,
                                                    const uint8_t* __restrict__ use, const double* __restrict__ w,
                                                    const uint8_t* __restrict__ bad, long long n_bins,
                                                    unsigned int* __restrict__ info) {
    __shared__ long long so[kTeMaxC + 1];
    for (int q = threadIdx.x; q <= C; q += 256) so[q] = off[q];
    __syncthreads();
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_bins) return;
    int lo = 0, hi = C;  // the chromosome q with so[q] <= x < so[q + 1] (so[0] = 0, so[C] = n_bins)
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (so[m] <= x) lo = m; else hi = m;
    }
    bool ok = !use || use[lo];
    if (ok && w) {
        const double t = w[x];
        ok = t - t == 0.0;  // finite
    }
    if (ok && bad && bad[x]) ok = false;
    info[x] = (unsigned int)lo | (ok ? 0u : kTeInvalid);
}

// pixel i is a trans pixel between two valid bins (both ids checked first)
__device__ __forceinline__ bool te_kept(long long a, long long b, const unsigned int* __restrict__ info,
                                        long long n_bins) {
    if ((unsigned long long)a >= (unsigned long long)n_bins || (unsigned long long)b >= (unsigned long long)n_bins)
        return false;
    const unsigned int ia = info[a], ib = info[b];
    return !((ia | ib) & kTeInvalid) && (ia & kTeChromMask) != (ib & kTeChromMask);
}

constexpr int kTeBlock = 256;  // pixels per block of the compaction: one count per block, not one flag per pixel

// the kept pixels of the block before thread t's pixel (exclusive), and the block's total in *tot;
// every thread of the block calls it (two barriers)
__device__ __forceinline__ int te_block_rank(bool k, int* __restrict__ wc, int* __restrict__ tot) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const unsigned long long m = __ballot(k);
    if (lane == 0) wc[wid] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int q = 0; q < kTeBlock / 64; ++q) {
        if (q < wid) before += wc[q];
        all += wc[q];
    }
    __syncthreads();
    *tot = all;
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

// nb[j] = the kept pixels among the pixels [256 j, 256 j + 256)
__global__ __launch_bounds__(kTeBlock) void k_te_keep(const int64_t* __restrict__ b1, const int64_t* __restrict__ b2,
                                                      long long nnz, const unsigned int* __restrict__ info,
                                                      long long n_bins, long long* __restrict__ nb) {
    __shared__ int wc[kTeBlock / 64];
    const long long i = (long long)blockIdx.x * kTeBlock + threadIdx.x;
    const bool k = i < nnz && te_kept((long long)b1[i], (long long)b2[i], info, n_bins);
    int all = 0;
    (void)te_block_rank(k, wc, &all);
    if (threadIdx.x == 0) nb[blockIdx.x] = all;
}

// rpU[f] = the kept pixels before the first pixel of row f: base of its block + the kept pixels of
// the block before it, counted again (rp: k_sd_rowptr's lower bounds in bin1, clamped to [0, nnz];
// base has n_blocks + 1 entries, the last one the total)
__global__ __launch_bounds__(256) void k_te_rowptr_u(const int64_t* __restrict__ b1, const int64_t* __restrict__ b2,
                                                     const unsigned int* __restrict__ info,
                                                     const long long* __restrict__ rp,
                                                     const long long* __restrict__ base, long long nnz,
                                                     long long n_bins, long long n_kept,
                                                     long long* __restrict__ rpU) {
    const int lane = threadIdx.x & 63;
    const long long f = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);  // one wave per row pointer
    if (f > n_bins) return;
    long long r = f == n_bins ? nnz : rp[f];
    r = min(max(r, 0ll), nnz);
    const long long j = r / kTeBlock;  // <= n_blocks, and = n_blocks only where r = nnz is a multiple of 256
    long long c = 0;
    for (long long i = j * kTeBlock + lane; i < r; i += 64)
        c += te_kept((long long)b1[i], (long long)b2[i], info, n_bins) ? 1 : 0;
    c = wave_sum_ll(c);
    if (lane == 0) rpU[f] = min(max(base[j] + c, 0ll), n_kept);
}

// rpL[f] = the first sorted key whose bin2 is >= f (n_kept where none)
__global__ __launch_bounds__(256) void k_te_rowptr_l(const unsigned long long* __restrict__ key, long long n_kept,
                                                     long long n_bins, long long* __restrict__ rpL) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f > n_bins) return;
    long long a = 0, b = n_kept;
    if (f == n_bins) a = n_kept;
    while (a < b) {
        const long long m = a + ((b - a) >> 1);
        if ((long long)(key[m] >> kTeSlotBits) < f) a = m + 1; else b = m;
    }
    rpL[f] = a;
}

__global__ __launch_bounds__(kTeBlock) void k_te_upper(const int64_t* __restrict__ b1, const int64_t* __restrict__ b2,
                                                       const double* __restrict__ cnt, const double* __restrict__ w,
                                                       long long nnz, const unsigned int* __restrict__ info,
                                                       long long n_bins, const long long* __restrict__ base,
                                                       long long n_kept, int32_t* __restrict__ row,
                                                       int32_t* __restrict__ partner, double* __restrict__ value,
                                                       unsigned long long* __restrict__ key) {
    __shared__ int wc[kTeBlock / 64];
    const long long i = (long long)blockIdx.x * kTeBlock + threadIdx.x;
    long long a = 0, b = 0;
    if (i < nnz) { a = (long long)b1[i]; b = (long long)b2[i]; }
    const bool k = i < nnz && te_kept(a, b, info, n_bins);  // as k_te_keep counted it
    int all = 0;
    const long long e = base[blockIdx.x] + te_block_rank(k, wc, &all);
    if (!k || e < 0 || e >= n_kept) return;  // (e < n_kept holds unless the table changed since k_te_keep)
    row[e] = (int32_t)a;  // a, b in range: the pixel was kept
    partner[e] = (int32_t)b;
    value[e] = te_value(cnt[i], w, a, b);
    key[e] = ((unsigned long long)b << kTeSlotBits) | (unsigned long long)e;
}

__global__ __launch_bounds__(256) void k_te_lower(const unsigned long long* __restrict__ key, long long n_kept,
                                                  const int32_t* __restrict__ row, const double* __restrict__ value,
                                                  int32_t* __restrict__ partner, double* __restrict__ out) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_kept) return;
    const unsigned long long e = key[j] & ((1ull << kTeSlotBits) - 1ull);
    if (e >= (unsigned long long)n_kept) return;  // (a permutation of the slots written above)
    partner[j] = row[e];
    out[j] = value[e];
}

__global__ __launch_bounds__(256) void k_te_dcheck(const double* __restrict__ d, const unsigned int* __restrict__ info,
                                                   long long n_bins, unsigned int* __restrict__ err) {
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_bins || (info[x] & kTeInvalid)) return;
    const double t = d[x];
    if (!(t >= 0.0) || t - t != 0.0) atomicOr(err, 1u);
}

struct TeTables {  // the two row-compressed tables on the device
    const long long *rpL, *rpU;
    const int32_t *pL, *pU;
    const double *vL, *vU;
    const unsigned int* info;
    long long n_bins;
};

// lane `lane` adds the entries s0 + lane, s0 + lane + 64, ... of [s0, s1)
template <int K, bool D>
__device__ __forceinline__ void te_walk(const int32_t* __restrict__ part, const double* __restrict__ val,
                                        long long s0, long long s1, int lane, const double* __restrict__ d,
                                        const double* __restrict__ X, long long n_bins, double (&acc)[K]) {
#pragma clang fp contract(off)
    long long i = s0 + lane;
    bool nv = i < s1;
    int nj = 0;
    double nx = 0.0;
    if (nv) { nj = part[i]; nx = val[i]; }
    while (nv) {
        const int j = nj;
        const double v = nx;
        i += 64;
        nv = i < s1;  // the next trip's loads are in flight while this one gathers
        if (nv) { nj = part[i]; nx = val[i]; }
        if ((unsigned int)j >= (unsigned long long)n_bins) continue;
        const double* __restrict__ xr = X + (long long)j * K;
        double x[K];
#pragma unroll
        for (int c = 0; c < K; ++c) x[c] = xr[c];
        if (D) {
            const double dj = d[j];
#pragma unroll
            for (int c = 0; c < K; ++c) x[c] = dj * x[c];
        }
#pragma unroll
        for (int c = 0; c < K; ++c) {
            const double t = v * x[c];
            acc[c] = acc[c] + t;
        }
    }
}

template <int K, bool D>
__global__ __launch_bounds__(1024) void k_te_apply(TeTables T, const double* __restrict__ d,
                                                   const double* __restrict__ X, double* __restrict__ Y) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * (blockDim.x >> 6) + wid;
    if (i >= T.n_bins) return;  // (no block barrier below: the waves are independent)
    double acc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) acc[c] = 0.0;
    const bool ok = !(T.info[i] & kTeInvalid);
    if (ok) {
        te_walk<K, D>(T.pL, T.vL, T.rpL[i], T.rpL[i + 1], lane, d, X, T.n_bins, acc);
        te_walk<K, D>(T.pU, T.vU, T.rpU[i], T.rpU[i + 1], lane, d, X, T.n_bins, acc);
#pragma unroll
        for (int c = 0; c < K; ++c) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc[c] = acc[c] + __shfl_xor(acc[c], o, 64);
        }
        if (D) {
            const double di = d[i];
#pragma unroll
            for (int c = 0; c < K; ++c) acc[c] = di * acc[c];
        }
    }
    if (lane == 0) {
        double* __restrict__ yr = Y + i * K;
#pragma unroll
        for (int c = 0; c < K; ++c) yr[c] = ok ? acc[c] : 0.0;
    }
}

}  // namespace hh

struct hh_teig {
    int device = 0;
    int64_t n_bins = 0, n_kept = 0;
    int32_t C = 0;
    hh::DBuf<unsigned int> info;
    hh::DBuf<long long> rpL, rpU;
    hh::DBuf<int32_t> pL, pU;
    hh::DBuf<double> vL, vU;
    hh::TeTables tables() const {
        return hh::TeTables{rpL.p, rpU.p, pL.p, pU.p, vL.p, vU.p, info.p, (long long)n_bins};
    }
};

namespace hh {
namespace {

template <int K>
void te_launch(const hh_teig& H, const double* d, const double* X, double* Y, int rows, hipStream_t s) {
    const dim3 grid((unsigned)((H.n_bins + rows - 1) / rows)), block(64 * rows);
    HH_KTIME("k_te_apply", s);
    if (d) hipLaunchKernelGGL((k_te_apply<K, true>), grid, block, 0, s, H.tables(), d, X, Y);
    else hipLaunchKernelGGL((k_te_apply<K, false>), grid, block, 0, s, H.tables(), d, X, Y);
}

void te_create(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz, const double* weight,
               int64_t n_weight, const int64_t* off, int32_t C, const uint8_t* use, const uint8_t* bad,
               int32_t on_device, hipStream_t s, hh_teig** out) {
    HH_REQUIRE(out, "null handle pointer");
    HH_REQUIRE(C >= 1 && C <= kTeMaxC, "C outside 1..HH_TRANS_MAX_CHROMS");
    HH_REQUIRE(off, "null chrom_offset");
    HH_REQUIRE(off[0] == 0, "chrom_offset must start at 0");
    for (int q = 0; q < C; ++q) HH_REQUIRE(off[q] < off[q + 1], "chrom_offset must be strictly ascending");
    HH_REQUIRE(off[C] < (int64_t(1) << 31), "n_bins must be below 2^31");
    HH_REQUIRE(nnz >= 0, "bad arguments");
    HH_REQUIRE(nnz == 0 || (bin1 && bin2 && count), "null pixel arrays");
    HH_REQUIRE(!weight || off[C] <= n_weight, "weights do not cover n_bins");
    const long long n_bins = off[C];
    auto H = std::make_unique<hh_teig>();
    PixStage<double> S;
    DBuf<long long> doff(C + 1), nb, base;
    DBuf<uint8_t> duse, dbad;
    DBuf<double> dw;
    DBuf<unsigned long long> key, tot(1);
    DBuf<int32_t> row;
    SyncOnExit sync{s};  // (destroyed before the buffers above and H)
    HIP_CHECK(hipGetDevice(&H->device));
    H->n_bins = n_bins;
    H->C = C;
    upload_pinned_sync(doff.p, (const long long*)off, (size_t)C + 1, s);
    if (use) { duse.alloc(C); upload_pinned_sync(duse.p, use, (size_t)C, s); }
    const double* w = weight;
    const uint8_t* pbad = bad;
    if (!on_device) {
        if (weight) { dw.alloc(n_bins); dw.upload(weight, n_bins, s); w = dw.p; }
        if (bad) { dbad.alloc(n_bins); dbad.upload(bad, n_bins, s); pbad = dbad.p; }
    }
    H->info.alloc(n_bins);
    {
        HH_KTIME("k_te_bininfo", s);
        hipLaunchKernelGGL(k_te_bininfo, dim3(grid_of(n_bins)), dim3(256), 0, s, doff.p, (int)C, duse.p, w, pbad,
                           n_bins, H->info.p);
    }
    H->rpL.alloc(n_bins + 1);
    H->rpU.alloc(n_bins + 1);
    H->rpL.zero(s);
    H->rpU.zero(s);
    HIP_CHECK(hipGetLastError());
    if (nnz > 0 && C > 1) {
        S.init(bin1, bin2, count, nnz, (const double*)nullptr, 0, n_bins, (const uint8_t*)nullptr, kPixRows,
               on_device, s);
        const long long n_blk = (nnz + kTeBlock - 1) / kTeBlock;
        HH_REQUIRE(n_blk < (int64_t(1) << 31), "too many pixels");
        nb.alloc(n_blk + 1);
        base.alloc(n_blk + 1);
        HIP_CHECK(hipMemsetAsync(nb.p + n_blk, 0, sizeof(long long), s));  // the scan's total lands in base[n_blk]
        {
            HH_KTIME("k_te_keep", s);
            hipLaunchKernelGGL(k_te_keep, dim3((unsigned)n_blk), dim3(kTeBlock), 0, s, S.X.b1, S.X.b2, (long long)nnz,
                               H->info.p, n_bins, nb.p);
        }
        HIP_CHECK(hipGetLastError());
        dev_excl_scan_i64(nb.p, base.p, n_blk + 1, tot.p, s);
        unsigned long long n_kept = 0;
        PinnedDown down;
        down.add(tot.p, &n_kept, 1);
        down.run(s);
        // (the radix sort's per-tile offsets are 32-bit)
        HH_REQUIRE(n_kept <= (unsigned long long)nnz && n_kept < (1ull << 32), "too many trans pixels (2^32 or more)");
        H->n_kept = (int64_t)n_kept;
        if (n_kept > 0) {
            const long long m = (long long)n_kept;
            H->pU.alloc(m); H->vU.alloc(m); H->pL.alloc(m); H->vL.alloc(m);
            row.alloc(m);
            key.alloc(m);
            {
                HH_KTIME("k_te_upper", s);
                hipLaunchKernelGGL(k_te_upper, dim3((unsigned)n_blk), dim3(kTeBlock), 0, s, S.X.b1, S.X.b2, S.X.cnt, w,
                                   (long long)nnz, H->info.p, n_bins, base.p, m, row.p, H->pU.p, H->vU.p, key.p);
            }
            HIP_CHECK(hipGetLastError());
            int bits = 1;
            while ((1ll << bits) < n_bins) ++bits;
            dev_sort_u64(key, m, bits, s, kTeSlotBits);
            {
                HH_KTIME("k_te_lower", s);
                hipLaunchKernelGGL(k_te_lower, dim3(grid_of(m)), dim3(256), 0, s, key.p, m, row.p, H->vU.p, H->pL.p,
                                   H->vL.p);
            }
            {
                HH_KTIME("k_te_rowptr", s);
                hipLaunchKernelGGL(k_te_rowptr_u, dim3((unsigned)((n_bins + 4) / 4)), dim3(256), 0, s, S.X.b1, S.X.b2,
                                   H->info.p, S.rp.p, base.p, (long long)nnz, n_bins, m, H->rpU.p);
                hipLaunchKernelGGL(k_te_rowptr_l, dim3(grid_of(n_bins + 1)), dim3(256), 0, s, key.p, m, n_bins,
                                   H->rpL.p);
            }
            HIP_CHECK(hipGetLastError());
        }
    }
    HIP_CHECK(hipStreamSynchronize(s));
    *out = H.release();
}

void te_apply(const hh_teig& H, const double* d, const double* X, int32_t k, double* Y, int32_t on_device,
              hipStream_t s) {
    HH_REQUIRE(k >= 1 && k <= HH_TEIG_MAX_K, "k outside 1..8");
    HH_REQUIRE(X && Y, "null arguments");
    const size_t n = (size_t)H.n_bins, nk = n * (size_t)k;
    DBuf<double> dd, dX, dY;
    DBuf<unsigned int> derr;
    SyncOnExit sync{s};  // (destroyed before the buffers above)
    const double *pd = d, *pX = X;
    double* pY = Y;
    if (!on_device) {
        if (d) { dd.alloc(n); dd.upload(d, n, s); pd = dd.p; }
        dX.alloc(nk); dX.upload(X, nk, s); pX = dX.p;
        dY.alloc(nk); pY = dY.p;
    }
    if (d) {  // before anything is written
        derr.alloc(1);
        derr.zero(s);
        hipLaunchKernelGGL(k_te_dcheck, dim3(grid_of(H.n_bins)), dim3(256), 0, s, pd, H.info.p, (long long)H.n_bins,
                           derr.p);
        HIP_CHECK(hipGetLastError());
        unsigned int herr = 0;
        PinnedDown down;
        down.add(derr.p, &herr, 1);
        down.run(s);
        HH_REQUIRE(!herr, "d has a negative or non-finite entry on a valid bin");
    }
    if (H.n_kept == 0) {  // no trans pixel: no launch on an empty table
        HIP_CHECK(hipMemsetAsync(pY, 0, nk * sizeof(double), s));
    } else {
        const int rows = g_teig_rows;
        switch (k) {
            case 1: te_launch<1>(H, pd, pX, pY, rows, s); break;
            case 2: te_launch<2>(H, pd, pX, pY, rows, s); break;
            case 3: te_launch<3>(H, pd, pX, pY, rows, s); break;
            case 4: te_launch<4>(H, pd, pX, pY, rows, s); break;
            case 5: te_launch<5>(H, pd, pX, pY, rows, s); break;
            case 6: te_launch<6>(H, pd, pX, pY, rows, s); break;
            case 7: te_launch<7>(H, pd, pX, pY, rows, s); break;
            default: te_launch<8>(H, pd, pX, pY, rows, s); break;
        }
        HIP_CHECK(hipGetLastError());
    }
    if (!on_device) dY.download(Y, nk, s);
    HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace
}  // namespace hh

using namespace hh;

extern "C" {

int hh_teig_create(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz, const double* weight,
                   int64_t n_weight, const int64_t* chrom_offset, int32_t C, const uint8_t* use, const uint8_t* bad,
                   int32_t on_device, void* stream, hh_teig** out) {
    return guard([&] {
        te_create(bin1, bin2, count, nnz, weight, n_weight, chrom_offset, C, use, bad, on_device, as_stream(stream),
                  out);
    });
}

int hh_teig_nnz(const hh_teig* h, int64_t* upper, int64_t* lower) {
    return guard([&] {
        HH_REQUIRE(h && upper && lower, "null arguments");
        *upper = h->n_kept;
        *lower = h->n_kept;
    });
}

int hh_teig_export(const hh_teig* h, int32_t which, int64_t* rowptr, int32_t* partner, double* value) {
    return guard([&] {
        HH_REQUIRE(h && rowptr, "null arguments");
        HH_REQUIRE(which == 0 || which == 1, "which must be 0 (upper) or 1 (lower)");
        HH_REQUIRE(h->n_kept == 0 || (partner && value), "null output arrays");
        DeviceScope dev(h->device);
        hipStream_t s = nullptr;
        const size_t m = (size_t)h->n_kept;
        (which ? h->rpL : h->rpU).download((long long*)rowptr, (size_t)h->n_bins + 1, s);
        if (m) {
            (which ? h->pL : h->pU).download(partner, m, s);
            (which ? h->vL : h->vU).download(value, m, s);
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int hh_teig_apply(const hh_teig* h, const double* d, const double* X, int32_t k, double* Y, int32_t on_device,
                  void* stream) {
    return guard([&] {
        HH_REQUIRE(h, "null handle");
        DeviceScope dev(h->device);
        te_apply(*h, d, X, k, Y, on_device, as_stream(stream));
    });
}

int hh_teig_free(hh_teig* h) {
    return guard([&] {
        if (!h) return;
        device_quiesce(h->device);
        delete h;
    });
}

}  // extern "C"
