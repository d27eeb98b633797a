// Trans block sums and trans saddle on cooler's own pixel table (DESIGN.md
// §4s; HiCHap has neither and cooltools is absent: the definitions are this
// project's).
//
// The genome is C chromosomes, chromosome q the global bins [off[q], off[q +
// 1]).  One call takes the rows of one chromosome p: the pixels with bin1 in
// p, one contiguous range [rp[0], rp[Np]) of the sorted table.  The value of a
// cell is v = count * w[a] * w[b] in that order (NaN -> 0), the raw count
// without weights; weights, `bad` and `cls` are global (one entry per bin of
// the genome).
//
//   k_tr_bininfo   info[x] = chromosome of x (bisection in the offsets staged
//                  in LDS), bit 15 set where the bin is invalid (chromosome not
//                  used, weight not finite, bad), bits 16-23 the class (255
//                  where invalid); flags a class in [K, 254].
//   k_tr_blocks    a wave owns one span of 64 T consecutive pixels of the range
//                  (T = hh_tune "trans_trips") and walks it in trips of 64,
//                  lane l the pixel l of the trip; the next trip's bin1, bin2
//                  and count are loaded before the current trip's gathers.
//                  The pixels are sorted, so inside a trip the pixels of one
//                  (row, partner chromosome q) are a contiguous lane segment: a
//                  segmented Hillis-Steele sum over the lanes (6 steps, x[l] +=
//                  x[l - o] where lane l - o is in the same segment; a pixel
//                  left out enters as +0.0) leaves the segment's sum and pixel
//                  count in its last lane, which adds them to the wave's acc[q]
//                  in LDS; a trip that crosses a row end may hold a q twice, so
//                  the segments are added one row at a time, in lane order.
//                  P[s][q] = the span's sums after its last trip.
//   k_tr_fold      Q[j][q] = the 64 span sums P[64 j .. 64 j + 63][q] added in
//                  ascending order from +0.0, one thread per (j, q); launched
//                  again on its own output until one row is left: a 64-ary tree
//                  whose shape depends on the number of spans alone.
//   k_tr_usable    us[q] = q > p and expected[q] finite and > 0.
//   k_tr_rows      k_sd_rows' scheme on the trans tail of a row (bin2 >= off[p
//                  + 1]): one wave per row, lane i owns class i; per trip of 64
//                  pixels the lanes stage (class of b, v / expected[q]) in LDS,
//                  class 255 where the pixel is left out; every lane walks the
//                  live entries in lane order and adds those of its class.
//   k_tr_u_part    PU[c][r][i] = sum of rows[a][i] over the rows a of chunk c
//                  (kTrRedRows rows) of class r, ascending a.
//   k_tr_u_sum     U[r][i] = the chunks' partials in ascending chunk order.
//
// Every fp64 sum has an order fixed by the table, T and the build constants
// (not by the grid or the timing; the span and trip edges count from the first
// pixel of the range, so the whole table and a slice that holds the rows of p
// give the same bits) and no floating-point atomic is used.  Products and the
// division are single IEEE operations (tr_value).
// Range checks: the range and the row pointers come from bisections bounded
// by [0, nnz]; a pixel's bin1 is compared against the chromosome and its bin2
// against n_bins before either indexes anything; the chromosome and the class
// read from info are < C and < K (or 255) by construction.  An unsorted table
// gives wrong sums (two lanes may meet on acc[q]), never an access outside the
// arrays.
#include "pixel_table.hpp"  // PixStage, k_sd_rowptr

namespace hh {

constexpr int kTrMaxC = HH_TRANS_MAX_CHROMS;
constexpr int kTrMaxK = 64;
constexpr int kTrWaves = 4;       // waves (spans) per k_tr_blocks block
constexpr int kTrRedRows = 512;   // rows per chunk of the saddle's row reduction
constexpr long long kTrFold = 64;  // span sums per group of the block sums' reduction tree
constexpr unsigned kTrInvalid = 0x8000u, kTrChromMask = 0x7FFFu;

// count * w[a] * w[b] (NaN -> 0), over e where `over`: single IEEE operations
__device__ __forceinline__ double tr_value(double c, const double* __restrict__ w, long long a, long long b, bool over,
                                           double e) {
#pragma clang fp contract(off)
    double v = c;
    if (w) {
        v = v * w[a] * w[b];
        if (v != v) v = 0.0;
    }
    if (over) v = v / e;
    return v;
}

// first pixel in [a, b) with bin2 >= target (b where none; a where b <= a)
__device__ __forceinline__ long long tr_lower_b2(const int64_t* __restrict__ b2, long long a, long long b,
                                                 long long target) {
    while (a < b) {
        const long long m = a + ((b - a) >> 1);
        if ((long long)b2[m] < target) a = m + 1; else b = m;
    }
    return a;
}

__global__ __launch_bounds__(256) void k_tr_bininfo(const long long* __restrict__ off, int C,
                                                    const uint8_t* __restrict__ use, const double* __restrict__ w,
                                                    const uint8_t* __restrict__ bad, const uint8_t* __restrict__ cls,
                                                    int K, long long n_bins, unsigned int* __restrict__ info,
                                                    unsigned int* __restrict__ err) {
    __shared__ long long so[kTrMaxC + 1];
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
    unsigned int c = 255u;
    if (cls) {
        c = cls[x];
        if (c != 255u && c >= (unsigned int)K) {
            atomicOr(err, 1u);
            c = 255u;
        }
    }
    if (!ok) c = 255u;
    info[x] = (unsigned int)lo | (ok ? 0u : kTrInvalid) | (c << 16);
}

struct TrGenome {  // the chromosome p of the call inside the genome
    long long lo, hi, n_bins;  // p = [lo, hi)
    int p, C;
};

__global__ __launch_bounds__(64 * kTrWaves) void k_tr_blocks(const int64_t* __restrict__ b1,
                                                             const int64_t* __restrict__ b2,
                                                             const double* __restrict__ cnt,
                                                             const double* __restrict__ w,
                                                             const unsigned int* __restrict__ info, TrGenome G,
                                                             long long r0, long long r1, long long g, int trips,
                                                             long long n_spans, double* __restrict__ P,
                                                             long long* __restrict__ Pn) {
    __shared__ double acc[kTrWaves][kTrMaxC];
    __shared__ int accn[kTrWaves][kTrMaxC];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long long s = (long long)blockIdx.x * kTrWaves + wid;
    if (s >= n_spans) return;  // (no block barrier below: the waves are independent)
    const long long start = r0 + s * 64 * trips, end = min(start + (long long)64 * trips, r1);
    for (int q = lane; q < G.C; q += 64) { acc[wid][q] = 0.0; accn[wid][q] = 0; }
    __builtin_amdgcn_wave_barrier();
    bool nv = start + lane < end;
    long long na = 0, nb = 0;
    double nc = 0.0;
    if (nv) { na = (long long)b1[start + lane]; nb = (long long)b2[start + lane]; nc = cnt[start + lane]; }
    for (long long i = start; i < end; i += 64) {
        const bool cv = nv;
        const long long a = na, b = nb;
        const double c = nc;
        nv = i + 64 + lane < end;  // the next trip's loads are in flight while this one is summed
        if (nv) { na = (long long)b1[i + 64 + lane]; nb = (long long)b2[i + 64 + lane]; nc = cnt[i + 64 + lane]; }
        unsigned int key = kTrChromMask;  // no chromosome: a lane past the end or a bin2 out of range
        int n = 0;
        double x = 0.0;
        if (cv && (unsigned long long)b < (unsigned long long)G.n_bins) {
            const unsigned int ib = info[b];
            key = ib & kTrChromMask;
            if (a >= G.lo && a < G.hi && !(ib & kTrInvalid) && !(info[a] & kTrInvalid) && (int)key >= G.p &&
                ((int)key > G.p || b - a >= g)) {
                n = 1;
                x = tr_value(c, w, a, b, false, 1.0);
            }
        }
        // the (row, q) segments of the trip, numbered in lane order (the table is sorted by (bin1,
        // bin2): the lanes of a segment are consecutive), and the segmented sum over them
        const unsigned int kp = __shfl_up(key, 1, 64);
        const long long ap = __shfl_up(a, 1, 64);
        const unsigned long long heads = __ballot(lane == 0 || kp != key || ap != a);
        const int seg = __popcll(heads & ((2ull << lane) - 1ull));
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int so = __shfl_up(seg, o, 64);
            const double xo = __shfl_up(x, o, 64);
            const int no = __shfl_up(n, o, 64);
            if (lane >= o && so == seg) { x = x + xo; n += no; }
        }
        // a segment's last lane holds its sums
        const bool last = (lane == 63 || ((heads >> (lane + 1)) & 1ull)) && n > 0 && key < (unsigned int)G.C;
        // A trip that holds the end of one row and the start of the next may hold a q twice: the
        // segments are added to acc one row at a time (inside a row the q are distinct), in lane order.
        unsigned long long m = __ballot(last);
        while (m) {
            const long long aj = __shfl(a, __ffsll((long long)m) - 1, 64);
            const bool go = last && a == aj && ((m >> lane) & 1ull);
            if (go) {
                acc[wid][key] += x;
                accn[wid][key] += n;
            }
            m &= ~__ballot(go);
            __builtin_amdgcn_wave_barrier();
        }
    }
    for (int q = lane; q < G.C; q += 64) {
        P[s * G.C + q] = acc[wid][q];
        Pn[s * G.C + q] = accn[wid][q];
    }
}

// Q[j][q] = P[64 j][q] + ... + P[64 j + 63][q] in ascending order from +0.0 (one thread per (j, q))
__global__ __launch_bounds__(256) void k_tr_fold(const double* __restrict__ P, const long long* __restrict__ Pn,
                                                 long long n, int C, double* __restrict__ Q,
                                                 long long* __restrict__ Qn) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long j = t / C;
    const int q = (int)(t - j * C);
    if (j * kTrFold >= n) return;
    const long long s1 = min((j + 1) * kTrFold, n);
    double x = 0.0;
    long long m = 0;
    for (long long s = j * kTrFold; s < s1; ++s) {
        x += P[s * C + q];
        m += Pn[s * C + q];
    }
    Q[t] = x;
    Qn[t] = m;
}

__global__ __launch_bounds__(kTrMaxC) void k_tr_usable(const double* __restrict__ expected, int p, int C,
                                                       uint8_t* __restrict__ us) {
    const int q = threadIdx.x;
    if (q >= C) return;
    const double x = expected[q];
    us[q] = (q > p && x - x == 0.0 && x > 0.0) ? 1 : 0;
}

// ec[r] = the class of row r of the chromosome, 255 where the bin is invalid or left out
__global__ __launch_bounds__(256) void k_tr_rowcls(const unsigned int* __restrict__ info, long long lo, long long N,
                                                   uint8_t* __restrict__ ec) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) ec[r] = (uint8_t)(info[lo + r] >> 16);
}

__global__ __launch_bounds__(256) void k_tr_rows(const int64_t* __restrict__ b2, const double* __restrict__ cnt,
                                                 const double* __restrict__ w, const unsigned int* __restrict__ info,
                                                 TrGenome G, const long long* __restrict__ rp,
                                                 const uint8_t* __restrict__ ec, const uint8_t* __restrict__ us,
                                                 const double* __restrict__ expected, double* __restrict__ rows) {
    __shared__ double sx[4][64];
    __shared__ int sc[4][64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * 4 + wid, N = G.hi - G.lo;
    if (r >= N || ec[r] == 255) return;  // (no block barrier below; a row left out is never read)
    const long long a = G.lo + r;
    const long long r1 = rp[r + 1];
    const long long s = tr_lower_b2(b2, rp[r], r1, G.hi);  // the trans tail of the row
    double acc = 0.0;
    bool nv = s + lane < r1;
    long long nb = 0;
    double nc = 0.0;
    if (nv) { nb = (long long)b2[s + lane]; nc = cnt[s + lane]; }
    for (long long i = s; i < r1; i += 64) {
        const bool cv = nv;
        const long long b = nb;
        const double cc = nc;
        nv = i + 64 + lane < r1;  // the next trip's loads are in flight while this one is added
        if (nv) { nb = (long long)b2[i + 64 + lane]; nc = cnt[i + 64 + lane]; }
        int c = 255;
        double x = 0.0;
        if (cv && (unsigned long long)b < (unsigned long long)G.n_bins) {
            const unsigned int ib = info[b];
            const int q = (int)(ib & kTrChromMask);  // < C by construction
            if (!(ib & kTrInvalid) && q > G.p && us[q]) {
                c = (int)(ib >> 16);
                if (c != 255) x = tr_value(cc, w, a, b, true, expected[q]);
            }
        }
        unsigned long long m = __ballot(c != 255);
        if (m) {
            sx[wid][lane] = x;
            sc[wid][lane] = c;
            __builtin_amdgcn_wave_barrier();
            while (m) {  // the live entries in lane order: the row's pixel order
                const int j = __ffsll((long long)m) - 1;
                m &= m - 1;
                if (sc[wid][j] == lane) acc += sx[wid][j];
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    rows[r * kTrMaxK + lane] = acc;
}

__global__ __launch_bounds__(64) void k_tr_u_part(const double* __restrict__ rows, const uint8_t* __restrict__ ec,
                                                  long long N, int K, double* __restrict__ PU) {
    const int r = blockIdx.x, q = threadIdx.x;
    const long long a0 = (long long)blockIdx.y * kTrRedRows, a1 = min(a0 + kTrRedRows, N);
    double s = 0.0;
    for (long long a = a0; a < a1; ++a)
        if (ec[a] == r) s += rows[a * kTrMaxK + q];
    PU[((long long)blockIdx.y * K + r) * kTrMaxK + q] = s;
}

__global__ __launch_bounds__(256) void k_tr_u_sum(const double* __restrict__ PU, long long n_chunks, int K,
                                                  double* __restrict__ U) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= K * K) return;
    const int r = t / K, q = t - r * K;
    double s = 0.0;
    for (long long c = 0; c < n_chunks; ++c) s += PU[(c * K + r) * kTrMaxK + q];
    U[t] = s;
}

namespace {

// The argument checks both entry points share, and the genome on the device:
// the offsets and `use` (host arrays in either form) uploaded, the global
// weights, `bad` and `cls` uploaded unless already there, and info.
struct TrStage {
    DBuf<long long> doff;
    DBuf<uint8_t> duse, dbad, dcls;
    DBuf<double> dw;
    DBuf<unsigned int> info, derr;
    const double* w = nullptr;
    TrGenome G{};

    static void check(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                      const double* weight, int64_t n_weight, const int64_t* off, int32_t C, int32_t p) {
        HH_REQUIRE(C >= 1 && C <= kTrMaxC, "C outside 1..HH_TRANS_MAX_CHROMS");
        HH_REQUIRE(off, "null chrom_offset");
        HH_REQUIRE(off[0] == 0, "chrom_offset must start at 0");
        for (int q = 0; q < C; ++q) HH_REQUIRE(off[q] < off[q + 1], "chrom_offset must be strictly ascending");
        HH_REQUIRE(p >= 0 && p < C, "p outside [0, C)");
        HH_REQUIRE(off[p + 1] - off[p] <= (int64_t(1) << 24), "chromosome p has more than 2^24 bins");
        HH_REQUIRE(nnz >= 0, "bad arguments");
        HH_REQUIRE(nnz == 0 || (bin1 && bin2 && count), "null pixel arrays");
        HH_REQUIRE(!weight || off[C] <= n_weight, "weights do not cover n_bins");
    }

    // returns false when a cls entry is neither below K nor 255
    bool init(const double* weight, const int64_t* off, int32_t C, const uint8_t* use, const uint8_t* bad,
              const uint8_t* cls, int32_t K, int32_t p, int32_t on_device, hipStream_t s) {
        const long long n_bins = off[C];
        G = TrGenome{(long long)off[p], (long long)off[p + 1], n_bins, p, C};
        doff.alloc(C + 1);
        upload_pinned_sync(doff.p, (const long long*)off, (size_t)C + 1, s);
        if (use) { duse.alloc(C); upload_pinned_sync(duse.p, use, (size_t)C, s); }
        w = weight;
        const uint8_t *pbad = bad, *pcls = cls;
        if (!on_device) {
            if (weight) { dw.alloc(n_bins); dw.upload(weight, n_bins, s); w = dw.p; }
            if (bad) { dbad.alloc(n_bins); dbad.upload(bad, n_bins, s); pbad = dbad.p; }
            if (cls) { dcls.alloc(n_bins); dcls.upload(cls, n_bins, s); pcls = dcls.p; }
        }
        info.alloc(n_bins);
        derr.alloc(1);
        derr.zero(s);
        {
            HH_KTIME("k_tr_bininfo", s);
            hipLaunchKernelGGL(k_tr_bininfo, dim3(grid_of(n_bins)), dim3(256), 0, s, doff.p, C, duse.p, w, pbad, pcls,
                               K, n_bins, info.p, derr.p);
        }
        HIP_CHECK(hipGetLastError());
        if (!cls) return true;
        unsigned int herr = 0;
        PinnedDown down;
        down.add(derr.p, &herr, 1);
        down.run(s);
        return !herr;
    }
};

}  // namespace
}  // namespace hh

using namespace hh;

extern "C" int hh_trans_blocks(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                               const double* weight, int64_t n_weight, const int64_t* chrom_offset, int32_t C,
                               const uint8_t* use, const uint8_t* bad, int32_t p, int32_t ignore_diags, double* sum,
                               int64_t* npix, int32_t on_device, void* stream) {
    return guard([&] {
        TrStage::check(bin1, bin2, count, nnz, weight, n_weight, chrom_offset, C, p);
        HH_REQUIRE(sum && npix, "null outputs");
        HH_REQUIRE(ignore_diags >= 0, "ignore_diags must be >= 0");
        const int trips = g_trans_trips;
        hipStream_t s = as_stream(stream);
        PixStage<double> S;
        TrStage T;
        DBuf<double> dsum, P, F[2];
        DBuf<long long> dnp, Pn, Fn[2];
        SyncOnExit sync{s};  // (destroyed before the buffers above)
        T.init(weight, chrom_offset, C, use, bad, nullptr, 0, p, on_device, s);
        const long long N = T.G.hi - T.G.lo;
        S.init(bin1, bin2, count, nnz, (const double*)nullptr, T.G.lo, N, (const uint8_t*)nullptr, kPixRows, on_device,
               s);
        long long r0 = 0, r1 = 0;  // the pixels of the rows of p
        if (nnz > 0) {
            PinnedDown down;
            down.add(S.rp.p, &r0, 1);
            down.add(S.rp.p + N, &r1, 1);
            down.run(s);
            HH_REQUIRE(r0 >= 0 && r0 <= r1 && r1 <= nnz, "row pointers out of range");
        }
        const long long span = (long long)64 * trips, n_spans = (r1 - r0 + span - 1) / span;
        HH_REQUIRE(n_spans * C < (int64_t(1) << 31), "too many pixels for the block sums");
        double* psum = sum;
        long long* pnp = (long long*)npix;
        if (!on_device) {
            dsum.alloc(C); psum = dsum.p;
            dnp.alloc(C); pnp = dnp.p;
        }
        if (n_spans > 0) {
            P.alloc((size_t)(n_spans * C));
            Pn.alloc((size_t)(n_spans * C));
            {
                HH_KTIME("k_tr_blocks", s);
                hipLaunchKernelGGL(k_tr_blocks, dim3((unsigned)((n_spans + kTrWaves - 1) / kTrWaves)),
                                   dim3(64 * kTrWaves), 0, s, S.X.b1, S.X.b2, S.X.cnt, T.w, T.info.p, T.G, r0, r1,
                                   (long long)ignore_diags, trips, n_spans, P.p, Pn.p);
            }
            // the 64-ary tree over the span sums; its last level writes the outputs
            const double* cur = P.p;
            const long long* curn = Pn.p;
            long long n = n_spans;
            int k = 0;
            for (int i = 0; i < 2; ++i) {  // two buffers, taken in turn: the levels shrink by 64
                n = (n + kTrFold - 1) / kTrFold;
                if (n > 1) { F[i].alloc((size_t)(n * C)); Fn[i].alloc((size_t)(n * C)); }
            }
            n = n_spans;
            HH_KTIME("k_tr_fold", s);
            do {
                const long long ng = (n + kTrFold - 1) / kTrFold;
                double* out = ng > 1 ? F[k].p : psum;
                long long* outn = ng > 1 ? Fn[k].p : pnp;
                hipLaunchKernelGGL(k_tr_fold, dim3(grid_of(ng * C)), dim3(256), 0, s, cur, curn, n, (int)C, out, outn);
                cur = out;
                curn = outn;
                n = ng;
                k ^= 1;
            } while (n > 1);
        } else {
            HIP_CHECK(hipMemsetAsync(psum, 0, sizeof(double) * (size_t)C, s));
            HIP_CHECK(hipMemsetAsync(pnp, 0, sizeof(long long) * (size_t)C, s));
        }
        HIP_CHECK(hipGetLastError());
        if (!on_device) {
            dsum.download(sum, C, s);
            dnp.download((long long*)npix, C, s);
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

extern "C" int hh_trans_saddle(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                               const double* weight, int64_t n_weight, const int64_t* chrom_offset, int32_t C,
                               const uint8_t* use, const uint8_t* bad, int32_t p, const double* expected,
                               const uint8_t* cls, int32_t K, double* U, int32_t on_device, void* stream) {
    return guard([&] {
        TrStage::check(bin1, bin2, count, nnz, weight, n_weight, chrom_offset, C, p);
        HH_REQUIRE(expected && cls && U, "null arguments");
        HH_REQUIRE(K >= 2 && K <= kTrMaxK, "K outside 2..64");
        const size_t kk = (size_t)K * K;
        hipStream_t s = as_stream(stream);
        PixStage<double> S;
        TrStage T;
        DBuf<double> dexp, dU(kk), rows, PU;
        DBuf<uint8_t> ec, us(C);
        SyncOnExit sync{s};  // (destroyed before the buffers above)
        HH_REQUIRE(T.init(weight, chrom_offset, C, use, bad, cls, K, p, on_device, s),
                   "a cls entry is neither a class id below K nor 255");
        const long long N = T.G.hi - T.G.lo, n_red = (N + kTrRedRows - 1) / kTrRedRows;
        S.init(bin1, bin2, count, nnz, (const double*)nullptr, T.G.lo, N, (const uint8_t*)nullptr, kPixRows, on_device,
               s);
        const double* pexp = expected;
        if (!on_device) { dexp.alloc(C); dexp.upload(expected, C, s); pexp = dexp.p; }
        if (nnz > 0) {
            ec.alloc(N);
            rows.alloc((size_t)N * kTrMaxK);
            PU.alloc((size_t)n_red * K * kTrMaxK);
            hipLaunchKernelGGL(k_tr_usable, dim3(1), dim3(kTrMaxC), 0, s, pexp, (int)p, (int)C, us.p);
            hipLaunchKernelGGL(k_tr_rowcls, dim3(grid_of(N)), dim3(256), 0, s, T.info.p, T.G.lo, N, ec.p);
            {
                HH_KTIME("k_tr_rows", s);
                hipLaunchKernelGGL(k_tr_rows, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, S.X.b2, S.X.cnt, T.w,
                                   T.info.p, T.G, S.rp.p, ec.p, us.p, pexp, rows.p);
            }
            {
                HH_KTIME("k_tr_u_part", s);
                hipLaunchKernelGGL(k_tr_u_part, dim3((unsigned)K, (unsigned)n_red), dim3(64), 0, s, rows.p, ec.p, N, K,
                                   PU.p);
            }
            {
                HH_KTIME("k_tr_u_sum", s);
                hipLaunchKernelGGL(k_tr_u_sum, dim3(grid_of((long long)kk)), dim3(256), 0, s, PU.p, n_red, K, dU.p);
            }
        } else {
            dU.zero(s);
        }
        HIP_CHECK(hipGetLastError());
        if (on_device) HIP_CHECK(hipMemcpyAsync(U, dU.p, kk * sizeof(double), hipMemcpyDeviceToDevice, s));
        else dU.download(U, kk, s);
        HIP_CHECK(hipStreamSynchronize(s));
    });
}
