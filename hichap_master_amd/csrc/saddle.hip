// Cis expected and compartment saddle on cooler's own pixel table
// (HiCHap has neither: the definitions are this project's).
//
// One chromosome is global bins [lo, lo + N).  The table is sorted by (bin1,
// bin2), so the pixels of local row a are one contiguous range [rp[a],
// rp[a + 1]) and inside it the diagonals d = b - a ascend.  The value of a
// cell is v = count * w[a] * w[b] in that order (NaN -> 0), the raw count
// without weights.  No N x N matrix is made.
//
//   k_sd_valid     valid[a] and its 64-bit masks (one ballot per word).
//   k_sd_rowptr    rp[a] = first pixel with bin1 >= lo + a (bisection in bin1).
//   k_sd_seg       seg[a][J] = first pixel of row a with d >= J T, clipped to
//                  the chromosome and to D + 1 (bisection in bin2 inside the
//                  row, one thread per (a, J)).
//   k_sd_expected  one block per (chunk of kSdRows rows, kSdWaves diagonal
//                  sub-tiles); a wave owns T diagonals in LDS and walks the
//                  rows of the chunk in ascending order, every row's segment
//                  [seg[a][J], seg[a][J + 1]) lane-strided; the pixels of a
//                  row have distinct diagonals, so no two lanes meet on a
//                  cell, and a cell is summed in ascending a.  The next
//                  trip's pixels (of the next row, when the segment ends) are
//                  loaded before the current trip is added.
//   k_sd_exp_sum   sum[d] = the chunks' partials in ascending chunk order.
//   k_sd_nvalid    nvalid[d] = sum over words of popcount(mask & (mask >> d)).
//   k_sd_ecls      ec[a] = cls[a], 255 where the bin is invalid; flags a class
//                  in [K, 254].       k_sd_usable: the usable diagonals.
//   k_sd_rows      one wave per row, lane q owns class q: per step of 64
//                  pixels the lanes stage (ec[b], v / expected[d]) in LDS,
//                  class 255 where the pixel is out of range, invalid or on
//                  an unusable diagonal; every lane then walks the live
//                  entries in lane order and adds those of its class.
//                  rows[a][q] = the row's sum into class q, in pixel order.
//   k_sd_u_part    PU[c][r][q] = sum of rows[a][q] over the rows a of chunk c
//                  (kSdRedRows rows) with ec[a] = r, ascending a.
//   k_sd_u_sum     U[r][q] = the chunks' partials in ascending chunk order.
//   k_sd_cu        Cu from ec and the usable diagonals alone: a block takes
//                  kSdCuRows rows, counts its (a, a + d) pairs in a K x K
//                  uint32 LDS histogram and adds the non-zero cells to Cu with
//                  64-bit integer atomics (integer adds commute).
//
// Every fp64 sum has an order fixed by the table and the build constants
// alone (not by T, the grid or the timing), and no floating-point atomic is
// used: two calls and the host / device forms give the same bits.
// Range checks: rp and seg come from bisections bounded by [0, nnz], a
// segment with end < start is empty, and a pixel's local column, diagonal
// and class are compared against N, the tile and K (ec is < K or 255 by
// construction) before they index anything.  An unsorted or duplicated table
// gives wrong sums (two lanes may then meet on an LDS cell), never an access
// outside the arrays.
#include "pixel_table.hpp"  // PixTable, k_sd_valid, k_sd_rowptr, PixStage

namespace hh {

constexpr int kSdRows = 128;     // rows per chunk of the expected sums (two segment bounds per lane)
constexpr int kSdWaves = 4;      // waves per k_sd_expected block = diagonal sub-tiles per block
constexpr int kSdRedRows = 512;  // rows per chunk of the saddle's row reduction
constexpr int kSdCuRows = 64;    // rows per k_sd_cu block
constexpr int kSdMaxK = 64;
constexpr int64_t kSdMaxN = int64_t(1) << 24;  // bins of one chromosome (k_sd_cu's uint32 cells, the work-item counts)

// first pixel in [a, b) with bin2 >= target (b where none; a where b <= a)
__device__ __forceinline__ long long sd_lower_b2(const int64_t* __restrict__ b2, long long a, long long b,
                                                 long long target) {
    while (a < b) {
        const long long m = a + ((b - a) >> 1);
        if ((long long)b2[m] < target) a = m + 1; else b = m;
    }
    return a;
}

__global__ __launch_bounds__(256) void k_sd_seg(const int64_t* __restrict__ b2, const long long* __restrict__ rp,
                                                long long lo, long long N, long long D, int T, int nJ,
                                                long long* __restrict__ seg) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = nJ + 1;
    if (t >= N * stride) return;
    const long long f = t / stride;
    const long long J = t - f * stride;
    const long long off = min(J * T, D + 1);
    seg[t] = sd_lower_b2(b2, rp[f], rp[f + 1], lo + min(f + off, N));
}

__global__ __launch_bounds__(64 * kSdWaves) void k_sd_expected(PixTable<double> X, const uint8_t* __restrict__ valid,
                                                               const long long* __restrict__ seg, long long D, int T,
                                                               int nJ, double* __restrict__ P) {
    __shared__ double acc[kSdWaves][HH_SADDLE_DIAG_TILE];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int J = blockIdx.y * kSdWaves + wid;
    const bool mine = J < nJ;
    const long long d0 = (long long)J * T;
    const int Tw = mine ? (int)min((long long)T, D + 1 - d0) : 0;
    const long long a0 = (long long)blockIdx.x * kSdRows;
    const int nr = (int)min((long long)kSdRows, X.N - a0);
    for (int q = lane; q < Tw; q += 64) acc[wid][q] = 0.0;
    // the chunk's segment bounds: lane l holds rows l and l + 64 (an invalid row has no segment)
    long long sb[2] = {0, 0}, se[2] = {0, 0};
    if (mine) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = h * 64 + lane;
            if (r < nr && valid[a0 + r]) {
                sb[h] = seg[(a0 + r) * (nJ + 1) + J];
                se[h] = seg[(a0 + r) * (nJ + 1) + J + 1];
            }
        }
    }
    __syncthreads();
    // the walk over (row, trip of 64 pixels); r, p, e are wave-uniform
    int r = -1;
    long long p = 0, e = 0;
    auto next_trip = [&]() -> bool {
        p += 64;
        while (p >= e) {
            if (++r >= nr) return false;
            p = __shfl(r < 64 ? sb[0] : sb[1], r & 63, 64);
            e = __shfl(r < 64 ? se[0] : se[1], r & 63, 64);
        }
        return true;
    };
    bool live = mine && next_trip();
    int nrow = r;
    bool nv = live && p + lane < e;
    long long nb = 0;
    double nc = 0.0;
    if (nv) { nb = (long long)X.b2[p + lane]; nc = X.cnt[p + lane]; }
    while (live) {
        const int row = nrow;
        const bool cv = nv;
        const long long cb = nb;
        const double cc = nc;
        live = next_trip();  // the next trip's loads are in flight while this one is added
        nrow = r;
        nv = live && p + lane < e;
        if (nv) { nb = (long long)X.b2[p + lane]; nc = X.cnt[p + lane]; }
        if (cv) {
            const long long a = a0 + row;
            const unsigned long long bl = (unsigned long long)(cb - X.lo);
            if (bl < (unsigned long long)X.N) {
                const unsigned long long cell = (unsigned long long)((long long)bl - a - d0);
                if (cell < (unsigned long long)Tw && valid[bl]) {
                    double v = cc;
                    if (X.w) {
                        v = v * X.w[a] * X.w[bl];
                        if (v != v) v = 0.0;
                    }
                    acc[wid][cell] += v;
                }
            }
        }
    }
    __syncthreads();
    for (int q = lane; q < Tw; q += 64) P[(long long)blockIdx.x * (D + 1) + d0 + q] = acc[wid][q];
}

__global__ __launch_bounds__(256) void k_sd_exp_sum(const double* __restrict__ P, long long n_chunks, long long D,
                                                    long long g, double* __restrict__ sum) {
    const long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > D) return;
    double s = 0.0;
    if (d >= g)
        for (long long c = 0; c < n_chunks; ++c) s += P[c * (D + 1) + d];
    sum[d] = s;
}

__global__ __launch_bounds__(256) void k_sd_nvalid(const unsigned long long* __restrict__ mask, long long nW,
                                                   long long D, long long g, long long* __restrict__ nvalid) {
    const long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > D) return;
    long long n = 0;
    if (d >= g) {
        const long long ws = d >> 6;
        const int bs = (int)(d & 63);
        for (long long w = 0; w + ws < nW; ++w) {  // mask has nW + 1 words, the last one 0
            unsigned long long x = mask[w + ws] >> bs;
            if (bs) x |= mask[w + ws + 1] << (64 - bs);
            n += __popcll(mask[w] & x);
        }
    }
    nvalid[d] = n;
}

__global__ __launch_bounds__(256) void k_sd_ecls(const uint8_t* __restrict__ cls, const uint8_t* __restrict__ valid,
                                                 long long N, int K, uint8_t* __restrict__ ec,
                                                 unsigned int* __restrict__ err) {
    const long long a = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= N) return;
    unsigned int c = cls[a];
    if (c != 255u && c >= (unsigned int)K) {
        atomicOr(err, 1u);
        c = 255u;
    }
    ec[a] = valid[a] ? (uint8_t)c : (uint8_t)255;
}

__global__ __launch_bounds__(256) void k_sd_usable(const double* __restrict__ expected, long long D, long long min_dist,
                                                   uint8_t* __restrict__ us) {
    const long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > D) return;
    const double x = expected[d];
    us[d] = (d >= min_dist && x - x == 0.0 && x > 0.0) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_sd_rows(PixTable<double> X, const long long* __restrict__ rp,
                                                 const uint8_t* __restrict__ ec, const uint8_t* __restrict__ us,
                                                 const double* __restrict__ expected, long long min_dist, long long D,
                                                 double* __restrict__ rows) {
    __shared__ double sx[4][64];
    __shared__ int sc[4][64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long long a = (long long)blockIdx.x * 4 + wid;
    if (a >= X.N || ec[a] == 255) return;  // (no block barrier below; a row left out is never read)
    // the row's pixels with d in [min_dist, D] inside the chromosome
    const long long r0 = rp[a], r1 = rp[a + 1];
    const long long s = sd_lower_b2(X.b2, r0, r1, X.lo + min(a + min_dist, X.N));
    const long long e = sd_lower_b2(X.b2, s, r1, X.lo + min(a + D + 1, X.N));
    double acc = 0.0;
    bool nv = s + lane < e;
    long long nb = 0;
    double nc = 0.0;
    if (nv) { nb = (long long)X.b2[s + lane]; nc = X.cnt[s + lane]; }
    for (long long p = s; p < e; p += 64) {
        const bool cv = nv;
        const long long cb = nb;
        const double cc = nc;
        nv = p + 64 + lane < e;  // the next step's loads are in flight while this one is added
        if (nv) { nb = (long long)X.b2[p + 64 + lane]; nc = X.cnt[p + 64 + lane]; }
        int c = 255;
        double x = 0.0;
        if (cv) {
            const unsigned long long bl = (unsigned long long)(cb - X.lo);
            if (bl < (unsigned long long)X.N) {
                const long long d = (long long)bl - a;
                if (d >= min_dist && d <= D && us[d]) {
                    c = ec[bl];
                    double v = cc;
                    if (X.w) {
                        v = v * X.w[a] * X.w[bl];
                        if (v != v) v = 0.0;
                    }
                    x = v / expected[d];
                }
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
    rows[a * kSdMaxK + lane] = acc;
}

__global__ __launch_bounds__(64) void k_sd_u_part(const double* __restrict__ rows, const uint8_t* __restrict__ ec,
                                                  long long N, int K, double* __restrict__ PU) {
    const int r = blockIdx.x, q = threadIdx.x;
    const long long a0 = (long long)blockIdx.y * kSdRedRows, a1 = min(a0 + kSdRedRows, N);
    double s = 0.0;
    for (long long a = a0; a < a1; ++a)
        if (ec[a] == r) s += rows[a * kSdMaxK + q];
    PU[((long long)blockIdx.y * K + r) * kSdMaxK + q] = s;
}

__global__ __launch_bounds__(256) void k_sd_u_sum(const double* __restrict__ PU, long long n_chunks, int K,
                                                  double* __restrict__ U) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= K * K) return;
    const int r = t / K, q = t - r * K;
    double s = 0.0;
    for (long long c = 0; c < n_chunks; ++c) s += PU[(c * K + r) * kSdMaxK + q];
    U[t] = s;
}

__global__ __launch_bounds__(256) void k_sd_cu(const uint8_t* __restrict__ ec, const uint8_t* __restrict__ us,
                                               long long N, long long min_dist, long long D, int K,
                                               unsigned long long* __restrict__ Cu) {
    __shared__ unsigned int hist[kSdMaxK * kSdMaxK];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int q = threadIdx.x; q < K * K; q += 256) hist[q] = 0u;
    __syncthreads();
    const long long a0 = (long long)blockIdx.x * kSdCuRows;
    for (int i = wid; i < kSdCuRows; i += 4) {  // at most 64 x 2^24 pairs per block: uint32 cells hold them
        const long long a = a0 + i;
        if (a >= N) break;
        const unsigned int ra = ec[a];
        if (ra == 255u) continue;
        const long long dmax = min(D, N - 1 - a);
        for (long long d = min_dist + lane; d <= dmax; d += 64) {
            const unsigned int cb = ec[a + d];
            if (us[d] && cb != 255u) atomicAdd(&hist[ra * K + cb], 1u);
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < K * K; q += 256)
        if (hist[q]) atomicAdd(&Cu[q], (unsigned long long)hist[q]);
}

}  // namespace hh

using namespace hh;

extern "C" int hh_expected_pixels(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                                  const double* weight, int64_t n_weight, int64_t lo, int64_t N, const uint8_t* bad,
                                  int32_t ignore_diags, int64_t max_dist, double* sum, int64_t* nvalid,
                                  int32_t on_device, void* stream) {
    return guard([&] {
        HH_REQUIRE(N >= 1 && N <= kSdMaxN, "N outside [1, 2^24]");
        check_pixel_table(bin1, bin2, count, nnz, weight, n_weight, lo, N);
        HH_REQUIRE(sum && nvalid, "null outputs");
        HH_REQUIRE(ignore_diags >= 0, "ignore_diags must be >= 0");
        HH_REQUIRE(max_dist >= 0 && max_dist <= N - 1, "max_dist outside [0, N - 1]");
        const long long D = max_dist, g = ignore_diags;
        const int T = g_saddle_diag_tile;
        const long long nJ = D / T + 1, n_chunks = (N + kSdRows - 1) / kSdRows, nBT = (nJ + kSdWaves - 1) / kSdWaves;
        const bool walk = nnz > 0 && g <= D;
        HH_REQUIRE(nBT <= 65535 && N * (nJ + 1) < (int64_t(1) << 36) && n_chunks * (D + 1) < (int64_t(1) << 32),
                   "chromosome too large for the expected sums");
        hipStream_t s = as_stream(stream);
        PixStage<double> S;
        DBuf<double> dsum, P;
        DBuf<long long> dnv, seg;
        SyncOnExit sync{s};  // (destroyed before the buffers above)
        S.init(bin1, bin2, count, nnz, weight, lo, N, bad, kPixMask | (walk ? kPixRows : 0), on_device, s);
        double* psum = sum;
        long long* pnv = (long long*)nvalid;
        if (!on_device) {
            dsum.alloc(D + 1); psum = dsum.p;
            dnv.alloc(D + 1); pnv = dnv.p;
        }
        if (walk) {
            seg.alloc((size_t)(N * (nJ + 1)));
            P.alloc((size_t)(n_chunks * (D + 1)));
            {
                HH_KTIME("k_sd_seg", s);
                hipLaunchKernelGGL(k_sd_seg, dim3(grid_of(N * (nJ + 1))), dim3(256), 0, s, S.X.b2, S.rp.p, S.X.lo,
                                   S.X.N, D, T, (int)nJ, seg.p);
            }
            {
                HH_KTIME("k_sd_expected", s);
                hipLaunchKernelGGL(k_sd_expected, dim3((unsigned)n_chunks, (unsigned)nBT), dim3(64 * kSdWaves), 0, s,
                                   S.X, S.valid.p, seg.p, D, T, (int)nJ, P.p);
            }
            {
                HH_KTIME("k_sd_exp_sum", s);
                hipLaunchKernelGGL(k_sd_exp_sum, dim3(grid_of(D + 1)), dim3(256), 0, s, P.p, n_chunks, D, g, psum);
            }
        }
        {
            HH_KTIME("k_sd_nvalid", s);
            hipLaunchKernelGGL(k_sd_nvalid, dim3(grid_of(D + 1)), dim3(256), 0, s, S.mask.p, S.nW, D, g, pnv);
        }
        HIP_CHECK(hipGetLastError());
        if (!walk) {
            if (on_device) HIP_CHECK(hipMemsetAsync(psum, 0, sizeof(double) * (size_t)(D + 1), s));
            else dsum.zero(s);
        }
        if (!on_device) {
            dsum.download(sum, D + 1, s);
            dnv.download((long long*)nvalid, D + 1, s);
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

extern "C" int hh_saddle_pixels(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                                const double* weight, int64_t n_weight, int64_t lo, int64_t N, const uint8_t* bad,
                                const double* expected, const uint8_t* cls, int32_t K, int64_t min_dist,
                                int64_t max_dist, double* U, int64_t* Cu, int32_t on_device, void* stream) {
    return guard([&] {
        HH_REQUIRE(N >= 1 && N <= kSdMaxN, "N outside [1, 2^24]");
        check_pixel_table(bin1, bin2, count, nnz, weight, n_weight, lo, N);
        HH_REQUIRE(expected && cls && U && Cu, "null arguments");
        HH_REQUIRE(max_dist >= 0 && max_dist <= N - 1, "max_dist outside [0, N - 1]");
        HH_REQUIRE(min_dist >= 1 && min_dist <= max_dist, "min_dist outside [1, max_dist]");
        HH_REQUIRE(K >= 2 && K <= kSdMaxK, "K outside 2..64");
        const long long D = max_dist;
        const long long n_red = (N + kSdRedRows - 1) / kSdRedRows;
        const size_t kk = (size_t)K * K;
        hipStream_t s = as_stream(stream);
        PixStage<double> S;
        DBuf<double> dexp, dU(kk), rows, PU;
        DBuf<uint8_t> dcls, ec(N), us(D + 1);
        DBuf<unsigned int> derr(1);
        DBuf<unsigned long long> dCu(kk);
        SyncOnExit sync{s};  // (destroyed before the buffers above)
        S.init(bin1, bin2, count, nnz, weight, lo, N, bad, kPixValid | kPixRows, on_device, s);
        const double* pexp = expected;
        const uint8_t* pcls = cls;
        if (!on_device) {
            dexp.alloc(D + 1); dexp.upload(expected, D + 1, s); pexp = dexp.p;
            dcls.alloc(N); dcls.upload(cls, N, s); pcls = dcls.p;
        }
        derr.zero(s);
        hipLaunchKernelGGL(k_sd_ecls, dim3(grid_of(N)), dim3(256), 0, s, pcls, S.valid.p, (long long)N, K, ec.p,
                           derr.p);
        hipLaunchKernelGGL(k_sd_usable, dim3(grid_of(D + 1)), dim3(256), 0, s, pexp, D, (long long)min_dist, us.p);
        HIP_CHECK(hipGetLastError());
        unsigned int herr = 0;
        PinnedDown down;
        down.add(derr.p, &herr, 1);
        down.run(s);
        HH_REQUIRE(!herr, "a cls entry is neither a class id below K nor 255");

        dCu.zero(s);
        if (nnz > 0) {
            rows.alloc((size_t)N * kSdMaxK);
            PU.alloc((size_t)n_red * K * kSdMaxK);
            {
                HH_KTIME("k_sd_rows", s);
                hipLaunchKernelGGL(k_sd_rows, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, S.X, S.rp.p, ec.p, us.p,
                                   pexp, (long long)min_dist, D, rows.p);
            }
            {
                HH_KTIME("k_sd_u_part", s);
                hipLaunchKernelGGL(k_sd_u_part, dim3((unsigned)K, (unsigned)n_red), dim3(64), 0, s, rows.p, ec.p,
                                   (long long)N, K, PU.p);
            }
            {
                HH_KTIME("k_sd_u_sum", s);
                hipLaunchKernelGGL(k_sd_u_sum, dim3(grid_of((long long)kk)), dim3(256), 0, s, PU.p, n_red, K, dU.p);
            }
        } else {
            dU.zero(s);
        }
        {
            HH_KTIME("k_sd_cu", s);
            hipLaunchKernelGGL(k_sd_cu, dim3((unsigned)((N + kSdCuRows - 1) / kSdCuRows)), dim3(256), 0, s, ec.p, us.p,
                               (long long)N, (long long)min_dist, D, K, dCu.p);
        }
        HIP_CHECK(hipGetLastError());
        if (on_device) {
            HIP_CHECK(hipMemcpyAsync(U, dU.p, kk * sizeof(double), hipMemcpyDeviceToDevice, s));
            HIP_CHECK(hipMemcpyAsync(Cu, dCu.p, kk * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        } else {
            dU.download(U, kk, s);
            dCu.download((unsigned long long*)Cu, kk, s);
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}
