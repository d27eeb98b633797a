// Stratum-adjusted correlation of two pixel tables of one chromosome
// (HiCHap has no reproducibility score: the definition is this
// project's).
//
// Table A is global bins [lo_a, lo_a + N), table B [lo_b, lo_b + N); both are
// sorted by (bin1, bin2), so the pixels of local row r are one range [rp[r],
// rp[r + 1]) with ascending columns.  x(a, b) is the symmetric value of A,
// (count * w[bin1]) * w[bin2] (NaN -> 0; the raw count without weights), 0
// where a bin is invalid on either side or |a - b| < ignore_diags; y the same
// of B.  SX(a, b) is the plain sum of x over the (2h + 1)^2 window around (a,
// b), X = SX / (nv(a) nv(b)), nv the valid bins of a bin's window.  Per
// stratum d the call returns the number of cells (a, a + d) between valid
// bins with SX or SY non-zero and the sums of X, Y, X^2, Y^2, X Y over them.
// No N x N matrix is made.
//
//   k_scc_valid    valid = valid_a & valid_b.
//   k_scc_nv       nv[a] = valid bins in [a - h, a + h], clipped to [0, N).
//   k_scc_moments  a work item is R rows by T = kSccT strata, rows [a0, a0 +
//                  R), strata [d0, d0 + T).  Its block keeps two fp64 patches
//                  in LDS, one per table, of PR = R + 2h rows [a0 - h, ...) by
//                  PC = R + T - 1 + 2h columns [a0 + d0 - h, ...):
//                  1. both patches are zeroed;
//                  2. a wave takes every 16th patch row; its lanes bisect, one
//                     row each and side by side, the row's first pixel at or
//                     right of the patch (and of the diagonal); then the wave
//                     stores row after row the at most PC <= 128 pixels from
//                     there that fall inside the patch, two per lane, with
//                     plain LDS stores;
//                     where the patch reaches below the diagonal (d0 < R +
//                     2h) a wave per patch column does the same with the
//                     table row of that column, transposed.  Pixels are
//                     unique and the two parts are disjoint: a cell is stored
//                     at most once;
//                  3. h > 0: every patch row is replaced by its sliding sums
//                     over 2h + 1 columns (a wave per row, sums in registers
//                     until every wave has read);
//                  4. a lane per cell adds the 2h + 1 rows above and below:
//                     4h + 2 LDS reads per cell for both tables; a half wave
//                     is one row's T strata, so a lane stays on its stratum
//                     and keeps n and the five sums in registers.
//                  A block takes kSccSegBlocks row blocks in ascending order,
//                  then the lanes of a stratum are added through LDS in lane
//                  order: partial[segment][stratum].
//   k_scc_sum      n[d], S[k][d] = the segments' partials in ascending order.
//
// Every fp64 sum has an order fixed by the tables, h and R alone, the two
// tables go through the same instructions, products are not contracted into
// the additions and no floating-point atomic is used: two calls and the host
// / device forms give the same bits, and swapping A and B swaps Sx / Sy and
// Sxx / Syy bitwise.
// Range checks: rp comes from bisections bounded by [0, nnz]; a patch row or
// column outside [0, N) is skipped; a pixel's local column is compared with
// the patch's clipped column range before it indexes valid, the weights or the
// patch.  An unsorted or duplicated table gives wrong sums, never an access
// outside the arrays.
#include "pixel_table.hpp"  // PixTable, PixStage, k_sd_rowptr

namespace hh {

constexpr int kSccT = 32;         // strata per work item: a half wave
constexpr int kSccThreads = 1024;
constexpr int kSccWaves = kSccThreads / 64;
constexpr int kSccMaxPR = 72;     // patch rows: R + 2h (R <= 72 - 2h by default, <= 32 when forced)
constexpr int kSccRowsPerWave = (2 * kSccMaxPR + kSccWaves - 1) / kSccWaves;  // of both patches, pass 3
constexpr int kSccSegBlocks = 8;  // row blocks per block
constexpr int64_t kSccMaxN = int64_t(1) << 24;

// rows per work item (hh_tune "scc_rows"; 0: 72 - 2h down to a multiple of 8, in [32, 64])
inline int scc_rows_of(int h) {
    if (g_scc_rows) return g_scc_rows;
    return std::min(64, std::max(32, (kSccMaxPR - 2 * h) / 8 * 8));
}

__global__ __launch_bounds__(256) void k_scc_valid(const uint8_t* __restrict__ va, const uint8_t* __restrict__ vb,
                                                   long long N, uint8_t* __restrict__ valid) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < N) valid[j] = (va[j] && vb[j]) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_scc_nv(const uint8_t* __restrict__ valid, long long N, int h,
                                                int* __restrict__ nv) {
    const long long a = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= N) return;
    int n = 0;
    for (long long j = max(0ll, a - h); j <= min(N - 1, a + h); ++j) n += valid[j];
    nv[a] = n;
}

// first pixel in [a, b) with bin2 >= target
__device__ __forceinline__ long long scc_lower_b2(const int64_t* __restrict__ b2, long long a, long long b,
                                                  long long target) {
    while (a < b) {
        const long long m = a + ((b - a) >> 1);
        if ((long long)b2[m] < target) a = m + 1; else b = m;
    }
    return a;
}

// The pixels (r, c) of table rows r in [tr0, tr0 + n_tr) with c in [tc0, tc0 + n_tc) and c - r >= dmin, stored at
// patch[(r - tr0) * sr + (c - tc0) * sc]; a wave per table row.
__device__ __forceinline__ void scc_fill(const PixTable<double>& X, const long long* __restrict__ rp,
                                         const uint8_t* __restrict__ valid, double* patch, long long tr0, int n_tr,
                                         long long tc0, int n_tc, long long dmin, int sr, int sc) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long long c_end = min(tc0 + n_tc, X.N);
    // lane u bisects the wave's u-th row, k = wid + u kSccWaves (n_tr <= 128: at most 8 rows), all rows at once
    long long ms = 0, me = 0;
    {
        const long long r = tr0 + wid + (long long)lane * kSccWaves;
        if (wid + lane * kSccWaves < n_tr && r >= 0 && r < X.N && valid[r]) {
            const long long c_lo = max(max(tc0, 0ll), r + dmin);
            if (c_lo < c_end) {
                me = rp[r + 1];
                ms = scc_lower_b2(X.b2, rp[r], me, X.lo + c_lo);
            }
        }
    }
    for (int u = 0, k = wid; k < n_tr; ++u, k += kSccWaves) {
        const long long s = __shfl(ms, u, 64), e = __shfl(me, u, 64);
        if (s >= e) continue;  // (wave-uniform) a skipped or empty row
        const long long r = tr0 + k;
        const long long c_lo = max(max(tc0, 0ll), r + dmin);
        // unique ascending columns: the row's pixels inside [c_lo, c_end) are among its first n_tc <= 128 from s
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const long long p = s + lane + 64 * v;
            if (p >= e) continue;
            const long long c = (long long)X.b2[p] - X.lo;
            if (c < c_lo || c >= c_end || !valid[c]) continue;
            double x = X.cnt[p];
            if (X.w) {
                x = x * X.w[r] * X.w[c];
                if (x != x) x = 0.0;
            }
            patch[k * sr + (int)(c - tc0) * sc] = x;
        }
    }
}

struct SccArgs {
    PixTable<double> A, B;
    const long long *rpa, *rpb;  // null: the table has no pixels
    const uint8_t* valid;
    const int* nv;
    long long D, g;
    int h, R, nJ;
    long long nRB;
};

__global__ __launch_bounds__(kSccThreads) void k_scc_moments(SccArgs q, double* __restrict__ P,
                                                             long long* __restrict__ Pn) {
#pragma clang fp contract(off)
    extern __shared__ double sh[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int h = q.h, R = q.R, PR = R + 2 * h, PC = R + kSccT - 1 + 2 * h;
    const long long N = q.A.N;
    double* pa = sh;
    double* pb = sh + PR * PC;
    const int J = (int)(blockIdx.x % (unsigned)q.nJ);
    const long long seg = blockIdx.x / (unsigned)q.nJ;
    const long long d0 = q.g + (long long)J * kSccT;
    const int t = lane & (kSccT - 1), sub = lane >> 5;  // the lane's stratum, and which row of the wave's two
    const long long d = d0 + t;
    long long n = 0;
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;

    for (long long rb = seg * kSccSegBlocks; rb < min(q.nRB, (seg + 1) * kSccSegBlocks); ++rb) {
        const long long a0 = rb * R;
        if (a0 + d0 >= N) break;  // no cell (a, a + d) with d >= d0 in this row block or a later one
        const long long r0 = a0 - h, c0 = a0 + d0 - h;  // the patch's first row and column
        __syncthreads();  // the last trip's reads
        for (int i = tid; i < 2 * PR * PC; i += kSccThreads) sh[i] = 0.0;
        __syncthreads();
        // 2. at and above the diagonal by row; below it (c0 < r0 + PR) by column, transposed
        if (q.rpa) scc_fill(q.A, q.rpa, q.valid, pa, r0, PR, c0, PC, q.g, PC, 1);
        if (q.rpb) scc_fill(q.B, q.rpb, q.valid, pb, r0, PR, c0, PC, q.g, PC, 1);
        if (c0 < r0 + PR) {
            const long long dl = max(q.g, 1ll);
            if (q.rpa) scc_fill(q.A, q.rpa, q.valid, pa, c0, PC, r0, PR, dl, 1, PC);
            if (q.rpb) scc_fill(q.B, q.rpb, q.valid, pb, c0, PC, r0, PR, dl, 1, PC);
        }
        __syncthreads();
        // 3. rows of both patches -> sliding sums over columns [j - h, j + h], j in [h, PC - h)
        if (h > 0) {
            double hs[kSccRowsPerWave][2];
#pragma unroll
            for (int u = 0; u < kSccRowsPerWave; ++u) {
                const int row = wid + u * kSccWaves;
#pragma unroll
                for (int v = 0; v < 2; ++v) {
                    const int j = h + lane + 64 * v;
                    double s = 0.0;
                    if (row < 2 * PR && j < PC - h) {
                        const double* src = sh + row * PC + j - h;
                        for (int k = 0; k <= 2 * h; ++k) s += src[k];
                    }
                    hs[u][v] = s;
                }
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < kSccRowsPerWave; ++u) {
                const int row = wid + u * kSccWaves;
#pragma unroll
                for (int v = 0; v < 2; ++v) {
                    const int j = h + lane + 64 * v;
                    if (row < 2 * PR && j < PC - h) sh[row * PC + j] = hs[u][v];
                }
            }
            __syncthreads();
        }
        // 4. cell (a0 + i, a0 + i + d): patch row i + h, column i + t + h
        for (int i = wid * 2 + sub; i < R; i += 2 * kSccWaves) {
            const long long a = a0 + i, b = a + d;
            if (d > q.D || b >= N || !q.valid[a] || !q.valid[b]) continue;
            const double* ca = pa + i * PC + i + t + h;
            const double* cb = pb + i * PC + i + t + h;
            double SX = 0.0, SY = 0.0;
            for (int k = 0; k <= 2 * h; ++k) {
                SX += ca[k * PC];
                SY += cb[k * PC];
            }
            if (SX == 0.0 && SY == 0.0) continue;
            const double w = (double)((long long)q.nv[a] * q.nv[b]);
            const double X = SX / w, Y = SY / w;
            ++n;
            sx += X;
            sy += Y;
            sxx += X * X;
            syy += Y * Y;
            sxy += X * Y;
        }
    }
    // the 2 kSccWaves lanes of a stratum, in (wave, half) order
    __syncthreads();
    double* red = sh;  // [6][kSccThreads]; the launch sizes the LDS for it
    red[0 * kSccThreads + tid] = sx;
    red[1 * kSccThreads + tid] = sy;
    red[2 * kSccThreads + tid] = sxx;
    red[3 * kSccThreads + tid] = syy;
    red[4 * kSccThreads + tid] = sxy;
    reinterpret_cast<long long*>(red)[5 * kSccThreads + tid] = n;
    __syncthreads();
    if (tid < 6 * kSccT) {
        const int k = tid / kSccT, tt = tid % kSccT;
        const long long out = ((long long)blockIdx.x) * kSccT + tt;  // (seg * nJ + J) * T + t
        if (k < 5) {
            double s = 0.0;
            for (int u = 0; u < 2 * kSccWaves; ++u) s += red[k * kSccThreads + u * kSccT + tt];
            P[out * 5 + k] = s;
        } else {
            long long s = 0;
            for (int u = 0; u < 2 * kSccWaves; ++u)
                s += reinterpret_cast<const long long*>(red)[5 * kSccThreads + u * kSccT + tt];
            Pn[out] = s;
        }
    }
}

__global__ __launch_bounds__(256) void k_scc_sum(const double* __restrict__ P, const long long* __restrict__ Pn,
                                                 long long n_seg, int nJ, long long D, long long g,
                                                 long long* __restrict__ n, double* __restrict__ S) {
    const long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > D) return;
    long long cn = 0;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (d >= g && P) {
        const long long stride = (long long)nJ * kSccT;
        for (long long c = 0; c < n_seg; ++c) {
            const long long at = c * stride + (d - g);
            cn += Pn[at];
#pragma unroll
            for (int k = 0; k < 5; ++k) s[k] += P[at * 5 + k];
        }
    }
    n[d] = cn;
#pragma unroll
    for (int k = 0; k < 5; ++k) S[k * (D + 1) + d] = s[k];
}

}  // namespace hh

using namespace hh;

extern "C" int hh_scc_pixels(const int64_t* bin1_a, const int64_t* bin2_a, const double* count_a, int64_t nnz_a,
                             const double* weight_a, int64_t n_weight_a, int64_t lo_a, const uint8_t* bad_a,
                             const int64_t* bin1_b, const int64_t* bin2_b, const double* count_b, int64_t nnz_b,
                             const double* weight_b, int64_t n_weight_b, int64_t lo_b, const uint8_t* bad_b,
                             int64_t N, int32_t h, int32_t ignore_diags, int64_t max_dist, int64_t* n, double* S,
                             int32_t on_device, void* stream) {
    return guard([&] {
        HH_REQUIRE(N >= 1 && N <= kSccMaxN, "N outside [1, 2^24]");
        HH_REQUIRE(h >= 0 && h <= HH_SCC_MAX_H, "h outside 0..HH_SCC_MAX_H");
        HH_REQUIRE(ignore_diags >= 0, "ignore_diags must be >= 0");
        HH_REQUIRE(max_dist >= 0 && max_dist <= N - 1, "max_dist outside [0, N - 1]");
        check_pixel_table(bin1_a, bin2_a, count_a, nnz_a, weight_a, n_weight_a, lo_a, N);
        check_pixel_table(bin1_b, bin2_b, count_b, nnz_b, weight_b, n_weight_b, lo_b, N);
        HH_REQUIRE(n && S, "null outputs");
        const long long D = max_dist, g = ignore_diags;
        const int R = scc_rows_of(h);
        const int PR = R + 2 * h, PC = R + kSccT - 1 + 2 * h;
        const bool work = (nnz_a > 0 || nnz_b > 0) && g <= D;
        const long long nJ = work ? (D - g) / kSccT + 1 : 0;
        const long long nRB = (N + R - 1) / R, n_seg = (nRB + kSccSegBlocks - 1) / kSccSegBlocks;
        HH_REQUIRE(n_seg * nJ < (int64_t(1) << 24), "chromosome too large for the stratum moments");
        const size_t lds = std::max(sizeof(double) * 2 * PR * PC, sizeof(double) * 6 * kSccThreads);
        HH_REQUIRE(PR <= kSccMaxPR && PC <= 128 && lds <= 160 * 1024, "scc_rows does not fit h");
        hipStream_t s = as_stream(stream);
        PixStage<double> SA, SB;
        DBuf<uint8_t> valid(N);
        DBuf<int> nv(N);
        DBuf<double> dS, P;
        DBuf<long long> dn, Pn;
        SyncOnExit sync{s};  // (destroyed before the buffers above)
        SA.init(bin1_a, bin2_a, count_a, nnz_a, weight_a, lo_a, N, bad_a, kPixValid | kPixRows, on_device, s);
        SB.init(bin1_b, bin2_b, count_b, nnz_b, weight_b, lo_b, N, bad_b, kPixValid | kPixRows, on_device, s);
        double* pS = S;
        long long* pn = (long long*)n;
        if (!on_device) {
            dS.alloc(5 * (D + 1)); pS = dS.p;
            dn.alloc(D + 1); pn = dn.p;
        }
        if (work) {
            hipLaunchKernelGGL(k_scc_valid, dim3(grid_of(N)), dim3(256), 0, s, SA.valid.p, SB.valid.p, (long long)N,
                               valid.p);
            hipLaunchKernelGGL(k_scc_nv, dim3(grid_of(N)), dim3(256), 0, s, valid.p, (long long)N, (int)h, nv.p);
            P.alloc((size_t)(n_seg * nJ * kSccT * 5));
            Pn.alloc((size_t)(n_seg * nJ * kSccT));
            SccArgs q{SA.X, SB.X, nnz_a > 0 ? SA.rp.p : nullptr, nnz_b > 0 ? SB.rp.p : nullptr, valid.p, nv.p, D, g,
                      (int)h, R, (int)nJ, nRB};
            HIP_CHECK(hipFuncSetAttribute((const void*)k_scc_moments, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)lds));
            HH_KTIME("k_scc_moments", s);
            hipLaunchKernelGGL(k_scc_moments, dim3((unsigned)(n_seg * nJ)), dim3(kSccThreads), lds, s, q, P.p, Pn.p);
        }
        {
            HH_KTIME("k_scc_sum", s);
            hipLaunchKernelGGL(k_scc_sum, dim3(grid_of(D + 1)), dim3(256), 0, s, P.p, Pn.p, n_seg, (int)nJ, D, g, pn,
                               pS);
        }
        HIP_CHECK(hipGetLastError());
        if (!on_device) {
            dS.download(S, 5 * (D + 1), s);
            dn.download((long long*)n, D + 1, s);
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}
