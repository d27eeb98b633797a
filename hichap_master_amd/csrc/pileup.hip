// Pileups (aggregate peak analysis) on cooler's own pixel table (DESIGN.md
// §4n; HiCHap has none: the definition is this project's), and below them the
// rescaled domain pileups (§4u).
//
// One chromosome is global bins [lo, lo + N) of a table sorted by (bin1,
// bin2); the value of a cell is v = count * w[a] * w[b] in that order (NaN ->
// 0), the raw count without weights, and valid[a] = 0 where a weight is not
// finite or bad[a] is set: hh_expected_pixels' conventions, and its helpers
// (pixel_table.hpp).  Feature k has the local centre (row[k], col[k]), row
// <= col; with flank f, W = 2 f + 1, window cell (u, v) of feature k is the
// cell i = row[k] - f + u, j = col[k] - f + v of the symmetric matrix, a =
// min(i, j), b = max(i, j), d = b - a.  The cell is eligible when i and j are
// inside the chromosome and valid, d >= min_dist and, with an expected,
// d < n_expected and expected[d] is finite and > 0.
//   Cn[u][v]  the features whose cell (u, v) is eligible, stored or not;
//   S[u][v]   the sum of v(a, b), with an expected of v(a, b) / expected[d]
//             (one IEEE division), over the features whose cell is eligible
//             and a stored pixel: chunks of C consecutive features (C =
//             hh_tune "pileup_chunk", HH_PILEUP_CHUNK by default) are summed
//             in ascending k from +0.0, then the chunk sums in ascending chunk
//             order from +0.0.
// No N x N matrix and no M x W x W stack is made.
//
//   k_pu_check   flags a feature with row > col or an end outside [0, N) (the
//                device form; the host form checks its host arrays).
//   k_pu_count   Cn from valid and expected alone: a thread owns a cell, a
//                block kPuCntFeats features; 64-bit integer atomics (integer
//                adds commute).
//   k_pu_sum     one block per (chunk of C features, tile of 16 window rows);
//                a wave owns 4 window rows of the tile in LDS for the whole
//                kernel and takes the features in ascending k, so a cell gets
//                its terms in ascending k with no atomics and no barriers.
//                Per feature, the four rows at once (independent loads next
//                to each other):
//                * the upper cells of window row i are the columns [max(col -
//                  f, i), col + f]: one contiguous run of table row i.  Its
//                  first pixel is found in [rp[i], rp[i + 1]) by a wave-wide
//                  64-ary search (a ballot per round: two rounds serve a row
//                  of 4096 pixels); the <= W pixels of the run are then read
//                  lane-parallel and added into the cell of their column;
//                * the mirrored cells (j < i, only where col - row <= 2 f)
//                  are table cells (j, i): lane l owns columns l and l + 64
//                  and bisects table row j once per feature, for the first of
//                  the wave's four rows (columns of a row are unique and >= j,
//                  so column i lies within the first i - j + 1 pixels: at most
//                  7 rounds); the four consecutive columns i are among the
//                  four pixels from there on.
//                The first search round of the next feature and the row
//                pointers of the one after it are loaded before the current
//                feature is walked.  The chunk's tile goes to P.
//   k_pu_reduce  S[cell] = the chunks' partials in ascending chunk order.
//
// Every fp64 sum has an order fixed by the features and C alone (not by the
// grid or the timing): two calls and the host / device forms give the same
// bits.  The products and the division are single IEEE operations, never
// contracted into the additions (pu_term).
// Range checks: the features are checked before the walk; a window row or
// column is compared against [0, N) before it indexes valid, w or rp; rp comes
// from bisections bounded by [0, nnz] and a range with end < start is empty; a
// pixel's local column is compared against the window's column range before
// it indexes valid, w or an LDS cell, and a distance against n_expected.  An
// unsorted or duplicated table gives wrong sums (two lanes may then meet on
// an LDS cell), never an access outside the arrays.
#include "pixel_table.hpp"

namespace hh {

constexpr int kPuRows = 16;        // window rows per k_pu_sum block
constexpr int kPuWaveRows = 4;     // of which a wave owns 4
constexpr int kPuStride = 128;     // LDS columns per row (W <= 127)
constexpr int kPuMaxFlank = 63;
constexpr int kPuCntFeats = 64;    // features per k_pu_count block

struct PuArgs {
    const int32_t *row, *col;
    long long M;
    int f, C;
    const double* expected;  // or null
    long long n_exp, min_dist;
};

// d >= min_dist and the expected of the diagonal usable (e = expected[d], 1 without an expected)
__device__ __forceinline__ bool pu_dist_ok(long long d, const PuArgs& A, double& e) {
    e = 1.0;
    if (d < A.min_dist) return false;
    if (!A.expected) return true;
    if (d >= A.n_exp) return false;
    e = A.expected[d];
    return e - e == 0.0 && e > 0.0;
}

// count * w[a] * w[b] (NaN -> 0), over e with an expected: single IEEE operations
__device__ __forceinline__ double pu_term(double c, const double* __restrict__ w, long long a, long long b, bool over,
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

__global__ __launch_bounds__(256) void k_pu_check(const int32_t* __restrict__ row, const int32_t* __restrict__ col,
                                                  long long M, long long N, unsigned int* __restrict__ err) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= M) return;
    const long long r = row[k], c = col[k];
    if (r < 0 || r > c || c >= N) atomicOr(err, 1u);
}

__global__ __launch_bounds__(256) void k_pu_count(const uint8_t* __restrict__ valid, long long N, PuArgs A,
                                                  unsigned long long* __restrict__ Cn) {
    const int W = 2 * A.f + 1;
    const int cell = blockIdx.y * 256 + threadIdx.x;
    if (cell >= W * W) return;
    const int u = cell / W, v = cell - u * W;
    const long long k0 = (long long)blockIdx.x * kPuCntFeats, k1 = min(k0 + kPuCntFeats, A.M);
    unsigned int n = 0;
    for (long long k = k0; k < k1; ++k) {
        const long long i = (long long)A.row[k] - A.f + u, j = (long long)A.col[k] - A.f + v;
        if ((unsigned long long)i < (unsigned long long)N && (unsigned long long)j < (unsigned long long)N) {
            double e;
            if (valid[i] && valid[j] && pu_dist_ok(i < j ? j - i : i - j, A, e)) ++n;
        }
    }
    if (n) atomicAdd(&Cn[cell], (unsigned long long)n);
}

struct PuHead {  // the wave's four window rows of one feature (wave-uniform)
    int rowk, colk;
    bool in[kPuWaveRows];   // the row is inside the window and the chromosome, and valid
    bool run[kPuWaveRows];  // and has upper cells
    long long r0[kPuWaveRows], r1[kPuWaveRows];
    long long stp[kPuWaveRows], bv[kPuWaveRows];  // the first round of the run search (per lane): piece length, probe
};

__global__ __launch_bounds__(256) void k_pu_sum(PixTable<double> X, const uint8_t* __restrict__ valid,
                                                const long long* __restrict__ rp, PuArgs A, double* __restrict__ P) {
    __shared__ double acc[kPuRows][kPuStride];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int f = A.f, W = 2 * f + 1;
    const int u0 = blockIdx.y * kPuRows + wid * kPuWaveRows;  // the wave's first window row
    if (u0 >= W) return;                                      // (no block barrier below)
    const long long k0 = (long long)blockIdx.x * A.C;
    const int nk = (int)min((long long)A.C, A.M - k0);
    const bool over = A.expected != nullptr;
#pragma unroll
    for (int r = 0; r < kPuWaveRows; ++r) {
        acc[wid * kPuWaveRows + r][lane] = 0.0;
        acc[wid * kPuWaveRows + r][lane + 64] = 0.0;
    }
    int fr = 0, fc = 0;  // lane l holds feature k0 + l (C <= 64)
    if (lane < nk) { fr = A.row[k0 + lane]; fc = A.col[k0 + lane]; }

    auto head = [&](int kk) {
        PuHead h;
        const bool live = kk < nk;
        h.rowk = __builtin_amdgcn_readlane(fr, live ? kk : 0);
        h.colk = __builtin_amdgcn_readlane(fc, live ? kk : 0);
#pragma unroll
        for (int r = 0; r < kPuWaveRows; ++r) {
            const long long i = (long long)h.rowk - f + u0 + r;
            h.in[r] = live && u0 + r < W && i >= 0 && i < X.N && valid[i];
            h.run[r] = h.in[r] && max((long long)h.colk - f, i) <= min((long long)h.colk + f, X.N - 1);
            h.r0[r] = h.r1[r] = 0;
            if (h.run[r]) { h.r0[r] = rp[i]; h.r1[r] = rp[i + 1]; }
        }
        return h;
    };

    // wave-wide 64-ary lower bound of a column in bin2[lo_, hi_): lane l probes the last pixel of piece l
    auto probe = [&](long long lo_, long long hi_, long long& stp) -> long long {
        const long long n = hi_ - lo_;
        stp = (n + 63) >> 6;
        const long long q = lo_ + (lane + 1) * stp - 1;
        return (n > 0 && q < hi_) ? (long long)X.b2[q] : 0x7fffffffffffffffll;
    };
    auto first_probes = [&](PuHead& h) {
#pragma unroll
        for (int r = 0; r < kPuWaveRows; ++r)
            h.bv[r] = probe(h.r0[r], h.run[r] ? max(h.r0[r], h.r1[r]) : h.r0[r], h.stp[r]);
    };

    PuHead cur = head(0);
    first_probes(cur);
    PuHead nxt = head(1);
    for (int kk = 0; kk < nk; ++kk) {
        const PuHead h = cur;
        // the next feature's first probes and the row pointers of the one after it are in flight
        // while this one is walked
        first_probes(nxt);
        cur = nxt;
        nxt = head(kk + 2);
        const long long i0 = (long long)h.rowk - f + u0, jmin = (long long)h.colk - f;
        const long long jmax = min((long long)h.colk + f, X.N - 1);

        // ---- upper cells: the run [max(col - f, i), col + f] of table row i, the four rows at once
        long long lo_[kPuWaveRows], hi_[kPuWaveRows], tgt[kPuWaveRows];
#pragma unroll
        for (int r = 0; r < kPuWaveRows; ++r) {
            lo_[r] = h.r0[r];
            hi_[r] = h.run[r] ? max(h.r0[r], h.r1[r]) : h.r0[r];
            tgt[r] = X.lo + max(jmin, i0 + r);
        }
        long long bv[kPuWaveRows], stp[kPuWaveRows];
#pragma unroll
        for (int r = 0; r < kPuWaveRows; ++r) { bv[r] = h.bv[r]; stp[r] = h.stp[r]; }  // the first round came with h
        for (;;) {
            bool any = false;
#pragma unroll
            for (int r = 0; r < kPuWaveRows; ++r) {
                if (hi_[r] - lo_[r] > 0) {
                    const int c = __popcll(__ballot(bv[r] < tgt[r]));  // the pieces that end below the target
                    lo_[r] += c * stp[r];
                    hi_[r] = min(hi_[r], lo_[r] + stp[r] - 1);
                }
            }
#pragma unroll
            for (int r = 0; r < kPuWaveRows; ++r) {
                bv[r] = probe(lo_[r], hi_[r], stp[r]);
                any |= hi_[r] - lo_[r] > 0;
            }
            if (!any) break;
        }
        long long pb[kPuWaveRows][2];
        double pc[kPuWaveRows][2];
#pragma unroll
        for (int r = 0; r < kPuWaveRows; ++r) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const long long p = lo_[r] + lane + 64 * t;
                const bool ok = h.run[r] && p < h.r1[r];
                pb[r][t] = ok ? (long long)X.b2[p] : -1;
                pc[r][t] = ok ? X.cnt[p] : 0.0;
            }
        }

        // ---- mirrored cells (j < i): table cells (j, i); lane l owns window columns l and l + 64
        const bool mirror = jmin < i0 + kPuWaveRows - 1;  // wave-uniform
        bool act[2] = {false, false};
        long long mj[2] = {0, 0};
        long long cb[2][kPuWaveRows];
        double cc[2][kPuWaveRows];
        if (mirror) {
            long long mlo[2], mhi[2], mend[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int v = lane + 64 * t;
                mj[t] = jmin + v;
                act[t] = v < W && mj[t] >= 0 && mj[t] < X.N && mj[t] < i0 + kPuWaveRows - 1;
                if (act[t]) act[t] = valid[mj[t]] != 0;
                mlo[t] = mend[t] = 0;
                if (act[t]) { mlo[t] = rp[mj[t]]; mend[t] = rp[mj[t] + 1]; }
                // columns of row j are unique and >= j: column i0 lies at most i0 - j pixels into the row
                mhi[t] = max(mlo[t], min(mend[t], mlo[t] + max(i0 - mj[t], 0ll) + 1));
            }
            const long long t0 = X.lo + i0;  // lower bound of the first row's column; the others follow it
            while (mlo[0] < mhi[0] || mlo[1] < mhi[1]) {
                long long mid[2], bv[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    mid[t] = mlo[t] + ((mhi[t] - mlo[t]) >> 1);
                    bv[t] = mlo[t] < mhi[t] ? (long long)X.b2[mid[t]] : 0;
                }
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    if (mlo[t] < mhi[t]) {
                        if (bv[t] < t0) mlo[t] = mid[t] + 1; else mhi[t] = mid[t];
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int q = 0; q < kPuWaveRows; ++q) {
                    const long long p = mlo[t] + q;
                    const bool ok = act[t] && p < mend[t];
                    cb[t][q] = ok ? (long long)X.b2[p] : -1;
                    cc[t][q] = ok ? X.cnt[p] : 0.0;
                }
            }
        }

        // ---- the adds: every cell of the wave's rows gets at most one term per feature
#pragma unroll
        for (int r = 0; r < kPuWaveRows; ++r) {
            const long long i = i0 + r;
            const long long jlo = max(jmin, i);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const long long bl = pb[r][t] - X.lo;
                if (h.run[r] && pb[r][t] >= 0 && bl >= jlo && bl <= jmax) {
                    double e;
                    if (valid[bl] && pu_dist_ok(bl - i, A, e))
                        acc[wid * kPuWaveRows + r][bl - jmin] += pu_term(pc[r][t], X.w, i, bl, over, e);
                }
            }
            if (mirror && h.in[r]) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    double e;
                    if (act[t] && mj[t] < i && pu_dist_ok(i - mj[t], A, e)) {
                        bool hit = false;
                        double c = 0.0;
#pragma unroll
                        for (int q = 0; q < kPuWaveRows; ++q)
                            if (cb[t][q] == X.lo + i) { hit = true; c = cc[t][q]; }
                        if (hit) acc[wid * kPuWaveRows + r][lane + 64 * t] += pu_term(c, X.w, mj[t], i, over, e);
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();  // the next feature's adds follow this one's
    }
    const long long base = (long long)blockIdx.x * W * W;
#pragma unroll
    for (int r = 0; r < kPuWaveRows; ++r) {
        if (u0 + r >= W) break;
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (lane + 64 * t < W) P[base + (long long)(u0 + r) * W + lane + 64 * t] = acc[wid * kPuWaveRows + r][lane + 64 * t];
    }
}

__global__ __launch_bounds__(256) void k_pu_reduce(const double* __restrict__ P, long long n_chunks, int WW,
                                                   double* __restrict__ S) {
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= WW) return;
    double s = 0.0;
#pragma unroll 8
    for (long long c = 0; c < n_chunks; ++c) s += P[c * WW + cell];  // (eight loads in flight; the adds in chunk order)
    S[cell] = s;
}


// ---------------------------------------------------------------- domain pileups
// Feature k is the half-open interval [start[k], end[k]) of local bins, L = end - start; the output grid has R
// cells across the body and P cells of flank on each side, G = R + 2 P <= 127.  All geometry is 64-bit integer
// in units of 1/R bin: output index u covers [start R + (u - P) L, + L), bin i covers [i R, (i + 1) R), o(u, i) is
// the length of their intersection.  Upper form: output cell (u, v), u <= v, takes the matrix cells a <= b with
// the integer weight c = o(u, a) o(v, b), doubled where a != b and u == v; eligibility is §4n's.
//   A_k(u, v)  the int64 sum of c over the eligible cells, stored or not;
//   T_k(u, v)  the sum of t * (double(c) / double(L L)) over the eligible stored cells, from +0.0 in ascending
//              (a, b): the order of the table;
//   S = sum_k T_k, Wn = sum_k double(A_k) / double(L_k L_k): both in §4n's order across features (chunks of C
//   in ascending k from +0.0, the chunk sums in ascending chunk order from +0.0), then mirrored.
//
//   k_dp_check   flags a feature with start < 0, end > N or start >= end.
//   k_dp_okd     ok[d] = the distance d is usable (min_dist, expected): the weight pass reads bytes.
//   k_dp_weight  a wave owns output row u of a chunk, lane l the cells (u, u + l) and (u, u + l + 64) in
//                registers; per feature the integer double loop over the bins of the cell.  No pixels.
//   k_dp_sum     the same ownership; per feature and matrix row a of output row u (ascending), a lane bisects
//                table row a for the first bin of its output column (columns of a row are unique and >= a, so
//                at most b - a pixels lie before column b: one probe there settles a row without gaps) and
//                walks the pixels of the column's bins in ascending b.  A cell has one owner and one order: no atomics, no LDS, no barriers.
//   k_dp_reduce  cell (u, v) of S and Wn = the chunks' partials of cell (min, max) in ascending chunk order.
// Range checks: a matrix row is clamped to [0, N) before it indexes valid or rp; a pixel index stays inside
// [rp[a], rp[a + 1]) and [0, nnz); a pixel's local column is compared against the column's bin range (inside
// [a, N)) before it indexes valid, w or ok; a distance against n_expected.
constexpr int kDpMaxG = 127;
constexpr int kDpWaves = 4;  // output rows per block of k_dp_weight / k_dp_sum

struct DpArgs {
    const int32_t *start, *end;
    long long M;
    int R, P, C;
};

// floor(x / R), R in 1..127, |x| < 2^52: the double quotient, then an exact integer correction
__device__ __forceinline__ long long dp_floor_div(long long x, int R) {
    long long q = (long long)floor((double)x / (double)R);
    if (q * R > x) --q;
    if ((q + 1) * R <= x) ++q;
    return q;
}

// the intersection of [x0, x0 + L) with bin i, in 1/R bin
__device__ __forceinline__ long long dp_overlap(long long x0, long long L, long long i, int R) {
    const long long a = max(x0, i * R), b = min(x0 + L, (i + 1) * R);
    return b > a ? b - a : 0;
}

__global__ __launch_bounds__(256) void k_dp_check(const int32_t* __restrict__ start, const int32_t* __restrict__ end,
                                                  long long M, long long N, unsigned int* __restrict__ err) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= M) return;
    const long long s = start[k], e = end[k];
    if (s < 0 || e > N || s >= e) atomicOr(err, 1u);
}

__global__ __launch_bounds__(256) void k_dp_okd(long long N, PuArgs A, uint8_t* __restrict__ ok) {
    const long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= N) return;
    double e;
    ok[d] = pu_dist_ok(d, A, e) ? 1 : 0;
}

__global__ __launch_bounds__(64 * kDpWaves) void k_dp_weight(const uint8_t* __restrict__ valid,
                                                             const uint8_t* __restrict__ ok, long long N, DpArgs D,
                                                             double* __restrict__ Pw) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int G = D.R + 2 * D.P, R = D.R;
    const int u = blockIdx.y * kDpWaves + wid;
    if (u >= G) return;
    const long long k0 = (long long)blockIdx.x * D.C;
    const int nk = (int)min((long long)D.C, D.M - k0);
    int fs = 0, fe = 1;  // lane l holds feature k0 + l (C <= 64)
    if (lane < nk) { fs = D.start[k0 + lane]; fe = D.end[k0 + lane]; }
    double acc[2] = {0.0, 0.0};
    for (int kk = 0; kk < nk; ++kk) {
        const long long s = __builtin_amdgcn_readlane(fs, kk), L = (long long)__builtin_amdgcn_readlane(fe, kk) - s;
        const long long x0 = s * R + (long long)(u - D.P) * L;
        const long long a0 = max(dp_floor_div(x0, R), 0ll), a1 = min(dp_floor_div(x0 + L - 1, R), N - 1);
        const double LL = (double)(L * L);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int v = u + lane + 64 * t;
            if (v >= G) continue;
            const long long y0 = s * R + (long long)(v - D.P) * L;
            const long long b0 = max(dp_floor_div(y0, R), 0ll), b1 = min(dp_floor_div(y0 + L - 1, R), N - 1);
            long long Ak = 0;
            for (long long a = a0; a <= a1; ++a) {
                if (!valid[a]) continue;
                const long long oa = dp_overlap(x0, L, a, R);
                long long row = 0;
                for (long long b = max(b0, a); b <= b1; ++b) {
                    if (!valid[b] || !ok[b - a]) continue;
                    const long long c = dp_overlap(y0, L, b, R);
                    row += (v == u && b != a) ? 2 * c : c;
                }
                Ak += oa * row;
            }
            acc[t] += (double)Ak / LL;
        }
    }
    const long long base = (long long)blockIdx.x * G * G + (long long)u * G;
#pragma unroll
    for (int t = 0; t < 2; ++t)
        if (u + lane + 64 * t < G) Pw[base + u + lane + 64 * t] = acc[t];
}

__global__ __launch_bounds__(64 * kDpWaves) void k_dp_sum(PixTable<double> X, const uint8_t* __restrict__ valid,
                                                          const long long* __restrict__ rp, PuArgs A, DpArgs D,
                                                          double* __restrict__ Ps) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int G = D.R + 2 * D.P, R = D.R;
    const int u = blockIdx.y * kDpWaves + wid;
    if (u >= G) return;
    const long long k0 = (long long)blockIdx.x * D.C;
    const int nk = (int)min((long long)D.C, D.M - k0);
    const bool over = A.expected != nullptr;
    int fs = 0, fe = 1;
    if (lane < nk) { fs = D.start[k0 + lane]; fe = D.end[k0 + lane]; }
    double acc[2] = {0.0, 0.0};
    for (int kk = 0; kk < nk; ++kk) {
        const long long s = __builtin_amdgcn_readlane(fs, kk), L = (long long)__builtin_amdgcn_readlane(fe, kk) - s;
        const long long x0 = s * R + (long long)(u - D.P) * L;
        const long long a0 = max(dp_floor_div(x0, R), 0ll), a1 = min(dp_floor_div(x0 + L - 1, R), X.N - 1);
        const double LL = (double)(L * L);
        long long y0[2], b0[2], b1[2];
        double T[2] = {0.0, 0.0};
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int v = u + lane + 64 * t;
            y0[t] = s * R + (long long)(v - D.P) * L;
            b0[t] = max(dp_floor_div(y0[t], R), 0ll);
            b1[t] = v < G ? min(dp_floor_div(y0[t] + L - 1, R), X.N - 1) : -1;  // (empty beyond the grid)
        }
        for (long long a = a0; a <= a1; ++a) {  // wave-uniform
            if (!valid[a]) continue;
            const long long r0 = min(max(rp[a], 0ll), X.nnz), r1 = min(max(rp[a + 1], r0), X.nnz);
            if (r1 <= r0) continue;
            const long long oa = dp_overlap(x0, L, a, R);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const long long bl = max(b0[t], a), bh = b1[t];
                if (bh < bl) continue;
                // lower bound of column bl: at most bl - a pixels lie before it; in a row without gaps up to
                // bl exactly that many, which one probe confirms, otherwise a bisection of that range
                long long p = r0, q = min(r1, r0 + (bl - a));
                const long long tgt = X.lo + bl;
                if (q < r1 && (long long)X.b2[q] == tgt) p = q;
                while (p < q) {
                    const long long m = p + ((q - p) >> 1);
                    if ((long long)X.b2[m] < tgt) p = m + 1; else q = m;
                }
                long long nb = p < r1 ? (long long)X.b2[p] - X.lo : bh + 1;
                while (nb <= bh) {  // (p < r1 here)
                    const long long b = nb;
                    const double cv = X.cnt[p];
                    ++p;
                    nb = p < r1 ? (long long)X.b2[p] - X.lo : bh + 1;  // the next column is in flight
                    double e;
                    if (b >= bl && valid[b] && pu_dist_ok(b - a, A, e)) {  // (b < bl: only in an unsorted table)
                        long long c = oa * dp_overlap(y0[t], L, b, R);
                        if (t == 0 && lane == 0 && b != a) c *= 2;  // v == u: the mirrored cell lands here too
                        const double phi = (double)c / LL;
                        T[t] += pu_term(cv, X.w, a, b, over, e) * phi;
                    }
                }
            }
        }
        acc[0] += T[0];
        acc[1] += T[1];
    }
    const long long base = (long long)blockIdx.x * G * G + (long long)u * G;
#pragma unroll
    for (int t = 0; t < 2; ++t)
        if (u + lane + 64 * t < G) Ps[base + u + lane + 64 * t] = acc[t];
}

// blockIdx.y = 0: S from Ps, 1: Wn from Pw; a null P gives zeros
__global__ __launch_bounds__(256) void k_dp_reduce(const double* __restrict__ Ps, const double* __restrict__ Pw,
                                                   long long n_chunks, int G, double* __restrict__ S,
                                                   double* __restrict__ Wn) {
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= G * G) return;
    const double* __restrict__ P = blockIdx.y ? Pw : Ps;
    const int u = cell / G, v = cell - u * G;
    const int src = min(u, v) * G + max(u, v);
    double s = 0.0;
    if (P) {
#pragma unroll 8
        for (long long c = 0; c < n_chunks; ++c) s += P[c * G * G + src];
    }
    (blockIdx.y ? Wn : S)[cell] = s;
}

}  // namespace hh

using namespace hh;

extern "C" int hh_pileup_pixels(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                                const double* weight, int64_t n_weight, int64_t lo, int64_t N, const uint8_t* bad,
                                const int32_t* row, const int32_t* col, int64_t M, int32_t flank,
                                const double* expected, int64_t n_expected, int64_t min_dist, double* S, int64_t* Cn,
                                int32_t on_device, void* stream) {
    return guard([&] {
        HH_REQUIRE(N >= 1 && N <= (int64_t(1) << 24), "N outside [1, 2^24]");  // the work-item counts
        check_pixel_table(bin1, bin2, count, nnz, weight, n_weight, lo, N);
        HH_REQUIRE(S && Cn, "null outputs");
        HH_REQUIRE(M >= 0 && M < (int64_t(1) << 31) && (M == 0 || (row && col)), "bad feature arrays");
        HH_REQUIRE(flank >= 0 && flank <= kPuMaxFlank, "flank outside 0..63");
        HH_REQUIRE(min_dist >= 0, "min_dist must be >= 0");
        HH_REQUIRE(!expected || (n_expected >= 1 && n_expected <= N), "n_expected outside [1, N]");
        const int W = 2 * flank + 1, WW = W * W;
        const int C = g_pileup_chunk;
        const long long n_chunks = (M + C - 1) / C;
        hipStream_t s = as_stream(stream);
        PixStage<double> St;
        DBuf<int32_t> drow, dcol;
        DBuf<double> dexp, dS(WW), P;
        DBuf<unsigned long long> dCn(WW);
        DBuf<unsigned int> derr;
        SyncOnExit sync{s};  // (destroyed before the buffers above)
        PuArgs A{row, col, (long long)M, flank, C, expected, expected ? (long long)n_expected : 0, (long long)min_dist};
        if (on_device) {  // the features' range check, before the walk
            if (M > 0) {
                derr.alloc(1);
                derr.zero(s);
                hipLaunchKernelGGL(k_pu_check, dim3(grid_of(M)), dim3(256), 0, s, row, col, (long long)M, (long long)N,
                                   derr.p);
                HIP_CHECK(hipGetLastError());
                unsigned int herr = 0;
                PinnedDown down;
                down.add(derr.p, &herr, 1);
                down.run(s);
                HH_REQUIRE(!herr, "a feature has row > col or an end outside [0, N)");
            }
        } else {
            for (int64_t k = 0; k < M; ++k)
                HH_REQUIRE(row[k] >= 0 && row[k] <= col[k] && col[k] < N,
                           "a feature has row > col or an end outside [0, N)");
            if (M > 0) {
                drow.alloc(M); drow.upload(row, M, s); A.row = drow.p;
                dcol.alloc(M); dcol.upload(col, M, s); A.col = dcol.p;
            }
            if (expected) { dexp.alloc(n_expected); dexp.upload(expected, n_expected, s); A.expected = dexp.p; }
        }
        const bool walk = M > 0 && nnz > 0;
        St.init(bin1, bin2, count, nnz, weight, lo, N, bad, kPixValid | (walk ? kPixRows : 0), on_device, s);
        dCn.zero(s);
        if (M > 0) {
            HH_KTIME("k_pu_count", s);
            hipLaunchKernelGGL(k_pu_count, dim3((unsigned)((M + kPuCntFeats - 1) / kPuCntFeats), (unsigned)((WW + 255) / 256)),
                               dim3(256), 0, s, St.valid.p, (long long)N, A, dCn.p);
        }
        if (walk) {
            P.alloc((size_t)n_chunks * WW);
            {
                HH_KTIME("k_pu_sum", s);
                hipLaunchKernelGGL(k_pu_sum, dim3((unsigned)n_chunks, (unsigned)((W + kPuRows - 1) / kPuRows)), dim3(256),
                                   0, s, St.X, St.valid.p, St.rp.p, A, P.p);
            }
            {
                HH_KTIME("k_pu_reduce", s);
                hipLaunchKernelGGL(k_pu_reduce, dim3(grid_of(WW)), dim3(256), 0, s, P.p, n_chunks, WW, dS.p);
            }
        } else {
            dS.zero(s);
        }
        HIP_CHECK(hipGetLastError());
        if (on_device) {
            HIP_CHECK(hipMemcpyAsync(S, dS.p, (size_t)WW * sizeof(double), hipMemcpyDeviceToDevice, s));
            HIP_CHECK(hipMemcpyAsync(Cn, dCn.p, (size_t)WW * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        } else {
            dS.download(S, WW, s);
            dCn.download((unsigned long long*)Cn, WW, s);
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

extern "C" int hh_domain_pileup_pixels(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                                       const double* weight, int64_t n_weight, int64_t lo, int64_t N,
                                       const uint8_t* bad, const int32_t* start, const int32_t* end, int64_t M,
                                       int32_t R, int32_t P, const double* expected, int64_t n_expected,
                                       int64_t min_dist, double* S, double* Wn, int32_t on_device, void* stream) {
    return guard([&] {
        HH_REQUIRE(N >= 1 && N <= (int64_t(1) << 24), "N outside [1, 2^24]");
        check_pixel_table(bin1, bin2, count, nnz, weight, n_weight, lo, N);
        HH_REQUIRE(S && Wn, "null outputs");
        HH_REQUIRE(M >= 0 && M < (int64_t(1) << 31) && (M == 0 || (start && end)), "bad feature arrays");
        HH_REQUIRE(R >= 1 && P >= 0 && (int64_t)R + 2 * (int64_t)P <= kDpMaxG, "grid: body >= 1, pad >= 0, body + 2 pad <= 127");
        HH_REQUIRE(min_dist >= 0, "min_dist must be >= 0");
        HH_REQUIRE(!expected || (n_expected >= 1 && n_expected <= N), "n_expected outside [1, N]");
        const int G = R + 2 * P, GG = G * G;
        const int C = g_pileup_chunk;
        const long long n_chunks = (M + C - 1) / C;
        hipStream_t s = as_stream(stream);
        PixStage<double> St;
        DBuf<int32_t> dstart, dend;
        DBuf<double> dexp, dS(GG), dW(GG), Ps, Pw;
        DBuf<uint8_t> dok;
        DBuf<unsigned int> derr;
        SyncOnExit sync{s};  // (destroyed before the buffers above)
        PuArgs A{nullptr, nullptr, (long long)M, 0, C, expected, expected ? (long long)n_expected : 0, (long long)min_dist};
        DpArgs D{start, end, (long long)M, R, P, C};
        const char* bad_feature = "a feature has start < 0, end > N or start >= end";
        if (on_device) {  // the features' range check, before the walk
            if (M > 0) {
                derr.alloc(1);
                derr.zero(s);
                hipLaunchKernelGGL(k_dp_check, dim3(grid_of(M)), dim3(256), 0, s, start, end, (long long)M, (long long)N,
                                   derr.p);
                HIP_CHECK(hipGetLastError());
                unsigned int herr = 0;
                PinnedDown down;
                down.add(derr.p, &herr, 1);
                down.run(s);
                HH_REQUIRE(!herr, bad_feature);
            }
        } else {
            for (int64_t k = 0; k < M; ++k) HH_REQUIRE(start[k] >= 0 && end[k] <= N && start[k] < end[k], bad_feature);
            if (M > 0) {
                dstart.alloc(M); dstart.upload(start, M, s); D.start = dstart.p;
                dend.alloc(M); dend.upload(end, M, s); D.end = dend.p;
            }
            if (expected) { dexp.alloc(n_expected); dexp.upload(expected, n_expected, s); A.expected = dexp.p; }
        }
        const bool walk = M > 0 && nnz > 0;
        St.init(bin1, bin2, count, nnz, weight, lo, N, bad, kPixValid | (walk ? kPixRows : 0), on_device, s);
        const dim3 grid((unsigned)n_chunks, (unsigned)((G + kDpWaves - 1) / kDpWaves));
        if (M > 0) {
            dok.alloc(N);
            hipLaunchKernelGGL(k_dp_okd, dim3(grid_of(N)), dim3(256), 0, s, (long long)N, A, dok.p);
            Pw.alloc((size_t)n_chunks * GG);
            HH_KTIME("k_dp_weight", s);
            hipLaunchKernelGGL(k_dp_weight, grid, dim3(64 * kDpWaves), 0, s, St.valid.p, dok.p, (long long)N, D, Pw.p);
        }
        if (walk) {
            Ps.alloc((size_t)n_chunks * GG);
            HH_KTIME("k_dp_sum", s);
            hipLaunchKernelGGL(k_dp_sum, grid, dim3(64 * kDpWaves), 0, s, St.X, St.valid.p, St.rp.p, A, D, Ps.p);
        }
        {
            HH_KTIME("k_dp_reduce", s);
            hipLaunchKernelGGL(k_dp_reduce, dim3(grid_of(GG), 2), dim3(256), 0, s, Ps.p, Pw.p, n_chunks, G, dS.p, dW.p);
        }
        HIP_CHECK(hipGetLastError());
        if (on_device) {
            HIP_CHECK(hipMemcpyAsync(S, dS.p, (size_t)GG * sizeof(double), hipMemcpyDeviceToDevice, s));
            HIP_CHECK(hipMemcpyAsync(Wn, dW.p, (size_t)GG * sizeof(double), hipMemcpyDeviceToDevice, s));
        } else {
            dS.download(S, GG, s);
            dW.download(Wn, GG, s);
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}
