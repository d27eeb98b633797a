// Per-bin coverage and virtual 4C from the symmetric pixel table (DESIGN.md
// §4v; symtab.hip builds the table).
//
// The genome, v(a, b) = count * w[a] * w[b] (in that order, NaN -> 0), `use`,
// `bad` and valid[x] are §4s's (trans.hip).  A[i][j] = v(min, max) for valid
// i, j with a stored pixel, 0 elsewhere; a diagonal pixel is one entry of its
// row's upper segment and enters the row once.  With d = |i - j| a cell is
// trans (different chromosomes), dropped (cis, d < ignore_diags), near (cis,
// ignore_diags <= d < near_bins) or far (cis, d >= max(near_bins,
// ignore_diags)).
//
//   k_cv_bininfo    info[x] = chromosome of x, bit 15 set where the bin is invalid
//                   (k_te_bininfo over the handle's chromosome ids).
//   k_cv_coverage   one wave per bin x: lane l takes the entries l, l + 64, ... of
//                   the bin's lower segment, then of its upper segment, into three
//                   running sums and three counts (near, far, trans); the next
//                   trip's partner and count are loaded before the current
//                   trip's gather of the partner's info and weight.  The 64 lane
//                   sums of a class go through a fixed xor butterfly (32, 16, ...,
//                   1) and lane 0 stores them; an invalid bin stores +0.0 and 0.
//   k_cv_viewpoints one thread per (viewpoint c, bin y): two bisections find the
//                   run of the lower segment of y whose partners lie in [lo_c,
//                   hi_c) (partners ascend inside a segment), its terms are added
//                   from +0.0 in ascending partner, then the run of the upper
//                   segment likewise.
//
// Every fp64 sum has an order fixed by the table and the arguments alone (not
// by the grid, hh_tune "cov_rows", K or the timing); no atomic
// of any kind is used and no product is contracted into an addition.
// Range checks: a row pointer is clamped to the table's length and a row whose
// pointers are out of order is empty; a partner read from either table is
// compared with n_bins before it indexes info or the weights.  The lower half
// reads the lower table's own copy of the count, not count[src_l]: the indexed
// load was measured 2.2 x slower.
#include "symtab.hpp"

namespace hh {

constexpr unsigned kCvInvalid = 0x8000u, kCvChromMask = 0x7FFFu;
enum { kCvNear = 0, kCvFar = 1, kCvTrans = 2, kCvDropped = 3 };

inline unsigned cv_grid(long long n) { return (unsigned)((n + 255) / 256); }

__global__ __launch_bounds__(256) void k_cv_bininfo(const unsigned short* __restrict__ chrom, int C,
                                                    const uint8_t* __restrict__ use, const double* __restrict__ w,
                                                    const uint8_t* __restrict__ bad, long long n_bins,
                                                    unsigned int* __restrict__ info) {
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_bins) return;
    const unsigned int q = chrom[x];
    bool ok = q < (unsigned int)C && (!use || use[q]);
    if (ok && w) {
        const double t = w[x];
        ok = t - t == 0.0;  // finite
    }
    if (ok && bad && bad[x]) ok = false;
    info[x] = (q & kCvChromMask) | (ok ? 0u : kCvInvalid);
}

// the class of the cell (x, j), both in range, from their info words; kCvDropped also for an invalid j
__device__ __forceinline__ int cv_class(unsigned int ix, unsigned int ij, long long x, long long j, long long ignore,
                                        long long near) {
    if (ij & kCvInvalid) return kCvDropped;
    if ((ix & kCvChromMask) != (ij & kCvChromMask)) return kCvTrans;
    const long long d = x > j ? x - j : j - x;
    if (d < ignore) return kCvDropped;
    return d < near ? kCvNear : kCvFar;
}

// count * w[a] * w[b] with a = min(x, j), b = max(x, j) (NaN -> 0): single IEEE operations, §4s's order
template <bool LOWER>
__device__ __forceinline__ double cv_value(double c, const double* __restrict__ w, double wx, long long j) {
#pragma clang fp contract(off)
    double v = c;
    if (w) {
        const double wj = w[j];
        v = LOWER ? v * wj * wx : v * wx * wj;
        if (v != v) v = 0.0;
    }
    return v;
}

// lane `lane` adds the entries s0 + lane, s0 + lane + 64, ... of [s0, s1) of one segment of bin x
template <bool LOWER>
__device__ __forceinline__ void cv_walk(const int32_t* __restrict__ part, const double* __restrict__ val,
                                        long long s0, long long s1, int lane, long long x,
                                        unsigned int ix, double wx, const double* __restrict__ w,
                                        const unsigned int* __restrict__ info, long long n_bins, long long ignore,
                                        long long near, double (&acc)[3], long long (&num)[3]) {
#pragma clang fp contract(off)
    long long i = s0 + lane;
    bool nv = i < s1;
    int nj = 0;
    double nc = 0.0;
    if (nv) { nj = part[i]; nc = val[i]; }
    while (nv) {
        const int j = nj;
        const double c = nc;
        i += 64;
        nv = i < s1;  // the next trip's loads are in flight while this one gathers
        if (nv) { nj = part[i]; nc = val[i]; }
        if ((unsigned long long)(long long)j >= (unsigned long long)n_bins) continue;
        const int k = cv_class(ix, info[j], x, (long long)j, ignore, near);
        if (k == kCvDropped) continue;
        const double v = cv_value<LOWER>(c, w, wx, (long long)j);
        if (k == kCvNear) { acc[0] = acc[0] + v; num[0] += 1; }
        else if (k == kCvFar) { acc[1] = acc[1] + v; num[1] += 1; }
        else { acc[2] = acc[2] + v; num[2] += 1; }
    }
}

__device__ __forceinline__ long long cv_clamp(long long v, long long hi) { return min(max(v, 0ll), hi); }

__global__ __launch_bounds__(1024) void k_cv_coverage(StTables T, const unsigned int* __restrict__ info,
                                                      const double* __restrict__ w, long long ignore, long long near,
                                                      double* __restrict__ S, long long* __restrict__ n) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long long x = (long long)blockIdx.x * (blockDim.x >> 6) + wid;
    if (x >= T.n_bins) return;  // (no block barrier below: the waves are independent)
    double acc[3] = {0.0, 0.0, 0.0};
    long long num[3] = {0, 0, 0};
    const unsigned int ix = info[x];
    const bool ok = !(ix & kCvInvalid);
    if (ok) {
        const double wx = w ? w[x] : 1.0;
        cv_walk<true>(T.pL, T.cL, cv_clamp(T.rpL[x], T.n_lower), cv_clamp(T.rpL[x + 1], T.n_lower), lane, x, ix, wx, w,
                      info, T.n_bins, ignore, near, acc, num);
        cv_walk<false>(T.pU, T.cU, cv_clamp(T.rpU[x], T.nnz), cv_clamp(T.rpU[x + 1], T.nnz), lane, x, ix, wx, w, info,
                       T.n_bins, ignore, near, acc, num);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc[k] = acc[k] + __shfl_xor(acc[k], o, 64);
            num[k] = wave_sum_ll(num[k]);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            S[x * 3 + k] = ok ? acc[k] : 0.0;
            n[x * 3 + k] = ok ? num[k] : 0;
        }
    }
}

struct CvViews {  // the intervals of a call, by value (n_bins < 2^31)
    int32_t lo[HH_SYMTAB_MAX_VIEWS], hi[HH_SYMTAB_MAX_VIEWS];
};

// the first entry of part[s0, s1) that is >= t (partners ascend inside a segment)
__device__ __forceinline__ long long cv_lower_bound(const int32_t* __restrict__ part, long long s0, long long s1,
                                                    long long t) {
    long long a = s0, b = s1;
    while (a < b) {
        const long long m = a + ((b - a) >> 1);
        if ((long long)part[m] < t) a = m + 1; else b = m;
    }
    return a;
}

// the entries of part[s0, s1) with a partner in [lo, hi), added in table order
template <bool LOWER>
__device__ __forceinline__ double cv_run(const int32_t* __restrict__ part, const double* __restrict__ val,
                                         long long s0, long long s1, long long lo, long long hi, long long y,
                                         unsigned int iy, double wy, const double* __restrict__ w,
                                         const unsigned int* __restrict__ info, long long n_bins, long long ignore,
                                         double sum) {
#pragma clang fp contract(off)
    if (s0 >= s1) return sum;
    const long long r0 = cv_lower_bound(part, s0, s1, lo);
    const long long r1 = cv_lower_bound(part, r0, s1, hi);
    for (long long i = r0; i < r1; ++i) {
        const long long x = (long long)part[i];
        // (an unsorted table: the run may hold partners outside the interval)
        if ((unsigned long long)x >= (unsigned long long)n_bins || x < lo || x >= hi) continue;
        if (cv_class(iy, info[x], y, x, ignore, 0) == kCvDropped) continue;
        sum = sum + cv_value<LOWER>(val[i], w, wy, x);
    }
    return sum;
}

__global__ __launch_bounds__(256) void k_cv_viewpoints(StTables T, const unsigned int* __restrict__ info,
                                                       const double* __restrict__ w, long long ignore, CvViews V,
                                                       double* __restrict__ P) {
#pragma clang fp contract(off)
    const long long y = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (y >= T.n_bins) return;
    const int c = blockIdx.y;
    const unsigned int iy = info[y];
    double sum = 0.0;
    if (!(iy & kCvInvalid)) {
        const long long lo = V.lo[c], hi = V.hi[c];
        const double wy = w ? w[y] : 1.0;
        sum = cv_run<true>(T.pL, T.cL, cv_clamp(T.rpL[y], T.n_lower), cv_clamp(T.rpL[y + 1], T.n_lower), lo, hi, y, iy,
                           wy, w, info, T.n_bins, ignore, sum);
        sum = cv_run<false>(T.pU, T.cU, cv_clamp(T.rpU[y], T.nnz), cv_clamp(T.rpU[y + 1], T.nnz), lo, hi, y, iy, wy, w,
                            info, T.n_bins, ignore, sum);
    }
    P[(long long)c * T.n_bins + y] = sum;
}

namespace {

// what the two calls share: the argument checks, `use` / weight / bad on the device and the bin-info pass
struct CvCall {
    DBuf<uint8_t> duse, dbad;
    DBuf<double> dw;
    DBuf<unsigned int> info;
    const double* w = nullptr;

    static void check(const hh_symtab& H, const double* weight, int64_t n_weight, int32_t ignore_diags) {
        HH_REQUIRE(ignore_diags >= 0, "ignore_diags must be >= 0");
        HH_REQUIRE(!weight || H.n_bins <= n_weight, "weights do not cover n_bins");
    }
    void stage(const hh_symtab& H, const double* weight, const uint8_t* use, const uint8_t* bad, int32_t on_device,
               hipStream_t s) {
        const size_t n = (size_t)H.n_bins;
        if (use) { duse.alloc(H.C); upload_pinned_sync(duse.p, use, (size_t)H.C, s); }
        w = weight;
        const uint8_t* pbad = bad;
        if (!on_device) {
            if (weight) { dw.alloc(n); dw.upload(weight, n, s); w = dw.p; }
            if (bad) { dbad.alloc(n); dbad.upload(bad, n, s); pbad = dbad.p; }
        }
        info.alloc(n);
        HH_KTIME("k_cv_bininfo", s);
        hipLaunchKernelGGL(k_cv_bininfo, dim3(cv_grid(H.n_bins)), dim3(256), 0, s, H.chrom.p, (int)H.C, duse.p, w,
                           pbad, (long long)H.n_bins, info.p);
        HIP_CHECK(hipGetLastError());
    }
};

void cv_coverage(const hh_symtab& H, const double* weight, int64_t n_weight, const uint8_t* use, const uint8_t* bad,
                 int32_t ignore_diags, int32_t near_bins, double* S, int64_t* n, int32_t on_device, hipStream_t s) {
    CvCall::check(H, weight, n_weight, ignore_diags);
    HH_REQUIRE(near_bins >= 0, "near_bins must be >= 0");
    HH_REQUIRE(S && n, "null outputs");
    const size_t m = (size_t)H.n_bins * 3;
    CvCall call;
    DBuf<double> dS;
    DBuf<long long> dn;
    SyncOnExit sync{s};  // (destroyed before the buffers above)
    double* pS = S;
    long long* pn = (long long*)n;
    if (!on_device) {
        dS.alloc(m); pS = dS.p;
        dn.alloc(m); pn = dn.p;
    }
    if (H.nnz == 0) {  // no launch over an empty table
        HIP_CHECK(hipMemsetAsync(pS, 0, m * sizeof(double), s));
        HIP_CHECK(hipMemsetAsync(pn, 0, m * sizeof(long long), s));
    } else {
        call.stage(H, weight, use, bad, on_device, s);
        const int rows = g_cov_rows;
        const dim3 grid((unsigned)((H.n_bins + rows - 1) / rows)), block(64 * rows);
        HH_KTIME("k_cv_coverage", s);
        hipLaunchKernelGGL(k_cv_coverage, grid, block, 0, s, st_tables(H), call.info.p, call.w,
                           (long long)ignore_diags, (long long)near_bins, pS, pn);
        HIP_CHECK(hipGetLastError());
    }
    if (!on_device) {
        dS.download(S, m, s);
        dn.download((long long*)n, m, s);
    }
    HIP_CHECK(hipStreamSynchronize(s));
}

void cv_viewpoints(const hh_symtab& H, const double* weight, int64_t n_weight, const uint8_t* use, const uint8_t* bad,
                   int32_t ignore_diags, const int64_t* lo, const int64_t* hi, int32_t K, double* P,
                   int32_t on_device, hipStream_t s) {
    CvCall::check(H, weight, n_weight, ignore_diags);
    HH_REQUIRE(K >= 1 && K <= HH_SYMTAB_MAX_VIEWS, "K outside 1..HH_SYMTAB_MAX_VIEWS");
    HH_REQUIRE(lo && hi, "null viewpoint intervals");
    HH_REQUIRE(P, "null outputs");
    CvViews V{};
    for (int c = 0; c < K; ++c) {
        HH_REQUIRE(lo[c] >= 0 && hi[c] <= H.n_bins && lo[c] < hi[c], "a viewpoint is not an interval inside [0, n_bins)");
        V.lo[c] = (int32_t)lo[c];
        V.hi[c] = (int32_t)hi[c];
    }
    const size_t m = (size_t)H.n_bins * (size_t)K;
    CvCall call;
    DBuf<double> dP;
    SyncOnExit sync{s};  // (destroyed before the buffers above)
    double* pP = P;
    if (!on_device) { dP.alloc(m); pP = dP.p; }
    if (H.nnz == 0) {  // no launch over an empty table
        HIP_CHECK(hipMemsetAsync(pP, 0, m * sizeof(double), s));
    } else {
        call.stage(H, weight, use, bad, on_device, s);
        HH_KTIME("k_cv_viewpoints", s);
        hipLaunchKernelGGL(k_cv_viewpoints, dim3(cv_grid(H.n_bins), (unsigned)K), dim3(256), 0, s, st_tables(H),
                           call.info.p, call.w, (long long)ignore_diags, V, pP);
        HIP_CHECK(hipGetLastError());
    }
    if (!on_device) dP.download(P, m, s);
    HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace
}  // namespace hh

using namespace hh;

extern "C" {

int hh_symtab_coverage(const hh_symtab* h, const double* weight, int64_t n_weight, const uint8_t* use,
                       const uint8_t* bad, int32_t ignore_diags, int32_t near_bins, double* S, int64_t* n,
                       int32_t on_device, void* stream) {
    return guard([&] {
        HH_REQUIRE(h, "null handle");
        DeviceScope dev(h->device);
        cv_coverage(*h, weight, n_weight, use, bad, ignore_diags, near_bins, S, n, on_device, as_stream(stream));
    });
}

int hh_symtab_viewpoints(const hh_symtab* h, const double* weight, int64_t n_weight, const uint8_t* use,
                         const uint8_t* bad, int32_t ignore_diags, const int64_t* lo, const int64_t* hi, int32_t K,
                         double* P, int32_t on_device, void* stream) {
    return guard([&] {
        HH_REQUIRE(h, "null handle");
        DeviceScope dev(h->device);
        cv_viewpoints(*h, weight, n_weight, use, bad, ignore_diags, lo, hi, K, P, on_device, as_stream(stream));
    });
}

}  // extern "C"
