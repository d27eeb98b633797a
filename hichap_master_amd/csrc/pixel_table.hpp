// One chromosome of cooler's pixel table on the device, shared by every
// per-chromosome path (comp.hip's band builds, select.hip, allelic.hip,
// saddle.hip, pileup.hip): the device view of the table, its
// argument checks, and the stage that uploads the table unless it is already
// there and derives the validity bytes, their 64-bit masks and the row
// pointers when asked for.
#pragma once

#include "hh_common.hpp"

namespace hh {

template <class C>
struct PixTable {  // device pointers of the table and the chromosome
    const int64_t *b1, *b2;
    const C* cnt;
    const double* w;  // weights of the chromosome's bins (local index) or null
    long long nnz, lo, N;
};

// valid[j] = the weight of bin j is finite and bad[j] is not set; with `mask`
// also the 64-bit words of valid (nW of them and a zero word behind)
static __global__ __launch_bounds__(256) void k_sd_valid(const double* __restrict__ w, const uint8_t* __restrict__ bad,
                                                         long long N, long long nW, uint8_t* __restrict__ valid,
                                                         unsigned long long* __restrict__ mask) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // lanes of a wave: one mask word
    bool ok = j < N;
    if (ok && w) {
        const double x = w[j];
        ok = x - x == 0.0;  // finite
    }
    if (ok && bad && bad[j]) ok = false;
    if (j < N) valid[j] = ok ? 1 : 0;
    const unsigned long long m = __ballot(ok);
    if (!mask) return;
    if ((threadIdx.x & 63) == 0 && (j >> 6) < nW) mask[j >> 6] = m;
    if (j == 0) mask[nW] = 0ull;  // the shifted read of the last word
}

static __global__ __launch_bounds__(256) void k_sd_rowptr(const int64_t* __restrict__ b1, long long nnz, long long lo,
                                                          long long N, long long* __restrict__ rp) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f > N) return;
    long long a = 0, b = nnz;
    while (a < b) {
        const long long m = a + ((b - a) >> 1);
        if ((long long)b1[m] < lo + f) a = m + 1; else b = m;
    }
    rp[f] = a;
}

namespace {

// What every caller requires of the table; limits on N, on the band or on the
// query lists stay with the caller.
template <class C>
void check_pixel_table(const int64_t* bin1, const int64_t* bin2, const C* count, int64_t nnz, const double* weight,
                       int64_t n_weight, int64_t lo, int64_t N) {
    HH_REQUIRE(nnz >= 0 && lo >= 0, "bad arguments");
    HH_REQUIRE(nnz == 0 || (bin1 && bin2 && count), "null pixel arrays");
    HH_REQUIRE(!weight || lo + N <= n_weight, "weights do not cover the chromosome");
}

enum : unsigned {  // the derived parts of a PixStage
    kPixValid = 1,  // valid
    kPixMask = 2,   // valid and its 64-bit masks
    kPixRows = 4,   // row pointers (made only when nnz > 0)
};

// The table on the device (uploaded unless already there) with the
// chromosome's slice of the weights, and the parts of `want`.  The weights
// (and `bad`) are staged only where something reads them: with pixels or for
// valid.  The caller keeps the stage alive until its stream is idle.
template <class C>
struct PixStage {
    DBuf<int64_t> d1, d2;
    DBuf<C> dc;
    DBuf<double> dw;
    DBuf<uint8_t> dbad, valid;
    DBuf<unsigned long long> mask;
    DBuf<long long> rp;
    PixTable<C> X{};
    long long nW = 0;

    void init(const int64_t* bin1, const int64_t* bin2, const C* count, int64_t nnz, const double* weight, int64_t lo,
              int64_t N, const uint8_t* bad, unsigned want, int32_t on_device, hipStream_t s) {
        const bool want_valid = want & (kPixValid | kPixMask);
        if (!(nnz > 0 || want_valid)) weight = nullptr;
        X = PixTable<C>{bin1, bin2, count, weight ? weight + lo : nullptr, (long long)nnz, (long long)lo, (long long)N};
        const uint8_t* pbad = bad;
        if (!on_device) {
            if (nnz > 0) {
                d1.alloc(nnz); d1.upload(bin1, nnz, s); X.b1 = d1.p;
                d2.alloc(nnz); d2.upload(bin2, nnz, s); X.b2 = d2.p;
                dc.alloc(nnz); dc.upload(count, nnz, s); X.cnt = dc.p;
            }
            if (weight) { dw.alloc(N); dw.upload(weight + lo, N, s); X.w = dw.p; }
            if (bad && want_valid) { dbad.alloc(N); dbad.upload(bad, N, s); pbad = dbad.p; }
        }
        if (want_valid) {
            nW = (N + 63) / 64;
            valid.alloc(N);
            if (want & kPixMask) mask.alloc(nW + 1);
            hipLaunchKernelGGL(k_sd_valid, dim3((unsigned)((nW * 64 + 255) / 256)), dim3(256), 0, s, X.w, pbad,
                               (long long)N, nW, valid.p, mask.p);
        }
        if ((want & kPixRows) && nnz > 0) {
            rp.alloc(N + 1);
            HH_KTIME("k_sd_rowptr", s);
            hipLaunchKernelGGL(k_sd_rowptr, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, s, X.b1, X.nnz, X.lo,
                               X.N, rp.p);
        }
        HIP_CHECK(hipGetLastError());
    }
};

}  // namespace

inline unsigned grid_of(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace hh
