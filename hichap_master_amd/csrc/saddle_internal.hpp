// What saddle.hip and pileup.hip share: the device view
// of one chromosome of cooler's pixel table, the validity bytes and their
// 64-bit masks, the row pointers, and the argument checks of the table.
#pragma once

#include "hh_common.hpp"

namespace hh {

struct SdPix {  // device pointers of the table and the chromosome
    const int64_t *b1, *b2;
    const double *cnt, *w;  // w: weights of the chromosome's bins (local index) or null
    long long nnz, lo, N;
};

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

constexpr int64_t kSdMaxN = int64_t(1) << 24;  // bins of one chromosome (k_sd_cu's uint32 cells, the work-item counts)

struct SyncOnExit {  // no buffer returns to the pool while work on it is in flight
    hipStream_t s;
    ~SyncOnExit() { (void)hipStreamSynchronize(s); }
};

void sd_check_table(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz, const double* weight,
                    int64_t n_weight, int64_t lo, int64_t N) {
    HH_REQUIRE(N >= 1 && N <= kSdMaxN, "N outside [1, 2^24]");
    HH_REQUIRE(nnz >= 0 && lo >= 0, "bad arguments");
    HH_REQUIRE(nnz == 0 || (bin1 && bin2 && count), "null pixel arrays");
    HH_REQUIRE(!weight || lo + N <= n_weight, "weights do not cover the chromosome");
}

// The table, the chromosome's weights and `bad` on the device (uploaded unless
// already there), valid and its masks, and the row pointers.
struct SdStage {
    DBuf<int64_t> d1, d2;
    DBuf<double> dc, dw;
    DBuf<uint8_t> dbad, valid;
    DBuf<unsigned long long> mask;
    DBuf<long long> rp;
    SdPix X{};
    long long nW = 0;

    void init(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz, const double* weight,
              int64_t lo, int64_t N, const uint8_t* bad, bool want_rows, int32_t on_device, hipStream_t s) {
        X = SdPix{bin1, bin2, count, weight ? weight + lo : nullptr, (long long)nnz, (long long)lo, (long long)N};
        const uint8_t* pbad = bad;
        if (!on_device) {
            if (nnz > 0) {
                d1.alloc(nnz); d1.upload(bin1, nnz, s); X.b1 = d1.p;
                d2.alloc(nnz); d2.upload(bin2, nnz, s); X.b2 = d2.p;
                dc.alloc(nnz); dc.upload(count, nnz, s); X.cnt = dc.p;
            }
            if (weight) { dw.alloc(N); dw.upload(weight + lo, N, s); X.w = dw.p; }
            if (bad) { dbad.alloc(N); dbad.upload(bad, N, s); pbad = dbad.p; }
        }
        nW = (N + 63) / 64;
        valid.alloc(N);
        mask.alloc(nW + 1);
        hipLaunchKernelGGL(k_sd_valid, dim3((unsigned)((nW * 64 + 255) / 256)), dim3(256), 0, s, X.w, pbad,
                           (long long)N, nW, valid.p, mask.p);
        if (want_rows && nnz > 0) {
            rp.alloc(N + 1);
            HH_KTIME("k_sd_rowptr", s);
            hipLaunchKernelGGL(k_sd_rowptr, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, s, X.b1, X.nnz, X.lo,
                               X.N, rp.p);
        }
        HIP_CHECK(hipGetLastError());
    }
};

unsigned grid_of(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace
}  // namespace hh
