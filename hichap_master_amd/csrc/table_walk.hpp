// What the table-to-table transforms of cooler's pixel table share
// (coarsen.hip, merge.hip): the row pointers of a sorted
// table, the error path that names a malformed table's first offending pixel,
// and the device scope of a handle's write / free calls.
#pragma once

#include "ice_internal.hpp"  // hh_common.hpp + dev_excl_scan_i64

namespace hh {

constexpr int kCoBlock = 512;  // threads per item = pixels per trip of the walk
constexpr int kCoRows = 64;    // segments (fine rows, or tables) walked as one flat range

// rp[f] = first pixel of row f (lower bound in bin1); rp[0] = 0 and rp[n_bins]
// = nnz are forced.  On ANY input the bisection returns s with key[s - 1] <
// target <= key[s] (virtual -inf / +inf past the ends).
template <class Id>
__global__ __launch_bounds__(256) void k_co_rowptr(const Id* __restrict__ b1, long long nnz, long long n_bins,
                                                   long long* __restrict__ rp) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f > n_bins) return;
    long long a = 0, b = nnz;
    if (f == n_bins) a = nnz;
    else if (f > 0)
        while (a < b) {
            const long long m = a + ((b - a) >> 1);
            if ((long long)b1[m] < f) a = m + 1; else b = m;
        }
    rp[f] = a;
}

// error path only: errs[code] = smallest offending pixel of that kind, the
// kinds and their order as hh_matrix_from_pixels_device reports them
template <class Id, class Cnt>
__global__ __launch_bounds__(256) void k_co_check(const Id* __restrict__ b1, const Id* __restrict__ b2,
                                                  const Cnt* __restrict__ cnt, long long nnz, long long n_bins,
                                                  unsigned long long* __restrict__ errs) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nnz) return;
    const long long a = (long long)b1[i], b = (long long)b2[i];
    int code = -1;
    if (a < 0 || b < 0 || a >= n_bins || b >= n_bins) code = 0;
    else if (a > b) code = 1;
    else if (i > 0) {
        const long long pa = (long long)b1[i - 1], pb = (long long)b2[i - 1];
        if (pa > a || (pa == a && pb > b)) code = 2;
        else if (pa == a && pb == b) code = 3;
    }
    if (code < 0 && (long long)cnt[i] < 0) code = 4;
    if (code >= 0) atomicMin(errs + code, (unsigned long long)i);
}

// A table that failed the count pass is read once more to name its first
// offending pixel: "<what> at pixel <i>", the caller's HH_ERR_ARG message.
template <class Id, class Cnt>
inline std::string first_bad_pixel(const Id* b1, const Id* b2, const Cnt* cnt, int64_t nnz, int64_t n_bins,
                                   hipStream_t s) {
    DBuf<unsigned long long> derrs(5);
    SyncOnExit sync{s};
    HIP_CHECK(hipMemsetAsync(derrs.p, 0xff, 5 * sizeof(unsigned long long), s));
    if (nnz > 0)
        hipLaunchKernelGGL((k_co_check<Id, Cnt>), dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, s, b1, b2, cnt,
                           (long long)nnz, (long long)n_bins, derrs.p);
    HIP_CHECK(hipGetLastError());
    unsigned long long e[5];
    PinnedDown down;
    down.add(derrs.p, e, 5);
    down.run(s);
    static const char* what[5] = {"bin id out of range", "bin1 > bin2 (not an upper-triangle pixel table)",
                                  "pixels not sorted by (bin1, bin2)",
                                  "duplicate pixel (cooler's pixel table has unique (bin1, bin2))",
                                  "counts must be non-negative integers"};
    int code = -1;
    unsigned long long at = ~0ull;
    for (int q = 0; q < 5; ++q)
        if (e[q] < at) { at = e[q]; code = q; }
    HH_REQUIRE(code >= 0, "the pixel table changed while it was read");
    return std::string(what[code]) + " at pixel " + std::to_string(at);
}

struct DeviceScope {  // run on `device`, restore the caller's on exit
    int prev = -1;
    explicit DeviceScope(int device) {
        int cur = 0;
        HIP_CHECK(hipGetDevice(&cur));
        if (cur != device) {
            HIP_CHECK(hipSetDevice(device));
            prev = cur;
        }
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

}  // namespace hh
