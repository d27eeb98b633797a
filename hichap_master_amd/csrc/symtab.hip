// The symmetric pixel table (HiCHap has no per-bin coverage or
// virtual 4C and cooltools is absent: the definitions are this project's).
//
// cooler stores the upper triangle, sorted by (bin1, bin2): row x of the
// symmetric matrix is the run of pixels with bin1 = x (the `upper` segment)
// and the pixels with bin2 = x, scattered over the table.  hh_symtab_create
// keeps the whole table (cis included, raw counts, nothing baked in) and its
// transpose, so that a row is two contiguous segments:
//
//   k_st_chrom     chrom[x] = the chromosome of bin x (a bisection in the offsets).
//   (k_sd_rowptr:  rpU[f] = the first pixel with bin1 >= f, pixel_table.hpp.)
//   k_st_upper     pU[i] = bin2 (-1 where it is outside [0, n_bins)), cU[i] = count,
//                  key[i] = bin2 << 33 | i for a pixel with bin1 < bin2 and both ids
//                  in range, n_bins << 33 | i for any other (diagonal, out of
//                  range, bin1 > bin2): those sort behind the last row.
//   (dev_sort_u64: the stable radix sort of pairs.hip, unchanged, on the bin2
//   bits.  i ascends in table order, so the entries of one bin2 follow each
//   other in ascending bin1.)
//   k_st_rowptr_l  rpL[f] = the first sorted key with bin2 >= f (a bisection);
//                  rpL[n_bins] is the number of lower entries.
//   k_st_lower     lower entry j = (bin1, index, count) of the j-th key: the
//                  transpose, a pure function of the input (no cursor, no timing).
//
// Nothing here reads a weight or a validity, and there is no compaction: one
// handle serves raw and balanced calls and any use / bad.  No atomic of any
// kind is used.
// Range checks: bin1 and bin2 are compared with n_bins before either decides a
// key; an index read back from a key is compared with nnz and the bin1 behind
// it with n_bins again; the row pointers are bisections bounded by the table's
// length.  A malformed table (unsorted, bin1 > bin2) gives wrong numbers, never
// an access outside the arrays.
#include "symtab.hpp"
#include "pixel_table.hpp"  // PixStage, grid_of

namespace hh {

__global__ __launch_bounds__(256) void k_st_chrom(const long long* __restrict__ off, int C, long long n_bins,
                                                  unsigned short* __restrict__ chrom) {
    __shared__ long long so[HH_TRANS_MAX_CHROMS + 1];
    for (int q = threadIdx.x; q <= C; q += 256) so[q] = off[q];
    __syncthreads();
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_bins) return;
    int lo = 0, hi = C;  // the chromosome q with so[q] <= x < so[q + 1] (so[0] = 0, so[C] = n_bins)
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (so[m] <= x) lo = m; else hi = m;
    }
    chrom[x] = (unsigned short)lo;
}

__global__ __launch_bounds__(256) void k_st_upper(const int64_t* __restrict__ b1, const int64_t* __restrict__ b2,
                                                  const double* __restrict__ cnt, long long nnz, long long n_bins,
                                                  int32_t* __restrict__ pU, double* __restrict__ cU,
                                                  unsigned long long* __restrict__ key) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nnz) return;
    const long long a = (long long)b1[i], b = (long long)b2[i];
    const bool in_a = (unsigned long long)a < (unsigned long long)n_bins;
    const bool in_b = (unsigned long long)b < (unsigned long long)n_bins;
    pU[i] = in_b ? (int32_t)b : -1;
    cU[i] = cnt[i];
    const unsigned long long row = in_a && in_b && a < b ? (unsigned long long)b : (unsigned long long)n_bins;
    key[i] = (row << kStSlotBits) | (unsigned long long)i;
}

// rpL[f] = the first sorted key whose bin2 field is >= f
__global__ __launch_bounds__(256) void k_st_rowptr_l(const unsigned long long* __restrict__ key, long long nnz,
                                                     long long n_bins, long long* __restrict__ rpL) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f > n_bins) return;
    long long a = 0, b = nnz;
    while (a < b) {
        const long long m = a + ((b - a) >> 1);
        if ((long long)(key[m] >> kStSlotBits) < f) a = m + 1; else b = m;
    }
    rpL[f] = a;
}

__global__ __launch_bounds__(256) void k_st_lower(const unsigned long long* __restrict__ key, long long n_lower,
                                                  const int64_t* __restrict__ b1, const double* __restrict__ cnt,
                                                  long long nnz, long long n_bins, int32_t* __restrict__ pL,
                                                  unsigned int* __restrict__ srcL, double* __restrict__ cL) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_lower) return;
    const unsigned long long e = key[j] & ((1ull << kStSlotBits) - 1ull);
    int32_t a = -1;
    unsigned int src = 0;
    double c = 0.0;
    if (e < (unsigned long long)nnz) {  // (a permutation of the indices written above)
        const long long r = (long long)b1[e];
        if ((unsigned long long)r < (unsigned long long)n_bins) a = (int32_t)r;
        src = (unsigned int)e;
        c = cnt[e];
    }
    pL[j] = a;
    srcL[j] = src;
    cL[j] = c;
}

namespace {

void st_create(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz, const int64_t* off,
               int32_t C, int32_t on_device, hipStream_t s, hh_symtab** out) {
    HH_REQUIRE(out, "null handle pointer");
    HH_REQUIRE(C >= 1 && C <= HH_TRANS_MAX_CHROMS, "C outside 1..HH_TRANS_MAX_CHROMS");
    HH_REQUIRE(off, "null chrom_offset");
    HH_REQUIRE(off[0] == 0, "chrom_offset must start at 0");
    for (int q = 0; q < C; ++q) HH_REQUIRE(off[q] < off[q + 1], "chrom_offset must be strictly ascending");
    HH_REQUIRE(off[C] < (int64_t(1) << 31), "n_bins must be below 2^31");
    // (the radix sort's per-tile offsets are 32-bit, and an index has 33 bits of the key)
    HH_REQUIRE(nnz >= 0 && nnz < (int64_t(1) << 32), "nnz must be in [0, 2^32)");
    HH_REQUIRE(nnz == 0 || (bin1 && bin2 && count), "null pixel arrays");
    const long long n_bins = off[C];
    auto H = std::make_unique<hh_symtab>();
    PixStage<double> S;
    DBuf<long long> doff(C + 1);
    DBuf<unsigned long long> key;
    SyncOnExit sync{s};  // (destroyed before the buffers above and H)
    HIP_CHECK(hipGetDevice(&H->device));
    H->n_bins = n_bins;
    H->nnz = nnz;
    H->C = C;
    upload_pinned_sync(doff.p, (const long long*)off, (size_t)C + 1, s);
    H->chrom.alloc(n_bins);
    {
        HH_KTIME("k_st_chrom", s);
        hipLaunchKernelGGL(k_st_chrom, dim3(grid_of(n_bins)), dim3(256), 0, s, doff.p, (int)C, n_bins, H->chrom.p);
    }
    HIP_CHECK(hipGetLastError());
    H->rpL.alloc(n_bins + 1);
    if (nnz > 0) {
        S.init(bin1, bin2, count, nnz, (const double*)nullptr, 0, n_bins, (const uint8_t*)nullptr, kPixRows,
               on_device, s);
        H->rpU = std::move(S.rp);
        H->pU.alloc(nnz);
        H->cU.alloc(nnz);
        key.alloc(nnz);
        {
            HH_KTIME("k_st_upper", s);
            hipLaunchKernelGGL(k_st_upper, dim3(grid_of(nnz)), dim3(256), 0, s, S.X.b1, S.X.b2, S.X.cnt,
                               (long long)nnz, n_bins, H->pU.p, H->cU.p, key.p);
        }
        HIP_CHECK(hipGetLastError());
        int bits = 1;
        while ((1ll << bits) <= n_bins) ++bits;  // the field holds 0 .. n_bins
        dev_sort_u64(key, nnz, bits, s, kStSlotBits);
        {
            HH_KTIME("k_st_rowptr_l", s);
            hipLaunchKernelGGL(k_st_rowptr_l, dim3(grid_of(n_bins + 1)), dim3(256), 0, s, key.p, (long long)nnz,
                               n_bins, H->rpL.p);
        }
        HIP_CHECK(hipGetLastError());
        long long n_lower = 0;
        PinnedDown down;
        down.add((const long long*)H->rpL.p + n_bins, &n_lower, 1);
        down.run(s);
        HH_REQUIRE(n_lower >= 0 && n_lower <= nnz, "the pixel table changed while it was read");
        H->n_lower = n_lower;
        if (n_lower > 0) {
            H->pL.alloc(n_lower);
            H->srcL.alloc(n_lower);
            H->cL.alloc(n_lower);
            HH_KTIME("k_st_lower", s);
            hipLaunchKernelGGL(k_st_lower, dim3(grid_of(n_lower)), dim3(256), 0, s, key.p, n_lower, S.X.b1, S.X.cnt,
                               (long long)nnz, n_bins, H->pL.p, H->srcL.p, H->cL.p);
        }
        HIP_CHECK(hipGetLastError());
    } else {
        H->rpU.alloc(n_bins + 1);
        H->rpU.zero(s);
        H->rpL.zero(s);
    }
    HIP_CHECK(hipStreamSynchronize(s));  // the caller's arrays and the stage are not read after this
    *out = H.release();
}

}  // namespace
}  // namespace hh

using namespace hh;

extern "C" {

int hh_symtab_create(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                     const int64_t* chrom_offset, int32_t C, int32_t on_device, void* stream, hh_symtab** out) {
    return guard([&] { st_create(bin1, bin2, count, nnz, chrom_offset, C, on_device, as_stream(stream), out); });
}

int hh_symtab_nnz(const hh_symtab* h, int64_t* upper, int64_t* lower) {
    return guard([&] {
        HH_REQUIRE(h && upper && lower, "null arguments");
        *upper = h->nnz;
        *lower = h->n_lower;
    });
}

int hh_symtab_export(const hh_symtab* h, int64_t* rowptr_u, int64_t* rowptr_l, int32_t* partner_l, uint32_t* src_l) {
    return guard([&] {
        HH_REQUIRE(h && rowptr_u && rowptr_l, "null arguments");
        HH_REQUIRE(h->n_lower == 0 || (partner_l && src_l), "null output arrays");
        DeviceScope dev(h->device);
        hipStream_t s = nullptr;
        h->rpU.download((long long*)rowptr_u, (size_t)h->n_bins + 1, s);
        h->rpL.download((long long*)rowptr_l, (size_t)h->n_bins + 1, s);
        if (h->n_lower) {
            h->pL.download(partner_l, (size_t)h->n_lower, s);
            h->srcL.download((unsigned int*)src_l, (size_t)h->n_lower, s);
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int hh_symtab_free(hh_symtab* h) {
    return guard([&] {
        if (!h) return;
        device_quiesce(h->device);
        delete h;
    });
}

}  // extern "C"
