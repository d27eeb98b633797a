// Down-sampling of cooler's pixel table: binomial thinning by a counter-based
// rule (the normative text).  For pixel (bin1, bin2) of count c
//
//   base = mix64(seed ^ mix64((uint64(bin1) << 32) | uint64(bin2)))
//   kept = #{ t in [0, c) : mix64(base + t) < thr }       (uint64, wrapping)
//
// and the pixels with kept == 0 are dropped, the others keep their order.  A
// contact's fate is a pure function of (seed, bin1, bin2, t): the result does
// not depend on the launch geometry, on which path below counted a pixel, or
// on what else is in the table.
//
//   k_sa_count  one thread per pixel, kSaBlock pixels per block.  kept is a
//               sum of predicates over t, split three ways by the count:
//                 c < kSaWaveCut (64)         the pixel's own lane;
//                 c < kSaBlockCut (2^16)      the wave, pixel after pixel
//                                             (ballot): lane l takes t = l,
//                                             l + 64, ..., the partial counts
//                                             are summed over the wave;
//                 otherwise                   the block, through LDS: thread
//                                             t takes t, t + kSaBlock, ...
//               Every pixel's kept is stored (at the width of the counts); the
//               block's number of kept pixels goes to cells[block], the kept
//               total and the largest kept count to two words (integer
//               atomics: the same on every run).  An id < 0 or a count < 0 is
//               reported by the smallest offending pixel index.
//   k_sa_write  compaction: a block writes its kept pixels at the exclusive
//               scan of cells (dev_excl_scan_i64), in pixel order.
#include "table_walk.hpp"

namespace hh {

constexpr int kSaBlock = 256;
constexpr long long kSaWaveCut = 64;         // counts from here on are thinned by the wave
constexpr long long kSaBlockCut = 1 << 16;   // and from here on by the block

__device__ __forceinline__ unsigned long long sa_base(unsigned long long seed, long long a, long long b) {
    return mix64(seed ^ mix64(((unsigned long long)a << 32) | (unsigned long long)b));
}

// #{ t = t0, t0 + step, ... < c : mix64(base + t) < thr }
__device__ __forceinline__ unsigned long long sa_kept(unsigned long long base, unsigned long long thr,
                                                      unsigned long long t0, unsigned long long step,
                                                      unsigned long long c) {
    unsigned long long k = 0;
#pragma unroll 4
    for (unsigned long long t = t0; t < c; t += step) k += mix64(base + t) < thr ? 1ull : 0ull;
    return k;
}

template <class Cnt>
__global__ __launch_bounds__(kSaBlock) void k_sa_count(const int32_t* __restrict__ b1, const int32_t* __restrict__ b2,
                                                       const Cnt* __restrict__ cnt, long long nnz,
                                                       unsigned long long thr, unsigned long long seed,
                                                       Cnt* __restrict__ kept, long long* __restrict__ cells,
                                                       unsigned long long* __restrict__ tot,   // kept total, max
                                                       unsigned long long* __restrict__ errs) {  // id, count
    __shared__ unsigned long long sbase[kSaBlock], sk[kSaBlock];
    __shared__ long long sc[kSaBlock];
    __shared__ int nbig;
    __shared__ int wn[kSaBlock / 64];
    __shared__ unsigned long long wsum[kSaBlock / 64], wmax[kSaBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const long long i = (long long)blockIdx.x * kSaBlock + tid;
    long long c = 0;
    unsigned long long base = 0ull;
    if (i < nnz) {
        const long long a = (long long)b1[i], b = (long long)b2[i];
        c = (long long)cnt[i];
        if (a < 0 || b < 0) {
            atomicMin(errs, (unsigned long long)i);
            c = 0;
        } else if (c < 0) {
            atomicMin(errs + 1, (unsigned long long)i);
            c = 0;
        }
        base = sa_base(seed, a, b);
    }
    if (tid == 0) nbig = 0;
    sk[tid] = 0ull;
    sc[tid] = c;
    sbase[tid] = base;
    __syncthreads();
    if (c >= kSaBlockCut) nbig = 1;  // (every writer stores the same value)

    unsigned long long k = 0ull;
    if (c < kSaWaveCut) k = sa_kept(base, thr, 0ull, 1ull, (unsigned long long)c);
    unsigned long long todo = __ballot(c >= kSaWaveCut && c < kSaBlockCut);
    while (todo) {  // wave-uniform
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const unsigned long long pb = (unsigned long long)__shfl((long long)base, l, 64);
        const unsigned long long pc = (unsigned long long)__shfl(c, l, 64);
        const unsigned long long part = (unsigned long long)wave_sum_ll((long long)sa_kept(pb, thr, lane, 64ull, pc));
        if (lane == l) k = part;
    }
    __syncthreads();
    if (nbig) {  // block-uniform
        for (int j = 0; j < kSaBlock; ++j) {
            const long long pc = sc[j];
            if (pc < kSaBlockCut) continue;
            const unsigned long long part = (unsigned long long)wave_sum_ll(
                (long long)sa_kept(sbase[j], thr, (unsigned long long)tid, (unsigned long long)kSaBlock,
                                   (unsigned long long)pc));
            if (lane == 0) atomicAdd(&sk[j], part);
        }
        __syncthreads();
        if (c >= kSaBlockCut) k = sk[tid];
    }

    if (i < nnz) kept[i] = (Cnt)k;
    const unsigned long long nzm = __ballot(k != 0ull);
    const unsigned long long s = (unsigned long long)wave_sum_ll((long long)k);
    unsigned long long mx = k;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned long long)__shfl_xor((long long)mx, o, 64));
    if (lane == 0) {
        wn[wid] = __popcll(nzm);
        wsum[wid] = s;
        wmax[wid] = mx;
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        unsigned long long ss = 0ull, mm = 0ull;
        for (int w = 0; w < kSaBlock / 64; ++w) {
            n += wn[w];
            ss += wsum[w];
            mm = max(mm, wmax[w]);
        }
        cells[blockIdx.x] = n;
        if (ss) atomicAdd(tot, ss);
        if (mm > __hip_atomic_load(tot + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(tot + 1, mm);
    }
}

template <class Cnt, class OutCnt>
__global__ __launch_bounds__(kSaBlock) void k_sa_write(const int32_t* __restrict__ b1, const int32_t* __restrict__ b2,
                                                       const Cnt* __restrict__ kept, long long nnz,
                                                       const long long* __restrict__ block_off, long long out_nnz,
                                                       int32_t* __restrict__ o1, int32_t* __restrict__ o2,
                                                       OutCnt* __restrict__ oc) {
    __shared__ int wn[kSaBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const long long i = (long long)blockIdx.x * kSaBlock + tid;
    const long long k = i < nnz ? (long long)kept[i] : 0;
    const unsigned long long nzm = __ballot(k != 0);
    if (lane == 0) wn[wid] = __popcll(nzm);
    __syncthreads();
    if (k == 0) return;
    long long pos = block_off[blockIdx.x] + __popcll(nzm & ((1ull << lane) - 1ull));
    for (int w = 0; w < wid; ++w) pos += wn[w];
    if (pos >= out_nnz) return;  // (the handle's own kept array: cannot happen)
    o1[pos] = b1[i];
    o2[pos] = b2[i];
    oc[pos] = (OutCnt)k;
}

}  // namespace hh

struct hh_sample {
    int device = 0;
    int cnt64 = 0;
    const int32_t *b1 = nullptr, *b2 = nullptr;  // device pointers (the caller's, or own[])
    hh::DBuf<char> own[3];                       // uploads of a host table
    hh::DBuf<char> kept;                         // nnz kept counts, at the width of the counts
    hh::DBuf<long long> block_off;
    int64_t nnz = 0, n_blocks = 0, out_nnz = 0, kept_total = 0, max_count = 0;
};

namespace hh {

// host64: a host table with int64 ids and counts (cooler's); ids that int32
// cannot hold go up as -1 and are reported at their pixel
static void sample_create(const void* bin1, const void* bin2, const void* count, int cnt64, int64_t nnz, uint64_t thr,
                          uint64_t seed, int host64, int on_device, hipStream_t s, hh_sample** out, int64_t* out_nnz,
                          int64_t* kept_total, int64_t* max_count) {
    HH_REQUIRE(out && out_nnz && kept_total && max_count, "null arguments");
    HH_REQUIRE(nnz >= 0 && (nnz == 0 || (bin1 && bin2 && count)), "null pixel arrays");
    auto H = std::make_unique<hh_sample>();
    DBuf<long long> cells;
    DBuf<unsigned long long> dtot, derrs;  // kept total, largest kept count, number of kept pixels; first bad id, count
    SyncOnExit sync{s};  // (destroyed before H and the buffers above)
    HIP_CHECK(hipGetDevice(&H->device));
    H->cnt64 = cnt64;
    H->nnz = nnz;
    H->n_blocks = (nnz + kSaBlock - 1) / kSaBlock;
    HH_REQUIRE(H->n_blocks < (int64_t(1) << 31), "too many pixels for one call");
    const void* src[3] = {bin1, bin2, count};
    if (!on_device && nnz > 0) {
        const size_t n = (size_t)nnz;
        std::vector<int32_t> narrow;
        for (int q = 0; q < 3; ++q) {
            DBuf<char>& d = H->own[q];
            if (host64 && q < 2) {
                const int64_t* id = (const int64_t*)src[q];
                narrow.resize(n);
                for (size_t i = 0; i < n; ++i) narrow[i] = (id[i] < 0 || id[i] > 2147483647ll) ? -1 : (int32_t)id[i];
                d.alloc(n * 4);
                upload_pinned_sync((char*)d.p, (const char*)narrow.data(), n * 4, s);  // `narrow` is reused
            } else {
                const size_t w = (q < 2) ? 4u : (cnt64 ? 8u : 4u);
                d.alloc(n * w);
                d.upload((const char*)src[q], n * w, s);
            }
            src[q] = d.p;
        }
    }
    H->b1 = (const int32_t*)src[0];
    H->b2 = (const int32_t*)src[1];
    H->kept.alloc((size_t)nnz * (cnt64 ? 8 : 4));
    H->block_off.alloc(H->n_blocks + 1);
    cells.alloc(H->n_blocks + 1);
    dtot.alloc(3);
    derrs.alloc(2);
    dtot.zero(s);
    cells.zero(s);
    HIP_CHECK(hipMemsetAsync(derrs.p, 0xff, 2 * sizeof(unsigned long long), s));
    if (nnz > 0) {
        HH_KTIME("k_sa_count", s);
        if (cnt64)
            hipLaunchKernelGGL(k_sa_count<int64_t>, dim3((unsigned)H->n_blocks), dim3(kSaBlock), 0, s, H->b1, H->b2,
                               (const int64_t*)src[2], (long long)nnz, (unsigned long long)thr,
                               (unsigned long long)seed, (int64_t*)H->kept.p, cells.p, dtot.p, derrs.p);
        else
            hipLaunchKernelGGL(k_sa_count<int32_t>, dim3((unsigned)H->n_blocks), dim3(kSaBlock), 0, s, H->b1, H->b2,
                               (const int32_t*)src[2], (long long)nnz, (unsigned long long)thr,
                               (unsigned long long)seed, (int32_t*)H->kept.p, cells.p, dtot.p, derrs.p);
    }
    HIP_CHECK(hipGetLastError());
    dev_excl_scan_i64(cells.p, H->block_off.p, H->n_blocks + 1, dtot.p + 2, s);
    unsigned long long ht[3] = {0, 0, 0}, he[2] = {~0ull, ~0ull};
    PinnedDown down;
    down.add(dtot.p, ht, 3);
    down.add(derrs.p, he, 2);
    down.run(s);
    if (he[0] != ~0ull || he[1] != ~0ull) {
        if (he[0] < he[1]) HH_THROW(HH_ERR_ARG, "bin id outside [0, 2^31) at pixel " + std::to_string(he[0]));
        HH_THROW(HH_ERR_ARG, "counts must be non-negative integers at pixel " + std::to_string(he[1]));
    }
    H->kept_total = (int64_t)ht[0];
    H->max_count = (int64_t)ht[1];
    H->out_nnz = (int64_t)ht[2];
    // the counts are not read again: the write pass needs the ids and `kept` only
    H->own[2].release();
    *out_nnz = H->out_nnz;
    *kept_total = H->kept_total;
    *max_count = H->max_count;
    *out = H.release();
}

template <class Cnt>
static void sample_write_t(const hh_sample& H, int32_t* o1, int32_t* o2, void* oc, int out64, hipStream_t s) {
    HH_KTIME("k_sa_write", s);
    if (out64)
        hipLaunchKernelGGL((k_sa_write<Cnt, int64_t>), dim3((unsigned)H.n_blocks), dim3(kSaBlock), 0, s, H.b1, H.b2,
                           (const Cnt*)H.kept.p, (long long)H.nnz, (const long long*)H.block_off.p,
                           (long long)H.out_nnz, o1, o2, (int64_t*)oc);
    else
        hipLaunchKernelGGL((k_sa_write<Cnt, int32_t>), dim3((unsigned)H.n_blocks), dim3(kSaBlock), 0, s, H.b1, H.b2,
                           (const Cnt*)H.kept.p, (long long)H.nnz, (const long long*)H.block_off.p,
                           (long long)H.out_nnz, o1, o2, (int32_t*)oc);
}

// device outputs o1 / o2 / oc of out_nnz entries
static void sample_write(const hh_sample& H, int32_t* o1, int32_t* o2, void* oc, int out64, hipStream_t s) {
    HH_REQUIRE(out64 || H.max_count <= 2147483647ll, "the largest kept count needs int64 counts (max_count)");
    if (H.out_nnz == 0) return;
    HH_REQUIRE(o1 && o2 && oc, "null output arrays");
    SyncOnExit sync{s};
    if (H.cnt64) sample_write_t<int64_t>(H, o1, o2, oc, out64, s);
    else sample_write_t<int32_t>(H, o1, o2, oc, out64, s);
    HIP_CHECK(hipGetLastError());
}

}  // namespace hh

using namespace hh;

extern "C" {

int hh_sample_count(const int32_t* bin1, const int32_t* bin2, const void* count, int32_t count_is_i64, int64_t nnz,
                    uint64_t thr, uint64_t seed, int32_t on_device, void* stream, hh_sample** out, int64_t* out_nnz,
                    int64_t* kept_total, int64_t* max_count) {
    return guard([&] {
        sample_create(bin1, bin2, count, count_is_i64 ? 1 : 0, nnz, thr, seed, 0, on_device, as_stream(stream), out,
                      out_nnz, kept_total, max_count);
    });
}

int hh_sample_count_host(const int64_t* bin1, const int64_t* bin2, const int64_t* count, int64_t nnz, uint64_t thr,
                         uint64_t seed, void* stream, hh_sample** out, int64_t* out_nnz, int64_t* kept_total,
                         int64_t* max_count) {
    return guard([&] {
        sample_create(bin1, bin2, count, 1, nnz, thr, seed, 1, 0, as_stream(stream), out, out_nnz, kept_total,
                      max_count);
    });
}

int hh_sample_write(const hh_sample* h, int32_t* out_bin1, int32_t* out_bin2, void* out_count, int32_t count_is_i64,
                    void* stream) {
    return guard([&] {
        HH_REQUIRE(h, "null handle");
        DeviceScope dev(h->device);
        sample_write(*h, out_bin1, out_bin2, out_count, count_is_i64 ? 1 : 0, as_stream(stream));
    });
}

int hh_sample_write_host(const hh_sample* h, int64_t* out_bin1, int64_t* out_bin2, void* out_count,
                         int32_t count_is_i64, void* stream) {
    return guard([&] {
        HH_REQUIRE(h, "null handle");
        DeviceScope dev(h->device);
        hipStream_t s = as_stream(stream);
        const size_t n = (size_t)h->out_nnz, cw = count_is_i64 ? 8 : 4;
        HH_REQUIRE(n == 0 || (out_bin1 && out_bin2 && out_count), "null output arrays");
        DBuf<int32_t> d1(n), d2(n);
        DBuf<char> dc(n * cw);
        sample_write(*h, d1.p, d2.p, dc.p, count_is_i64 ? 1 : 0, s);
        if (n == 0) return;
        std::vector<int32_t> h1(n), h2(n);
        d1.download(h1.data(), n, s);
        d2.download(h2.data(), n, s);
        dc.download((char*)out_count, n * cw, s);
        HIP_CHECK(hipStreamSynchronize(s));
        for (size_t i = 0; i < n; ++i) {
            out_bin1[i] = h1[i];
            out_bin2[i] = h2[i];
        }
    });
}

int hh_sample_free(hh_sample* h) {
    return guard([&] {
        if (!h) return;
        device_quiesce(h->device);
        delete h;
    });
}

}  // extern "C"
