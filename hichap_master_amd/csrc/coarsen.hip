// cooler's `coarsen` on cooler's own pixel table.
//
// Fine bin i of chromosome c maps to coarse bin coff_c + (i - off_c) / k, with
// coff the running sum of ceil(nbins_c / k); a coarse pixel's count is the
// exact integer sum of the fine pixels that map to it.  No key is sorted: the
// table is sorted by (bin1, bin2), so the fine rows of one coarse row are one
// contiguous pixel range and within a fine row the coarse columns are
// non-decreasing.
//
//   k_co_map     cmap[i] = coarse bin of fine bin i (int32, L2-resident).
//   k_co_cstart  cstart[I] = first fine bin of coarse bin I.
//   k_co_rowptr  rp[f] = first pixel of fine row f (lower bound in bin1).
//   k_co_seg     seg[f][J] = first pixel of fine row f whose coarse column is
//                in column tile J or later (lower bound in bin2 inside the
//                row; tiles of T coarse columns).  One thread per (f, J): the
//                dependent loads of the searches hide behind each other.
//   k_co_item    one block per work item (coarse row I, column tile J >= the
//                tile of I): the <= k fine-row segments [seg[f][J],
//                seg[f][J + 1]) are walked as one flat range, kCoBlock pixels
//                per trip; counts are added into T int64 cells in LDS
//                (ds_add_u64; integer adds commute, so the sums do not depend
//                on the order), then the touched cells are compacted in
//                column order.  COUNT mode stores the item's cell count and
//                the largest sum and checks every pixel it reads; WRITE mode
//                writes the cells at the item's offset (exclusive scan of the
//                cell counts, dev_excl_scan_i64).  Items are in (I, J) order,
//                so the output is sorted by construction and bitwise the
//                same on every run.
//
// Validation rides on the count pass.  rp and seg are lower bounds found by
// bisection, which on ANY input returns s with key[s - 1] < target <= key[s]
// (virtual -inf / +inf past the ends); rp[0] = 0 and rp[n_bins] = nnz are
// forced.  The chain rp[f] = seg[f][g] .. seg[f][nJ] = rp[f + 1] therefore
// runs from 0 to nnz, every pixel lies in at least one forward step [seg[f][J],
// seg[f][J + 1]), and the item of that step checks bin1 == f, the column in
// tile J and >= f, the count >= 0 and the next column of the step larger.  A
// table that passes is strictly sorted upper-triangle (an out-of-order
// neighbour pair would need a step starting between them, which the bisection
// invariant excludes).  Only a table that fails is read once more
// (k_co_check) to name its first offending pixel.
#include "table_walk.hpp"  // kCoBlock, kCoRows, k_co_rowptr, first_bad_pixel, DeviceScope (shared with merge.hip)

namespace hh {


struct CoGeom {
    const int32_t* cmap;     // n_bins: coarse bin of a fine bin
    const long long* cstart; // nbc + 1: first fine bin of a coarse bin (n_bins past the last)
    const long long* seg;    // n_bins x (nJ + 1)
    long long n_bins, nbc, nnz;
    int T, nJ;
};

// chromosome holding position x of the offsets o (o[c] <= x < o[c + 1])
__device__ __forceinline__ int co_chrom(const long long* __restrict__ o, int n_chroms, long long x) {
    int a = 0, b = n_chroms;
    while (b - a > 1) {
        const int m = (a + b) >> 1;
        if (o[m] <= x) a = m; else b = m;
    }
    return a;
}

// first fine bin of coarse bin I (n_bins past the last coarse bin)
__device__ __forceinline__ long long co_fine_start(const CoGeom& G, long long I) {
    return G.cstart[min(I, G.nbc)];
}

__global__ __launch_bounds__(256) void k_co_map(const long long* __restrict__ off, const long long* __restrict__ coff,
                                                int n_chroms, long long n_bins, long long k,
                                                int32_t* __restrict__ cmap) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_bins) return;
    const int c = co_chrom(off, n_chroms, i);
    cmap[i] = (int32_t)(coff[c] + (i - off[c]) / k);
}

// every coarse bin holds at least one fine bin, so every entry is written
__global__ __launch_bounds__(256) void k_co_cstart(const int32_t* __restrict__ cmap, long long n_bins, long long nbc,
                                                   long long* __restrict__ cstart) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_bins) return;
    if (i == n_bins) cstart[nbc] = n_bins;
    else if (i == 0 || cmap[i] != cmap[i - 1]) cstart[cmap[i]] = i;
}

template <class Id>
__global__ __launch_bounds__(256) void k_co_seg(const Id* __restrict__ b2, const long long* __restrict__ rp,
                                                CoGeom G, long long* __restrict__ seg) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = G.nJ + 1;
    if (t >= G.n_bins * stride) return;
    const long long f = t / stride;
    const int J = (int)(t - f * stride);
    long long a = rp[f], b = rp[f + 1];
    if (J == G.nJ) a = b;
    else if (J > G.cmap[f] / G.T) {  // tiles up to the row's own start at the row's first pixel
        const long long target = co_fine_start(G, (long long)J * G.T);
        while (a < b) {
            const long long m = a + ((b - a) >> 1);
            if ((long long)b2[m] < target) a = m + 1; else b = m;
        }
    }
    seg[t] = a;
}

template <class Id, class Cnt, class OutCnt, bool WRITE>
__global__ __launch_bounds__(kCoBlock) void k_co_item(const Id* __restrict__ b1, const Id* __restrict__ b2,
                                                      const Cnt* __restrict__ cnt, CoGeom G,
                                                      long long* __restrict__ cells,  // COUNT: per item, out
                                                      const long long* __restrict__ item_off,  // WRITE: per item
                                                      long long out_nnz, int32_t* __restrict__ o1,
                                                      int32_t* __restrict__ o2, OutCnt* __restrict__ oc,
                                                      unsigned long long* __restrict__ maxc,
                                                      unsigned int* __restrict__ err) {
    __shared__ unsigned long long acc[HH_COARSEN_TILE];
    __shared__ unsigned int zbit[HH_COARSEN_TILE / 32];  // cells touched by a pixel of count 0
    __shared__ long long pre[kCoRows + 1], sstart[kCoRows];
    __shared__ int wsum[kCoBlock / 64];
    __shared__ unsigned long long wmax[kCoBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

    // item = I nJ + J -> (coarse row I, column tile J); tiles left of the row's own hold nothing
    // (their cell counts stay at the memset's 0).  Four independent loads give the item's geometry.
    const long long item = blockIdx.x;
    const long long I = item / G.nJ;
    const int J = (int)(item - I * G.nJ);
    if (J < I / G.T) return;
    const long long f0 = G.cstart[I], f1 = G.cstart[I + 1];
    const long long col0 = (long long)J * G.T;
    const int Tw = (int)min((long long)G.T, G.nbc - col0);
    const long long lo_f = co_fine_start(G, col0), hi_f = co_fine_start(G, col0 + G.T);
    const long long stride = G.nJ + 1;

    unsigned int bad = 0;
    bool cleared = false;
    for (long long fr = f0; fr < f1; fr += kCoRows) {
        const int nr = (int)min((long long)kCoRows, f1 - fr);
        if (wid == 0) {  // the chunk's segments and the exclusive scan of their lengths
            long long s = 0, len = 0;
            if (lane < nr) {
                s = G.seg[(fr + lane) * stride + J];
                len = max(G.seg[(fr + lane) * stride + J + 1] - s, 0ll);
            }
            long long x = len;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const long long y = __shfl_up(x, o, 64);
                if (lane >= o) x += y;
            }
            sstart[lane] = s;
            pre[lane] = x - len;
            if (lane == 63) pre[64] = x;
        }
        __syncthreads();
        const long long tot = pre[64];
        if (tot > 0) {
            if (!cleared) {
                for (int q = tid; q < Tw; q += kCoBlock) acc[q] = 0ull;
                for (int q = tid; q < (Tw + 31) / 32; q += kCoBlock) zbit[q] = 0u;
                __syncthreads();
                cleared = true;
            }
            for (long long q = tid; q < tot; q += kCoBlock) {  // one trip: kCoBlock pixels
                int a = 0, b = nr;  // row r of the chunk: pre[r] <= q < pre[r + 1]
                while (b - a > 1) {
                    const int m = (a + b) >> 1;
                    if (pre[m] <= q) a = m; else b = m;
                }
                const long long p = sstart[a] + (q - pre[a]);
                const long long f = fr + a;
                const long long c2 = (long long)b2[p];
                const long long v = (long long)cnt[p];
                if (!WRITE) {
                    if ((long long)b1[p] != f || v < 0) bad = 1u;
                    if (q + 1 < pre[a + 1] && (long long)b2[p + 1] <= c2) bad = 1u;
                }
                if (c2 < max(lo_f, f) || c2 >= hi_f) { bad = 1u; continue; }
                const unsigned cell = (unsigned)(G.cmap[c2] - col0);
                if (cell >= (unsigned)Tw) { bad = 1u; continue; }
                atomicAdd(&acc[cell], (unsigned long long)v);
                if (v == 0) atomicOr(&zbit[cell >> 5], 1u << (cell & 31));
            }
        }
        __syncthreads();
    }
    if (bad) atomicOr(err, 1u);
    if (!cleared) {  // no pixel: no cell
        if (!WRITE && tid == 0) cells[item] = 0;
        return;
    }

    // compaction in column order: thread t owns cells [t cpt, (t + 1) cpt)
    const int cpt = (Tw + kCoBlock - 1) / kCoBlock;
    const int q0 = min(tid * cpt, Tw), q1 = min(q0 + cpt, Tw);
    int n = 0;
    unsigned long long mx = 0ull;
    for (int q = q0; q < q1; ++q) {
        const unsigned long long a = acc[q];
        n += (a != 0ull || ((zbit[q >> 5] >> (q & 31)) & 1u)) ? 1 : 0;
        mx = max(mx, a);
    }
    int x = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wid] = x;
    if (!WRITE) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned long long)__shfl_xor((long long)mx, o, 64));
        if (lane == 0) wmax[wid] = mx;
    }
    __syncthreads();
    int base = 0, total = 0;
    for (int w = 0; w < kCoBlock / 64; ++w) {
        if (w < wid) base += wsum[w];
        total += wsum[w];
    }
    if (!WRITE) {
        if (tid == 0) {
            cells[item] = total;
            // one atomic per item at most, and only while it can still raise the maximum: every
            // item hitting the one word (8 waves x 1.5e6 items on the 10 kb genome) was 2/3 of the pass
            for (int w = 0; w < kCoBlock / 64; ++w) mx = max(mx, wmax[w]);
            if (mx > __hip_atomic_load(maxc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(maxc, mx);
        }
    } else {
        long long pos = item_off[item] + base + x - n;
        for (int q = q0; q < q1; ++q) {
            const unsigned long long a = acc[q];
            if (a != 0ull || ((zbit[q >> 5] >> (q & 31)) & 1u)) {
                if (pos < out_nnz) {  // (holds unless the table changed since the count pass)
                    o1[pos] = (int32_t)I;
                    o2[pos] = (int32_t)(col0 + q);
                    oc[pos] = (OutCnt)a;
                } else {
                    atomicOr(err, 1u);
                }
                ++pos;
            }
        }
    }
}

}  // namespace hh

struct hh_coarsen {
    int device = 0;
    int id64 = 0, cnt64 = 0;  // width of the source ids / counts
    const void *b1 = nullptr, *b2 = nullptr, *cnt = nullptr;  // device pointers (the caller's, or own[])
    hh::DBuf<char> own[3];    // uploads of a host table
    int64_t nnz = 0, n_bins = 0, nbc = 0, k = 1, n_items = 0, out_nnz = 0, max_count = 0;
    int32_t n_chroms = 0, T = 0, nJ = 0;
    hh::DBuf<long long> off, coff, cstart, seg, item_off;
    hh::DBuf<int32_t> cmap;
    hh::CoGeom geom() const {
        return hh::CoGeom{cmap.p, cstart.p, seg.p, (long long)n_bins, (long long)nbc, (long long)nnz, T, nJ};
    }
};

namespace hh {

template <class Id, class Cnt>
static void coarsen_count(hh_coarsen& H, hipStream_t s) {
    const Id *b1 = (const Id*)H.b1, *b2 = (const Id*)H.b2;
    const Cnt* cnt = (const Cnt*)H.cnt;
    const int64_t n_bins = H.n_bins, nnz = H.nnz;
    H.cmap.alloc(n_bins);
    H.cstart.alloc(H.nbc + 1);
    H.seg.alloc((size_t)n_bins * (H.nJ + 1));
    H.item_off.alloc(H.n_items + 1);
    DBuf<long long> rp(n_bins + 1), cells(H.n_items + 1);
    DBuf<unsigned long long> dmax(2);  // largest sum, number of coarse pixels
    DBuf<unsigned int> derr(1);
    SyncOnExit sync{s};  // (destroyed before the buffers above)
    dmax.zero(s);
    derr.zero(s);
    cells.zero(s);
    {
        HH_KTIME("k_co_map", s);
        hipLaunchKernelGGL(k_co_map, dim3((unsigned)((n_bins + 255) / 256)), dim3(256), 0, s, H.off.p, H.coff.p,
                           H.n_chroms, (long long)n_bins, (long long)H.k, H.cmap.p);
    }
    {
        HH_KTIME("k_co_cstart", s);
        hipLaunchKernelGGL(k_co_cstart, dim3((unsigned)((n_bins + 1 + 255) / 256)), dim3(256), 0, s, H.cmap.p,
                           (long long)n_bins, (long long)H.nbc, H.cstart.p);
    }
    {
        HH_KTIME("k_co_rowptr", s);
        hipLaunchKernelGGL(k_co_rowptr<Id>, dim3((unsigned)((n_bins + 1 + 255) / 256)), dim3(256), 0, s, b1,
                           (long long)nnz, (long long)n_bins, rp.p);
    }
    const CoGeom G = H.geom();
    {
        HH_KTIME("k_co_seg", s);
        const int64_t n = n_bins * (H.nJ + 1);
        hipLaunchKernelGGL(k_co_seg<Id>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, b2, rp.p, G, H.seg.p);
    }
    {
        HH_KTIME("k_co_count", s);
        hipLaunchKernelGGL((k_co_item<Id, Cnt, int32_t, false>), dim3((unsigned)H.n_items), dim3(kCoBlock), 0, s, b1,
                           b2, cnt, G, cells.p, (const long long*)nullptr, 0ll, (int32_t*)nullptr, (int32_t*)nullptr,
                           (int32_t*)nullptr, dmax.p, derr.p);
    }
    HIP_CHECK(hipGetLastError());
    dev_excl_scan_i64(cells.p, H.item_off.p, H.n_items + 1, dmax.p + 1, s);
    unsigned long long hmax[2] = {0, 0};
    unsigned int herr = 0;
    PinnedDown down;
    down.add(dmax.p, hmax, 2);
    down.add(derr.p, &herr, 1);
    down.run(s);
    if (herr) HH_THROW(HH_ERR_ARG, first_bad_pixel(b1, b2, cnt, nnz, n_bins, s));
    H.max_count = (int64_t)hmax[0];
    H.out_nnz = (int64_t)hmax[1];
}

template <class Id, class Cnt, class OutCnt>
static void coarsen_write_t(const hh_coarsen& H, int32_t* o1, int32_t* o2, OutCnt* oc, unsigned int* derr,
                            hipStream_t s) {
    HH_KTIME("k_co_write", s);
    hipLaunchKernelGGL((k_co_item<Id, Cnt, OutCnt, true>), dim3((unsigned)H.n_items), dim3(kCoBlock), 0, s,
                       (const Id*)H.b1, (const Id*)H.b2, (const Cnt*)H.cnt, H.geom(), (long long*)nullptr,
                       (const long long*)H.item_off.p, (long long)H.out_nnz, o1, o2, oc,
                       (unsigned long long*)nullptr, derr);
}

// device outputs o1 / o2 / oc of out_nnz entries
static void coarsen_write(const hh_coarsen& H, int32_t* o1, int32_t* o2, void* oc, int out64, hipStream_t s) {
    HH_REQUIRE(out64 || H.max_count <= 2147483647ll, "the largest coarse count needs int64 counts (max_count)");
    if (H.out_nnz == 0) return;
    HH_REQUIRE(o1 && o2 && oc, "null output arrays");
    DBuf<unsigned int> derr(1);
    SyncOnExit sync{s};
    derr.zero(s);
    if (H.id64) {
        if (out64) coarsen_write_t<int64_t, int64_t, int64_t>(H, o1, o2, (int64_t*)oc, derr.p, s);
        else coarsen_write_t<int64_t, int64_t, int32_t>(H, o1, o2, (int32_t*)oc, derr.p, s);
    } else if (H.cnt64) {
        if (out64) coarsen_write_t<int32_t, int64_t, int64_t>(H, o1, o2, (int64_t*)oc, derr.p, s);
        else coarsen_write_t<int32_t, int64_t, int32_t>(H, o1, o2, (int32_t*)oc, derr.p, s);
    } else {
        if (out64) coarsen_write_t<int32_t, int32_t, int64_t>(H, o1, o2, (int64_t*)oc, derr.p, s);
        else coarsen_write_t<int32_t, int32_t, int32_t>(H, o1, o2, (int32_t*)oc, derr.p, s);
    }
    HIP_CHECK(hipGetLastError());
    unsigned int herr = 0;
    PinnedDown down;
    down.add(derr.p, &herr, 1);
    down.run(s);
    if (herr) HH_THROW(HH_ERR_STATE, "the pixel table changed between hh_coarsen_count and hh_coarsen_write");
}

// the geometry of a level and the count pass; `src` = device pointers of the
// table, or host arrays (upload) with their element sizes
static void coarsen_create(const void* bin1, const void* bin2, const void* count, int id64, int cnt64, int64_t nnz,
                           int64_t n_bins, const int64_t* chrom_offsets, int32_t n_chroms, int64_t factor,
                           int on_device, hipStream_t s, hh_coarsen** out, int64_t* out_nnz, int64_t* max_count) {
    HH_REQUIRE(out && out_nnz && max_count && chrom_offsets, "null arguments");
    HH_REQUIRE(nnz >= 0 && (nnz == 0 || (bin1 && bin2 && count)), "null pixel arrays");
    HH_REQUIRE(n_chroms >= 1 && factor >= 1, "n_chroms and factor must be >= 1");
    HH_REQUIRE(n_bins >= 1 && n_bins <= kMaxBins, "n_bins outside [1, 2^30]");
    HH_REQUIRE(chrom_offsets[0] == 0 && chrom_offsets[n_chroms] == n_bins,
               "chrom_offsets must run from 0 to n_bins");
    std::vector<long long> off(n_chroms + 1), coff(n_chroms + 1, 0);
    for (int c = 0; c <= n_chroms; ++c) off[c] = chrom_offsets[c];
    for (int c = 0; c < n_chroms; ++c) {
        HH_REQUIRE(off[c + 1] >= off[c], "chrom_offsets must not decrease");
        coff[c + 1] = coff[c] + (off[c + 1] - off[c] + factor - 1) / factor;
    }
    auto H = std::make_unique<hh_coarsen>();
    SyncOnExit sync{s};  // (destroyed before H)
    HIP_CHECK(hipGetDevice(&H->device));
    H->id64 = id64;
    H->cnt64 = cnt64;
    H->nnz = nnz;
    H->n_bins = n_bins;
    H->n_chroms = n_chroms;
    H->k = factor;
    H->nbc = coff[n_chroms];
    H->T = (int32_t)g_coarsen_tile;
    H->nJ = (int32_t)((H->nbc + H->T - 1) / H->T);
    H->n_items = H->nbc * H->nJ;  // item I nJ + J; those left of the row's own tile return at once
    HH_REQUIRE(H->n_items < (int64_t(1) << 31), "too many (coarse row, column tile) work items");
    HH_REQUIRE(n_bins * (H->nJ + 1) < (int64_t(1) << 36), "too many (fine row, column tile) segments");
    H->off = to_device(off, s);
    H->coff = to_device(coff, s);
    const void* src[3] = {bin1, bin2, count};
    if (!on_device && nnz > 0) {
        const size_t w[3] = {id64 ? 8u : 4u, id64 ? 8u : 4u, cnt64 ? 8u : 4u};
        for (int q = 0; q < 3; ++q) {
            H->own[q].alloc((size_t)nnz * w[q]);
            H->own[q].upload((const char*)src[q], (size_t)nnz * w[q], s);
            src[q] = H->own[q].p;
        }
    }
    H->b1 = src[0];
    H->b2 = src[1];
    H->cnt = src[2];
    if (id64) coarsen_count<int64_t, int64_t>(*H, s);
    else if (cnt64) coarsen_count<int32_t, int64_t>(*H, s);
    else coarsen_count<int32_t, int32_t>(*H, s);
    *out_nnz = H->out_nnz;
    *max_count = H->max_count;
    *out = H.release();
}

}  // namespace hh

using namespace hh;

extern "C" {

int hh_coarsen_tile(int32_t* tile) {
    return guard([&] {
        HH_REQUIRE(tile, "null argument");
        *tile = (int32_t)g_coarsen_tile;
    });
}

int hh_coarsen_count(const int32_t* bin1, const int32_t* bin2, const void* count, int32_t count_is_i64, int64_t nnz,
                     int64_t n_bins, const int64_t* chrom_offsets, int32_t n_chroms, int64_t factor,
                     int32_t on_device, void* stream, hh_coarsen** out, int64_t* out_nnz, int64_t* max_count) {
    return guard([&] {
        coarsen_create(bin1, bin2, count, 0, count_is_i64 ? 1 : 0, nnz, n_bins, chrom_offsets, n_chroms, factor,
                       on_device, as_stream(stream), out, out_nnz, max_count);
    });
}

int hh_coarsen_count_host(const int64_t* bin1, const int64_t* bin2, const int64_t* count, int64_t nnz, int64_t n_bins,
                          const int64_t* chrom_offsets, int32_t n_chroms, int64_t factor, void* stream,
                          hh_coarsen** out, int64_t* out_nnz, int64_t* max_count) {
    return guard([&] {
        coarsen_create(bin1, bin2, count, 1, 1, nnz, n_bins, chrom_offsets, n_chroms, factor, 0, as_stream(stream),
                       out, out_nnz, max_count);
    });
}

int hh_coarsen_write(const hh_coarsen* h, int32_t* out_bin1, int32_t* out_bin2, void* out_count,
                     int32_t count_is_i64, void* stream) {
    return guard([&] {
        HH_REQUIRE(h, "null handle");
        DeviceScope dev(h->device);
        coarsen_write(*h, out_bin1, out_bin2, out_count, count_is_i64 ? 1 : 0, as_stream(stream));
    });
}

int hh_coarsen_write_host(const hh_coarsen* h, int64_t* out_bin1, int64_t* out_bin2, void* out_count,
                          int32_t count_is_i64, void* stream) {
    return guard([&] {
        HH_REQUIRE(h, "null handle");
        DeviceScope dev(h->device);
        hipStream_t s = as_stream(stream);
        const size_t n = (size_t)h->out_nnz, cw = count_is_i64 ? 8 : 4;
        HH_REQUIRE(n == 0 || (out_bin1 && out_bin2 && out_count), "null output arrays");
        DBuf<int32_t> d1(n), d2(n);
        DBuf<char> dc(n * cw);
        coarsen_write(*h, d1.p, d2.p, dc.p, count_is_i64 ? 1 : 0, s);
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

int hh_coarsen_free(hh_coarsen* h) {
    return guard([&] {
        if (!h) return;
        device_quiesce(h->device);
        delete h;
    });
}

}  // extern "C"
