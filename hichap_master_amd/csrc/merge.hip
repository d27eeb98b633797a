// cooler's `merge` on cooler's own pixel tables: the union of
// K <= 64 tables over one bin table, counts summed exactly.
//
// Merging is coarsening by 1 over several tables, and the walk is coarsen.hip's
// with "fine row of one table" replaced by "row I of table t": no key is
// sorted, every table is sorted by (bin1, bin2), so row I of table t is one
// contiguous pixel range with non-decreasing columns.
//
//   k_co_rowptr  rp_t[f] = first pixel of row f of table t (table_walk.hpp).
//   k_mg_seg     seg_t[f][J] = first pixel of row f of table t whose column is
//                in column tile J or later (tiles of T columns; T is
//                hh_tune "coarsen_tile").  One thread per (t, f, J).
//   k_mg_item    one block per work item (row I, column tile J >= the tile of
//                I): the <= K segments [seg_t[I][J], seg_t[I][J + 1]) are
//                walked as one flat range, kCoBlock pixels per trip; counts
//                are added into T int64 cells in LDS (ds_add_u64), then the
//                touched cells are compacted in column order.  COUNT mode
//                stores the item's cell count and the largest sum and checks
//                every pixel it reads; WRITE mode writes the cells at the
//                item's offset (exclusive scan of the cell counts).  Items are
//                in (I, J) order: the output is sorted by construction and
//                bitwise the same on every run and for every order of the
//                tables (integer adds commute).
//
// Validation rides on the count pass, per table, by the argument of
// coarsen.hip (the chain seg_t[f][g] .. seg_t[f][nJ] covers every pixel of
// table t, and the item of a step checks the pixel against the step): the
// tables that fail set their bit of a 64-bit mask, and only the first of them
// is read once more (k_co_check) to name its first offending pixel.  Every
// index is a bisection result inside [0, nnz_t]: a malformed table is never
// read out of range.
#include "table_walk.hpp"

namespace hh {

struct MgTable {
    const int32_t *b1, *b2;
    const void* cnt;
    const long long* seg;  // n_bins x (nJ + 1)
    long long nnz;
    int cnt64, pad_;
};

struct MgGeom {
    const MgTable* tab;  // K (device)
    long long n_bins;
    int K, T, nJ;
};

__global__ __launch_bounds__(256) void k_mg_seg(MgGeom G, const long long* __restrict__ rp,  // K x (n_bins + 1)
                                                long long* __restrict__ seg) {              // K x n_bins x (nJ + 1)
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = G.nJ + 1, per = G.n_bins * stride;
    if (t >= per * G.K) return;
    const int k = (int)(t / per);
    const long long r = t - k * per;
    const long long f = r / stride;
    const int J = (int)(r - f * stride);
    const long long* rpk = rp + (long long)k * (G.n_bins + 1);
    const int32_t* __restrict__ b2 = G.tab[k].b2;
    long long a = rpk[f], b = rpk[f + 1];
    if (J == G.nJ) a = b;
    else if (J > f / G.T) {  // tiles up to the row's own start at the row's first pixel
        const long long target = (long long)J * G.T;
        while (a < b) {
            const long long m = a + ((b - a) >> 1);
            if ((long long)b2[m] < target) a = m + 1; else b = m;
        }
    }
    seg[t] = a;
}

template <class OutCnt, bool WRITE>
__global__ __launch_bounds__(kCoBlock) void k_mg_item(MgGeom G,
                                                      long long* __restrict__ cells,  // COUNT: per item, out
                                                      const long long* __restrict__ item_off,  // WRITE: per item
                                                      long long out_nnz, int32_t* __restrict__ o1,
                                                      int32_t* __restrict__ o2, OutCnt* __restrict__ oc,
                                                      unsigned long long* __restrict__ maxc,
                                                      unsigned long long* __restrict__ err) {  // bit t: table t failed
    __shared__ unsigned long long acc[HH_COARSEN_TILE];
    __shared__ unsigned int zbit[HH_COARSEN_TILE / 32];  // cells touched by a pixel of count 0
    __shared__ long long pre[kCoRows + 1], sstart[kCoRows];
    __shared__ int wsum[kCoBlock / 64];
    __shared__ unsigned long long wmax[kCoBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

    // item = I nJ + J -> (row I, column tile J); tiles left of the row's own hold nothing
    // (their cell counts stay at the memset's 0)
    const long long item = blockIdx.x;
    const long long I = item / G.nJ;
    const int J = (int)(item - I * G.nJ);
    if (J < I / G.T) return;
    const long long col0 = (long long)J * G.T;
    const int Tw = (int)min((long long)G.T, G.n_bins - col0);
    const long long lo = max(col0, I), hi = col0 + Tw;
    const long long at = I * (G.nJ + 1) + J;

    if (wid == 0) {  // the tables' segments of this item and the exclusive scan of their lengths
        long long s = 0, len = 0;
        if (lane < G.K) {
            const long long* __restrict__ seg = G.tab[lane].seg;
            s = seg[at];
            len = max(seg[at + 1] - s, 0ll);
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
    if (tot == 0) {  // no pixel: no cell
        if (!WRITE && tid == 0) cells[item] = 0;
        return;
    }
    for (int q = tid; q < Tw; q += kCoBlock) acc[q] = 0ull;
    for (int q = tid; q < (Tw + 31) / 32; q += kCoBlock) zbit[q] = 0u;
    __syncthreads();
    unsigned long long bad = 0ull;
    for (long long q = tid; q < tot; q += kCoBlock) {  // one trip: kCoBlock pixels
        int a = 0, b = G.K;  // table a: pre[a] <= q < pre[a + 1]
        while (b - a > 1) {
            const int m = (a + b) >> 1;
            if (pre[m] <= q) a = m; else b = m;
        }
        const MgTable& Tb = G.tab[a];
        const long long p = sstart[a] + (q - pre[a]);
        const long long c2 = (long long)Tb.b2[p];
        const long long v = Tb.cnt64 ? (long long)((const int64_t*)Tb.cnt)[p] : (long long)((const int32_t*)Tb.cnt)[p];
        if (!WRITE) {
            if ((long long)Tb.b1[p] != I || v < 0) bad |= 1ull << a;
            if (q + 1 < pre[a + 1] && (long long)Tb.b2[p + 1] <= c2) bad |= 1ull << a;
        }
        if (c2 < lo || c2 >= hi) { bad |= 1ull << a; continue; }
        const unsigned cell = (unsigned)(c2 - col0);
        atomicAdd(&acc[cell], (unsigned long long)v);
        if (v == 0) atomicOr(&zbit[cell >> 5], 1u << (cell & 31));
    }
    if (bad) atomicOr(err, bad);
    __syncthreads();

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
            // one atomic per item at most, and only while it can still raise the maximum (coarsen.hip)
            for (int w = 0; w < kCoBlock / 64; ++w) mx = max(mx, wmax[w]);
            if (mx > __hip_atomic_load(maxc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(maxc, mx);
        }
    } else {
        long long pos = item_off[item] + base + x - n;
        for (int q = q0; q < q1; ++q) {
            const unsigned long long a = acc[q];
            if (a != 0ull || ((zbit[q >> 5] >> (q & 31)) & 1u)) {
                if (pos < out_nnz) {  // (holds unless a table changed since the count pass)
                    o1[pos] = (int32_t)I;
                    o2[pos] = (int32_t)(col0 + q);
                    oc[pos] = (OutCnt)a;
                } else {
                    atomicOr(err, 1ull);
                }
                ++pos;
            }
        }
    }
}

}  // namespace hh

struct hh_merge {
    int device = 0;
    int32_t K = 0, T = 0, nJ = 0;
    int64_t n_bins = 0, n_items = 0, out_nnz = 0, max_count = 0;
    std::vector<hh::MgTable> tab;     // host copy (device pointers)
    std::vector<hh::DBuf<char>> own;  // uploads of host tables (3 per table)
    hh::DBuf<hh::MgTable> dtab;
    hh::DBuf<long long> seg, item_off;
    hh::MgGeom geom() const { return hh::MgGeom{dtab.p, (long long)n_bins, K, T, nJ}; }
};

namespace hh {

static void merge_count(hh_merge& H, hipStream_t s) {
    const int64_t n_bins = H.n_bins;
    const int K = H.K;
    const int64_t per = n_bins * (H.nJ + 1);
    H.seg.alloc((size_t)per * K);
    H.item_off.alloc(H.n_items + 1);
    for (int t = 0; t < K; ++t) H.tab[t].seg = H.seg.p + (size_t)per * t;
    H.dtab = to_device(H.tab, s);
    DBuf<long long> rp((size_t)(n_bins + 1) * K), cells(H.n_items + 1);
    DBuf<unsigned long long> dmax(3);  // largest sum, number of merged pixels, mask of the tables that failed
    SyncOnExit sync{s};  // (destroyed before the buffers above)
    dmax.zero(s);
    cells.zero(s);
    {
        HH_KTIME("k_mg_rowptr", s);
        for (int t = 0; t < K; ++t)
            hipLaunchKernelGGL(k_co_rowptr<int32_t>, dim3((unsigned)((n_bins + 1 + 255) / 256)), dim3(256), 0, s,
                               H.tab[t].b1, (long long)H.tab[t].nnz, (long long)n_bins,
                               rp.p + (size_t)(n_bins + 1) * t);
    }
    const MgGeom G = H.geom();
    {
        HH_KTIME("k_mg_seg", s);
        const int64_t n = per * K;
        hipLaunchKernelGGL(k_mg_seg, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, G, rp.p, H.seg.p);
    }
    {
        HH_KTIME("k_mg_count", s);
        hipLaunchKernelGGL((k_mg_item<int32_t, false>), dim3((unsigned)H.n_items), dim3(kCoBlock), 0, s, G, cells.p,
                           (const long long*)nullptr, 0ll, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr,
                           dmax.p, dmax.p + 2);
    }
    HIP_CHECK(hipGetLastError());
    dev_excl_scan_i64(cells.p, H.item_off.p, H.n_items + 1, dmax.p + 1, s);
    unsigned long long h[3] = {0, 0, 0};
    PinnedDown down;
    down.add(dmax.p, h, 3);
    down.run(s);
    if (h[2]) {
        int t = 0;
        while (!((h[2] >> t) & 1ull)) ++t;
        const MgTable& B = H.tab[t];
        const std::string msg = B.cnt64 ? first_bad_pixel(B.b1, B.b2, (const int64_t*)B.cnt, B.nnz, n_bins, s)
                                        : first_bad_pixel(B.b1, B.b2, (const int32_t*)B.cnt, B.nnz, n_bins, s);
        HH_THROW(HH_ERR_ARG, "table " + std::to_string(t) + ": " + msg);
    }
    H.max_count = (int64_t)h[0];
    H.out_nnz = (int64_t)h[1];
}

// device outputs o1 / o2 / oc of out_nnz entries
static void merge_write(const hh_merge& H, int32_t* o1, int32_t* o2, void* oc, int out64, hipStream_t s) {
    HH_REQUIRE(out64 || H.max_count <= 2147483647ll, "the largest merged count needs int64 counts (max_count)");
    if (H.out_nnz == 0) return;
    HH_REQUIRE(o1 && o2 && oc, "null output arrays");
    DBuf<unsigned long long> derr(1);
    SyncOnExit sync{s};
    derr.zero(s);
    {
        HH_KTIME("k_mg_write", s);
        if (out64)
            hipLaunchKernelGGL((k_mg_item<int64_t, true>), dim3((unsigned)H.n_items), dim3(kCoBlock), 0, s, H.geom(),
                               (long long*)nullptr, (const long long*)H.item_off.p, (long long)H.out_nnz, o1, o2,
                               (int64_t*)oc, (unsigned long long*)nullptr, derr.p);
        else
            hipLaunchKernelGGL((k_mg_item<int32_t, true>), dim3((unsigned)H.n_items), dim3(kCoBlock), 0, s, H.geom(),
                               (long long*)nullptr, (const long long*)H.item_off.p, (long long)H.out_nnz, o1, o2,
                               (int32_t*)oc, (unsigned long long*)nullptr, derr.p);
    }
    HIP_CHECK(hipGetLastError());
    unsigned long long herr = 0;
    PinnedDown down;
    down.add(derr.p, &herr, 1);
    down.run(s);
    if (herr) HH_THROW(HH_ERR_STATE, "a pixel table changed between hh_merge_count and hh_merge_write");
}

// host64: host tables with int64 ids and counts (cooler's); their ids are
// narrowed on the way up, an id that int32 cannot hold becoming -1, which the
// count pass reports as out of range at that pixel
static void merge_create(const void* const* bin1, const void* const* bin2, const void* const* count,
                         const int32_t* count_is_i64, const int64_t* nnz, int32_t K, int64_t n_bins, int host64,
                         int on_device, hipStream_t s, hh_merge** out, int64_t* out_nnz, int64_t* max_count) {
    HH_REQUIRE(out && out_nnz && max_count, "null arguments");
    HH_REQUIRE(K >= 1 && K <= kCoRows, "n_tables outside [1, 64]");
    HH_REQUIRE(bin1 && bin2 && count && nnz && (host64 || count_is_i64), "null table arrays");
    HH_REQUIRE(n_bins >= 1 && n_bins <= kMaxBins, "n_bins outside [1, 2^30]");
    for (int t = 0; t < K; ++t)
        HH_REQUIRE(nnz[t] >= 0 && (nnz[t] == 0 || (bin1[t] && bin2[t] && count[t])),
                   "table " + std::to_string(t) + ": null pixel arrays");
    auto H = std::make_unique<hh_merge>();
    SyncOnExit sync{s};  // (destroyed before H)
    HIP_CHECK(hipGetDevice(&H->device));
    H->K = K;
    H->n_bins = n_bins;
    H->T = (int32_t)g_coarsen_tile;
    H->nJ = (int32_t)((n_bins + H->T - 1) / H->T);
    H->n_items = n_bins * H->nJ;  // item I nJ + J; those left of the row's own tile return at once
    HH_REQUIRE(H->n_items < (int64_t(1) << 31), "too many (row, column tile) work items");
    // The segment table is 8 B per (table, row, column tile): 1.5 GB for four 10 kb genomes (607 282 bins, 75
    // tiles).  This bound only keeps the index products far inside int64; memory runs out long before it (2^36
    // segments are 512 GiB), and then the allocation in merge_count fails with HH_ERR_OOM and no handle is made.
    HH_REQUIRE(n_bins * (H->nJ + 1) * K < (int64_t(1) << 36), "too many (table, row, column tile) segments");
    H->tab.resize(K);
    H->own.resize((size_t)3 * K);
    std::vector<int32_t> narrow;
    for (int t = 0; t < K; ++t) {
        MgTable& B = H->tab[t];
        B.nnz = nnz[t];
        B.cnt64 = host64 || count_is_i64[t] ? 1 : 0;
        B.pad_ = 0;
        B.seg = nullptr;
        const void* src[3] = {bin1[t], bin2[t], count[t]};
        if (!on_device && nnz[t] > 0) {
            const size_t n = (size_t)nnz[t];
            for (int q = 0; q < 3; ++q) {
                DBuf<char>& d = H->own[(size_t)3 * t + q];
                if (host64 && q < 2) {
                    const int64_t* id = (const int64_t*)src[q];
                    narrow.resize(n);
                    for (size_t i = 0; i < n; ++i)
                        narrow[i] = (id[i] < 0 || id[i] > 2147483647ll) ? -1 : (int32_t)id[i];
                    d.alloc(n * 4);
                    upload_pinned_sync((char*)d.p, (const char*)narrow.data(), n * 4, s);  // `narrow` is reused
                } else {
                    const size_t w = (q < 2) ? 4u : (B.cnt64 ? 8u : 4u);
                    d.alloc(n * w);
                    d.upload((const char*)src[q], n * w, s);
                }
                src[q] = d.p;
            }
        }
        B.b1 = (const int32_t*)src[0];
        B.b2 = (const int32_t*)src[1];
        B.cnt = src[2];
    }
    merge_count(*H, s);
    *out_nnz = H->out_nnz;
    *max_count = H->max_count;
    *out = H.release();
}

}  // namespace hh

using namespace hh;

extern "C" {

int hh_merge_count(const int32_t* const* bin1, const int32_t* const* bin2, const void* const* count,
                   const int32_t* count_is_i64, const int64_t* nnz, int32_t n_tables, int64_t n_bins,
                   int32_t on_device, void* stream, hh_merge** out, int64_t* out_nnz, int64_t* max_count) {
    return guard([&] {
        merge_create((const void* const*)bin1, (const void* const*)bin2, count, count_is_i64, nnz, n_tables, n_bins,
                     0, on_device, as_stream(stream), out, out_nnz, max_count);
    });
}

int hh_merge_count_host(const int64_t* const* bin1, const int64_t* const* bin2, const int64_t* const* count,
                        const int64_t* nnz, int32_t n_tables, int64_t n_bins, void* stream, hh_merge** out,
                        int64_t* out_nnz, int64_t* max_count) {
    return guard([&] {
        merge_create((const void* const*)bin1, (const void* const*)bin2, (const void* const*)count, nullptr, nnz,
                     n_tables, n_bins, 1, 0, as_stream(stream), out, out_nnz, max_count);
    });
}

int hh_merge_write(const hh_merge* h, int32_t* out_bin1, int32_t* out_bin2, void* out_count, int32_t count_is_i64,
                   void* stream) {
    return guard([&] {
        HH_REQUIRE(h, "null handle");
        DeviceScope dev(h->device);
        merge_write(*h, out_bin1, out_bin2, out_count, count_is_i64 ? 1 : 0, as_stream(stream));
    });
}

int hh_merge_write_host(const hh_merge* h, int64_t* out_bin1, int64_t* out_bin2, void* out_count,
                        int32_t count_is_i64, void* stream) {
    return guard([&] {
        HH_REQUIRE(h, "null handle");
        DeviceScope dev(h->device);
        hipStream_t s = as_stream(stream);
        const size_t n = (size_t)h->out_nnz, cw = count_is_i64 ? 8 : 4;
        HH_REQUIRE(n == 0 || (out_bin1 && out_bin2 && out_count), "null output arrays");
        DBuf<int32_t> d1(n), d2(n);
        DBuf<char> dc(n * cw);
        merge_write(*h, d1.p, d2.p, dc.p, count_is_i64 ? 1 : 0, s);
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

int hh_merge_free(hh_merge* h) {
    return guard([&] {
        if (!h) return;
        device_quiesce(h->device);
        delete h;
    });
}

}  // extern "C"
