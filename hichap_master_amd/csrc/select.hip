// Diagonal rank of called pixels from cooler's pixel table: the numeric core
// of StructureFind.Loop_Selecting (HiCHap/StructureFind.py:2063-2094).
//
// The reference copies diagonal d = c - r of the dense raw matrix, sorts it
// and takes bisect_left(diagonal, M[r][c]).  Diagonal d has N - d entries and
// all but its stored pixels are zero, so for a raw count IF > 0
//     bisect_left = (N - d - nnz_d) + #{pixels on d with count < IF}
// and 0 for IF = 0: integer compares over the pixel table, no N x N matrix.
//
// One call = two passes over the pixels (one thread per pixel, grid-stride):
//   k_rank_lookup  value[q] = count of the pixel at (qrow, qcol).  dmap[d]
//                  names the group of queried diagonal d (-1: not queried);
//                  the pixel binary-searches its row among the group's sorted
//                  distinct query rows.  Unique pixels: one writer per slot.
//                  Also raises the error flags (negative count, bin1 > bin2).
//   k_rank_count   per queried diagonal the host sorts the distinct positive
//                  values into thresholds t_0 < ... < t_{m-1}; a pixel with
//                  count c bumps bucket ub(c) = #{t_k <= c} of the m + 1
//                  buckets of its diagonal.  Then
//                      nnz_d = sum of the buckets,
//                      #{count < t_k} = buckets 0 .. k (a prefix sum, host).
//   Buckets are integer counters bumped with integer atomics, so the result
//   does not depend on the order of the adds.  A diagonal's buckets live in
//   LDS (uint32 per block, flushed once per block) while they fit in what is
//   left of the block's LDS bucket budget (hh_tune "rank_lds_buckets", default
//   8192 = 32 KiB), in global memory (uint64 atomics) otherwise; diagonals are
//   packed in ascending order, LDS diagonals first in the bucket array so an
//   LDS slot and its global bucket share one index.
#include "pixel_table.hpp"

namespace hh {

constexpr int kRankBlock = 256;
constexpr int kRankMaxLds = 8192;  // uint32 LDS buckets per block at most (32 KiB)

// chromosome-local (i, j) of a pixel; false when either end is outside
__device__ __forceinline__ bool rank_local(long long p, long long q, long long lo, long long N, long long& i,
                                           long long& j) {
    i = p - lo;
    j = q - lo;
    return i >= 0 && i < N && j >= 0 && j < N;
}

__global__ __launch_bounds__(kRankBlock) void k_rank_lookup(
    const int64_t* __restrict__ b1, const int64_t* __restrict__ b2, const int64_t* __restrict__ cnt, long long nnz,
    long long lo, long long N, const int32_t* __restrict__ dmap, const int32_t* __restrict__ uoff,
    const int32_t* __restrict__ urow, long long* __restrict__ uval, unsigned int* __restrict__ flags) {
    unsigned int bad = 0;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < nnz;
         t += (long long)gridDim.x * blockDim.x) {
        long long i, j;
        if (!rank_local(b1[t], b2[t], lo, N, i, j)) continue;
        const long long c = cnt[t];
        if (c < 0) bad |= 1u;
        if (i > j) { bad |= 2u; continue; }
        const int g = dmap[j - i];
        if (g < 0) continue;
        int a = uoff[g], b = uoff[g + 1];  // first row >= i in urow[a, b)
        const int end = b;
        while (a < b) {
            const int mid = a + ((b - a) >> 1);
            if (urow[mid] < i) a = mid + 1; else b = mid;
        }
        if (a < end && urow[a] == i) uval[a] = c;
    }
    if (bad) atomicOr(flags, bad);
}

__global__ __launch_bounds__(kRankBlock) void k_rank_count(
    const int64_t* __restrict__ b1, const int64_t* __restrict__ b2, const int64_t* __restrict__ cnt, long long nnz,
    long long lo, long long N, const int32_t* __restrict__ dmap, const int32_t* __restrict__ toff,
    const int32_t* __restrict__ boff, const long long* __restrict__ thr, int n_lds,
    unsigned long long* __restrict__ buckets) {
    extern __shared__ unsigned int sh_bucket[];
    for (int s = threadIdx.x; s < n_lds; s += blockDim.x) sh_bucket[s] = 0u;
    __syncthreads();
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < nnz;
         t += (long long)gridDim.x * blockDim.x) {
        long long i, j;
        if (!rank_local(b1[t], b2[t], lo, N, i, j) || i > j) continue;
        const int g = dmap[j - i];
        if (g < 0) continue;
        const long long c = cnt[t];
        const int t0 = toff[g];
        int a = t0, b = toff[g + 1];  // first threshold > c in thr[a, b)
        while (a < b) {
            const int mid = a + ((b - a) >> 1);
            if (thr[mid] <= c) a = mid + 1; else b = mid;
        }
        const int slot = boff[g] + (a - t0);
        if (slot < n_lds) atomicAdd(&sh_bucket[slot], 1u);
        else atomicAdd(&buckets[slot], 1ull);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < n_lds; s += blockDim.x) {
        const unsigned int v = sh_bucket[s];
        if (v) atomicAdd(&buckets[s], (unsigned long long)v);
    }
}

}  // namespace hh

using namespace hh;

extern "C" int hh_diag_rank_pixels(const int64_t* bin1, const int64_t* bin2, const int64_t* count, int64_t nnz,
                                   int64_t lo, int64_t N, const int32_t* qrow, const int32_t* qcol, int64_t nq,
                                   int64_t* value, int64_t* less, int32_t on_device, void* stream) {
    return guard([&] {
        HH_REQUIRE(nq >= 0 && N > 0, "bad arguments");
        HH_REQUIRE(N < (int64_t(1) << 31) && nq < (int64_t(1) << 30), "chromosome or query list too large");
        check_pixel_table(bin1, bin2, count, nnz, nullptr, 0, lo, N);
        HH_REQUIRE(nq == 0 || (qrow && qcol && value && less), "null query arrays");
        for (int64_t q = 0; q < nq; ++q)
            if (!(qrow[q] >= 0 && qrow[q] <= qcol[q] && qcol[q] < N))
                HH_THROW(HH_ERR_ARG, "query " + std::to_string(q) + " (" + std::to_string(qrow[q]) + ", " +
                                         std::to_string(qcol[q]) + ") outside 0 <= row <= col < " + std::to_string(N));
        hipStream_t s = as_stream(stream);

        // distinct queries sorted by (diagonal, row); group g = one queried diagonal
        std::vector<int32_t> order(nq);
        for (int64_t q = 0; q < nq; ++q) order[q] = (int32_t)q;
        auto key = [&](int32_t q) { return std::make_pair(qcol[q] - qrow[q], qrow[q]); };
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key(a) < key(b); });
        std::vector<int32_t> uidx(nq), urow, gdiag, uoff;  // query -> distinct slot; slot rows; diagonals; slots of g
        for (int64_t k = 0; k < nq; ++k) {
            const int32_t q = order[k];
            const int32_t d = qcol[q] - qrow[q];
            if (k == 0 || key(order[k - 1]) != key(q)) {
                if (gdiag.empty() || gdiag.back() != d) {
                    gdiag.push_back(d);
                    uoff.push_back((int32_t)urow.size());
                }
                urow.push_back(qrow[q]);
            }
            uidx[q] = (int32_t)urow.size() - 1;
        }
        uoff.push_back((int32_t)urow.size());
        const int ng = (int)gdiag.size();
        const size_t nu = urow.size();

        PixStage<int64_t> St;  // pixel table on the device
        St.init(bin1, bin2, count, nnz, nullptr, lo, N, nullptr, 0, on_device, s);
        const int64_t *p1 = St.X.b1, *p2 = St.X.b2, *pc = St.X.cnt;
        std::vector<int32_t> dmap(N, -1);
        for (int g = 0; g < ng; ++g) dmap[gdiag[g]] = g;
        DBuf<int32_t> ddmap = to_device(dmap, s), duoff = to_device(uoff, s);
        DBuf<int32_t> durow(std::max<size_t>(nu, 1));
        durow.upload(urow.data(), nu, s);
        DBuf<long long> duval(std::max<size_t>(nu, 1));
        duval.zero(s);
        DBuf<unsigned int> dflags(1);
        dflags.zero(s);
        const unsigned grid = (unsigned)std::min<int64_t>((nnz + kRankBlock - 1) / kRankBlock, 2048);
        std::vector<long long> uval(nu, 0);
        unsigned int flags = 0;
        if (nnz > 0) {
            HH_KTIME("k_rank_lookup", s);
            hipLaunchKernelGGL(k_rank_lookup, dim3(grid), dim3(kRankBlock), 0, s, p1, p2, pc, (long long)nnz,
                               (long long)lo, (long long)N, ddmap.p, duoff.p, durow.p, duval.p, dflags.p);
        }
        HIP_CHECK(hipGetLastError());
        duval.download(uval.data(), nu, s);
        dflags.download(&flags, 1, s);
        HIP_CHECK(hipStreamSynchronize(s));
        HH_REQUIRE(!(flags & 1u), "negative count in the chromosome's pixels");
        HH_REQUIRE(!(flags & 2u), "bin1 > bin2 in the chromosome's pixels (upper-triangle pixels expected)");

        // thresholds: per diagonal the sorted distinct positive values; bucket layout
        std::vector<long long> thr;
        std::vector<int32_t> toff(ng + 1, 0), boff(ng, 0), utix(nu, -1);
        for (int g = 0; g < ng; ++g) {
            toff[g] = (int32_t)thr.size();
            std::vector<long long> v;
            for (int32_t u = uoff[g]; u < uoff[g + 1]; ++u)
                if (uval[u] > 0) v.push_back(uval[u]);
            std::sort(v.begin(), v.end());
            v.erase(std::unique(v.begin(), v.end()), v.end());
            for (int32_t u = uoff[g]; u < uoff[g + 1]; ++u)
                if (uval[u] > 0) utix[u] = (int32_t)(std::lower_bound(v.begin(), v.end(), uval[u]) - v.begin());
            thr.insert(thr.end(), v.begin(), v.end());
        }
        toff[ng] = (int32_t)thr.size();
        const int lds_cap = std::min<int>(std::max<int>(g_rank_lds_buckets, 0), kRankMaxLds);
        int n_lds = 0;
        std::vector<char> in_lds(ng, 0);
        for (int g = 0; g < ng; ++g) {  // a diagonal's m + 1 buckets go to LDS while they fit
            const int nb = toff[g + 1] - toff[g] + 1;
            if (n_lds + nb <= lds_cap) { boff[g] = n_lds; n_lds += nb; in_lds[g] = 1; }
        }
        int n_buckets = n_lds;
        for (int g = 0; g < ng; ++g)
            if (!in_lds[g]) { boff[g] = n_buckets; n_buckets += toff[g + 1] - toff[g] + 1; }
        std::vector<unsigned long long> buckets(n_buckets, 0);
        if (nnz > 0 && ng > 0) {
            DBuf<long long> dthr(std::max<size_t>(thr.size(), 1));
            dthr.upload(thr.data(), thr.size(), s);
            DBuf<int32_t> dtoff = to_device(toff, s), dboff = to_device(boff, s);
            DBuf<unsigned long long> dbk(n_buckets);
            dbk.zero(s);
            {
                HH_KTIME("k_rank_count", s);
                hipLaunchKernelGGL(k_rank_count, dim3(grid), dim3(kRankBlock), sizeof(unsigned int) * (size_t)n_lds,
                                   s, p1, p2, pc, (long long)nnz, (long long)lo, (long long)N, ddmap.p, dtoff.p,
                                   dboff.p, dthr.p, n_lds, dbk.p);
            }
            HIP_CHECK(hipGetLastError());
            dbk.download(buckets.data(), n_buckets, s);
            HIP_CHECK(hipStreamSynchronize(s));
        }

        // per-diagonal prefix sums: less of threshold k = zeros + buckets 0 .. k
        std::vector<long long> tless(thr.size(), 0);
        for (int g = 0; g < ng; ++g) {
            const int m = toff[g + 1] - toff[g];
            long long nnz_d = 0;
            for (int k = 0; k <= m; ++k) nnz_d += (long long)buckets[boff[g] + k];
            long long run = (long long)N - gdiag[g] - nnz_d;
            for (int k = 0; k < m; ++k) {
                run += (long long)buckets[boff[g] + k];
                tless[toff[g] + k] = run;
            }
        }
        for (int64_t q = 0; q < nq; ++q) {
            const int32_t u = uidx[q];
            value[q] = uval[u];
            // group of slot u: the diagonal of the query
            const int g = dmap[qcol[q] - qrow[q]];
            less[q] = utix[u] < 0 ? 0 : tless[toff[g] + utix[u]];
        }
    });
}
