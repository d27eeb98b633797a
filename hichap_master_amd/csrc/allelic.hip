// The two data-movement cores of HiCHap/AllelicSpecificity.py.
//
// hh_pixel_windows  LoopAllelicSpecificity / BoundaryAllelicSpecificity read
//   one cell per loop, or a 2*offset square per boundary, of the dense raw
//   matrix of M<chrom> / P<chrom> (matrix(balance=False).fetch, :79-80,
//   :291-292).  Here the windows are gathered from cooler's pixel table: one
//   thread per output cell lower-bounds its row in bin1, then its column in
//   bin2 inside that row (the table is sorted by (bin1, bin2)).  Every cell has
//   one writer and copies one stored count, so the result is exact and the same
//   on every run.  k_win_check raises the error flags in one pass over the
//   pixels (non-finite count, bin1 > bin2, adjacent pairs out of order).
//
// hh_pairdiff_rank  CompartmentAllelicSpecificity.BackGround (:460-485) sorts
//   the list of all a_i - b_j and Calculating bisects it per candidate
//   (:509).  less[q] = #{(i, j) : fl(a_i - b_j) < q} is that bisect_left
//   without the list: with b sorted ascending fl(a_i - b_j) is non-increasing
//   in j (rounding is monotone), so the predicate holds on a suffix of b found
//   by one binary search per (q, i); the suffix lengths are integers, summed
//   per thread, per wave, then with one integer atomic per wave.  The subtract
//   is the plain fp64 one (no fast-math in the build, nothing to contract).
#include "pixel_table.hpp"

namespace hh {

constexpr int kWinBlock = 256;
constexpr int kPdBlock = 256;
constexpr int kPdMaxLds = 8192;  // sorted b in LDS up to this many doubles (64 KiB)

__global__ __launch_bounds__(kWinBlock) void k_win_check(const int64_t* __restrict__ b1,
                                                         const int64_t* __restrict__ b2,
                                                         const double* __restrict__ cnt, long long nnz, long long lo,
                                                         long long N, unsigned int* __restrict__ flags) {
    unsigned int bad = 0;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < nnz;
         t += (long long)gridDim.x * blockDim.x) {
        const long long p = b1[t], q = b2[t];
        if (t + 1 < nnz) {
            const long long pn = b1[t + 1], qn = b2[t + 1];
            if (pn < p || (pn == p && qn <= q)) bad |= 4u;
        }
        const long long i = p - lo, j = q - lo;
        if (i < 0 || i >= N || j < 0 || j >= N) continue;
        if (!isfinite(cnt[t])) bad |= 1u;
        if (i > j) bad |= 2u;
    }
    if (bad) atomicOr(flags, bad);
}

__global__ __launch_bounds__(kWinBlock) void k_win_gather(const int64_t* __restrict__ b1,
                                                          const int64_t* __restrict__ b2,
                                                          const double* __restrict__ cnt, long long nnz, long long lo,
                                                          const int32_t* __restrict__ wrow,
                                                          const int32_t* __restrict__ wcol, int h, int w,
                                                          long long total, double* __restrict__ out) {
    const long long hw = (long long)h * w;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const long long k = t / hw, rc = t - k * hw;
        const long long i = wrow[k] + rc / w, j = wcol[k] + rc % w;
        const long long gr = lo + (i < j ? i : j), gc = lo + (i < j ? j : i);
        long long a = 0, b = nnz;  // first pixel of row gr (or of a later row)
        while (a < b) {
            const long long mid = a + ((b - a) >> 1);
            if (b1[mid] < gr) a = mid + 1; else b = mid;
        }
        b = nnz;  // inside [a, nnz) bin1 >= gr: first pixel at or after (gr, gc)
        while (a < b) {
            const long long mid = a + ((b - a) >> 1);
            if (b1[mid] == gr && b2[mid] < gc) a = mid + 1; else b = mid;
        }
        out[t] = (a < nnz && b1[a] == gr && b2[a] == gc) ? cnt[a] : 0.0;
    }
}

// blockIdx.x = query, blockIdx.y = a slice of a; bs = b sorted ascending
__global__ __launch_bounds__(kPdBlock) void k_pairdiff_rank(const double* __restrict__ a, int na,
                                                            const double* __restrict__ bs, int nb,
                                                            const double* __restrict__ q, int per_slice, int b_in_lds,
                                                            unsigned long long* __restrict__ less) {
    extern __shared__ double sh_b[];
    const double* bb = bs;
    if (b_in_lds) {
        for (int s = threadIdx.x; s < nb; s += blockDim.x) sh_b[s] = bs[s];
        __syncthreads();
        bb = sh_b;
    }
    const double qv = q[blockIdx.x];
    const int i0 = blockIdx.y * per_slice;
    const int i1 = min(i0 + per_slice, na);
    long long sum = 0;
    for (int i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
        const double ai = a[i];
        int lo = 0, hi = nb;  // first j with ai - b_j < q
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (ai - bb[mid] < qv) hi = mid; else lo = mid + 1;
        }
        sum += nb - lo;
    }
    sum = wave_sum_ll(sum);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&less[blockIdx.x], (unsigned long long)sum);
}

}  // namespace hh

using namespace hh;

extern "C" int hh_pixel_windows(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                                int64_t lo, int64_t N, const int32_t* wrow, const int32_t* wcol, int64_t nw,
                                int32_t h, int32_t w, double* out, int32_t on_device, void* stream) {
    return guard([&] {
        HH_REQUIRE(nw >= 0 && N > 0, "bad arguments");
        HH_REQUIRE(N < (int64_t(1) << 31) && nw < (int64_t(1) << 30), "chromosome or window list too large");
        HH_REQUIRE(h >= 1 && w >= 1 && h <= N && w <= N, "window shape outside 1 <= h, w <= N");
        check_pixel_table(bin1, bin2, count, nnz, nullptr, 0, lo, N);
        HH_REQUIRE(nw == 0 || (wrow && wcol && out), "null window arrays");
        for (int64_t k = 0; k < nw; ++k)
            if (!(wrow[k] >= 0 && (int64_t)wrow[k] + h <= N && wcol[k] >= 0 && (int64_t)wcol[k] + w <= N))
                HH_THROW(HH_ERR_ARG, "window " + std::to_string(k) + " at (" + std::to_string(wrow[k]) + ", " +
                                         std::to_string(wcol[k]) + ") of " + std::to_string(h) + " x " +
                                         std::to_string(w) + " leaves [0, " + std::to_string(N) + ")");
        const int64_t total = nw * (int64_t)h * w;
        HH_REQUIRE(total < (int64_t(1) << 36), "window list too large");
        hipStream_t s = as_stream(stream);

        PixStage<double> St;
        St.init(bin1, bin2, count, nnz, nullptr, lo, N, nullptr, 0, on_device, s);
        const int64_t *p1 = St.X.b1, *p2 = St.X.b2;
        const double* pc = St.X.cnt;
        DBuf<double> dout;
        double* po = out;
        if (!on_device) {
            dout.alloc(total);
            po = dout.p;
        }
        DBuf<unsigned int> dflags(1);
        dflags.zero(s);
        unsigned int flags = 0;
        if (nnz > 0) {
            const unsigned grid = (unsigned)std::min<int64_t>((nnz + kWinBlock - 1) / kWinBlock, 2048);
            HH_KTIME("k_win_check", s);
            hipLaunchKernelGGL(k_win_check, dim3(grid), dim3(kWinBlock), 0, s, p1, p2, pc, (long long)nnz,
                               (long long)lo, (long long)N, dflags.p);
        }
        HIP_CHECK(hipGetLastError());
        dflags.download(&flags, 1, s);
        HIP_CHECK(hipStreamSynchronize(s));
        HH_REQUIRE(!(flags & 2u), "bin1 > bin2 in the chromosome's pixels (upper-triangle pixels expected)");
        HH_REQUIRE(!(flags & 4u), "pixel table not sorted by (bin1, bin2) or with a repeated pixel");
        HH_REQUIRE(!(flags & 1u), "non-finite count in the chromosome's pixels");
        if (total == 0) return;

        DBuf<int32_t> dwr(nw), dwc(nw);
        dwr.upload(wrow, nw, s);
        dwc.upload(wcol, nw, s);
        {
            const unsigned grid = (unsigned)std::min<int64_t>((total + kWinBlock - 1) / kWinBlock, 1 << 20);
            HH_KTIME("k_win_gather", s);
            hipLaunchKernelGGL(k_win_gather, dim3(grid), dim3(kWinBlock), 0, s, p1, p2, pc, (long long)nnz,
                               (long long)lo, dwr.p, dwc.p, (int)h, (int)w, (long long)total, po);
        }
        HIP_CHECK(hipGetLastError());
        if (!on_device) dout.download(out, total, s);
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

extern "C" int hh_pairdiff_rank(const double* a, int64_t na, const double* b, int64_t nb, const double* q,
                                int64_t nq, int64_t* less, int32_t on_device, void* stream) {
    return guard([&] {
        HH_REQUIRE(na >= 0 && nb >= 0 && nq >= 0, "bad arguments");
        HH_REQUIRE(na < (int64_t(1) << 31) && nb < (int64_t(1) << 31) && nq < (int64_t(1) << 31),
                   "more than 2^31 - 1 values");
        HH_REQUIRE((na == 0 || a) && (nb == 0 || b) && (nq == 0 || (q && less)), "null arrays");
        hipStream_t s = as_stream(stream);

        // the inputs are O(K) numbers: device arrays are staged through the
        // host for the finiteness check and the sort of b
        std::vector<double> ha(na), hb(nb), hq(nq);
        if (on_device) {
            if (na) HIP_CHECK(hipMemcpyAsync(ha.data(), a, na * sizeof(double), hipMemcpyDeviceToHost, s));
            if (nb) HIP_CHECK(hipMemcpyAsync(hb.data(), b, nb * sizeof(double), hipMemcpyDeviceToHost, s));
            if (nq) HIP_CHECK(hipMemcpyAsync(hq.data(), q, nq * sizeof(double), hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
        } else {
            std::copy(a, a + na, ha.begin());
            std::copy(b, b + nb, hb.begin());
            std::copy(q, q + nq, hq.begin());
        }
        auto finite = [](const std::vector<double>& v) {
            return std::all_of(v.begin(), v.end(), [](double x) { return std::isfinite(x); });
        };
        HH_REQUIRE(finite(ha), "non-finite value in a");
        HH_REQUIRE(finite(hb), "non-finite value in b");
        HH_REQUIRE(finite(hq), "non-finite value in q");
        if (nq == 0) return;
        std::sort(hb.begin(), hb.end());

        DBuf<unsigned long long> dless(nq);
        dless.zero(s);
        if (na > 0 && nb > 0) {
            DBuf<double> da = to_device(ha, s), db = to_device(hb, s), dq = to_device(hq, s);
            // slices of a so that a short query list still fills the device
            const int64_t max_slices = (na + kPdBlock - 1) / kPdBlock;
            const int64_t slices = std::min<int64_t>(std::max<int64_t>((1024 + nq - 1) / nq, 1),
                                                     std::min<int64_t>(max_slices, 65535));
            const int per_slice = (int)((na + slices - 1) / slices);
            const int ny = (int)((na + per_slice - 1) / per_slice);
            const int in_lds = nb <= kPdMaxLds ? 1 : 0;
            HH_KTIME("k_pairdiff_rank", s);
            hipLaunchKernelGGL(k_pairdiff_rank, dim3((unsigned)nq, (unsigned)ny), dim3(kPdBlock),
                               in_lds ? sizeof(double) * (size_t)nb : 0, s, da.p, (int)na, db.p, (int)nb, dq.p,
                               per_slice, in_lds, dless.p);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipStreamSynchronize(s));  // da, db, dq return to the pool below
        }
        if (on_device) {
            HIP_CHECK(hipMemcpyAsync(less, dless.p, nq * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        } else {
            dless.download(reinterpret_cast<unsigned long long*>(less), nq, s);
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}
