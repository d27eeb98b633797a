// Baum-Welch training of the TAD HMM (StructureFind.updateParameter /
// modelTrain, StructureFind.py:1052-1110, which run ghmm's `baumWelch` over
// every DI segment of the genome).  ghmm is absent, so the algorithm is
// defined here and pinned by exhaustive enumeration and a
// NumPy restatement (tests/hmm_train_ref.py), not by ghmm itself.
//
// One EM iteration over K sequences with T observations in all, fp64:
//   k_bw_emit    one thread per observation: the S*M log terms
//                log w - log sqrt(2 pi v) - (x - mu)^2 / 2v, shifted by their
//                maximum before exp (no finite observation underflows to a
//                zero likelihood; the shift goes back into log P);
//   k_bw_fb<S>   one wave per sequence, longest first, lane j = state j:
//                scaled forward pass, then the backward pass, which turns the
//                stored alpha into gamma and sums xi and gamma in registers;
//   k_bw_stats   one wave per (sequence, mixture component): the three
//                emission sums, and the sequence's log likelihood;
//   k_bw_reduce  one block per statistic: the per-sequence partial sums
//                added in a fixed tree over the sequence index.
// No floating-point atomics anywhere: two runs give the same bits.  The
// M-step (a few dozen numbers) and the stopping rule run on the host.
#include <cmath>
#include <limits>
#include <numeric>
#include <vector>

#include "hh_common.hpp"

namespace hh {
namespace {

constexpr int kBwMaxS = 8, kBwMaxM = 8;
constexpr int kBwChunk = 8;  // observations prefetched ahead of the serial chain

// device parameter block: A (S*S), pi (S), then per component k = i*M + m:
// lc[k] = log w - log sqrt(2 pi v) (-inf for w = 0), nh[k] = -1 / 2v, mu[k]
struct BwLayout {
    int S, M;
    __host__ __device__ int a() const { return 0; }
    __host__ __device__ int pi() const { return S * S; }
    __host__ __device__ int lc() const { return S * S + S; }
    __host__ __device__ int nh() const { return lc() + S * M; }
    __host__ __device__ int mu() const { return nh() + S * M; }
    __host__ __device__ int size() const { return mu() + S * M; }
    // statistic columns (each K partial sums, then one total)
    __host__ __device__ int c_xi() const { return 0; }                 // S*S  sum_t xi_t(i, j)
    __host__ __device__ int c_gex() const { return S * S; }            // S    sum_{t < n-1} gamma_t(i)
    __host__ __device__ int c_gall() const { return S * S + S; }       // S    sum_t gamma_t(i)
    __host__ __device__ int c_g1() const { return S * S + 2 * S; }     // S    gamma_0(i)
    __host__ __device__ int c_em() const { return S * S + 3 * S; }     // 3*S*M  sum g, sum g d, sum g d^2
    __host__ __device__ int c_logp() const { return c_em() + 3 * S * M; }
    __host__ __device__ int cols() const { return c_logp() + 1; }
};

// e[k*T + t] = exp(l_k(t) - shift_t), bs[i*T + t] = sum_m e[(i*M+m)*T + t]
__global__ __launch_bounds__(256) void k_bw_emit(const double* __restrict__ obs, long long T, BwLayout L,
                                                 const double* __restrict__ par, double* __restrict__ e,
                                                 double* __restrict__ bs, double* __restrict__ shift) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const double x = obs[t];
    const int SM = L.S * L.M;
    const double* lc = par + L.lc();
    const double* nh = par + L.nh();
    const double* mu = par + L.mu();
    double mx = -INFINITY;
    for (int k = 0; k < SM; ++k) {
        const double d = x - mu[k];
        mx = fmax(mx, lc[k] + nh[k] * d * d);
    }
    shift[t] = mx;
    for (int i = 0; i < L.S; ++i) {
        double b = 0.0;
        for (int m = 0; m < L.M; ++m) {
            const int k = i * L.M + m;
            const double d = x - mu[k];
            const double v = exp(lc[k] + nh[k] * d * d - mx);
            e[(long long)k * T + t] = v;
            b += v;
        }
        bs[(long long)i * T + t] = b;
    }
}

__device__ __forceinline__ double bcast(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// Forward and backward recursion of one sequence per wave.  Lane j < S owns
// state j (the other lanes shadow state S - 1 and store nothing).
//   forward:  u_j = (sum_i ah_{t-1}(i) a_ij) b_j(t), c_t = sum_j u_j,
//             ah_t(j) = u_j / c_t; stores ah, c and bq_j(t) = b_j(t) / c_t
//   backward: v_j = bq_j(t+1) bh_{t+1}(j), bh_t(i) = sum_j a_ij v_j,
//             xi(i, j) += ah_t(i) a_ij v_j, gamma_t(i) = ah_t(i) bh_t(i)
//             (gamma overwrites ah)
// Operands of the next kBwChunk observations are loaded before the chain
// needs them, so a step costs ALU latency only.
template <int S>
__global__ __launch_bounds__(64) void k_bw_fb(const long long* __restrict__ seq_off,
                                              const int* __restrict__ order, long long T, long long K,
                                              BwLayout L, const double* __restrict__ par,
                                              const double* __restrict__ bs, double* __restrict__ ag,
                                              double* __restrict__ c, double* __restrict__ bq,
                                              double* __restrict__ part, int* __restrict__ bad) {
    const long long seq = order[blockIdx.x];
    const long long off = seq_off[seq];
    const long long n = seq_off[seq + 1] - off;
    const int lane = threadIdx.x;
    const bool own = lane < S;
    const int j = own ? lane : S - 1;
    const double* A = par + L.a();
    double acol[S], arow[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
        acol[i] = A[i * S + j];
        arow[i] = A[j * S + i];
    }
    const double* bj = bs + (long long)j * T + off;
    double* aj = ag + (long long)j * T + off;
    double* qj = bq + (long long)j * T + off;
    double* cs = c + off;

    // ---------------------------------------------------------- forward
    bool ok = true;
    double a = 0.0;
    double cur[kBwChunk], nxt[kBwChunk];
#pragma unroll
    for (int u = 0; u < kBwChunk; ++u) cur[u] = u < n ? bj[u] : 0.0;
    for (long long base = 0; base < n && ok; base += kBwChunk) {
#pragma unroll
        for (int u = 0; u < kBwChunk; ++u) {
            const long long t = base + kBwChunk + u;
            nxt[u] = t < n ? bj[t] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kBwChunk; ++u) {
            const long long t = base + u;
            if (t < n && ok) {
                double s;
                if (t == 0) {
                    s = par[L.pi() + j];
                } else {
                    s = 0.0;
#pragma unroll
                    for (int i = 0; i < S; ++i) s += bcast(a, i) * acol[i];
                }
                const double un = s * cur[u];
                double ct = 0.0;
#pragma unroll
                for (int i = 0; i < S; ++i) ct += bcast(un, i);
                if (!(ct > 0.0)) {  // wave-uniform: no path reaches observation t
                    ok = false;
                } else {
                    const double inv = 1.0 / ct;
                    a = un * inv;
                    if (own) {
                        aj[t] = a;
                        qj[t] = cur[u] * inv;
                    }
                    if (lane == 0) cs[t] = ct;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kBwChunk; ++u) cur[u] = nxt[u];
    }
    double xi[S];
#pragma unroll
    for (int i = 0; i < S; ++i) xi[i] = 0.0;
    double gex = 0.0, glast = 0.0, g1 = 0.0;
    if (!ok) {
        if (lane == 0) atomicMin(bad, (int)seq);
    } else {
        // ------------------------------------------------------- backward
        // `a` is ah_{n-1}: gamma_{n-1} = ah_{n-1} (bh_{n-1} = 1), already stored
        glast = a;
        g1 = a;
        double beta = 1.0;
        double qc[kBwChunk], ac[kBwChunk], qn[kBwChunk], an[kBwChunk];
        // step t reads bq(t + 1) and ah(t), t = n - 2 ... 0
#pragma unroll
        for (int u = 0; u < kBwChunk; ++u) {
            const long long t = n - 2 - u;
            qc[u] = t >= 0 ? qj[t + 1] : 0.0;
            ac[u] = t >= 0 ? aj[t] : 0.0;
        }
        for (long long top = n - 2; top >= 0; top -= kBwChunk) {
#pragma unroll
            for (int u = 0; u < kBwChunk; ++u) {
                const long long t = top - kBwChunk - u;
                qn[u] = t >= 0 ? qj[t + 1] : 0.0;
                an[u] = t >= 0 ? aj[t] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < kBwChunk; ++u) {
                const long long t = top - u;
                if (t >= 0) {
                    const double v = qc[u] * beta;
                    double nb = 0.0;
#pragma unroll
                    for (int i = 0; i < S; ++i) {
                        const double term = arow[i] * bcast(v, i);
                        nb += term;
                        xi[i] += ac[u] * term;
                    }
                    beta = nb;
                    g1 = ac[u] * beta;
                    gex += g1;
                    if (own) aj[t] = g1;
                }
            }
#pragma unroll
            for (int u = 0; u < kBwChunk; ++u) {
                qc[u] = qn[u];
                ac[u] = an[u];
            }
        }
    }
    if (own) {
#pragma unroll
        for (int i = 0; i < S; ++i) part[(long long)(L.c_xi() + lane * S + i) * K + seq] = xi[i];
        part[(long long)(L.c_gex() + lane) * K + seq] = gex;
        part[(long long)(L.c_gall() + lane) * K + seq] = gex + glast;
        part[(long long)(L.c_g1() + lane) * K + seq] = g1;
    }
}

// blockIdx.x = sequence, blockIdx.y = component k = i*M + m (one wave):
// g_t = gamma_t(i) e_k(t) / b_i(t), d = x_t - mu_k: sum g, sum g d, sum g d^2;
// blockIdx.y = S*M: the sequence's log likelihood sum_t log c_t + shift_t.
// Lane l adds t = l, l + 64, ... in order, then a fixed butterfly.
__global__ __launch_bounds__(64) void k_bw_stats(const double* __restrict__ obs,
                                                 const long long* __restrict__ seq_off, long long T,
                                                 long long K, BwLayout L, const double* __restrict__ par,
                                                 const double* __restrict__ e, const double* __restrict__ bs,
                                                 const double* __restrict__ ag, const double* __restrict__ c,
                                                 const double* __restrict__ shift, const int* __restrict__ bad,
                                                 double* __restrict__ part) {
    const long long seq = blockIdx.x;
    const int k = blockIdx.y;
    const long long off = seq_off[seq];
    const long long n = seq_off[seq + 1] - off;
    const int lane = threadIdx.x;
    const bool live = *bad >= K;  // a failed E-step leaves c / gamma unwritten: the call fails, sum nothing
    if (k == L.S * L.M) {
        double lp = 0.0;
        if (live)
            for (long long t = lane; t < n; t += kWave) lp += log(c[off + t]) + shift[off + t];
        lp = wave_sum(lp);
        if (lane == 0) part[(long long)L.c_logp() * K + seq] = lp;
        return;
    }
    const int i = k / L.M;
    const double mu = par[L.mu() + k];
    const double* ek = e + (long long)k * T + off;
    const double* bi = bs + (long long)i * T + off;
    const double* gi = ag + (long long)i * T + off;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (live)
        for (long long t = lane; t < n; t += kWave) {
            const double b = bi[t];
            const double g = b > 0.0 ? gi[t] * (ek[t] / b) : 0.0;
            const double d = obs[off + t] - mu;
            s0 += g;
            s1 += g * d;
            s2 += g * d * d;
        }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) {
        part[(long long)(L.c_em() + 3 * k + 0) * K + seq] = s0;
        part[(long long)(L.c_em() + 3 * k + 1) * K + seq] = s1;
        part[(long long)(L.c_em() + 3 * k + 2) * K + seq] = s2;
    }
}

// one block per statistic column: thread r adds sequences r, r + 256, ... in
// order, then the block's fixed tree
__global__ __launch_bounds__(256) void k_bw_reduce(const double* __restrict__ part, long long K,
                                                   double* __restrict__ red) {
    __shared__ double sh[16];
    const double* p = part + (long long)blockIdx.x * K;
    double s = 0.0;
    for (long long q = threadIdx.x; q < K; q += blockDim.x) s += p[q];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) red[blockIdx.x] = s;
}

using FbKernel = void (*)(const long long*, const int*, long long, long long, BwLayout, const double*,
                          const double*, double*, double*, double*, double*, int*);
template <int S>
FbKernel fb_pick(int s) {
    if constexpr (S == 0) {
        return nullptr;
    } else {
        return s == S ? (FbKernel)k_bw_fb<S> : fb_pick<S - 1>(s);
    }
}

}  // namespace
}  // namespace hh

using namespace hh;

struct hh_hmm_bw {
    int device = 0;
    BwLayout L{0, 0};
    long long T = 0, K = 0;
    hipStream_t stream = nullptr;
    DBuf<double> obs, e, bs, ag, c, bq, shift, part, red, par;
    DBuf<long long> seq_off;
    DBuf<int> order, bad;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = 0.f;
    ~hh_hmm_bw() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

namespace {

struct BwStepOut {
    double logp = 0.0;
    int floored = 0;
};

// One EM iteration: E-step on the device under the given parameters, M-step
// on the host, in place.
BwStepOut bw_step(hh_hmm_bw* h, double* A, double* pi, double* mean, double* var, double* weight,
                  double var_floor) {
    const BwLayout L = h->L;
    const int S = L.S, M = L.M, SM = S * M;
    const long long T = h->T, K = h->K;
    HH_REQUIRE(var_floor >= 0.0, "var_floor must be >= 0");
    std::vector<double> par(L.size());
    bool any_w = false;
    for (int q = 0; q < S * S; ++q) {
        HH_REQUIRE(A[q] >= 0.0 && std::isfinite(A[q]), "transition probabilities must be finite and >= 0");
        par[L.a() + q] = A[q];
    }
    for (int i = 0; i < S; ++i) {
        HH_REQUIRE(pi[i] >= 0.0 && std::isfinite(pi[i]), "initial probabilities must be finite and >= 0");
        par[L.pi() + i] = pi[i];
    }
    for (int k = 0; k < SM; ++k) {
        HH_REQUIRE(var[k] > 0.0 && std::isfinite(var[k]) && weight[k] >= 0.0 && std::isfinite(weight[k]) &&
                       std::isfinite(mean[k]),
                   "variances must be > 0, weights >= 0, all finite");
        any_w |= weight[k] > 0.0;
        par[L.lc() + k] = weight[k] > 0.0 ? std::log(weight[k]) - 0.5 * std::log(2.0 * M_PI * var[k])
                                          : -std::numeric_limits<double>::infinity();
        par[L.nh() + k] = -0.5 / var[k];
        par[L.mu() + k] = mean[k];
    }
    HH_REQUIRE(any_w, "every mixture weight is 0");
    hipStream_t s = h->stream;
    upload_pinned_sync(h->par.p, par.data(), par.size(), s);
    HIP_CHECK(hipMemcpyAsync(h->bad.p, h->bad.p + 1, sizeof(int), hipMemcpyDeviceToDevice, s));  // = INT_MAX
    HIP_CHECK(hipEventRecord(h->ev0, s));
    {
        HH_KTIME("k_bw_emit", s);
        k_bw_emit<<<dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s>>>(h->obs.p, T, L, h->par.p, h->e.p,
                                                                           h->bs.p, h->shift.p);
    }
    {
        HH_KTIME("k_bw_fb", s);
        fb_pick<kBwMaxS>(S)<<<dim3((unsigned)K), dim3(64), 0, s>>>(h->seq_off.p, h->order.p, T, K, L, h->par.p,
                                                                    h->bs.p, h->ag.p, h->c.p, h->bq.p, h->part.p,
                                                                    h->bad.p);
    }
    {
        HH_KTIME("k_bw_stats", s);
        k_bw_stats<<<dim3((unsigned)K, (unsigned)(SM + 1)), dim3(64), 0, s>>>(
            h->obs.p, h->seq_off.p, T, K, L, h->par.p, h->e.p, h->bs.p, h->ag.p, h->c.p, h->shift.p, h->bad.p,
            h->part.p);
    }
    {
        HH_KTIME("k_bw_reduce", s);
        k_bw_reduce<<<dim3((unsigned)L.cols()), dim3(256), 0, s>>>(h->part.p, K, h->red.p);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(h->ev1, s));
    std::vector<double> red(L.cols());
    int bad = 0;
    PinnedDown down;
    down.add(h->red.p, red.data(), red.size());
    down.add(h->bad.p, &bad, 1);
    down.run(s);
    (void)hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1);
    if (bad < K)
        HH_THROW(HH_ERR_ARG, "sequence " + std::to_string(bad) +
                                 " has zero likelihood under the model (no state path with nonzero probability)");
    BwStepOut out;
    out.logp = red[L.c_logp()];
    HH_REQUIRE(std::isfinite(out.logp), "log likelihood is not finite");
    // ------------------------------------------------------------ M-step
    // a quantity whose denominator is 0 keeps its old value
    for (int i = 0; i < S; ++i) pi[i] = red[L.c_g1() + i] / (double)K;
    for (int i = 0; i < S; ++i) {
        const double den = red[L.c_gex() + i];
        if (den > 0.0)
            for (int j = 0; j < S; ++j) A[i * S + j] = red[L.c_xi() + i * S + j] / den;  // a_ij = 0 stays 0
        const double gall = red[L.c_gall() + i];
        for (int m = 0; m < M; ++m) {
            const int k = i * M + m;
            const double s0 = red[L.c_em() + 3 * k], s1 = red[L.c_em() + 3 * k + 1],
                         s2 = red[L.c_em() + 3 * k + 2];
            if (gall > 0.0) weight[k] = s0 / gall;
            if (s0 > 0.0) {
                const double dm = s1 / s0;
                mean[k] += dm;
                double v = s2 / s0 - dm * dm;
                if (!(v >= var_floor)) {
                    v = var_floor;
                    ++out.floored;
                }
                HH_REQUIRE(v > 0.0, "re-estimated variance is 0 and var_floor is 0");
                var[k] = v;
            }
        }
    }
    return out;
}

}  // namespace

extern "C" int hh_hmm_bw_create(const double* obs, const int64_t* seq_off, int64_t n_seq, int32_t S, int32_t M,
                                void* stream, hh_hmm_bw** out) {
    return guard([&] {
        HH_REQUIRE(obs && seq_off && out, "null argument");
        HH_REQUIRE(S >= 1 && S <= kBwMaxS && M >= 1 && M <= kBwMaxM, "1 <= states, components <= 8");
        HH_REQUIRE(n_seq >= 1 && n_seq < (int64_t(1) << 31) - 1, "1 <= n_seq < 2^31 - 1");
        HH_REQUIRE(seq_off[0] == 0, "seq_off[0] must be 0");
        for (int64_t q = 0; q < n_seq; ++q)
            if (!(seq_off[q + 1] > seq_off[q])) HH_THROW(HH_ERR_ARG, "sequence " + std::to_string(q) + " is empty");
        const int64_t T = seq_off[n_seq];
        for (int64_t t = 0; t < T; ++t)
            if (!std::isfinite(obs[t])) HH_THROW(HH_ERR_ARG, "observation " + std::to_string(t) + " is not finite");
        auto h = std::make_unique<hh_hmm_bw>();
        HIP_CHECK(hipGetDevice(&h->device));
        h->L = BwLayout{S, M};
        h->T = T;
        h->K = n_seq;
        h->stream = as_stream(stream);
        hipStream_t s = h->stream;
        // longest first (ties by index): the long serial chains start at once
        std::vector<int> order(n_seq);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
            return seq_off[a + 1] - seq_off[a] > seq_off[b + 1] - seq_off[b];
        });
        std::vector<long long> off(seq_off, seq_off + n_seq + 1);
        h->obs.alloc(T);
        h->seq_off.alloc(n_seq + 1);
        h->order.alloc(n_seq);
        h->bad.alloc(2);
        h->e.alloc((size_t)T * S * M);
        h->bs.alloc((size_t)T * S);
        h->ag.alloc((size_t)T * S);
        h->bq.alloc((size_t)T * S);
        h->c.alloc(T);
        h->shift.alloc(T);
        h->part.alloc((size_t)h->L.cols() * n_seq);
        h->red.alloc(h->L.cols());
        h->par.alloc(h->L.size());
        const int badinit[2] = {std::numeric_limits<int>::max(), std::numeric_limits<int>::max()};
        h->obs.upload(obs, T, s);
        h->seq_off.upload(off.data(), off.size(), s);
        h->order.upload(order.data(), order.size(), s);
        h->bad.upload(badinit, 2, s);
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipEventCreate(&h->ev0));
        HIP_CHECK(hipEventCreate(&h->ev1));
        *out = h.release();
    });
}

extern "C" int hh_hmm_bw_free(hh_hmm_bw* h) {
    return guard([&] {
        if (h) device_quiesce(h->device);
        delete h;
    });
}

extern "C" int hh_hmm_bw_step(hh_hmm_bw* h, double* A, double* pi, double* mean, double* var, double* weight,
                              double var_floor, double* logp) {
    return guard([&] {
        HH_REQUIRE(h && A && pi && mean && var && weight && logp, "null argument");
        *logp = bw_step(h, A, pi, mean, var, weight, var_floor).logp;
    });
}

extern "C" int hh_hmm_bw_last_step_ms(hh_hmm_bw* h, double* ms) {
    return guard([&] {
        HH_REQUIRE(h && ms, "null argument");
        *ms = h->last_ms;
    });
}

extern "C" int hh_hmm_bw_train(hh_hmm_bw* h, double* A, double* pi, double* mean, double* var, double* weight,
                               int32_t max_iter, double eps, double var_floor, int32_t* iters, double* logp_trace,
                               int32_t* status) {
    return guard([&] {
        HH_REQUIRE(h && A && pi && mean && var && weight && iters && status, "null argument");
        HH_REQUIRE(max_iter >= 0 && (logp_trace || max_iter == 0), "max_iter >= 0 and a trace of max_iter entries");
        HH_REQUIRE(eps >= 0.0, "eps must be >= 0");
        int st = HH_BW_MAX_ITER, k = 0;
        double prev = 0.0;
        while (k < max_iter) {
            const BwStepOut o = bw_step(h, A, pi, mean, var, weight, var_floor);
            logp_trace[k] = o.logp;
            if (o.floored) st |= HH_BW_VAR_FLOORED;
            const double d = o.logp - prev;
            ++k;
            if (k >= 2) {
                if (d < -1e-9 * std::fabs(o.logp)) st |= HH_BW_LOGP_DROPPED;
                if (d >= 0.0 && d < eps * std::fabs(o.logp)) {
                    st &= ~HH_BW_MAX_ITER;
                    break;
                }
            }
            prev = o.logp;
        }
        *iters = k;
        *status = st;
    });
}
