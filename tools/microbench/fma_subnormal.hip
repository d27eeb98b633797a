// Gate of the upper-band sweep's exponent-zero count operands:
// a count n in the high dword of a register pair over a zero low dword is the
// subnormal double n * 2^-1042, so the sweep can feed the extracted count to
// v_fma_f64 without v_cvt_f64_u32 when the biases are staged times 2^512.
//   1. bits: fma(n * 2^-1042, w * 2^512, acc * 2^-530) * 2^530 against
//      fma((double)n, w, acc) for n = 0..255 and 4096 (w, acc) pairs with |w|
//      over [2^-400, 2^400];
//   2. rate: a stream of independent v_fma_f64 with a normal and with an
//      exponent-zero multiplicand.
// Exit status 0: no mismatch and the subnormal-operand rate within 3 % of the
// normal one.
// hipcc --offload-arch=gfx950 -O2 -o fma_subnormal fma_subnormal.hip
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { std::printf("%s\n", hipGetErrorString(e)); std::exit(1); } } while (0)

constexpr int kPairs = 4096, kCounts = 256;

__global__ void k_bits(const double* __restrict__ w, const double* __restrict__ acc, unsigned long long* bad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= kPairs * kCounts) return;
    const int n = i % kCounts, p = i / kCounts;
    const double conv = fma((double)n, w[p], acc[p]);
    const double opnd = __hiloint2double(n, 0);  // n * 2^-1042
    const double fast = fma(opnd, w[p] * 0x1p512, acc[p] * 0x1p-530) * 0x1p530;
    if (__double_as_longlong(conv) != __double_as_longlong(fast)) atomicAdd(bad, 1ull);
}

// 16 independent chains per lane: no FMA waits for the one before it
__global__ void k_rate(double c, double w, int iters, double* out) {
    double a[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = (double)(threadIdx.x + k) * (c * w);
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int k = 0; k < 16; ++k) a[k] = fma(c, w, a[k]);
        asm volatile("" : "+v"(c), "+v"(w));  // the operands stay registers the loop cannot fold
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += a[k];
    if (s == 12345.678) out[0] = s;  // keeps the chains alive
}

int main() {
    std::mt19937_64 rng(20240607);
    std::uniform_real_distribution<double> ex(-400.0, 400.0), mant(1.0, 2.0), u(0.0, 1.0);
    std::vector<double> w(kPairs), acc(kPairs);
    for (int p = 0; p < kPairs; ++p) {
        double v = std::ldexp(mant(rng), (int)std::floor(ex(rng)));
        if (p == 0) v = 0x1p-400;
        if (p == 1) v = 0x1p400;
        if (p == 2) v = 0.0;
        if (v > 0x1p400) v = 0x1p400;
        if (p & 1) v = -v;
        w[p] = v;
        // a running sum of such products (either sign), or an empty one
        acc[p] = p % 7 == 0 ? 0.0 : (u(rng) - 0.3) * 4096.0 * std::fabs(v);
    }
    double *dw, *dacc, *dout;
    unsigned long long* dbad;
    CK(hipMalloc(&dw, kPairs * sizeof(double)));
    CK(hipMalloc(&dacc, kPairs * sizeof(double)));
    CK(hipMalloc(&dout, sizeof(double)));
    CK(hipMalloc(&dbad, sizeof(unsigned long long)));
    CK(hipMemcpy(dw, w.data(), kPairs * sizeof(double), hipMemcpyHostToDevice));
    CK(hipMemcpy(dacc, acc.data(), kPairs * sizeof(double), hipMemcpyHostToDevice));
    CK(hipMemset(dbad, 0, sizeof(unsigned long long)));
    hipLaunchKernelGGL(k_bits, dim3(kPairs * kCounts / 256), dim3(256), 0, 0, dw, dacc, dbad);
    CK(hipGetLastError());
    unsigned long long bad = 0;
    CK(hipMemcpy(&bad, dbad, sizeof(bad), hipMemcpyDeviceToHost));
    std::printf("bits: %d (count, bias, sum) triples, %llu mismatches\n", kPairs * kCounts, bad);

    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int blocks = prop.multiProcessorCount * 8, iters = 8192;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const double sub = 3 * 4.9406564584124654e-324 * 4294967296.0;  // 3 * 2^-1042: high dword 3, low dword 0
    uint64_t bits;
    std::memcpy(&bits, &sub, 8);
    if (bits != (3ull << 32)) {
        std::printf("host flushed the subnormal operand\n");
        return 1;
    }
    double best[2] = {1e30, 1e30};
    for (int rep = 0; rep < 4; ++rep)  // (the first pair warms up)
        for (int v = 0; v < 2; ++v) {
            CK(hipEventRecord(e0, 0));
            hipLaunchKernelGGL(k_rate, dim3(blocks), dim3(256), 0, 0, v ? sub : 3.0, v ? 0x1p512 * 1e-3 : 1e-3, iters, dout);
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float ms = 0.f;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (rep && ms < best[v]) best[v] = ms;
        }
    const double fmas = (double)blocks * 256 * iters * 16;
    std::printf("rate: normal operand %.3f ms (%.1f GFMA/s), exponent-zero operand %.3f ms (%.1f GFMA/s), ratio %.4f\n",
                best[0], fmas / best[0] * 1e-6, best[1], fmas / best[1] * 1e-6, best[0] / best[1]);
    const bool ok = bad == 0 && best[1] <= best[0] * 1.03;
    std::printf("%s\n", ok ? "gate: pass" : "gate: FAIL");
    return ok ? 0 : 1;
}
