// jtail_reduce.hip - test-only program of tests/test_gpu_jtail.py::test_reduction_bits.  One wave runs, on the same inputs, the half
// list's j-force reduction as it was spelled before jforce_reduce8 (mdx_pair_dev.h) - three registers through the three DPP levels,
// then the lane selects its component and negates it - and the helper the entry loop calls now.
//
//   ref   = -(select(tree(g)))                         the three-register form
//   a     = -jforce_reduce8(g)                         the same adds on the same operands: the bits of ref, always
//   b     =  jforce_reduce8(-g)                        how the entry loop uses it (pair_eval accumulates the reaction with the sign it
//                                                      leaves with): the bits of ref, except that a sum that is exactly ZERO may carry
//                                                      the other sign (x + (-x) is +0 whichever way round) - a sign an add into
//                                                      memory cannot see.  The host accepts b == ref == 0 there and nothing else.
// Lanes ii = lane & 7 < 3 of all eight j rows are compared, bit for bit, no tolerance.  Prints JTAIL-REDUCE-OK and exits 0, or the
// first mismatches and exits 1.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "mdx_pair_dev.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

__global__ __launch_bounds__(64) void jtail_kernel(const float* __restrict__ in, float* __restrict__ ref, float* __restrict__ a,
                                                   float* __restrict__ b, int rounds) {
    const int lane = threadIdx.x & 63, ii = lane & 7;
    const bool sel_x = ii == 0 || ii == 7, sel_y = ii == 1 || ii == 6;
    for (int r = 0; r < rounds; ++r) {
        const size_t k = (size_t)r * 64 + lane;
        float g[3] = {in[k * 3], in[k * 3 + 1], in[k * 3 + 2]};
        float t[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) t[d] = dpp_xadd<0x141>(dpp_xadd<0x4E>(dpp_xadd<0xB1>(g[d])));
        const float v = ii == 0 ? t[0] : (ii == 1 ? t[1] : t[2]);
        ref[k] = -v;
        a[k] = -jforce_reduce8(g, sel_x, sel_y);
        const float ng[3] = {-g[0], -g[1], -g[2]};
        b[k] = jforce_reduce8(ng, sel_x, sel_y);
    }
}

static uint64_t s_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { s_rng ^= s_rng << 13; s_rng ^= s_rng >> 7; s_rng ^= s_rng << 17; return (uint32_t)(s_rng >> 32); }

// magnitudes from 1e-30 to 1e30 (log-uniform), either sign; one value in 16 is +0, -0 or a denormal
static float draw() {
    const uint32_t c = rnd() & 15u;
    uint32_t bits;
    if (c == 0) {
        const uint32_t w = rnd() % 3u;
        bits = w == 0 ? 0u : (w == 1 ? 0x80000000u : ((rnd() & 0x007FFFFFu) | (rnd() & 0x80000000u)));
    } else {
        // 1e-30 = 2^-99.7, 1e30 = 2^99.7: biased exponents 28 .. 226
        bits = (rnd() & 0x80000000u) | ((28u + rnd() % 199u) << 23) | (rnd() & 0x007FFFFFu);
    }
    float f; std::memcpy(&f, &bits, 4);
    return f;
}

int main() {
    const int rounds = 4096;
    const size_t n = (size_t)rounds * 64;
    std::vector<float> h_in(n * 3);
    for (auto& x : h_in) x = draw();
    // a few rounds of nothing but zeros of either sign, and of denormals only
    for (size_t k = 0; k < 64 * 3; ++k) { h_in[k] = (rnd() & 1u) ? 0.0f : -0.0f; }
    for (size_t k = 64 * 3; k < 2 * 64 * 3; ++k) { const uint32_t bt = (rnd() & 0x807FFFFFu); std::memcpy(&h_in[k], &bt, 4); }
    float *d_in = nullptr, *d_ref = nullptr, *d_a = nullptr, *d_b = nullptr;
    CHECK(hipMalloc((void**)&d_in, n * 3 * sizeof(float)));
    CHECK(hipMalloc((void**)&d_ref, n * sizeof(float)));
    CHECK(hipMalloc((void**)&d_a, n * sizeof(float)));
    CHECK(hipMalloc((void**)&d_b, n * sizeof(float)));
    CHECK(hipMemcpy(d_in, h_in.data(), n * 3 * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(jtail_kernel, dim3(1), dim3(64), 0, 0, d_in, d_ref, d_a, d_b, rounds);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<uint32_t> ref(n), a(n), b(n);
    CHECK(hipMemcpy(ref.data(), d_ref, n * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(a.data(), d_a, n * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(b.data(), d_b, n * 4, hipMemcpyDeviceToHost));
    size_t bad = 0, compared = 0, zero_sign = 0, nonzero = 0;
    for (size_t k = 0; k < n; ++k) {
        if ((k & 7u) >= 3u) continue;      // lanes ii >= 3 carry sums nobody reads
        ++compared;
        nonzero += (ref[k] << 1) != 0u;
        bool ok = ref[k] == a[k];
        if (ref[k] != b[k]) {
            if ((ref[k] << 1) == 0u && (b[k] << 1) == 0u) ++zero_sign; else ok = false;
        }
        if (!ok && bad++ < 8) std::printf("round %zu lane %zu: three-register form %08x, -helper(g) %08x, helper(-g) %08x\n", k >> 6, k & 63u, ref[k], a[k], b[k]);
    }
    // (the host's own sum of lane 0's x over the eight lanes of round 2, same tree: the kernel is not comparing garbage with garbage)
    {
        const size_t r = 2;
        float q[8];
        for (int l = 0; l < 8; ++l) q[l] = h_in[(r * 64 + l) * 3];
        const float lo = (q[0] + q[1]) + (q[2] + q[3]), hi = (q[7] + q[6]) + (q[5] + q[4]);
        const float want = -(lo + hi);
        uint32_t wb; std::memcpy(&wb, &want, 4);
        if (wb != ref[r * 64]) { std::printf("host tree %08x, device %08x\n", wb, ref[r * 64]); ++bad; }
    }
    (void)hipFree(d_in); (void)hipFree(d_ref); (void)hipFree(d_a); (void)hipFree(d_b);
    std::printf("rounds %d, compared %zu lane results (%zu non-zero), mismatches %zu, zero sums of the other sign in helper(-g) %zu\n", rounds,
                compared, nonzero, bad, zero_sign);
    if (bad || nonzero < compared / 2) return 1;
    std::printf("JTAIL-REDUCE-OK\n");
    return 0;
}
