// mdx_mixing_rule.h - the rule of mdx_solubility_mixing (include/mdx.h states it): the solubility mixing diagnostics of n_copies solute
// copies in water.  Plain C++, no HIP types: the kernels of mdx_mixing.hip call the pair functions on the device, the library runs the
// tail (mx_tail) on the host from the device's sums and contact bits, and a stand-alone host program can include this file and run the
// whole rule on one thread (mx_host_sums + mx_tail: tests/cpp/mixing_driver.cpp, tools/mixing_time.py).
//
// Pair arithmetic in fp32 (one d2 and three exponentials per pair), every sum in fp64, the tail in fp64 with one rounding to fp32 per
// field; the three aggregation fractions are fp32 ratios of integers.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MDX_MX_HD __host__ __device__
#else
#define MDX_MX_HD
#endif

#define MDX_MX_MAX_COPIES 4096u                // MDX_SOLUTE_MAX_COPIES of include/mdx.h: the contact bit matrix stays at 2 MiB
#define MDX_MX_SIGMA0 4.0f                     // Gaussian widths, A
#define MDX_MX_SIGMA1 7.0f
#define MDX_MX_SIGMA2 10.0f
#define MDX_MX_CONTACT 4.2f                    // contact cutoff, A
#define MDX_MX_PENALTY_STRENGTH 3.5
#define MDX_MX_LOG_GAIN 80.0
#define MDX_MX_WATER 0xFFFFFFFFu               // the copy id of a water oxygen in the gathered array

struct mx_params {
    float lo[3], L[3], invL[3];      // L = box_hi - box_lo in fp32, invL = 1.0f / L
    float sigma[3];                  // the clipped widths
    float k2[3];                     // -log2(e) / (2 sigma^2): the weight is exp2(d2 k2)
    float cut2;                      // 4.2f * 4.2f
};

inline void mx_setup(const float lo[3], const float hi[3], mx_params& p) {
    for (int d = 0; d < 3; ++d) { p.lo[d] = lo[d]; p.L[d] = hi[d] - lo[d]; p.invL[d] = 1.0f / p.L[d]; }
    const float e = fminf(fminf(p.L[0], p.L[1]), p.L[2]);
    const float half = 0.5f * fmaxf(e, 1.0f);
    const float s[3] = {MDX_MX_SIGMA0, MDX_MX_SIGMA1, MDX_MX_SIGMA2};
    for (int k = 0; k < 3; ++k) {
        p.sigma[k] = fmaxf(fminf(s[k], 0.9f * half), 1.0f);
        p.k2[k] = (float)(-1.4426950408889634 / (2.0 * (double)p.sigma[k] * (double)p.sigma[k]));
    }
    p.cut2 = MDX_MX_CONTACT * MDX_MX_CONTACT;
}

// the library's minimum image of one axis: d - rintf(d invL) L
MDX_MX_HD inline float mx_image(float d, float L, float invL) { return d - rintf(d * invL) * L; }

// squared minimum-image distance from a to b
MDX_MX_HD inline float mx_d2(float ax, float ay, float az, float bx, float by, float bz, const mx_params& p) {
    const float dx = mx_image(bx - ax, p.L[0], p.invL[0]);
    const float dy = mx_image(by - ay, p.L[1], p.invL[1]);
    const float dz = mx_image(bz - az, p.L[2], p.invL[2]);
    return dx * dx + dy * dy + dz * dz;
}

// exp(-d2 / 2 sigma^2) as one exp2
MDX_MX_HD inline float mx_weight(float d2, float k2) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_exp2f(d2 * k2);
#else
    return exp2f(d2 * k2);
#endif
}

#include <vector>

// The sums of every selected solute atom on one host thread: what a caller without the device path runs.  g: the gathered atoms
// [n_rows + n_waters][4] = x, y, z, copy id as bits (MDX_MX_WATER for an oxygen), solute rows first, copy by copy.  sums [n_rows][3][2]:
// S and W per sigma before normalisation; bits [n_copies][w32]: bit (own copy, partner copy) of every pair of selected atoms within the
// cutoff.
inline void mx_host_sums(uint32_t n_rows, uint32_t n_waters, const float* g, const mx_params& p, double* sums, uint32_t* bits, uint32_t w32) {
    const uint32_t n = n_rows + n_waters;
    for (uint32_t i = 0; i < n_rows; ++i) {
        const float* a = g + 4 * (size_t)i;
        uint32_t own;
        memcpy(&own, a + 3, 4);
        double acc[3][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
        for (uint32_t j = 0; j < n; ++j) {
            const float* b = g + 4 * (size_t)j;
            uint32_t pc;
            memcpy(&pc, b + 3, 4);
            if (pc == own) continue;
            const float d2 = mx_d2(a[0], a[1], a[2], b[0], b[1], b[2], p);
            const int w = pc == MDX_MX_WATER ? 1 : 0;
            for (int k = 0; k < 3; ++k) acc[k][w] += (double)mx_weight(d2, p.k2[k]);
            if (!w && d2 <= p.cut2) bits[(size_t)own * w32 + (pc >> 5)] |= 1u << (pc & 31u);
        }
        for (int k = 0; k < 3; ++k) { sums[6 * (size_t)i + 2 * k] = acc[k][0]; sums[6 * (size_t)i + 2 * k + 1] = acc[k][1]; }
    }
}

static inline double mx_clamp01(double v) { return v < 0.0 ? 0.0 : v > 1.0 ? 1.0 : v; }
static inline uint32_t mx_find(std::vector<uint32_t>& parent, uint32_t i) {
    while (parent[i] != i) { parent[i] = parent[parent[i]]; i = parent[i]; }
    return i;
}

// The tail: per-atom scores, aggregation from the contact bits, centres and dispersion, the final scalars.  out[10] in the order of
// mdx_solubility.  n_waters >= 1, n_copies >= 1, n_sel >= 1.
inline void mx_tail(uint32_t n_copies, uint32_t n_sel, uint32_t n_waters, const float* g, const double* sums, const uint32_t* bits, uint32_t w32,
                    const mx_params& p, float out[10]) {
    const uint32_t n_rows = n_copies * n_sel;
    // local mixing
    const double s_norm = (double)(n_rows - n_sel > 1u ? n_rows - n_sel : 1u), w_norm = (double)n_waters;
    double total = 0.0;
    for (int k = 0; k < 3; ++k) {
        double scale = 0.0;
        for (uint32_t i = 0; i < n_rows; ++i) {
            const double S = sums[6 * (size_t)i + 2 * k] / s_norm, W = sums[6 * (size_t)i + 2 * k + 1] / w_norm, dens = S + W;
            scale += dens > (double)FLT_EPSILON ? mx_clamp01(2.0 * W / dens) : 0.0;
        }
        total += scale / (double)n_rows;
    }
    const double local = total / 3.0;
    // aggregation
    float f_largest = 0.f, f_contacted = 0.f, f_pairs = 0.f;
    double penalty = 0.0, factor = 1.0;
    if (n_copies >= 2u) {
        std::vector<uint32_t> parent(n_copies), degree(n_copies, 0u), size(n_copies, 0u);
        for (uint32_t i = 0; i < n_copies; ++i) parent[i] = i;
        uint64_t pairs = 0;
        auto bit = [&](uint32_t i, uint32_t j) { return (bits[(size_t)i * w32 + (j >> 5)] >> (j & 31u)) & 1u; };
        for (uint32_t i = 0; i < n_copies; ++i)
            for (uint32_t j = i + 1u; j < n_copies; ++j)
                if (bit(i, j) | bit(j, i)) {
                    const uint32_t a = mx_find(parent, i), b = mx_find(parent, j);
                    if (a != b) parent[b] = a;
                    degree[i] += 1u; degree[j] += 1u; pairs += 1u;
                }
        uint32_t largest = 1u, contacted = 0u;
        for (uint32_t i = 0; i < n_copies; ++i) {
            const uint32_t r = mx_find(parent, i);
            size[r] += 1u;
            if (size[r] > largest) largest = size[r];
            if (degree[i]) contacted += 1u;
        }
        f_contacted = (float)contacted / (float)n_copies;
        f_pairs = (float)pairs / (float)((uint64_t)n_copies * (n_copies - 1u) / 2u);
        f_largest = (float)(largest - 1u) / (float)(n_copies - 1u);
        penalty = mx_clamp01(0.55 * pow((double)f_largest, 1.25) + 0.30 * (double)f_contacted * (double)f_contacted + 0.15 * sqrt((double)f_pairs));
        factor = mx_clamp01(exp(-MDX_MX_PENALTY_STRENGTH * penalty));
    }
    // dispersion
    double disp = 1.0;
    if (n_copies >= 2u) {
        const double L[3] = {(double)p.L[0], (double)p.L[1], (double)p.L[2]}, lo[3] = {(double)p.lo[0], (double)p.lo[1], (double)p.lo[2]};
        std::vector<double> c(3 * (size_t)n_copies);
        for (uint32_t m = 0; m < n_copies; ++m) {
            const float* a0 = g + 4 * (size_t)m * n_sel;
            for (int d = 0; d < 3; ++d) {
                const double anchor = (double)a0[d] - L[d] * floor(((double)a0[d] - lo[d]) / L[d]);
                double sum = 0.0;
                for (uint32_t k = 0; k < n_sel; ++k) {
                    const double dd = (double)a0[4 * (size_t)k + d] - anchor;
                    sum += anchor + (dd - L[d] * rint(dd / L[d]));
                }
                const double mean = sum / (double)n_sel;
                c[3 * (size_t)m + d] = mean - L[d] * floor((mean - lo[d]) / L[d]);
            }
        }
        double d2_sum = 0.0;
        for (uint32_t i = 0; i < n_copies; ++i)
            for (uint32_t j = i + 1u; j < n_copies; ++j) {
                double d2 = 0.0;
                for (int d = 0; d < 3; ++d) {
                    double dd = c[3 * (size_t)j + d] - c[3 * (size_t)i + d];
                    dd -= L[d] * rint(dd / L[d]);
                    d2 += dd * dd;
                }
                d2_sum += d2;
            }
        const double n_pairs = (double)((uint64_t)n_copies * (n_copies - 1u) / 2u);
        const double expected = sqrt((L[0] * L[0] + L[1] * L[1] + L[2] * L[2]) / 12.0);
        disp = mx_clamp01(sqrt(d2_sum / n_pairs) / expected);
    }
    const double mixture = local * (0.60 + 0.40 * disp);
    const double raw = mx_clamp01(factor * mixture);
    const double score = log(1.0 + MDX_MX_LOG_GAIN * raw) / log(1.0 + MDX_MX_LOG_GAIN);
    out[0] = (float)score; out[1] = (float)raw; out[2] = (float)local; out[3] = (float)disp; out[4] = (float)mixture;
    out[5] = (float)factor; out[6] = (float)penalty; out[7] = f_largest; out[8] = f_contacted; out[9] = f_pairs;
}
