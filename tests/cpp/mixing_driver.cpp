// The rule of mdx_solubility_mixing on one host thread, from the rule header alone (no HIP, no library): reads
//   n_copies n_sel n_waters / lo[3] hi[3] / the selected solute atoms copy by copy, then the water oxygens (x y z each)
// from stdin and prints the ten fields, then the sums [n_rows][3][2].  tests/test_mixing_host.py builds it with the sanitizers.
#include "mdx_mixing_rule.h"
#include <cstdio>
#include <vector>

int main() {
    unsigned n_copies = 0, n_sel = 0, n_w = 0;
    float lo[3], hi[3];
    if (std::scanf("%u %u %u", &n_copies, &n_sel, &n_w) != 3 || !n_copies || !n_sel || !n_w || n_copies > MDX_MX_MAX_COPIES) return 2;
    if (std::scanf("%f %f %f %f %f %f", lo, lo + 1, lo + 2, hi, hi + 1, hi + 2) != 6) return 2;
    const uint32_t n_rows = n_copies * n_sel, n = n_rows + n_w, w32 = (n_copies + 31u) / 32u;
    std::vector<float> g(4 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
        if (std::scanf("%f %f %f", &g[4 * (size_t)i], &g[4 * (size_t)i + 1], &g[4 * (size_t)i + 2]) != 3) return 2;
        const uint32_t tag = i < n_rows ? i / n_sel : MDX_MX_WATER;
        memcpy(&g[4 * (size_t)i + 3], &tag, 4);
    }
    mx_params p;
    mx_setup(lo, hi, p);
    std::vector<double> sums(6 * (size_t)n_rows, 0.0);
    std::vector<uint32_t> bits((size_t)n_copies * w32, 0u);
    mx_host_sums(n_rows, n_w, g.data(), p, sums.data(), bits.data(), w32);
    float out[10];
    mx_tail(n_copies, n_sel, n_w, g.data(), sums.data(), bits.data(), w32, p, out);
    for (int k = 0; k < 10; ++k) std::printf("%.9g\n", (double)out[k]);
    for (double v : sums) std::printf("%.17g\n", v);
    return 0;
}
