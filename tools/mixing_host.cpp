// The path a caller of libmdx has without mdx_solubility_mixing, as a shared object for tools/mixing_time.py: from downloaded positions
// [N][3] gather the selected solute atoms and the water oxygens, then the rule of mdx_mixing_rule.h on one host thread - the same fp32
// pair loop (one d2, three exponentials per pair), fp64 sums, the same tail.
#include "mdx_mixing_rule.h"
#include <vector>

extern "C" int mixing_host(const float* pos, unsigned first, unsigned n_copies, unsigned apc, const unsigned* sel, unsigned n_sel,
                           unsigned water_first, unsigned water_sites, unsigned n_w, const float* lo, const float* hi, float* out10) {
    const uint32_t n_rows = n_copies * n_sel, w32 = (n_copies + 31u) / 32u;
    std::vector<float> g(4 * ((size_t)n_rows + n_w));
    for (uint32_t i = 0; i < n_rows + n_w; ++i) {
        const uint32_t tag = i < n_rows ? i / n_sel : MDX_MX_WATER;
        const uint32_t atom = i < n_rows ? first + tag * apc + sel[i % n_sel] : water_first + (i - n_rows) * water_sites;
        memcpy(&g[4 * (size_t)i], pos + 3 * (size_t)atom, 12);
        memcpy(&g[4 * (size_t)i + 3], &tag, 4);
    }
    mx_params p;
    mx_setup(lo, hi, p);
    std::vector<double> sums(6 * (size_t)n_rows, 0.0);
    std::vector<uint32_t> bits((size_t)n_copies * w32, 0u);
    mx_host_sums(n_rows, n_w, g.data(), p, sums.data(), bits.data(), w32);
    mx_tail(n_copies, n_sel, n_w, g.data(), sums.data(), bits.data(), w32, p, out10);
    return 0;
}
