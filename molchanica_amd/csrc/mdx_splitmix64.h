// mdx_splitmix64.h - the counter-based RNG the library shares (bit for bit) with the oracle and with the numpy restatements of the tests.
// Plain C++, no HIP types: mdx_internal.h includes it for the kernels, mdx_search_step.h for the kernels and for stand-alone host programs.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint64_t mdx_splitmix64(uint64_t* s) {
    uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
