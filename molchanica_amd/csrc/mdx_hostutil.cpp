// mdx_hostutil.cpp - host-only helpers of libmdx.so that need x86 intrinsics (a HIP translation unit cannot include <immintrin.h>).
// The fingerprint of a system's static arrays, by which the stateless scorer (mdx_single_point, mdx_api.hip) recognises the next
// pose of the molecules it scored last  [ref: compute_energy_snapshot is called pose after pose, src/docking/mod.rs:235].
#include <cstdint>
#include <cstddef>
#include <cstring>
#include <array>
#include <map>
#if defined(__x86_64__) || defined(__i386__)
#define MDX_HOST_X86 1
#include <immintrin.h>
#endif

static uint64_t fp_mix_scalar(uint64_t h, const void* p, size_t bytes) {
    // four independent multiply-rotate lanes over 32-byte blocks (the multiplies pipeline: ~8 B per cycle), folded at the end
    const unsigned char* b = (const unsigned char*)p;
    const uint64_t K = 0x9E3779B97F4A7C15ull;
    uint64_t x0 = h ^ 0x243F6A8885A308D3ull, x1 = h ^ 0x13198A2E03707344ull, x2 = h ^ 0xA4093822299F31D0ull, x3 = h ^ 0x082EFA98EC4E6C89ull;
    auto rotl = [](uint64_t v, int r) { return (v << r) | (v >> (64 - r)); };
    size_t k = 0;
    for (; k + 32 <= bytes; k += 32) {
        uint64_t w[4]; std::memcpy(w, b + k, 32);
        x0 = rotl(x0 ^ w[0], 29) * K; x1 = rotl(x1 ^ w[1], 31) * K; x2 = rotl(x2 ^ w[2], 33) * K; x3 = rotl(x3 ^ w[3], 37) * K;
    }
    for (; k + 8 <= bytes; k += 8) { uint64_t w; std::memcpy(&w, b + k, 8); x0 = rotl(x0 ^ w, 29) * K; }
    uint64_t w = 0; std::memcpy(&w, b + k, bytes - k);
    x1 = rotl(x1 ^ w ^ (uint64_t)bytes, 31) * K;
    h = (x0 ^ rotl(x1, 17) ^ rotl(x2, 31) ^ rotl(x3, 47)) * 0xBF58476D1CE4E5B9ull;
    return h ^ (h >> 31);
}
// The same job on AVX2 hosts, 128 bytes per iteration: four 256-bit accumulators, each adding the 32 x 32 -> 64-bit product of
// the two halves of every keyed 64-bit word plus the word itself with its halves swapped (the accumulation step of XXH3).  ~30 B
// per cycle against ~8: the 6 MB of static arrays of a 51 k-atom complex take ~70 us instead of ~230, which hides behind the
// 150 us the device needs for the pose (mdx_single_point).  Not a cryptographic hash: it tells a docking loop's next pose from
// another molecule set.  The key advances with the stripe (as XXH3 walks its secret): two arrays that hold the same 128-byte blocks
// in a different order - charges of atoms 0-31 swapped with those of atoms 32-63 - mix differently.
#ifdef MDX_HOST_X86
__attribute__((target("avx2"))) static uint64_t fp_mix_avx2(uint64_t h, const void* p, size_t bytes) {
    const unsigned char* b = (const unsigned char*)p;
    const __m256i key[4] = {_mm256_set_epi64x(0x243F6A8885A308D3ll, 0x13198A2E03707344ll, (long long)0xA4093822299F31D0ull, 0x082EFA98EC4E6C89ll),
                            _mm256_set_epi64x(0x452821E638D01377ll, (long long)0xBE5466CF34E90C6Cull, (long long)0xC0AC29B7C97C50DDull, 0x3F84D5B5B5470917ll),
                            _mm256_set_epi64x((long long)0x9216D5D98979FB1Bull, (long long)0xD1310BA698DFB5ACull, 0x2FFD72DBD01ADFB7ll, (long long)0xB8E1AFED6A267E96ull),
                            _mm256_set_epi64x((long long)0xBA7C9045F12C7F99ull, 0x24A19947B3916CF7ll, 0x0801F2E2858EFC16ll, 0x636920D871574E69ll)};
    __m256i acc[4];
    for (int i = 0; i < 4; ++i) acc[i] = _mm256_xor_si256(key[i], _mm256_set1_epi64x((long long)h));
    size_t k = 0;
    __m256i walk = _mm256_setzero_si256();
    const __m256i stride = _mm256_set_epi64x((long long)0x9E3779B97F4A7C15ull, (long long)0xC2B2AE3D27D4EB4Full, 0x165667B19E3779F9ll, (long long)0x85EBCA77C2B2AE63ull);   // odd words
    for (; k + 128 <= bytes; k += 128) {
        walk = _mm256_add_epi64(walk, stride);
        for (int i = 0; i < 4; ++i) {
            const __m256i d = _mm256_loadu_si256((const __m256i*)(b + k + 32 * i));
            const __m256i dk = _mm256_xor_si256(d, _mm256_add_epi64(key[i], walk));
            acc[i] = _mm256_add_epi64(acc[i], _mm256_mul_epu32(dk, _mm256_shuffle_epi32(dk, 0x31)));
            acc[i] = _mm256_add_epi64(acc[i], _mm256_shuffle_epi32(d, 0x4E));
        }
    }
    uint64_t lanes[16];
    for (int i = 0; i < 4; ++i) _mm256_storeu_si256((__m256i*)(lanes + 4 * i), acc[i]);
    uint64_t x = h ^ (uint64_t)bytes;
    for (int i = 0; i < 16; ++i) { x = (x ^ lanes[i]) * 0x9E3779B97F4A7C15ull; x ^= x >> 29; }
    return fp_mix_scalar(x, b + k, bytes - k);      // (the tail, and the final avalanche)
}
#endif
// One Lennard-Jones atom type?  lj = the per-atom records (sigma / 2, sqrt(24 eps)) as [n][2] floats (mdx_api.hip create_impl).  True iff
// at least one atom has a well (record .y != 0; an alchemical window's sign flag on a well-free atom, -0.0, is no well) and every atom
// that has one carries bit for bit the same sigma / 2 = h.  Then sigma_ij^2 of every pair whose LJ term is not multiplied by 0 is the
// one f32 value *c_out = fl(fl(h + h) * fl(h + h)) - computed here the way the pair kernel computes it, an add and a multiply in f32 -
// and the pair kernel's constant-sigma^2 body (pair_eval<..., UNI>) gives the bits of the general one.  Atoms without a well may carry
// any sigma.  Never under the geometric rule (sigma_ij is a product there) and never under an alchemical window (the soft core needs
// sigma_ij of the pair).
bool mdx_uniform_lj(const float* lj, size_t n, bool geometric, bool alch_on, float* c_out) {
    if (c_out) *c_out = 0.f;
    if (!lj || geometric || alch_on) return false;
    bool have = false;
    uint32_t hbits = 0;
    for (size_t i = 0; i < n; ++i) {
        if (lj[2 * i + 1] == 0.f) continue;
        uint32_t b; std::memcpy(&b, &lj[2 * i], 4);
        if (!have) { have = true; hbits = b; }
        else if (b != hbits) return false;
    }
    if (!have) return false;
    float h; std::memcpy(&h, &hbits, 4);
    volatile float sig = h + h;      // (volatile: the sum is rounded to f32 before it is squared, whatever the host's evaluation method)
    const float s = sig;
    volatile float c = s * s;
    if (c_out) *c_out = c;
    return true;
}

// Triads: is every atom's role list either empty or (one angle record with partners a, b; then one or two bond records, each to a or
// to b)?  A box of flexible three-site water is.  Then an atom's bonded work is named by 8 bytes instead of an offset and two or three
// 16-byte records, and the fused bonded + kick + drift pass (mdx_integrate.hip, the TRIAD flavour) reads those:
//   tri[2 i]     = a | (code & 0xFF) << 24
//   tri[2 i + 1] = b | (code >> 8)   << 24          code 0: no roles (a = b = 0)
//   shapes[4 code ..] = { meta of the angle record, meta of the first bond record, meta of the second (0 without one),
//                         number of bonds | (first bond's partner is b) << 8 | (second bond's partner is b) << 9 }
// shapes[0 .. 3] = 0 is the shape of code 0.  The record list of atom i is then, field for field,
//   {a, b, 0, shapes[4c]}, {sel0 ? b : a, 0, 0, shapes[4c + 1]}, and with two bonds {sel1 ? b : a, 0, 0, shapes[4c + 2]}.
// off = the caller-order role offsets [n + 1], rec = the records as four words each (p[0], p[1], p[2], meta: RoleRec, mdx_internal.h),
// shapes = room for 4 * shape_cap words (shape_cap <= 65536: the code has 16 bits), tri = room for 2 n words.  All or nothing: false
// (and *n_shapes = 0) when one atom's list is anything else - another kind, a second angle, a bond to a third atom, a lone bond, three
// bonds, a bond before the angle, a partner index of 2^24 or more, a non-zero unused field - or when the distinct shapes outnumber
// shape_cap - 1.  *n_shapes: distinct shapes, the empty one not counted.
bool mdx_triad_build(const uint32_t* off, const uint32_t* rec, size_t n, uint32_t* tri, uint32_t* shapes, uint32_t shape_cap, uint32_t* n_shapes) {
    if (n_shapes) *n_shapes = 0;
    if (!off || !tri || !shapes || shape_cap < 1u || (off[n] && !rec)) return false;
    if (shape_cap > 65536u) shape_cap = 65536u;
    const uint32_t KIND_BOND = 0u, KIND_ANGLE = 1u;      // (ROLE_BOND, ROLE_ANGLE)
    std::map<std::array<uint32_t, 4>, uint32_t> code_of;
    uint32_t count = 0;
    shapes[0] = shapes[1] = shapes[2] = shapes[3] = 0u;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t b0 = off[i], len = off[i + 1] - b0;
        if (off[i + 1] < b0) return false;
        if (len == 0) { tri[2 * i] = tri[2 * i + 1] = 0u; continue; }
        if (len < 2 || len > 3) return false;
        const uint32_t* an = rec + 4 * (size_t)b0;
        if ((an[3] & 0xFu) != KIND_ANGLE || ((an[3] >> 4) & 0xFu) > 2u || an[2] != 0u) return false;
        const uint32_t a = an[0], b = an[1];
        if (a >= (1u << 24) || b >= (1u << 24)) return false;
        std::array<uint32_t, 4> sh = {an[3], 0u, 0u, len - 1u};
        for (uint32_t k = 1; k < len; ++k) {
            const uint32_t* bd = an + 4 * (size_t)k;
            if ((bd[3] & 0xFu) != KIND_BOND || bd[1] != 0u || bd[2] != 0u) return false;
            if (bd[0] != a && bd[0] != b) return false;
            sh[k] = bd[3];
            if (bd[0] != a) sh[3] |= 1u << (7 + k);
        }
        auto it = code_of.find(sh);
        uint32_t code;
        if (it == code_of.end()) {
            if (count + 1u >= shape_cap) return false;
            code = ++count;
            code_of.emplace(sh, code);
            for (int w = 0; w < 4; ++w) shapes[4 * (size_t)code + w] = sh[w];
        } else code = it->second;
        tri[2 * i] = a | ((code & 0xFFu) << 24);
        tri[2 * i + 1] = b | ((code >> 8) << 24);
    }
    if (n_shapes) *n_shapes = count;
    return true;
}

uint64_t mdx_fp_mix(uint64_t h, const void* p, size_t bytes) {
    if (!p) return (h ^ 0x9E3779B97F4A7C15ull) * 0xBF58476D1CE4E5B9ull;
#ifdef MDX_HOST_X86
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2 && bytes >= 512) return fp_mix_avx2(h, p, bytes);
#endif
    return fp_mix_scalar(h, p, bytes);      // (any other host: the portable flavour)
}
