// mdx_nonbonded_impl.h - the pair kernels (templates) and their launcher launch_variant<ENERGY, COUL>; the description is at the head of
// mdx_nonbonded.hip.  Included by mdx_nb_inst.hip, which the Makefile compiles once per (ENERGY, COUL) pair: the 650-odd kernel
// instantiations build as eight translation units side by side (one unit took 3.5 minutes).
#pragma once
#include "mdx_internal.h"
#include "mdx_bonded_dev.h"
#include "mdx_pair_dev.h"
#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <type_traits>

constexpr int NB_WAVES = MDX_NB_WAVES;      // least waves per workgroup (mdx_internal.h)
#ifdef NB_DRAIN_TRACE
extern uint4* g_mdx_drain; extern size_t g_mdx_drain_cap; extern uint32_t g_mdx_drain_n; extern int g_mdx_drain_on;      // mdx_nonbonded.hip
#endif
#ifndef NB_ASM_PAIR
#define NB_ASM_PAIR 0     // 1: the default flavour's pair evaluation is the hand-written block pair_eval_asm (v_cmpx exec handling):
                          // measured round 3 - inner-list walk 0.4566 / 0.4517 ms against 0.4565 / 0.4572 with the compiler's
                          // v_cmp + s_and_saveexec + s_cbranch_execz + s_or, pruning pass SLOWER (no early-out for the 40 % of its
                          // cluster pairs without a lane in range): 0.4936 vs 0.4809 ms per step.  Two scalar instructions fewer per
                          // cluster pair buy nothing; kept as an A/B arm (make EXTRA=-DNB_ASM_PAIR=1), parity-tested once
#endif
#ifndef NB_HALF_FLUSH
#define NB_HALF_FLUSH 0   // 1: j-forces leave once per chunk from LDS; 0: one 24-lane atomic per entry
#endif
#ifndef NB_SPLIT_MASKED
#define NB_SPLIT_MASKED 1 // 1: the chunk loop exists twice, masked chunks and plain ones (nb_cluster_body)
#endif
#ifndef NB_LATCH2
#define NB_LATCH2 1       // 1: the one-wave half-list UNI kernels keep two sets of the chunk pipeline's registers and wait for vector
                          // memory once per two chunks (nb_cluster_body, LATCH2); 0: every kernel has the one-set loop
#endif

// The force-only pair evaluation of the default flavour (shifted-cutoff Coulomb, Lorentz-Berthelot, one cutoff, half list) as ONE
// block of hand-written gfx950 instructions (round 3).  Same arithmetic, instruction for instruction, as hipcc's code for
// pair_eval<..., BRANCHY, HALF>; what differs is the exec-mask handling.  The compiler brackets the in-range part with
//     v_cmp_gt_f32 vcc / s_and_saveexec_b64 / s_cbranch_execz ... s_or_b64 exec
// and this loop is issue-bound with scalar instructions costing as much as vector ones (65 M SALU are
// 17 % of the launch).  Here v_cmpx_gt_f32 narrows EXEC itself and one s_mov_b64 restores it: one scalar instruction per cluster
// pair instead of three.  Preconditions, all true in nb_cluster_body's entry loop: EXEC is all ones on entry (whole waves, no
// divergent region around the call); nothing after the block reads VCC.  Hazards: the only EXEC write by a VALU instruction is
// the v_cmpx, and 21 VALU instructions separate it from whatever follows the block (DPP and v_readlane want 5 / 4 wait states
// after a VALU write of EXEC; an s_mov of EXEC needs none); the first use of the v_rsq result is four instructions behind it.  BIAS: the masked chunks' NaN-coded exclusion
// bit enters r^2 as the addend of the first FMA.  R2OUT: the pruning pass wants r^2 (of every lane, in range or not).
template <bool BIAS, bool R2OUT>
__device__ __forceinline__ void pair_eval_asm(float xi, float yi, float zi, float qi, float sgi, float epi, const float4 pj,
                                              const float2 lj, float rc2, float bias, float& fx, float& fy, float& fz,
                                              float& g0, float& g1, float& g2, float& r2_out) {
    float dx, dy, dz, r2, t1, t2, t3, t4;
    if (BIAS) {
        asm volatile(
            "v_sub_f32 %[dy], %[yi], %[yj]\n\t"
            "v_sub_f32 %[dx], %[xi], %[xj]\n\t"
            "v_fma_f32 %[r2], %[dy], %[dy], %[bias]\n\t"
            "v_sub_f32 %[dz], %[zi], %[zj]\n\t"
            "v_fmac_f32 %[r2], %[dx], %[dx]\n\t"
            "v_fmac_f32 %[r2], %[dz], %[dz]\n\t"
            : [dx] "=&v"(dx), [dy] "=&v"(dy), [dz] "=&v"(dz), [r2] "=&v"(r2)
            : [xi] "v"(xi), [yi] "v"(yi), [zi] "v"(zi), [xj] "v"(pj.x), [yj] "v"(pj.y), [zj] "v"(pj.z), [bias] "v"(bias));
    } else {
        asm volatile(
            "v_sub_f32 %[dy], %[yi], %[yj]\n\t"
            "v_sub_f32 %[dx], %[xi], %[xj]\n\t"
            "v_mul_f32 %[r2], %[dy], %[dy]\n\t"
            "v_sub_f32 %[dz], %[zi], %[zj]\n\t"
            "v_fmac_f32 %[r2], %[dx], %[dx]\n\t"
            "v_fmac_f32 %[r2], %[dz], %[dz]\n\t"
            : [dx] "=&v"(dx), [dy] "=&v"(dy), [dz] "=&v"(dz), [r2] "=&v"(r2)
            : [xi] "v"(xi), [yi] "v"(yi), [zi] "v"(zi), [xj] "v"(pj.x), [yj] "v"(pj.y), [zj] "v"(pj.z));
    }
    if (R2OUT) r2_out = r2;
    asm volatile(
        "v_cmpx_gt_f32 vcc, %[rc2], %[r2]\n\t"            // EXEC &= (r^2 < rc^2); a NaN r^2 (excluded pair) fails
        "v_rsq_f32 %[r2], %[r2]\n\t"                      // 1 / r
        "v_add_f32 %[t1], %[sgi], %[ljx]\n\t"             // sigma_ij = sigma_i / 2 + sigma_j / 2
        "v_mul_f32 %[t1], %[t1], %[t1]\n\t"
        "v_mul_f32 %[t2], %[epi], %[ljy]\n\t"             // 24 eps_ij
        "v_mul_f32 %[t3], %[r2], %[r2]\n\t"               // 1 / r^2
        "v_mul_f32 %[t1], %[t1], %[t3]\n\t"               // s2 = sigma^2 / r^2
        "v_mul_f32 %[t4], %[t1], %[t1]\n\t"
        "v_mul_f32 %[t1], %[t1], %[t4]\n\t"               // s6
        "v_mul_f32 %[t2], %[t2], %[t1]\n\t"               // 24 eps s6
        "v_fma_f32 %[t1], %[t1], 2.0, -1.0\n\t"           // 2 s6 - 1
        "v_mul_f32 %[t1], %[t2], %[t1]\n\t"               // LJ force * r^2
        "v_mul_f32 %[t2], %[qi], %[qj]\n\t"               // k_e q_i q_j
        "v_fmac_f32 %[t1], %[t2], %[r2]\n\t"              // + Coulomb force * r^2
        "v_mul_f32 %[t1], %[t3], %[t1]\n\t"               // fs = (...) / r^2
        "v_fmac_f32 %[fx], %[dx], %[t1]\n\t"
        "v_fmac_f32 %[fy], %[dy], %[t1]\n\t"
        "v_fmac_f32 %[fz], %[dz], %[t1]\n\t"
        "v_fma_f32 %[g0], -%[dx], %[t1], %[g0]\n\t"       // the force on j, with the sign it leaves with
        "v_fma_f32 %[g1], -%[dy], %[t1], %[g1]\n\t"
        "v_fma_f32 %[g2], -%[dz], %[t1], %[g2]\n\t"
        "s_mov_b64 exec, -1\n\t"
        : [fx] "+v"(fx), [fy] "+v"(fy), [fz] "+v"(fz), [g0] "+v"(g0), [g1] "+v"(g1), [g2] "+v"(g2), [r2] "+v"(r2),
          [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3), [t4] "=&v"(t4)
        : [rc2] "s"(rc2), [sgi] "v"(sgi), [epi] "v"(epi), [ljx] "v"(lj.x), [ljy] "v"(lj.y), [qi] "v"(qi), [qj] "v"(pj.w),
          [dx] "v"(dx), [dy] "v"(dy), [dz] "v"(dz)
        : "vcc");
}

// which instantiations of nb_cluster_body keep two sets of the chunk pipeline's registers (LATCH2 there; launch_variant reports it)
constexpr bool nb_latch2(bool half, bool uni, int wpt, bool energy, bool alch, bool step) {
    return NB_LATCH2 && NB_SPLIT_MASKED && half && !NB_HALF_FLUSH && uni && wpt == 1 && !energy && !alch && !step;
}

template <bool ENERGY, int COUL, bool GEOM, bool SAMECUT, bool MASKED>
__device__ __forceinline__ void chunk_pairs(const float4* __restrict__ sx, const float2* __restrict__ sl,
                                            unsigned long long mask, float xi, float yi, float zi, float qi,
                                            float sgi, float epi, const NbParams& p, float& fx, float& fy,
                                            float& fz, double& elj, double& ecoul, double& evir) {
    float e1 = 0.f, e2 = 0.f, e3 = 0.f;
#pragma unroll 8
    for (int jj = 0; jj < 64; ++jj) {
        const bool allowed = MASKED ? (bool)((mask >> jj) & 1ull) : true;
        pair_eval<ENERGY, COUL, GEOM, SAMECUT, false>(xi, yi, zi, qi, sgi, epi, sx[jj], sl[jj], allowed, p, fx, fy, fz,
                                               e1, e2, nullptr, ENERGY ? &e3 : nullptr);
    }
    if (ENERGY) { elj += (double)e1; ecoul += (double)e2; evir += (double)e3; }
}

template <bool ENERGY, int COUL, bool GEOM, bool SAMECUT>
__global__ __launch_bounds__(NB_WAVES * 64) void nb_tile_kernel(NbArgs a) {
    if (a.gate && *a.gate > a.thr_bits) return;
    __shared__ float4 s_xyzq[NB_WAVES][64];
    __shared__ float2 s_lj[NB_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // XCD-aware remap: block b is dispatched to XCD b%8; give each XCD a contiguous tile range
    const uint32_t nblocks = (a.T + NB_WAVES - 1) / NB_WAVES;
    const uint32_t per_xcd = (nblocks + 7) >> 3;
    const uint32_t blk = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
    if (blk >= nblocks) return;
    const uint32_t t = blk * NB_WAVES + wave;
    if (t >= a.T) return;

    const uint32_t islot = t * MDX_TILE + lane;
    const float4 pi = a.posq[islot];
    const float2 li = a.lj[islot];
    const ListCounts cnt = a.counts[t];
    const uint32_t e0 = a.entry_off[t];
    const uint32_t nmc = cnt.n_masked >> 3, nchunks = (cnt.n_masked + cnt.n_plain) >> 3;
    const uint32_t mbase = a.mchunk_off[t];
    float4* sx = s_xyzq[wave];
    float2* sl = s_lj[wave];

    float fx = 0.f, fy = 0.f, fz = 0.f;
    double elj = 0.0, ecoul = 0.0, evir = 0.0;

    // prefetch chunk 0
    float4 nj = make_float4(0.f, 0.f, 0.f, 0.f);
    float2 nl = make_float2(0.f, 0.f);
    uint32_t ncode = 13;
    if (nchunks) {
        const uint2 ent = a.entries[e0 + (lane >> 3)];
        const uint32_t js = ent.x * MDX_CLUSTER + (lane & 7);
        nj = a.posq[js]; nl = a.lj[js]; ncode = ent.y & 31u;
    }
    for (uint32_t c = 0; c < nchunks; ++c) {
        {   // image shift, then park in LDS
            float rx, ry, rz;
            image_shift_row(ncode, a.p.shift, rx, ry, rz);
            nj.x += rx; nj.y += ry; nj.z += rz;
            sx[lane] = nj;
            sl[lane] = nl;
        }
        WAVE_LDS_SYNC();
        if (c + 1 < nchunks) {
            const uint2 ent = a.entries[e0 + (c + 1) * 8 + (lane >> 3)];
            const uint32_t js = ent.x * MDX_CLUSTER + (lane & 7);
            nj = a.posq[js]; nl = a.lj[js]; ncode = ent.y & 31u;
        }
        if (c < nmc) {
            const unsigned long long m = a.masks[(size_t)(mbase + c) * 64 + lane];
            chunk_pairs<ENERGY, COUL, GEOM, SAMECUT, true>(sx, sl, m, pi.x, pi.y, pi.z, pi.w, li.x, li.y, a.p,
                                                           fx, fy, fz, elj, ecoul, evir);
        } else {
            chunk_pairs<ENERGY, COUL, GEOM, SAMECUT, false>(sx, sl, ~0ull, pi.x, pi.y, pi.z, pi.w, li.x, li.y,
                                                            a.p, fx, fy, fz, elj, ecoul, evir);
        }
        WAVE_LDS_SYNC();
    }
    a.force[islot] = make_float4(fx, fy, fz, 0.f);
    if (ENERGY) {
        if (!(a.slot_flags[islot] & 2u)) { elj = 0.0; ecoul = 0.0; evir = 0.0; }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            elj += __shfl_xor(elj, m);
            ecoul += __shfl_xor(ecoul, m);
            evir += __shfl_xor(evir, m);
        }
        if (lane == 0) {   // every pair is seen from both sides
            double* q = a.energy + EN_COUNT + 8 + MDX_ESTRIDE * (blk & (MDX_EPART - 1));
            atomicAdd(q, 0.5 * elj); atomicAdd(q + 1, 0.5 * ecoul); atomicAdd(q + 2, 0.5 * evir);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Variant 2 (default): cluster-masked tile kernel.  Same list, same LDS staging, but a lane is the
// pair (i-atom ii = lane&7 of every i-cluster, j-atom jj = lane>>3 of the current entry): the
// eight i-clusters of the tile sit in registers, and an entry is evaluated only against the
// i-clusters whose bounding box is within the list radius of the j-cluster (the entry's 8-bit
// imask, a wave-uniform branch).  That removes the corner (i-cluster, j-cluster) pairs a
// whole-tile test lets through - about 40 % of the pair evaluations at rc 10 + skin 2 - at the
// price of one cross-lane reduction per tile.  Still one owner per i-atom, no atomics,
// deterministic.
//
// WPT = waves per tile.  WPT = 1: a workgroup is 4 tiles.  WPT = 4: the 4 waves of a workgroup
// share ONE tile, wave w takes chunks w, w+4, ... of its list and the partial forces are summed
// through LDS in a fixed order.  A tile's list is a ~270 us dependency chain for one wave, so a
// launch with fewer tiles than the chip has wave slots (strong scaling: 1/8 of the box per GPU,
// or any system below ~250 k atoms) is latency-bound; splitting the list 4 ways fills the SIMDs.
//
// HALF = true (variant 5) walks a half list: a cluster pair lives in ONE tile's list, the force on
// the i-atoms accumulates in registers as before and the reaction on the eight j-atoms of an entry
// is summed over the eight i-lanes with three DPP steps and leaves as ONE 24-lane f32 atomic
// (x, y, z of 8 consecutive float4 records = 128 contiguous bytes).  The budget of these atomics is REQUESTS, not words: gfx950
// executes an f32 atomic at the memory side and every wave-instruction leaves L2 as one uncached 64-B request per 64-B segment it
// touches, at ~1.3 TB/s of requests chip-wide.  A 1 M-atom inner walk issues 2.33 M entry atomics of two segments each (298 MB) plus
// the tiles' i-force write-back, 361 MB in all before the write-back was shaped to its rows (iforce_add_rows: 16 requests per unit
// instead of 48) and 316 MB since: 0.24 ms at the full rate beside ~0.3 ms of VALU issue, the two floors level.
// No instruction shape may hit the same 128-B line twice in a row (x, then y, then z of the same
// atoms is 3x slower).  Measured and rejected: collecting a chunk's j-forces in LDS and flushing
// them once per chunk (NB_HALF_FLUSH=1: 0.79 vs 0.66 ms, it needs 137 VGPRs = 3 waves/SIMD);
// any form of LDS look-ahead of the next entry's j record (+6..8 %, both kernels).
// The force array must be zero when the kernel starts.
// What runs once per ENTRY around the cluster pairs is trimmed to the instructions the result needs (mdx_pair_dev.h jforce_reduce8:
// select the component first, then one mirror add; the reaction accumulates with the sign it leaves with; the atomic's address is a
// scalar base plus a loop-invariant lane offset; the eps strip has the position strip's stride, one LDS address register for both).

// DUAL (dual pair list, half-list force flavour only): 0 = plain list; 1 = walk the INNER list, a no-op when this step
// must prune; 2 = the pruning pass (walks the Verlet list, writes the inner list), a no-op unless this step must prune.  The step loop enqueues 1 and 2 back to back
// and the device decides which one runs (a gated-off launch costs ~3 us).  A single kernel with a run-time switch was
// measured first: the two scalar instructions it adds per cluster pair cost 11 % (0.537 -> 0.598 ms) - every
// instruction in this loop is ~5 cycles of a latency-bound wave.
// The body of the cluster kernel.  DUAL here is 0, 1 or 2; the __global__ wrapper below owns the LDS arrays and, for the
// merged dual-list launch (DUAL 3), picks the inner-walk or the pruning body at run time: one launch per step instead
// of a pair of which the device runs one (the gated-off twin cost ~4 us per step - 5 % of a 23 k-atom step).
// STEP (round 6, "one launch per step": NbArgs::st_*): the tile's wave first FINISHES THE LAST STEP for its 64 atoms - position x = Y + w F
// from the two rows every reader uses (mdx_bonded_dev.h step_pos), full kick, the next step's Y, path length, the words that gate the next
// launch - then evaluates the pairs at x as below, j-atoms reconstructed from the same two rows, and its atoms' bonded roles.  The separate
// bonded + kick + drift pass (35 us of a 513 us step at 1 M atoms, 112 B per atom) rides inside this compute-bound launch instead.
// UNI (handles with one Lennard-Jones atom type, mdx_uniform_lj; force-only Lorentz-Berthelot flavours without STEP): sigma_ij^2 is the
// constant a.p.uni_c (pair_eval<..., UNI>), so the eight sgi registers, the .x of the j-side pipeline registers and of the per-entry
// LDS read are gone: of a record of the strip s_lj only .x is used, sqrt(24 eps).  The lj[] rows in memory keep both halves.
template <bool ENERGY, int COUL, bool GEOM, bool SAMECUT, int WPT, bool HALF, bool ALCH, int DUAL, int BW, bool STEP = false, bool UNI = false>
__device__ __forceinline__ void nb_cluster_body(const NbArgs& a, const bool owned_prune, float4 (*s_xyzq)[64], float4 (*s_lj)[64],
                                                float (*s_red)[3][64], float (*s_ownj)[64], float4 (*s_g)[64],
                                                unsigned long long (*s_mask)[64], const float4* __restrict__ etab = nullptr) {
    // the wave index is wave-uniform: say so, and tile number, list bounds and the chunk loop
    // live in SGPRs with scalar branches instead of VGPR compares and exec-mask loops
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // BW < WPT: the WPT waves of a tile sit in WPT / BW workgroups (systems of a few hundred tiles: with one workgroup per
    // tile 370 tiles land on 256 CUs as one or two per CU and the launch lasts as long as the CUs that got two)
    constexpr int SPLIT = BW < WPT ? WPT / BW : 1;
    static_assert(!UNI || (!ENERGY && !GEOM && !ALCH && !STEP), "the constant-sigma^2 body: force-only, Lorentz-Berthelot, no alchemical window");
    static_assert(SPLIT == 1 || HALF, "a tile split over workgroups returns its i-forces through atomics");
    constexpr int TPB = SPLIT > 1 ? 1 : BW / WPT;             // tiles per workgroup
    const uint32_t ntiles = a.tile_order ? a.t_count : a.T;   // (a decomposed handle launches its interior and boundary tiles apart)
    const uint32_t nblocks = SPLIT > 1 ? ntiles * SPLIT : (ntiles + TPB - 1) / TPB;
    const uint32_t per_xcd = (nblocks + 7) >> 3;
    // a decomposed rank's tile range is owned bricks (long lists) and halo shells (short lists) in spatial order: a
    // contiguous eighth per XCD would leave whole XCDs with halo tiles only, so there the tiles go round-robin
    constexpr bool TAIL = WPT == 1 && HALF && DUAL != 0 && !STEP && BW == 1;      // (mixed waves per tile, below)
    const bool tail_on = TAIL && a.tail_w > 1u;
    const uint32_t blk = (a.xcd_interleave || tail_on) ? blockIdx.x : (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
    if (!tail_on && blk >= nblocks) return;                   // whole workgroup
    const int tib = SPLIT > 1 ? 0 : wave / WPT;               // tile within the workgroup
    int part = SPLIT > 1 ? (int)(blk % SPLIT) * BW + wave : wave % WPT;   // which share of the tile's chunks
    uint32_t tidx = SPLIT > 1 ? blk / SPLIT : blk * TPB + tib;
    // Mixed waves per tile (one-wave class, dual list; NbArgs::tail_w): the launch is a list of work UNITS, per XCD range first the
    // head tiles as one unit each, then every closing tile as tail_w units - one-wave workgroups that share the tile's chunks the way
    // the waves of a 2 / 4-wave tile do (chunk c goes to unit c mod tail_w) and add their i-forces to the tile's rows with the
    // atomics this flavour uses anyway.  The units are what the hardware dispatches last: a quarter of a tile instead of a whole one
    // is what a SIMD may be left holding when its neighbours run dry.
    uint32_t wv = WPT;                                        // waves (units) this tile's chunks are shared between
    if (tail_on) {
        const uint32_t xcd = blockIdx.x & 7u, u = blockIdx.x >> 3;      // (the host sends this geometry out with xcd_interleave off only)
        tidx = xcd * a.tail_group + u;
        if (u >= a.tail_head) {
            const uint32_t v = u - a.tail_head;
            wv = a.tail_w;                                    // 2 or 4
            part = (int)(v & (wv - 1u));
            tidx = xcd * a.tail_group + a.tail_head + (v >> (wv == 4u ? 2 : 1));
        }
    }
    const bool t_ok = tidx < ntiles;                          // (the last workgroup may have a tile too many)
    if (WPT == 1 && !t_ok) return;
    // a.T = the null tile: empty list, nothing stored
    const uint32_t t = t_ok ? (a.tile_order ? __builtin_amdgcn_readfirstlane(a.tile_order[a.t_first + tidx]) : tidx) : a.T;
    const int ii = lane & 7, jj = lane >> 3;

    float xi[8], yi[8], zi[8], qi[8], sgi[8], epi[8], fx[8], fy[8], fz[8];
    if constexpr (STEP) {
        static_assert(HALF && !ENERGY && !ALCH && DUAL != 0, "one launch per step: half list, dual list");
        // lane = slot.  Every wave of the tile reconstructs the tile's positions (it needs them as i-atoms); the tile's FIRST wave also
        // finishes the last step for them: kick, next Y, path length, the words of the next launch.
        const uint32_t s = t * MDX_TILE + lane;
        const float4 Y = a.posq[s], Fp = a.st_fprev[s];
        const float4 x = step_pos(Y, Fp);        // (static and dummy slots carry w = 0)
        if (part == 0 && t_ok) {
            float4 v = a.st_vel[s];
            float d2w = 0.f, pw = 0.f;       // what this lane contributes to the words of the NEXT launch
            bool viol = false;
            if (v.w != 0.f) {   // w = 418.4/m; 0 marks static and dummy slots
                // (the chunk's first launch finishes a step that opens with a HALF kick: its force rows carry w / 2, st_kick is 0.5)
                const float w = Fp.w, kdt = a.st_kick * a.st_dt * v.w;
                const float4 Fm = a.st_fnext[s];                                // the forces of the stage before Fp's (the buffer this launch zeroes)
                const float kx = w * Fp.x, ky = w * Fp.y, kz = w * Fp.z;       // the kick's share of this step's displacement
                const float sx_ = fmaf(a.st_dt, v.x, kx), sy_ = fmaf(a.st_dt, v.y, ky), sz_ = fmaf(a.st_dt, v.z, kz);      // x - x(previous stage)
                v.x = fmaf(kdt, Fp.x, v.x); v.y = fmaf(kdt, Fp.y, v.y); v.z = fmaf(kdt, Fp.z, v.z);
                float path;
                const float4 r = a.ref[s];
                const float dpr = __builtin_sqrtf((x.x - r.x) * (x.x - r.x) + (x.y - r.y) * (x.y - r.y) + (x.z - r.z) * (x.z - r.z));      // |x - ref|, exactly
                if (DUAL == 2) {   // this launch is a pruning pass: the inner list it writes is exact at x, paths count from here
                    path = 0.f;
                    a.dprune[s] = dpr;
                } else path = a.path[s] + __builtin_sqrtf(sx_ * sx_ + sy_ * sy_ + sz_ * sz_);
                a.path[s] = path;
                // The words that let this launch run were raised by the launch before it from Y and a GRANT for the kick it could not know
                // (below).  Now the stage is known exactly: had the words been raised from it, would this launch walk the inner list although
                // the path budget is spent, or run at all although the list is stale?  Then its forces are not to be trusted - the host
                // takes the step back to a list rebuild (rare: the atom that decides the word must also be the one that outran its grant).
                {
                    float dt2 = dpr * dpr;
                    if (!(dt2 < 1.0e30f)) dt2 = 3.0e38f;
                    viol = (DUAL != 2 && !(path <= a.st_path_thr)) || __float_as_uint(dt2) > a.thr_bits;
                }
                float4 yo = x;
                if (!a.st_last) {
                    yo.x = fmaf(a.st_dt, v.x, x.x); yo.y = fmaf(a.st_dt, v.y, x.y); yo.z = fmaf(a.st_dt, v.z, x.z);
                    // The next stage is yo + w F(x), F not known before this launch ends: the words that gate the next launch grant the
                    // kick w (|2 Fp - Fm| + |Fp - Fm| + 30 kcal/mol/A) - the force extrapolated from the last two stages and room for its
                    // curvature; ~0.01 A for a water hydrogen at 0.5 fs - and the next launch checks the words against what the stage turned out to be.
                    const float wf = a.st_dt * a.st_dt * v.w;
                    const float ex = 2.f * Fp.x - Fm.x, ey = 2.f * Fp.y - Fm.y, ez = 2.f * Fp.z - Fm.z;
                    const float gx = Fp.x - Fm.x, gy = Fp.y - Fm.y, gz = Fp.z - Fm.z;
                    const float m = a.st_grant * wf * (__builtin_sqrtf(ex * ex + ey * ey + ez * ez) + __builtin_sqrtf(gx * gx + gy * gy + gz * gz) + 30.f);
                    pw = path + a.st_dt * __builtin_sqrtf(v.x * v.x + v.y * v.y + v.z * v.z) + m;
                    const float db = __builtin_sqrtf((yo.x - r.x) * (yo.x - r.x) + (yo.y - r.y) * (yo.y - r.y) + (yo.z - r.z) * (yo.z - r.z)) + m;
                    d2w = db * db;
                    if (!(d2w < 1.0e30f)) d2w = 3.0e38f;      // NaN / inf -> huge, forces a stop
                }
                a.st_vel[s] = v;
                a.st_yout[s] = yo;
            } else a.st_yout[s] = Y;
            a.st_fnext[s] = make_float4(0.f, 0.f, 0.f, a.st_dt * a.st_dt * v.w);
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) { d2w = fmaxf(d2w, __shfl_xor(d2w, m)); pw = fmaxf(pw, __shfl_xor(pw, m)); }
            const bool any_viol = __any(viol);
            if (lane == 0) {
                if (a.st_disp_out && __float_as_uint(d2w) > a.thr_bits) atomicMax(a.st_disp_out, __float_as_uint(d2w));
                if (a.st_prune_out && !(pw <= a.st_path_thr)) *a.st_prune_out = 1u;
                if (any_viol) { *a.st_viol = 1u; if (a.st_disp_out) atomicMax(a.st_disp_out, __float_as_uint(1.0e20f)); }      // (the launches behind this one stay no-ops)
            }
            // one wave per tile: the bonded roles of this tile's atoms at x as well, partners through the same two rows; the force leaves
            // right away (three atomics per atom into the buffer this launch accumulates - nothing of this stays live across the chunk
            // loop).  (Eight waves per tile: the roles ride in extra workgroups of the launch, bonded_workgroup.)
            if (WPT == 1 && a.b_role_off) {
                const uint32_t rb = a.b_role_off[s], re = a.b_role_off[s + 1];
                if (re > rb) {
                    float bx = 0.f, by = 0.f, bz = 0.f;
                    RoleEnergies en;
                    for (uint32_t k = rb; k < re; ++k) role_eval_step<false>(a.b_roles[k], a.b_prm, x, a.posq, a.st_fprev, a.b_p, bx, by, bz, en);
                    float* const fb_ = reinterpret_cast<float*>(a.force) + (size_t)s * 4;
                    unsafeAtomicAdd(fb_, bx); unsafeAtomicAdd(fb_ + 1, by); unsafeAtomicAdd(fb_ + 2, bz);
                }
            }
        }
        s_xyzq[wave][lane] = x;
        WAVE_LDS_SYNC();
#pragma unroll
        for (int ci = 0; ci < 8; ++ci) {
            const float4 pi = s_xyzq[wave][ci * MDX_CLUSTER + ii];
            const float2 li = a.lj[t * MDX_TILE + ci * MDX_CLUSTER + ii];
            xi[ci] = pi.x; yi[ci] = pi.y; zi[ci] = pi.z; qi[ci] = pi.w; sgi[ci] = li.x; epi[ci] = li.y;
            fx[ci] = 0.f; fy[ci] = 0.f; fz[ci] = 0.f;
        }
        WAVE_LDS_SYNC();
    } else {
#pragma unroll
    for (int ci = 0; ci < 8; ++ci) {
        const uint32_t s = t * MDX_TILE + ci * MDX_CLUSTER + ii;
        const float4 pi = a.posq[s];
        const float2 li = UNI ? make_float2(0.f, reinterpret_cast<const float*>(a.lj)[2 * s + 1]) : a.lj[s];      // (UNI: sgi[] is never read)
        xi[ci] = pi.x; yi[ci] = pi.y; zi[ci] = pi.z; qi[ci] = pi.w; sgi[ci] = li.x; epi[ci] = li.y;
        fx[ci] = 0.f; fy[ci] = 0.f; fz[ci] = 0.f;
    }
    }
    ListCounts cnt = a.counts[t_ok ? t : 0];
    if (!t_ok) { cnt.n_masked = 0; cnt.n_plain = 0; }
    const uint32_t e0 = a.entry_off[t_ok ? t : 0];
    // DUAL == 1: the inner list.  Same offsets and the same masked run as the Verlet list (exclusion masks are addressed
    // by chunk position); of the plain run, wave `part` finds the survivors of ITS chunks (c = part, part + WPT, ...)
    // compacted into the first of those chunk positions, and its own loop bound in inner_nch.
    const uint2* __restrict__ const entries = DUAL == 1 ? a.entries_in : a.entries;
    const uint32_t nmc = cnt.n_masked >> 3;
    const uint32_t nchunks = DUAL == 1 ? (t_ok ? a.inner_nch[t * 8 + part] : 0u) : (cnt.n_masked + cnt.n_plain) >> 3;
    const uint32_t mbase = a.mchunk_off[t_ok ? t : 0];
    float4* sx = s_xyzq[wave];
    // the wave's Lennard-Jones strip, one record per 16 B like the position strip (the entry loop reads both through ONE address
    // register, the second at an immediate offset): .x, .y = the j-atom's float2; UNI: .x = its sqrt(24 eps)
    float4* const sl = s_lj[wave];
    const float* __restrict__ const lj_eps = reinterpret_cast<const float*>(a.lj) + 1;      // (UNI) the .y of record k at [2 k]
    double elj = 0.0, ecoul = 0.0, evir = 0.0, ecross = 0.0, edudl = 0.0;
    uint32_t own_bits = 0xFFu;   // ENERGY only: bit ci set <=> i-atom (ci, ii) is owned by this rank
    if (ENERGY && !a.energy_all) {
        own_bits = 0;
#pragma unroll
        for (int ci = 0; ci < 8; ++ci)
            own_bits |= ((a.slot_flags[t * MDX_TILE + ci * MDX_CLUSTER + ii] >> 1) & 1u) << ci;
    }

    // two-deep software pipeline: entries of the wave's next-but-one chunk, atoms AND exclusion masks
    // of its next chunk are in flight while the current chunk is evaluated.  Everything a chunk
    // needs from HBM is issued one iteration ahead and consumed at the top of the loop, so the one
    // s_waitcnt vmcnt(0) per chunk sits where the data is a whole chunk old and the entry loop has
    // no vector-memory instruction in it (a mask fetched at its point of use - or an atomic issued
    // per entry - drags a vmcnt(0) into the loop and serialises the wave on memory latency).
    //
    // LATCH2 (the one-wave half-list kernels with the constant-sigma^2 body: plain list, the dual-list twins, the merged launch): in the
    // PLAIN chunks the pipeline exists twice.  In a half-list loop that one wait sits a handful of instructions behind the chunk's last
    // j-force atomic.  The atomic leaves from inside the entry loop, whose every entry may skip it, so the compiler cannot count the
    // operations behind the loads and waits for zero (and a count would not help: loads and no-return atomics share vmcnt and retire in no
    // fixed order among each other): the wave pays close to an atomic's round trip at every chunk.  With two register sets, each a
    // pipeline of its own over every second plain chunk of the wave's share (each fetches atoms one and entries two of ITS chunks ahead),
    // and the chunk loop unrolled by two, the wait at the head of set 0's chunk retires set 1's loads as well - they are a whole chunk
    // old by then - and set 1's chunk begins without one: one vmcnt(0) per two chunks, none written by hand (plain_pass2 below).  The
    // strip is one.  Nine more registers in the plain loop.  The masked chunks at the head of the list (5 - 10 %) keep one set: with two
    // there, exclusion words included, every one of these kernels went to 128 VGPRs and 100 - 250 B of scratch.  Taken where the register
    // report leaves four waves per SIMD without scratch: the general bodies (122 - 128 VGPRs), the multi-wave classes, STEP and the energy
    // flavours keep one set throughout, and the full lists have no atomic to wait for.
    struct JSet {
        float4 nj, nf;               // the chunk in flight: j-atom of this lane (STEP: nf = the force row beside the j-atom's Y),
        float2 nl;                   // its Lennard-Jones record,
        uint32_t ny, njc;            // its entry's word and j-cluster,
        float nown;                  // (ENERGY, HALF) 1.0 <=> the j-atom is owned here,
        unsigned long long nmq;      // its exclusion bits (masked chunks)
        uint2 ent;                   // the entry of the set's chunk after that one
    };
    constexpr bool LATCH2 = nb_latch2(HALF, UNI, WPT, ENERGY, ALCH, STEP);
    JSet S0 = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), make_float2(0.f, 0.f), 13u, 0u, 0.f, ~0ull, make_uint2(0u, 13u)};
    JSet S1 = S0;
    auto prime = [&](JSet& X, const uint32_t c0) __attribute__((always_inline)) {
        if (c0 < nchunks) {
            const uint2 ent = entries[e0 + c0 * 8 + (lane >> 3)];
            if (c0 < nmc) X.nmq = a.masks[(size_t)(mbase + c0) * 64 + lane];
            if (c0 + wv < nchunks) X.ent = entries[e0 + (c0 + wv) * 8 + (lane >> 3)];
            const uint32_t js = ent.x * MDX_CLUSTER + (lane & 7);
            X.nj = a.posq[js]; X.ny = ent.y; X.njc = ent.x;
            if (UNI) X.nl.y = lj_eps[2 * js]; else X.nl = a.lj[js];
            if (STEP) X.nf = a.st_fprev[js];
            if (ENERGY && HALF) X.nown = a.energy_all ? 1.0f : (float)((a.slot_flags[js] >> 1) & 1u);
        }
    };
    prime(S0, (uint32_t)part);
    float* const fbase = reinterpret_cast<float*>(a.force);
    // (HALF) loop invariants of the per-entry j-force tail: which component this lane carries through the last reduction level, and
    // the byte offset of its word in the j-cluster's eight force rows
    const bool jsel_x = ii == 0 || ii == 7, jsel_y = ii == 1 || ii == 6;
    const uint32_t jlane_off = (uint32_t)(jj * 4 + ii) * 4u;
    float4* const sg = s_g[HALF ? wave : 0];
    // Dual pair list.  Normal launch (DUAL 1): the list is the INNER one: cluster pairs that had an atom pair within
    // cutoff + inner_skin at the last pruning pass.  Pruning launch (DUAL 2; forced by the host after a rebuild, or asked
    // for by the drift pass through the step's prune word when some atom's path length since the last pass exceeded
    // inner_skin/2): walk the Verlet list, evaluate as usual, and while the distances are at hand ballot every cluster
    // pair against the inner radius; the surviving masks go to the inner list (masked run in place, this wave's plain
    // entries compacted), and the tile's path accumulators are cleared.  Decided on the device: the host enqueues blind.
    constexpr bool prune = DUAL == 2;
    uint32_t kept = 0;
#ifdef NB_HALF_STATS
    uint32_t dbg_jh = 0, dbg_ih = 0, dbg_q = 0, dbg_pairs = 0;
#endif
    // (pruning launch) first plain chunk of this wave's share, and how many compacted plain entries it has written
    const uint32_t c_first = nmc + (TAIL ? (((uint32_t)part + wv - (nmc & (wv - 1u))) & (wv - 1u)) : ((uint32_t)part + WPT - nmc % WPT) % WPT);
    uint32_t wcur = 0;
    // HALF: the j-forces of a chunk collect in the wave's LDS strip and leave as three 64-lane
    // atomics (x, y, z of j-atom `lane`) when the chunk is done: always three, issued AFTER the
    // prefetch loads, so the loads' waits at the top of the next chunk are vmcnt(3) and the
    // atomics stay in flight (lanes of list padding add 0 to their own i-slot)
    // (HALF) retire the prologue's loads here: the loop then never waits at its top, where the
    // atomics of the previous chunk are still in flight
    if (HALF && NB_HALF_FLUSH) __builtin_amdgcn_s_waitcnt(0x0F70);
    const float rc2_s = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a.p.rc2_lj)));   // an SGPR operand of v_cmpx
    // The chunk loop exists twice (round 3): the masked chunks at the head of the wave's share, then the plain ones - see the
    // entry loop.  The software pipeline's state (JSet) carries over from the first loop into the second.
    // One chunk: c = its position, X = the set that holds it, ps = the chunk stride of that set (two sets: 2 wv).
    auto chunk = [&](auto masked_tag, auto two_tag, const uint32_t c, JSet& X) __attribute__((always_inline)) {
        constexpr bool MASKED_CHUNK = decltype(masked_tag)::value, TWO = decltype(two_tag)::value;
        const uint32_t ps = TWO ? 2u * wv : wv;
        uint32_t cur_y = X.ny, cur_jc = X.njc;
        // (two sets: the copies are made HERE, behind the wait that retired the set.  Left to the allocator, a set's registers rotate at
        // the end of its chunk - entry -> word in flight -> current word - and a copy there waits for the loads just issued.)
        if (TWO) asm volatile("" : "+v"(cur_y), "+v"(cur_jc));
        constexpr bool masked = MASKED_CHUNK;
        if (masked) s_mask[wave][lane] = X.nmq;                 // read back a byte per entry: two VGPRs fewer
        if (ENERGY && HALF) s_ownj[wave][lane] = X.nown;
        if (HALF && NB_HALF_FLUSH) {
            // the lane that staged j-atom `lane` also flushes its force: remember where it goes.
            // List padding (imask 0) has no force: it will add 0 to this lane's own i-slot.
            const bool live = ((X.ny >> 8) & 0xFFu) != 0u;
            sg[lane] = make_float4(0.f, 0.f, 0.f, __uint_as_float(live ? X.njc * MDX_CLUSTER + (uint32_t)ii : t * MDX_TILE + lane));
        }
        {   // image shift, then park in LDS
            const uint32_t code = X.ny & 31u;
            // (in place, as the load below is: shifted atom, LDS store and the next load share one register tuple - through a copy
            // the tuple splits and the compiler mends it with moves right behind the load, each a wait for the load just issued)
            if (STEP) X.nj = step_pos(X.nj, X.nf);
            float rx, ry, rz;
            image_shift_row(code, a.p.shift, rx, ry, rz);
            X.nj.x += rx; X.nj.y += ry; X.nj.z += rz;
            sx[lane] = X.nj;
            // (once per chunk; the 16-B stride makes this store a 4-way bank conflict)
            if (UNI) sl[lane].x = X.nl.y; else *reinterpret_cast<float2*>(&sl[lane]) = X.nl;
        }
        WAVE_LDS_SYNC();
        if constexpr (TWO) {
            // Every load unconditional: behind a branch the loaded registers meet their old values in a phi, the compiler resolves it
            // with copies right behind the load, and the copies wait for the load just issued.  A set with no chunk left reads the
            // current chunk's records again (valid addresses, lines this wave has just had), and nothing uses them.
            // (X.ent is a list entry at all times - the set's next one, the null entry of the prologue or such a re-read - so js is an atom.)
            const uint32_t ce = c + 2u * ps < nchunks ? c + 2u * ps : c;
            const uint32_t js = X.ent.x * MDX_CLUSTER + (lane & 7);
            X.ny = X.ent.y; X.njc = X.ent.x;
            asm volatile("" : "+v"(X.ny), "+v"(X.njc));
            X.nj = a.posq[js];
            X.nl.y = lj_eps[2 * js];
            X.ent = entries[e0 + ce * 8 + (lane >> 3)];
        } else {
        if (c + ps < nmc) X.nmq = a.masks[(size_t)(mbase + c + ps) * 64 + lane];
        if (c + ps < nchunks) {
            const uint32_t js = X.ent.x * MDX_CLUSTER + (lane & 7);
            X.ny = X.ent.y; X.njc = X.ent.x;
            // (copied HERE: sunk below the entry's load, the copies keep the load out of the entry's registers.  Not in the STEP bodies,
            // which sit at 128 VGPRs with scratch and took 4 - 16 B more of it with the pin)
            if (!STEP) asm volatile("" : "+v"(X.ny), "+v"(X.njc));
            X.nj = a.posq[js];
            if (UNI) X.nl.y = lj_eps[2 * js]; else X.nl = a.lj[js];
            if (STEP) X.nf = a.st_fprev[js];
            if (ENERGY && HALF) X.nown = a.energy_all ? 1.0f : (float)((a.slot_flags[js] >> 1) & 1u);
            if (c + 2 * ps < nchunks) X.ent = entries[e0 + (c + 2 * ps) * 8 + (lane >> 3)];
        }
        }
        float celj = 0.f, cecoul = 0.f, cevir = 0.f, cecross = 0.f, cedudl = 0.f;   // (ENERGY) fp32 partial sums of this chunk
        uint32_t newy = cur_y & 0xFFu;                                // (pruning launch) this lane's entry word with the inner mask
        // entry loop: each entry's j record is read from LDS where it is needed (any look-ahead measured slower).
        // Two copies of it (round 3, NB_SPLIT_MASKED): exclusion bits only exist in the masked chunks at the head of a tile's list;
        // the plain chunks (90-95 %) run a body without the per-pair v_bfe_i32 that turns a mask bit into the NaN addend of r^2
        // (one VALU instruction of ~29 per cluster pair; 16 k extra bytes of code).
#pragma unroll 1
        for (int e = 0; e < 8; ++e) {
            const float4 pj = sx[e * 8 + jj];
            const float2 lj = UNI ? make_float2(0.f, sl[e * 8 + jj].x) : *reinterpret_cast<const float2*>(&sl[e * 8 + jj]);
            const uint32_t im = (__builtin_amdgcn_readlane(cur_y, e * 8) >> 8) & 0xFFu;  // wave-uniform
            if (im == 0) continue;
            uint32_t newm = 0;
            // (as EXCLUDED bits: bit ci set <=> this lane's pair with i-cluster ci is masked out)
            const int x8 = MASKED_CHUNK ? (int)(~(uint32_t)reinterpret_cast<const uint8_t*>(&s_mask[wave][lane])[e]) : 0;
            float g[3] = {-0.f, -0.f, -0.f};      // the force on j (pair_eval subtracts into it; -0: the negative of a sum that starts at +0)
            float wj = 0.f;
            if (ENERGY && HALF) wj = 0.5f * s_ownj[wave][e * 8 + jj];
#pragma unroll
            for (int ci = 0; ci < 8; ++ci) {
                if (im & (1u << ci)) {
                    float e1 = 0.f, e2 = 0.f, e3 = 0.f, e4 = 0.f, e5 = 0.f;
                    // 0.0f or NaN: sign-extend bit ci of the exclusion byte over the word (one v_bfe_i32)
                    const float bias = MASKED_CHUNK ? __int_as_float((x8 << (31 - ci)) >> 31) : 0.f;
                    float r2v = 0.f;
                    constexpr bool ASM_PAIR = NB_ASM_PAIR && !ENERGY && COUL == CM_SHIFTED && !GEOM && SAMECUT && HALF && !ALCH && !UNI;
                    if constexpr (ASM_PAIR)
                        pair_eval_asm<MASKED_CHUNK, prune>(xi[ci], yi[ci], zi[ci], qi[ci], sgi[ci], epi[ci], pj, lj, rc2_s, bias, fx[ci], fy[ci], fz[ci],
                                                           g[0], g[1], g[2], r2v);
                    else
                    pair_eval<ENERGY, COUL, GEOM, SAMECUT, true, HALF, ALCH, MASKED_CHUNK, UNI>(xi[ci], yi[ci], zi[ci], qi[ci], sgi[ci], epi[ci],
                                                                             pj, lj, true, a.p, fx[ci], fy[ci],
                                                                             fz[ci], e1, e2, g, ENERGY ? &e3 : nullptr,
                                                                             (ENERGY && ALCH) ? &e4 : nullptr, bias,
                                                                             prune ? &r2v : nullptr, (ENERGY && ALCH) ? &e5 : nullptr, etab);
                    if (prune) {   // any allowed atom pair of this cluster pair inside the inner radius?
                        const unsigned long long bb = __ballot(r2v < a.rin2);
                        if (bb != 0ull) newm |= 1u << ci;
#ifdef NB_HALF_STATS
                        if (bb != 0ull) {
                            const unsigned long long ilo = 0x0F0F0F0F0F0F0F0Full;
                            dbg_jh += ((uint32_t)bb != 0u) + ((bb >> 32) != 0ull);
                            dbg_ih += ((bb & ilo) != 0ull) + ((bb & ~ilo) != 0ull);
                            dbg_q += (((uint32_t)bb & 0x0F0F0F0Fu) != 0u) + (((uint32_t)bb & 0xF0F0F0F0u) != 0u) +
                                     (((uint32_t)(bb >> 32) & 0x0F0F0F0Fu) != 0u) + (((uint32_t)(bb >> 32) & 0xF0F0F0F0u) != 0u);
                            dbg_pairs += __popcll(bb);
                        }
#endif
                    }
                    if (ENERGY && HALF) {   // a pair's energy is split between the owners of its two atoms
                        const float w = wj + (((own_bits >> ci) & 1u) ? 0.5f : 0.f);
                        celj += w * e1; cecoul += w * e2; cevir += w * e3; cecross += w * e4; cedudl += w * e5;
                    } else if (ENERGY && ((own_bits >> ci) & 1u)) { celj += e1; cecoul += e2; cevir += e3; cecross += e4; cedudl += e5; }
                }
            }
            if (prune) {
                kept += __popc(newm);
                if (jj == e) newy |= newm << 8;
            }
            if (HALF && NB_HALF_FLUSH) {
                // (the experiment keeps the three-register form: every lane ends with the three totals)
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    g[d] = dpp_xadd<0xB1>(g[d]);
                    g[d] = dpp_xadd<0x4E>(g[d]);
                    g[d] = dpp_xadd<0x141>(g[d]);
                }
                if (ii < 3) reinterpret_cast<float*>(sg)[(e * 8 + jj) * 4 + ii] = ii == 0 ? g[0] : (ii == 1 ? g[1] : g[2]);
            } else if (HALF) {
                // sum over the eight i-lanes of every j-atom, in full exec (jforce_reduce8); lanes ii < 3 then hold x, y, z of the
                // j-atom's force and add it to its row: 24 lanes, one 128-B line, at a wave-uniform base + this lane's offset
                const float v = jforce_reduce8(g, jsel_x, jsel_y);
                // (keep the base in scalar registers: the atomic then takes it as its saddr operand with the lane offset beside it;
                // otherwise fbase + lane offset is hoisted as a 64-bit vector pointer and every entry pays a v_lshl_add_u64)
                typedef __attribute__((address_space(1))) char gchar;
                gchar* frow = (gchar*)(fbase + (size_t)__builtin_amdgcn_readlane(cur_jc, e * 8) * (MDX_CLUSTER * 4));
                asm("" : "+s"(frow));
                if (ii < 3) {
                    uint32_t off = jlane_off;
                    asm("" : "+v"(off));      // (the 32-bit offset is widened HERE, where instruction selection sees it beside the atomic)
#ifdef NB_EXP_NOATOMIC
                    if (v == 1.2345e30f)
#endif
                    unsafeAtomicAdd((float*)(frow + off), v);
                }
            }
        }
        if (ENERGY) { elj += (double)celj; ecoul += (double)cecoul; evir += (double)cevir; ecross += (double)cecross; edudl += (double)cedudl; }
        if (prune) {
            if (masked) {                       // exclusion masks are addressed by chunk position: the entry stays where it is
                if (ii == 0) a.entries_in[e0 + c * 8 + jj] = make_uint2(cur_jc, newy);
            } else {                            // plain run: survivors move up into this wave's first chunk positions
                const bool alive = ii == 0 && (newy >> 8) != 0u;
                const unsigned long long bal = __ballot(alive);
                if (alive) {
                    const uint32_t k = wcur + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
                    a.entries_in[e0 + (c_first + (k >> 3) * wv) * 8 + (k & 7u)] = make_uint2(cur_jc, newy);
                }
                wcur += (uint32_t)__popcll(bal);
            }
        }
        WAVE_LDS_SYNC();
        if (HALF && NB_HALF_FLUSH) {
            // Flush: 192 floats = 3 instructions x 64 lanes, lane l of instruction k taking float
            // k*64 + l of the packed [64 atoms][xyz] view, so consecutive lanes hit consecutive words
            // and an instruction touches each 128-B line once.  (x of all atoms, then y, then z hits
            // every line three times in a row and is 3x slower; a per-entry 24-lane atomic inside the
            // entry loop makes every wait in the loop a vmcnt(0): tools/ubench/atomic_flush.hip.)
            // The prefetch issued before this chunk's arithmetic has landed long ago: retire it here,
            // so that nothing after the atomics has to wait on the vector-memory counter.
            __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0), expcnt/lgkmcnt untouched
            const float* const sgf = reinterpret_cast<const float*>(sg);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint32_t fidx = (uint32_t)(k * 64 + lane), atom = (fidx * 171u) >> 9, comp = fidx - 3u * atom;
                const uint32_t slot = __float_as_uint(sgf[atom * 4 + 3]);
                unsafeAtomicAdd(fbase + (size_t)slot * 4 + comp, sgf[atom * 4 + comp]);
            }
        }
    };
    auto chunk_pass = [&](auto masked_tag, const uint32_t c_begin, const uint32_t c_end) __attribute__((always_inline)) {
        for (uint32_t c = c_begin; c < c_end; c += wv) chunk(masked_tag, std::false_type{}, c, S0);
    };
    // (LATCH2) the plain chunks, two per trip: set 0, then set 1.  At the hand-over set 0 holds the first plain chunk and the entry of the
    // second, as the one-set loop in front left them; set 1 is loaded from that entry, and each set fetches the entry of ITS next chunk.
    // These few loads are waited for once per tile.  (X.ent is a list entry at all times, chunk(): the addresses are atoms.)
    auto plain_pass2 = [&](const uint32_t c_begin, const uint32_t c_end) __attribute__((always_inline)) {
        if (c_begin >= c_end) return;
        {
            const uint32_t js = S0.ent.x * MDX_CLUSTER + (lane & 7);
            S1.ny = S0.ent.y; S1.njc = S0.ent.x;
            S1.nj = a.posq[js];
            S1.nl.y = lj_eps[2 * js];
            const uint32_t c2 = c_begin + 2u * wv < nchunks ? c_begin + 2u * wv : c_begin, c3 = c_begin + 3u * wv < nchunks ? c_begin + 3u * wv : c_begin;
            // (set 0's entry LAST: the first chunk needs it at once, and the wait for the youngest load retires them all - with
            // a younger one in flight the compiler's count for set 1's entry stays in the loop as a second wait per trip)
            S1.ent = entries[e0 + c3 * 8 + (lane >> 3)];
            S0.ent = entries[e0 + c2 * 8 + (lane >> 3)];
        }
        for (uint32_t c = c_begin; c < c_end; c += wv) {
            chunk(std::false_type{}, std::true_type{}, c, S0);
            c += wv;
            if (c >= c_end) break;
            chunk(std::false_type{}, std::true_type{}, c, S1);
        }
    };
#ifndef NB_SPLIT_MASKED
#define NB_SPLIT_MASKED 1
#endif
    if (NB_SPLIT_MASKED) {
        const uint32_t c_mid = c_first < nchunks ? c_first : nchunks;      // this wave's first plain chunk
        chunk_pass(std::true_type{}, (uint32_t)part, c_mid);
        if constexpr (LATCH2) plain_pass2(c_mid, nchunks);
        else chunk_pass(std::false_type{}, c_mid, nchunks);
    } else chunk_pass(std::true_type{}, (uint32_t)part, nchunks);
    // sum the eight j-lanes of every i-atom (lanes ii, ii+8, ..., ii+56), then lane (ii, jj) keeps
    // i-cluster ci == jj: slot tile*64 + jj*8 + ii == tile*64 + lane, a coalesced store.
    float ox = 0.f, oy = 0.f, oz = 0.f;
#pragma unroll
    for (int ci = 0; ci < 8; ++ci) {
        float x = fx[ci], y = fy[ci], z = fz[ci];
#pragma unroll
        for (int m = 8; m < 64; m <<= 1) {
            x += __shfl_xor(x, m); y += __shfl_xor(y, m); z += __shfl_xor(z, m);
        }
        if (jj == ci) { ox = x; oy = y; oz = z; }
    }
    float* const fi = fbase + (size_t)(t * MDX_TILE + lane) * 4;
    // (the one-launch-per-step bodies keep the strided form: two of them, at 128 VGPRs, would pay for the strip's round trip with scratch)
    constexpr bool IFORCE_ROWS = HALF && NB_IFORCE_ROWS && !STEP;
    if (prune && t_ok) {
        // pad the last compacted chunk with null entries (imask 0), publish this wave's loop bound
        const uint32_t nfull = (wcur + 7u) >> 3;
        if ((uint32_t)lane < nfull * 8u - wcur) {
            const uint32_t k = wcur + (uint32_t)lane;
            a.entries_in[e0 + (c_first + (k >> 3) * wv) * 8 + (k & 7u)] = make_uint2(a.T * MDX_CL_PER_TILE, 13u);
        }
        if (lane == 0) a.inner_nch[t * 8 + part] = nfull ? c_first + (nfull - 1u) * wv + 1u : nmc;
    }
    if (prune) {
        // path lengths count from this pass (a boundary pass asked for by the ghosts alone restarts the ghosts only)
        if (!STEP && part == 0 && t_ok && (owned_prune || !(a.slot_flags[t * MDX_TILE + lane] & 2u))) {      // (STEP: the tile's wave did this where it had x)
            const uint32_t s = t * MDX_TILE + lane;
            if (a.path) {      // path split: the accumulator restarts, and the displacement reached so far is kept for the drift pass's bound
                const float4 x = a.posq[s], r = a.ref[s];
                const float dx = x.x - r.x, dy = x.y - r.y, dz = x.z - r.z;
                a.path[s] = 0.f; a.dprune[s] = __builtin_sqrtf(dx * dx + dy * dy + dz * dz);
            } else a.ref[s].w = 0.f;
        }
        if (lane == 0 && kept) atomicAdd(a.inner_count + ((blk * BW + wave) & (MDX_EPART - 1)), (unsigned long long)kept);
        if (lane == 0 && blk == 0 && wave == 0) atomicAdd(a.inner_count + MDX_EPART, 1ull);
#ifdef NB_HALF_STATS
        if (lane == 0) {
            atomicAdd(a.inner_count + MDX_EPART + 1, (unsigned long long)dbg_jh); atomicAdd(a.inner_count + MDX_EPART + 2, (unsigned long long)dbg_ih);
            atomicAdd(a.inner_count + MDX_EPART + 3, (unsigned long long)dbg_q); atomicAdd(a.inner_count + MDX_EPART + 4, (unsigned long long)kept);
            atomicAdd(a.inner_count + MDX_EPART + 5, (unsigned long long)dbg_pairs);
        }
#endif
    }
    if (WPT > 1) {   // fixed-order sum of the waves' partial forces
        s_red[wave][0][lane] = ox; s_red[wave][1][lane] = oy; s_red[wave][2][lane] = oz;
        __syncthreads();
        if ((SPLIT > 1 ? wave == 0 : part == 0) && t_ok) {
            const int w0 = SPLIT > 1 ? 0 : tib * WPT;
            ox = s_red[w0][0][lane]; oy = s_red[w0][1][lane]; oz = s_red[w0][2][lane];
#pragma unroll
            for (int w = 1; w < (SPLIT > 1 ? BW : WPT); ++w) { ox += s_red[w0 + w][0][lane]; oy += s_red[w0 + w][1][lane]; oz += s_red[w0 + w][2][lane]; }
            // (HALF: the tile's rows as four contiguous 256-B atomics through this wave's own strip, mdx_pair_dev.h iforce_add_rows)
            if (IFORCE_ROWS) iforce_add_rows(fbase + (size_t)t * (MDX_TILE * 4), sx, lane, ox, oy, oz);
            else if (HALF) { unsafeAtomicAdd(fi, ox); unsafeAtomicAdd(fi + 1, oy); unsafeAtomicAdd(fi + 2, oz); }
            else a.force[t * MDX_TILE + lane] = make_float4(ox, oy, oz, 0.f);
        }
    } else {
        if (IFORCE_ROWS) iforce_add_rows(fbase + (size_t)t * (MDX_TILE * 4), sx, lane, ox, oy, oz);
        else if (HALF) { unsafeAtomicAdd(fi, ox); unsafeAtomicAdd(fi + 1, oy); unsafeAtomicAdd(fi + 2, oz); }
        else a.force[t * MDX_TILE + lane] = make_float4(ox, oy, oz, 0.f);
    }
    if (ENERGY) {
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            elj += __shfl_xor(elj, m);
            ecoul += __shfl_xor(ecoul, m);
            evir += __shfl_xor(evir, m);
            if (ALCH) { ecross += __shfl_xor(ecross, m); edudl += __shfl_xor(edudl, m); }
        }
        if (lane == 0) {   // full list: every pair is seen from both sides.  The atomics are spread over MDX_EPART
                           // slots: 65 k waves adding into three words took 2 ms (contended f64 atomics, ~10 ns each)
            double* q = a.energy + EN_COUNT + 8 + MDX_ESTRIDE * ((blk * BW + wave) & (MDX_EPART - 1));
            atomicAdd(q, HALF ? elj : 0.5 * elj);
            atomicAdd(q + 1, HALF ? ecoul : 0.5 * ecoul);
            atomicAdd(q + 2, HALF ? evir : 0.5 * evir);
            if (ALCH) { atomicAdd(q + 3, HALF ? ecross : 0.5 * ecross); atomicAdd(q + 4, HALF ? edudl : 0.5 * edudl); }
        }
    }
}

// The bonded gather as extra workgroups of the pair launch (DUAL 4, systems of a few hundred tiles): the pair tiles of
// such a system fill a fraction of the chip, so the gather's waves run beside them on idle CUs and the step is one
// launch shorter - at 23 k atoms the separate gather was 9.7 us of kernel and a ~4 us launch gap in a 72 us step.  Four
// lanes per atom as in bonded_gather_kernel (mdx_bonded.hip); the force leaves through atomics, as the pair kernel's
// does.  (At 1 M atoms the same arrangement costs more than it hides - the two compete for the memory-side atomic
// path, DESIGN.md section 4 - so the large-system classes keep the separate launch.)
template <bool STEP = false>
__device__ __forceinline__ void bonded_workgroup(const NbArgs& a, uint32_t wg, uint32_t wg_threads) {
    const uint32_t tid = wg * wg_threads + threadIdx.x;
    const uint32_t s = tid >> 2, q4 = tid & 3u;
    if (s >= a.b_S) return;
    const uint32_t rb = a.b_role_off[s], re = a.b_role_off[s + 1];
    if (re <= rb) return;      // quad-uniform
    // (one launch per step: positions in the step form, every atom reconstructed from its two rows - mdx_bonded_dev.h step_pos)
    const float4 self = STEP ? step_pos(a.posq[s], a.st_fprev[s]) : a.posq[s];
    float fx = 0.f, fy = 0.f, fz = 0.f;
    RoleEnergies en;
    for (uint32_t k = rb + q4; k < re; k += 4) {
        const RoleRec r = a.b_roles[k];
        if (STEP) role_eval_step<false>(r, a.b_prm, self, a.posq, a.st_fprev, a.b_p, fx, fy, fz, en);
        else role_eval<false>(r, a.b_prm, self, a.posq, a.b_p, fx, fy, fz, en);
    }
    fx = dpp_xadd<0xB1>(fx); fy = dpp_xadd<0xB1>(fy); fz = dpp_xadd<0xB1>(fz);   // lane ^ 1
    fx = dpp_xadd<0x4E>(fx); fy = dpp_xadd<0x4E>(fy); fz = dpp_xadd<0x4E>(fz);   // lane ^ 2
    if (q4 < 3) {
        float* const f = reinterpret_cast<float*>(a.force) + (size_t)s * 4;
        unsafeAtomicAdd(f + q4, q4 == 0 ? fx : (q4 == 1 ? fy : fz));
    }
}

#ifndef NB_STEP_WAVES3
#define NB_STEP_WAVES3 0      // one launch per step: 1 = three waves per SIMD (168 VGPRs) instead of four (128)
#endif
#ifndef NB_MERGED_NOINLINE
#define NB_MERGED_NOINLINE 0
#endif
template <bool ENERGY, int COUL, bool GEOM, bool SAMECUT, int WPT, bool HALF, bool ALCH, int DUAL, int BW>
__device__ __attribute__((noinline)) void nb_cluster_body_call(const NbArgs& a, const bool owned_prune, float4 (*s_xyzq)[64], float4 (*s_lj)[64],
                                                               float (*s_red)[3][64], float (*s_ownj)[64], float4 (*s_g)[64],
                                                               unsigned long long (*s_mask)[64], const float4* __restrict__ etab = nullptr) {
    nb_cluster_body<ENERGY, COUL, GEOM, SAMECUT, WPT, HALF, ALCH, DUAL, BW>(a, owned_prune, s_xyzq, s_lj, s_red, s_ownj, s_g, s_mask, etab);
}

template <bool ENERGY, int COUL, bool GEOM, bool SAMECUT, int WPT, bool HALF, bool ALCH = false, int DUAL = 0, bool FB = false, int SPLIT = 1, bool UNI = false>
__global__ __launch_bounds__((SPLIT > 1 ? WPT / SPLIT : (WPT > NB_WAVES ? WPT : NB_WAVES)) * 64, ((HALF && NB_HALF_FLUSH) || ENERGY || (DUAL == 5 && NB_STEP_WAVES3)) ? 3 : 4) void nb_cluster_kernel(NbArgs a) {
    if (a.gate && *a.gate > a.thr_bits) {
        // (one launch per step: the stale word travels on, the launches behind this one stay no-ops too)
        if ((DUAL == 5 || DUAL == 6) && a.st_disp_out && blockIdx.x == 0 && threadIdx.x == 0) atomicMax(a.st_disp_out, *a.gate);
        return;
    }
    // one launch per step: DUAL 5 = the merged launch of the one-wave class, the tile's wave evaluates its atoms' roles; DUAL 6 = the merged
    // launch of the eight-waves class with the bonded gather in extra workgroups (as DUAL 4)
    static_assert(DUAL != 5 || (WPT == 1 && !FB && SPLIT == 1), "one launch per step: the one-wave-per-tile class");
    static_assert(DUAL != 6 || (WPT == 8 && !FB), "one launch per step: the eight-waves-per-tile class");
    constexpr bool STEP = DUAL == 5 || DUAL == 6;
    static_assert(!UNI || (!ENERGY && !GEOM && !ALCH && !STEP && !FB && SPLIT == 1 && DUAL <= 3), "the constant-sigma^2 bodies that exist (launch_cluster)");
    static_assert(DUAL == 0 || (HALF && !ENERGY), "the dual list exists for the half-list force kernel");
    static_assert(!FB || DUAL != 0, "the bonded workgroups ride with the dual-list launches");
    constexpr int BW = SPLIT > 1 ? WPT / SPLIT : (WPT > NB_WAVES ? WPT : NB_WAVES);       // waves per workgroup
    if ((DUAL == 4 || DUAL == 6 || FB) && blockIdx.x >= a.pair_grid) {
        // (a twin launch: the bonded workgroups run in whichever of the two the device executes)
        if (DUAL == 1 || DUAL == 2) {
            const bool want_prune = (a.force_prune | *a.prune_flag) != 0u || (a.prune_flag2 && *a.prune_flag2 != 0u);
            if (want_prune != (DUAL == 2)) return;
        }
        bonded_workgroup<STEP>(a, blockIdx.x - a.pair_grid, BW * 64);
        return;
    }
    __shared__ float4 s_xyzq[BW][64];
    __shared__ float4 s_lj[BW][64];                           // the position strip's stride (UNI: .x only, else .x and .y of a record)
    __shared__ float s_red[WPT > 1 ? BW : 1][3][64];
    __shared__ float s_ownj[(ENERGY && HALF) ? BW : 1][64];   // 1.0 <=> the staged j-atom is owned here
    __shared__ float4 s_g[HALF ? BW : 1][64];                 // minus the chunk's j-forces (.w: the j-slot), until flushed
    __shared__ unsigned long long s_mask[BW][64];             // a masked chunk's per-lane exclusion bits
    // Ewald force flavour: the table of the smooth part (mdx_pair_dev.h) in dynamic LDS, one copy per workgroup
    extern __shared__ float4 s_dyn_etab[];
    const float4* etab = nullptr;
    if (COUL == CM_EWALD_TAB && !ENERGY && !ALCH) {
        for (uint32_t k = threadIdx.x; k < a.p.etab_n; k += BW * 64) s_dyn_etab[k] = a.p.etab[k];
        __syncthreads();
        // (biased by the byte offset of the table's first binade: pair_eval adds the masked bits of x, shifted, and nothing else)
        etab = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_dyn_etab) - ((EWALD_TAB_CBITS >> a.p.etab_shift) << 4));
    }
#ifdef NB_DRAIN_TRACE
    const unsigned long long drain_t0 = wall_clock64();
#endif
    if (DUAL == 0) {
        nb_cluster_body<ENERGY, COUL, GEOM, SAMECUT, WPT, HALF, ALCH, 0, BW, false, UNI>(a, true, s_xyzq, s_lj, s_red, s_ownj, s_g, s_mask, etab);
    } else {
        const bool owned_prune = (a.force_prune | *a.prune_flag) != 0u;
        const bool want_prune = owned_prune || (a.prune_flag2 && *a.prune_flag2 != 0u);
        if (DUAL >= 3) {        // merged launch: the device picks the body
#if NB_MERGED_NOINLINE
            static_assert(!UNI, "the experiment has the general bodies only");
            // (experiment: the two bodies as real functions, so that each keeps the register allocation of its stand-alone kernel)
            if (want_prune) nb_cluster_body_call<ENERGY, COUL, GEOM, SAMECUT, WPT, HALF, ALCH, 2, BW>(a, owned_prune, s_xyzq, s_lj, s_red, s_ownj, s_g, s_mask, etab);
            else nb_cluster_body_call<ENERGY, COUL, GEOM, SAMECUT, WPT, HALF, ALCH, 1, BW>(a, owned_prune, s_xyzq, s_lj, s_red, s_ownj, s_g, s_mask, etab);
#else
            if (want_prune) nb_cluster_body<ENERGY, COUL, GEOM, SAMECUT, WPT, HALF, ALCH, 2, BW, STEP, UNI>(a, owned_prune, s_xyzq, s_lj, s_red, s_ownj, s_g, s_mask, etab);
            else nb_cluster_body<ENERGY, COUL, GEOM, SAMECUT, WPT, HALF, ALCH, 1, BW, STEP, UNI>(a, owned_prune, s_xyzq, s_lj, s_red, s_ownj, s_g, s_mask, etab);
#endif
        } else {
            if (want_prune != (DUAL == 2)) return;
            nb_cluster_body<ENERGY, COUL, GEOM, SAMECUT, WPT, HALF, ALCH, DUAL == 2 ? 2 : 1, BW, false, UNI>(a, owned_prune, s_xyzq, s_lj, s_red, s_ownj, s_g, s_mask, etab);
        }
#ifdef NB_DRAIN_TRACE
        // every wave: the constant-rate clock at entry and at exit (after its atomics have left), HW_ID and XCC_ID (which SIMD of which
        // CU of which XCD it ran on), written by lane 0 with ordinary vector stores
        if (DUAL == 3 && a.drain) {
            __builtin_amdgcn_s_waitcnt(0);
            const unsigned long long t1 = wall_clock64();
            if ((threadIdx.x & 63u) == 0u) {
                uint4* const o = a.drain + 2 * ((size_t)blockIdx.x * BW + (threadIdx.x >> 6));
                o[0] = make_uint4((uint32_t)drain_t0, (uint32_t)(drain_t0 >> 32), (uint32_t)t1, (uint32_t)(t1 >> 32));
                o[1] = make_uint4(__builtin_amdgcn_s_getreg(4 | (31 << 11)), __builtin_amdgcn_s_getreg(20 | (31 << 11)), want_prune ? 1u : 0u, 1u);
            }
        }
#endif
    }
}

// The launches that exist with a constant-sigma^2 body (UNI; handles with one LJ atom type, `uni`): force-only, Lorentz-Berthelot, not
// the softened Coulomb - the one-wave half-list kernels (plain list, the dual-list twins, the merged launch) and the full-list
// kernels of four and eight waves per tile.  Everything else, and every handle that is not eligible, gets the general body.
// Returns the body that went out (mdx_pair_body_info): bit 0 = the UNI body, bit 1 = its chunk loop with two register sets (LATCH2).
template <bool ENERGY, int COUL, bool G, bool S, int WPT, bool HALF, int DUAL>
static uint32_t launch_cluster(bool uni, dim3 g, dim3 b, uint32_t lds, hipStream_t st, const NbArgs& a) {
    if constexpr (!ENERGY && !G && COUL != CM_SOFT) {
        if (uni) {
            hipLaunchKernelGGL((nb_cluster_kernel<false, COUL, false, S, WPT, HALF, false, DUAL, false, 1, true>), g, b, lds, st, a);
            return 1u | (nb_latch2(HALF, true, WPT, false, false, false) ? 2u : 0u);
        }
    }
    hipLaunchKernelGGL((nb_cluster_kernel<ENERGY, COUL, G, S, WPT, HALF, false, DUAL>), g, b, lds, st, a);
    return 0u;
}

template <bool ENERGY, int COUL>
void launch_variant(mdx_handle* h, const NbArgs& a_in, bool geom, bool samecut) {
    NbArgs a = a_in;
    const bool uni = h->uni_lj && !h->alch_on && !geom && a.p.uni_c != 0.f;
    uint32_t uni_used = 0u;      // (launch_cluster's word)
    const int var = mdx_nb_variant(h);
    // waves per tile: split a tile's list over the 4 waves of its workgroup when the launch has
    // fewer tiles than ~3 per SIMD (the chip holds 4 waves/SIMD of this kernel on 1024 SIMDs)
    int wpt = 1;
    const bool half = var == 5;
    // measured: 4 beats 1 at every size, 8 below ~130 k atoms (round 3: 192 k atoms / 3.1 k tiles 0.137 ms with 8, 0.125 with 4, 0.127
    // with 2; one rank of an 8-rank water1M - 2.0 k owned + 1.3 k ghost tiles - 0.111 / 0.106 / 0.112)
    // with 2; one rank of an 8-rank water1M - 2.0 k owned + 1.3 k ghost tiles - 0.111 with the bonded gather inside / 0.106 + 0.010 for its
    // own launch / 0.112: a decomposed handle, whose step loop cannot fuse the gather into the drift pass, keeps 8 up to 4096 tiles)
    if (var == 2) wpt = (a.T < mdx_wpt8_below(h)) ? 8 : 4;
    if (half) wpt = mdx_nb_wpt_half(h, a.T);               // (shared with the tile order of the list rebuild: mdx_internal.h)
    if (var == 4) wpt = 4;
    const uint32_t bw = std::max(wpt, NB_WAVES);
    const uint32_t tpb = (var == 1) ? NB_WAVES : bw / wpt;
    const uint32_t nblocks = ((a.tile_order ? a.t_count : a.T) + tpb - 1) / tpb;
    const uint32_t grid = ((nblocks + 7) / 8) * 8;
    if (nblocks == 0) return;
    dim3 g(grid), b(bw * 64);
    // mixed waves per tile (mdx_tail_plan): dual-list launches of the one-wave class over the order by length inside the XCD ranges - per
    // range tail_head one-unit tiles, then tail_w units for each closing tile.  Everything else keeps the grid above.
    if (half && wpt == 1 && a.inner && !ENERGY && !a.st_fprev && h->tail_w > 1u && h->tile_lpt_on && a.tile_order == h->d.tile_lpt && !a.xcd_interleave) {
        a.tail_group = (a.T + 7u) >> 3;
        const uint32_t tail = std::min(h->tail_tiles, a.tail_group);
        a.tail_w = h->tail_w; a.tail_head = a.tail_group - tail;
        g = dim3(8u * (a.tail_head + a.tail_w * tail));
    }
    if (a.inner) {      // (mdx_pair_launch_info: units per closing tile, closing tiles in the launch - the last XCD's range may be short)
        uint32_t n_tail = 0;
        for (uint32_t x = 0; a.tail_w && x < 8u; ++x) {
            const uint32_t in_range = a.T > x * a.tail_group ? std::min(a.T - x * a.tail_group, a.tail_group) : 0u;
            n_tail += in_range > a.tail_head ? in_range - a.tail_head : 0u;
        }
        h->pair_info_tail[0] = a.tail_w; h->pair_info_tail[1] = n_tail;
    }
#ifdef NB_DRAIN_TRACE
    if (a.inner && g_mdx_drain_on) {      // (the merged dual-list launch only; the buffer is sized by the largest grid seen)
        const size_t want = (size_t)g.x * bw * 2;
        if (want > g_mdx_drain_cap) {
            if (g_mdx_drain) (void)hipFree(g_mdx_drain);
            (void)hipMalloc((void**)&g_mdx_drain, sizeof(uint4) * want);
            g_mdx_drain_cap = want;
        }
        (void)hipMemsetAsync(g_mdx_drain, 0, sizeof(uint4) * want, h->stream);
        a.drain = g_mdx_drain; g_mdx_drain_n = (uint32_t)(g.x * bw);
    }
#endif
    // MDX_NB_LDS_PAD=<bytes> (experiment): dynamic LDS the pair kernel asks for and never touches, on handles whose reciprocal-space
    // chain runs on a side stream.  Four waves of this kernel per SIMD hold the whole register file, so the chain's kernels only get
    // a CU when a pair workgroup retires - the two time-slice instead of overlapping; padding the LDS footprint caps the pair
    // workgroups per CU and leaves registers and LDS for the chain.
    static const uint32_t lds_pad_env = [] { const char* e = std::getenv("MDX_NB_LDS_PAD"); return e ? (uint32_t)std::atoi(e) : 0u; }();
    const uint32_t lds_pad = ((h->pme_on && h->pme_overlap && !ENERGY) ? lds_pad_env : 0u) +
                             ((COUL == CM_EWALD_TAB && !ENERGY) ? a.p.etab_n * (uint32_t)sizeof(float4) : 0u);      // + the Ewald table
    // ONE kernel picks the inner-walk or the pruning body on the device (round 2 measured the merged launch at +1 % for 23 k atoms
    // and -0.4 % at 1 M, and launched the two flavours back to back for the large classes, the device running exactly one; since
    // the chunk loop exists twice the merged kernel is faster there too: the gated-off twin was ~5 us of a 550 us step).
    // MDX_DUAL_MERGED=0: never merge; 1: the eight-waves-per-tile class only.
    static const bool dual_merged = [] { const char* e = std::getenv("MDX_DUAL_MERGED"); return !(e && e[0] == '0'); }();
    // (round 3, after the two chunk loops: merged wins at every size - water1M 1812 -> 1827 steps/s; MDX_DUAL_MERGED=1: small class only)
    static const bool merge_all = [] { const char* e = std::getenv("MDX_DUAL_MERGED"); return !(e && (e[0] == '0' || e[0] == '1')); }();
    // below ~1000 tiles a tile's eight waves go to two workgroups of four (MDX_TILE_SPLIT=0 / 1 forces)
    static const int split_env = [] { const char* e = std::getenv("MDX_TILE_SPLIT"); return e ? (e[0] == '0' ? 0 : 1) : -1; }();
    const bool split2 = split_env >= 0 ? split_env == 1 : (a.tile_order ? a.t_count : a.T) < 1024u;
    static const bool fb_all = [] { const char* e = std::getenv("MDX_FUSE_BONDED"); return e && e[0] == '2'; }();   // A/B: also the twin launches of the large classes
    // which instantiation goes out (mdx_pair_launch_info: the parity tests name the body they hold against the oracle)
    auto note = [&](int dual, int w, int split, int fb) {
        uint32_t* const o = a.inner ? h->pair_info_step : h->pair_info_any;
        o[0] = (uint32_t)w; o[1] = (uint32_t)dual; o[2] = half ? 1u : 0u; o[3] = (uint32_t)COUL; o[4] = ENERGY ? 1u : 0u;
        o[5] = (uint32_t)split; o[6] = (uint32_t)fb; o[7] = a.tile_order ? a.t_count : a.T;
    };
    // dual list: the inner-walk kernel and the pruning kernel back to back, the device runs exactly one of them
#define NB_STEP(G, S)                                                                                                 \
    do {                                                                                                               \
        if constexpr (!ENERGY && !G && COUL != CM_SOFT) {                                                              \
            if (wpt == 1 && half && a.inner) {                                                                         \
                hipLaunchKernelGGL((nb_cluster_kernel<false, COUL, false, S, 1, true, false, 5>), g, b, lds_pad, h->stream, a); \
                note(5, 1, 1, 0);                                                                                      \
            } else if (wpt == 8 && half && a.inner && split2) {   /* a tile = two workgroups of four waves */          \
                NbArgs af = a;                                                                                         \
                const uint32_t nb2 = (a.tile_order ? a.t_count : a.T) * 2u;                                            \
                af.pair_grid = ((nb2 + 7) / 8) * 8;                                                                    \
                const dim3 gf(af.pair_grid + (a.b_S ? (uint32_t)(((size_t)a.b_S * 4 + 255) / 256) : 0u)), bf(256);     \
                hipLaunchKernelGGL((nb_cluster_kernel<false, COUL, false, S, 8, true, false, 6, false, 2>), gf, bf, lds_pad, h->stream, af); \
                note(6, 8, 2, 0);                                                                                      \
            } else if (wpt == 8 && half && a.inner) {                                                                  \
                NbArgs af = a; af.pair_grid = grid;                                                                    \
                const dim3 gf(grid + (a.b_S ? (uint32_t)(((size_t)a.b_S * 4 + bw * 64 - 1) / (bw * 64)) : 0u));        \
                hipLaunchKernelGGL((nb_cluster_kernel<false, COUL, false, S, 8, true, false, 6>), gf, b, lds_pad, h->stream, af); \
                note(6, 8, 1, 0);                                                                                      \
            } else h->onepass_refused = true;                                                                          \
        } else h->onepass_refused = true;                                                                              \
    } while (0)
#define NB_DUAL(G, S, D)                                                                                              \
    do {                                                                                                               \
        if (ENERGY) break;                                                                                             \
        if (fb_all && a.b_S && (wpt == 2 || wpt == 4)) {   /* bonded workgroups behind the pair grid of both twins */  \
            NbArgs af = a; af.pair_grid = grid;                                                                        \
            const dim3 gf(grid + (uint32_t)(((size_t)a.b_S * 4 + bw * 64 - 1) / (bw * 64)));                           \
            if (wpt == 2) hipLaunchKernelGGL((nb_cluster_kernel<false, COUL, G, S, 2, true, false, D, true>), gf, b, lds_pad, h->stream, af); \
            else hipLaunchKernelGGL((nb_cluster_kernel<false, COUL, G, S, 4, true, false, D, true>), gf, b, lds_pad, h->stream, af);          \
            h->bonded_fused = true; note(D, wpt, 1, 1);                                                                \
            break;                                                                                                     \
        }                                                                                                              \
        note(D, wpt == 8 || wpt == 2 || wpt == 1 ? wpt : 4, 1, 0);                                                     \
        if (wpt == 8) hipLaunchKernelGGL((nb_cluster_kernel<false, COUL, G, S, 8, true, false, D>), g, b, lds_pad, h->stream, a); \
        else if (wpt == 2) hipLaunchKernelGGL((nb_cluster_kernel<false, COUL, G, S, 2, true, false, D>), g, b, lds_pad, h->stream, a); \
        else if (wpt == 1) uni_used = launch_cluster<false, COUL, G, S, 1, true, D>(uni, g, b, lds_pad, h->stream, a);                 \
        else hipLaunchKernelGGL((nb_cluster_kernel<false, COUL, G, S, 4, true, false, D>), g, b, lds_pad, h->stream, a);               \
    } while (0)
#define NB_LAUNCH(G, S)                                                                                    \
    do {                                                                                                   \
        note(0, var == 1 ? 0 : ((h->alch_on && wpt != 8) ? 4 : wpt), 1, 0);   /* (the dual-list branches below overwrite it) */ \
        if (h->alch_on && wpt == 8) hipLaunchKernelGGL((nb_cluster_kernel<ENERGY, COUL, G, S, 8, true, COUL != CM_EWALD_TAB>), g, b, lds_pad, h->stream, a); \
        else if (h->alch_on) hipLaunchKernelGGL((nb_cluster_kernel<ENERGY, COUL, G, S, 4, true, COUL != CM_EWALD_TAB>), g, b, lds_pad, h->stream, a); \
        else if (a.st_fprev) { NB_STEP(G, S); }                                                                    \
        else if (var == 1) hipLaunchKernelGGL((nb_tile_kernel<ENERGY, COUL, G, S>), g, b, lds_pad, h->stream, a);     \
        else if (half && a.inner && dual_merged && wpt == 8 && split2 && !ENERGY) {   /* a tile = two workgroups of four waves */ \
            NbArgs af = a;                                                                                         \
            const uint32_t nb2 = (a.tile_order ? a.t_count : a.T) * 2u;                                            \
            af.pair_grid = ((nb2 + 7) / 8) * 8;                                                                    \
            const dim3 gf(af.pair_grid + (a.b_S ? (uint32_t)(((size_t)a.b_S * 4 + 255) / 256) : 0u)), bf(256);     \
            if (a.b_S) { hipLaunchKernelGGL((nb_cluster_kernel<false, COUL, G, S, 8, true, false, 4, false, 2>), gf, bf, lds_pad, h->stream, af); h->bonded_fused = true; note(4, 8, 2, 0); } \
            else { hipLaunchKernelGGL((nb_cluster_kernel<false, COUL, G, S, 8, true, false, 3, false, 2>), gf, bf, lds_pad, h->stream, af); note(3, 8, 2, 0); } \
        }                                                                                                          \
        else if (half && a.inner && dual_merged && wpt == 8 && a.b_S && !ENERGY) {                                 \
            NbArgs af = a; af.pair_grid = grid;                                                                    \
            const dim3 gf(grid + (uint32_t)(((size_t)a.b_S * 4 + bw * 64 - 1) / (bw * 64)));                       \
            hipLaunchKernelGGL((nb_cluster_kernel<false, COUL, G, S, 8, true, false, 4>), gf, b, lds_pad, h->stream, af); \
            h->bonded_fused = true; note(4, 8, 1, 0);                                                              \
        }                                                                                                          \
        else if (half && a.inner && dual_merged && (wpt == 8 || merge_all)) { NB_DUAL(G, S, 3); }                  \
        else if (half && a.inner) { if (!a.force_prune) NB_DUAL(G, S, 1); NB_DUAL(G, S, 2); }   /* (a pass the host forces: no twin) */ \
        else if (half && wpt == 8) hipLaunchKernelGGL((nb_cluster_kernel<ENERGY, COUL, G, S, 8, true>), g, b, lds_pad, h->stream, a); \
        else if (half && wpt == 2) hipLaunchKernelGGL((nb_cluster_kernel<ENERGY, COUL, G, S, 2, true>), g, b, lds_pad, h->stream, a); \
        else if (half && wpt == 1) uni_used = launch_cluster<ENERGY, COUL, G, S, 1, true, 0>(uni, g, b, lds_pad, h->stream, a);    \
        else if (half) hipLaunchKernelGGL((nb_cluster_kernel<ENERGY, COUL, G, S, 4, true>), g, b, lds_pad, h->stream, a); \
        else if (wpt == 8) uni_used = launch_cluster<ENERGY, COUL, G, S, 8, false, 0>(uni, g, b, lds_pad, h->stream, a);           \
        else if (wpt == 4) uni_used = launch_cluster<ENERGY, COUL, G, S, 4, false, 0>(uni, g, b, lds_pad, h->stream, a);           \
        else hipLaunchKernelGGL((nb_cluster_kernel<ENERGY, COUL, G, S, 1, false>), g, b, lds_pad, h->stream, a);        \
    } while (0)
    if (geom) { if (samecut) NB_LAUNCH(true, true); else NB_LAUNCH(true, false); }
    else      { if (samecut) NB_LAUNCH(false, true); else NB_LAUNCH(false, false); }
#undef NB_LAUNCH
#undef NB_DUAL
#undef NB_STEP
    // (mdx_pair_body_info: did the constant-sigma^2 body go out - by the step loop, by anything)
    if (a.inner || (h->nb_step >= 0 && a.gate)) h->pair_body_step = uni_used;
    h->pair_body_any = uni_used;
}

