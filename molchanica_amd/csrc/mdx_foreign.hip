// mdx_foreign.hip - foreign-lambda energy differences of an alchemical window (mdx_set_foreign_lambdas / mdx_foreign_energies):
//
//   dU_k = U(lambda_k) - U(lambda) at the current positions, for the configured lambda_1 .. lambda_K (K <= MDX_MAX_FOREIGN_LAMBDAS),
//
// the inputs of BAR / MBAR (molchanica_amd/alchemical.py).  Under the coupling form of mdx.h only two parts of U depend on lambda:
//   - real space: every cross pair (exactly one atom in the coupled molecule) contributes (1 - lambda) u(r_sc(lambda));
//   - the SPME reciprocal sum, LINEAR in lambda: its share is (lambda_k - lambda) x the reciprocal dU/dlambda the energy evaluation
//     already has (-2 E_env,mol), added on the host - exact.
// Everything else (bonded, 1-4, intramolecular non-bonded, Ewald self / background, kinetic) cancels.
//
// One dedicated pass over the Verlet list, modelled on nb_group_kernel (mdx_groups.hip): the lane mapping of nb_cluster_kernel, the
// SAME pair_eval in its energy + alchemical flavour, so dU_k is made of the pair terms mdx_energy sums.  The step loop's kernels are
// not touched.  Cost control: a per-cluster "holds coupled atoms" byte (foreign_cluster_kernel, from the sign of the slot's packed
// sqrt(24 eps)) lets a wave skip every (tile, entry) whose i- and j-clusters hold no coupled atom - a 50-atom solute in a large box
// costs a read of the list entries, not a full energy pass.  A live cross pair is evaluated once at the window's own lambda and once
// per foreign lambda (r^2 is loop-invariant), and the lane accumulates the per-pair DIFFERENCE in fp64: no cancellation of two
// totals, and lambda_k == lambda is skipped outright (exactly 0).  The workgroups reduce in a fixed order into an [n_blocks x K] fp64
// slab that a second kernel sums in a fixed order: no atomics, the same state gives the same bits.
#include "mdx_comm.h"
#include "mdx_pair_dev.h"
#include <cmath>
#include <cstring>

#define FAIL(code, msg) do { mdx_set_error(msg); return (code); } while (0)

#define FOREIGN_BLOCKS 1024u     // workgroups of the pair pass (tiles are strided over them): the slab is FOREIGN_BLOCKS x K doubles

struct ForeignArgs {
    NbArgs nb;                                  // the window's own parameters (alch_scale = 1 - lambda, sc_al = alpha lambda)
    const uint8_t* hot;                         // [S / 8] cluster holds an atom of the coupled molecule
    double* slab;                               // [gridDim.x * K]
    uint32_t K;
    uint32_t half;                              // the list holds every cluster pair once
    uint32_t mask_layout;                       // as GroupArgs (mdx_groups.hip)
    uint32_t skip;                              // bit k: lambda_k == lambda (dU_k = 0, not evaluated)
    float scale[MDX_MAX_FOREIGN_LAMBDAS];       // 1 - lambda_k, rounded as mdx_fill_nb_params rounds 1 - lambda
    float sc_al[MDX_MAX_FOREIGN_LAMBDAS];       // alpha lambda_k, likewise
};

__global__ __launch_bounds__(256) void foreign_cluster_kernel(uint32_t n_clusters, const float2* __restrict__ lj,
                                                              const uint32_t* __restrict__ orig_of, uint8_t* __restrict__ hot) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_clusters) return;
    uint32_t h = 0;
#pragma unroll
    for (int i = 0; i < MDX_CLUSTER; ++i) {
        const uint32_t s = c * MDX_CLUSTER + i;
        h |= (orig_of[s] != MDX_INVALID && __float_as_int(lj[s].y) < 0) ? 1u : 0u;
    }
    hot[c] = (uint8_t)h;
}

template <int COUL, bool GEOM>
__global__ __launch_bounds__(256) void nb_foreign_kernel(ForeignArgs fa) {
    const NbArgs& a = fa.nb;
    __shared__ float4 s_ixyzq[64];
    __shared__ float2 s_ilj[64];
    __shared__ float4 s_xyzq[4][64];
    __shared__ float2 s_lj[4][64];
    __shared__ uint32_t s_meta[4][64];      // hot j-cluster | owned << 8
    __shared__ double s_red[4][MDX_MAX_FOREIGN_LAMBDAS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ii = lane & 7, jj = lane >> 3;
    const float rcmax2 = fmaxf(a.p.rc2_lj, a.p.rc2_coul);
    double acc[MDX_MAX_FOREIGN_LAMBDAS];
#pragma unroll
    for (int k = 0; k < MDX_MAX_FOREIGN_LAMBDAS; ++k) acc[k] = 0.0;
    for (uint32_t t = blockIdx.x; t < a.T; t += gridDim.x) {     // (uniform over the workgroup)
        uint32_t ihot = 0;
#pragma unroll
        for (int ci = 0; ci < 8; ++ci) ihot |= (uint32_t)fa.hot[t * 8 + ci] << ci;
        const ListCounts cnt = a.counts[t];
        const uint32_t e0 = a.entry_off[t], nmc = cnt.n_masked >> 3, nchunks = (cnt.n_masked + cnt.n_plain) >> 3;
        const uint32_t mbase = a.mchunk_off[t];
        __syncthreads();                    // (the previous tile's i-atoms are no longer read)
        if (threadIdx.x < 64) {
            const uint32_t s = t * MDX_TILE + threadIdx.x;
            s_ixyzq[threadIdx.x] = a.posq[s];
            s_ilj[threadIdx.x] = a.lj[s];
        }
        __syncthreads();
        uint32_t own_bits = 0;
#pragma unroll
        for (int ci = 0; ci < 8; ++ci)
            own_bits |= (a.energy_all ? 1u : ((a.slot_flags[t * MDX_TILE + ci * MDX_CLUSTER + ii] >> 1) & 1u)) << ci;
        for (uint32_t c = (uint32_t)wave; c < nchunks; c += 4) {
            const uint2 ent = a.entries[e0 + c * 8 + (lane >> 3)];
            const uint32_t hot_j = fa.hot[ent.x];
            if (!ihot && !__ballot(hot_j != 0u)) continue;             // no coupled atom on either side of the chunk (wave-uniform)
            const uint32_t js = ent.x * MDX_CLUSTER + (lane & 7);
            float4 nj = a.posq[js];
            {
                const uint32_t code = ent.y & 31u;
                const int kx = (int)(code % 3u) - 1, ky = (int)((code / 3u) % 3u) - 1, kz = (int)(code / 9u) - 1;
                nj.x += (float)kx * a.p.shift[0]; nj.y += (float)ky * a.p.shift[1]; nj.z += (float)kz * a.p.shift[2];
            }
            unsigned long long mq = c < nmc ? a.masks[(size_t)(mbase + c) * 64 + lane] : ~0ull;
            if (fa.mask_layout == 1 && c < nmc) {      // the whole-tile kernel's layout, transposed into this lane mapping (nb_group_kernel)
                const unsigned long long m = mq;
                mq = 0ull;
#pragma unroll
                for (int ci = 0; ci < 8; ++ci) {
                    const unsigned long long mp = __shfl(m, ci * 8 + ii);
#pragma unroll
                    for (int e = 0; e < 8; ++e) mq |= ((mp >> (8 * e + jj)) & 1ull) << (8 * e + ci);
                }
            }
            s_xyzq[wave][lane] = nj;
            s_lj[wave][lane] = a.lj[js];
            s_meta[wave][lane] = hot_j | ((a.energy_all ? 1u : ((a.slot_flags[js] >> 1) & 1u)) << 8);
            WAVE_LDS_SYNC();
#pragma unroll 1
            for (int e = 0; e < 8; ++e) {
                const uint32_t im = (__builtin_amdgcn_readlane(ent.y, e * 8) >> 8) & 0xFFu;     // wave-uniform
                const uint32_t jhot = __builtin_amdgcn_readlane(hot_j, e * 8);
                const uint32_t live_ci = im & (jhot ? 0xFFu : ihot);                          // i-clusters with a possible cross pair
                if (live_ci == 0) continue;
                const float4 pj = s_xyzq[wave][e * 8 + jj];
                const float2 lj = s_lj[wave][e * 8 + jj];
                const uint32_t own_j = (s_meta[wave][e * 8 + jj] >> 8) & 1u;
                const uint32_t allowed8 = (uint32_t)(mq >> (8 * e)) & 0xFFu;
#pragma unroll 1
                for (int ci = 0; ci < 8; ++ci) {
                    if (!(live_ci & (1u << ci))) continue;
                    const float4 pi = s_ixyzq[ci * 8 + ii];
                    const float2 li = s_ilj[ci * 8 + ii];
                    const float bias = ((allowed8 >> ci) & 1u) ? 0.f : __builtin_nanf("");
                    const bool cross = __float_as_int(li.y * lj.y) < 0;           // the flag pair_eval reads
                    float fx = 0.f, fy = 0.f, fz = 0.f, e1 = 0.f, e2 = 0.f, r2 = 0.f;
                    pair_eval<true, COUL, GEOM, false, true, false, true, true>(pi.x, pi.y, pi.z, pi.w, li.x, li.y, pj, lj, true, a.p,
                                                                               fx, fy, fz, e1, e2, nullptr, nullptr, nullptr, bias, &r2);
                    if (!(cross && r2 < rcmax2)) continue;                             // (NaN: excluded)
                    const uint32_t own_i = (own_bits >> ci) & 1u;
                    // weights of nb_group_kernel: half list - once here (half weight per owned atom without the half shell); full list:
                    // every pair comes by twice
                    const double w = fa.half ? 0.5 * (double)(own_i + own_j) : (own_i ? 0.5 : 0.0);
                    if (w == 0.0) continue;
                    const double es0 = (double)(e1 + e2);
#pragma unroll
                    for (int k = 0; k < MDX_MAX_FOREIGN_LAMBDAS; ++k) {     // (fixed trip count: acc[] stays in registers)
                        if ((uint32_t)k < fa.K && !((fa.skip >> k) & 1u)) {
                            NbParams pk = a.p;
                            pk.alch_scale = fa.scale[k]; pk.sc_al = fa.sc_al[k];
                            float gx = 0.f, gy = 0.f, gz = 0.f, f1 = 0.f, f2 = 0.f;
                            pair_eval<true, COUL, GEOM, false, true, false, true, true>(pi.x, pi.y, pi.z, pi.w, li.x, li.y, pj, lj, true, pk,
                                                                                       gx, gy, gz, f1, f2, nullptr, nullptr, nullptr, bias);
                            acc[k] += w * ((double)(f1 + f2) - es0);
                        }
                    }
                }
            }
            WAVE_LDS_SYNC();
        }
    }
    // fixed-order reduction: butterfly within the wave, then the four waves in order
#pragma unroll
    for (int k = 0; k < MDX_MAX_FOREIGN_LAMBDAS; ++k) {
        if ((uint32_t)k < fa.K) {
            double v = acc[k];
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
            if (lane == 0) s_red[wave][k] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x < fa.K)
        fa.slab[(size_t)blockIdx.x * fa.K + threadIdx.x] =
            ((s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + s_red[2][threadIdx.x]) + s_red[3][threadIdx.x];
}

// out[k] = sum over the slab's rows, in a fixed order (one workgroup per k: strided partial sums, then a fixed tree)
__global__ __launch_bounds__(256) void foreign_sum_kernel(const double* __restrict__ slab, uint32_t rows, uint32_t K, double* __restrict__ out) {
    __shared__ double s[256];
    const uint32_t k = blockIdx.x;
    double v = 0.0;
    for (uint32_t r = threadIdx.x; r < rows; r += 256) v += slab[(size_t)r * K + k];
    s[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t m = 128; m > 0; m >>= 1) {
        if (threadIdx.x < m) s[threadIdx.x] += s[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[k] = s[0];
}

template <int COUL>
static void launch_foreign(mdx_handle* h, const ForeignArgs& fa, uint32_t blocks, bool geom) {
    if (geom) hipLaunchKernelGGL((nb_foreign_kernel<COUL, true>), dim3(blocks), dim3(256), 0, h->stream, fa);
    else hipLaunchKernelGGL((nb_foreign_kernel<COUL, false>), dim3(blocks), dim3(256), 0, h->stream, fa);
}

// dU_k of the current state (real space on the device, the reciprocal part from the last energy evaluation's dU/dlambda, which the
// caller has made current).  Collective on a decomposed handle.
int mdx_foreign_evaluate(mdx_handle* h, double* du) {
    const uint32_t K = (uint32_t)h->foreign_lams.size();
    if (!h->alch_on || !K) FAIL(MDX_EPARAM, "foreign energies need an active alchemical window (mdx_configure_alchemical_window) and foreign lambdas");
    MDX_TRY(mdx_ensure_ready(h));          // list, constraints, ghosts and virtual sites of the current state
    hipStream_t st = h->stream;
    DeviceState& d = h->d;
    const uint32_t n_cl = h->S / MDX_CLUSTER;
    if (!d.fl_slab) {
        HIP_TRY(hipMalloc((void**)&d.fl_slab, sizeof(double) * ((size_t)FOREIGN_BLOCKS * MDX_MAX_FOREIGN_LAMBDAS + MDX_MAX_FOREIGN_LAMBDAS)));
    }
    if (d.fl_hot_cap < n_cl) {
        if (d.fl_hot) { (void)hipFree(d.fl_hot); d.fl_hot = nullptr; d.fl_hot_cap = 0; }
        const uint32_t cap = n_cl + n_cl / 4 + 64;
        HIP_TRY(hipMalloc((void**)&d.fl_hot, cap));
        d.fl_hot_cap = cap;
    }
    double* out_dev = d.fl_slab + (size_t)FOREIGN_BLOCKS * MDX_MAX_FOREIGN_LAMBDAS;
    ForeignArgs fa{};
    NbArgs& a = fa.nb;
    a.T = h->T; a.posq = d.posq; a.lj = d.lj; a.counts = d.list_counts; a.entry_off = d.entry_off; a.mchunk_off = d.mchunk_off;
    a.entries = d.entries; a.masks = d.masks; a.slot_flags = d.slot_flags;
    a.energy_all = mdx_dd_half_shell(h) ? 1u : 0u;
    int mode = 0; bool geom = false, samecut = false;
    mdx_fill_nb_params(h, a.p, &mode, &geom, &samecut);
    fa.hot = d.fl_hot; fa.slab = d.fl_slab; fa.K = K;
    fa.half = mdx_nb_half(h) ? 1u : 0u;
    fa.mask_layout = mdx_nb_variant(h) >= 2 ? 2u : 1u;
    for (uint32_t k = 0; k < K; ++k) {
        const double lk = h->foreign_lams[k];
        fa.scale[k] = (float)(1.0 - lk);
        fa.sc_al[k] = (float)(h->sc_alpha * lk);
        if (lk == h->alch_lambda) fa.skip |= 1u << k;
    }
    const uint32_t blocks = std::max(1u, std::min(h->T, FOREIGN_BLOCKS));
    if (h->T) {
        hipLaunchKernelGGL(foreign_cluster_kernel, dim3((n_cl + 255) / 256), dim3(256), 0, st, n_cl, d.lj, d.orig_of, d.fl_hot);
        switch (mode) {
        case CM_SHIFTED: launch_foreign<CM_SHIFTED>(h, fa, blocks, geom); break;
        case CM_SOFT: launch_foreign<CM_SOFT>(h, fa, blocks, geom); break;
        case CM_RF: launch_foreign<CM_RF>(h, fa, blocks, geom); break;
        default: launch_foreign<CM_EWALD>(h, fa, blocks, geom); break;
        }
        hipLaunchKernelGGL(foreign_sum_kernel, dim3(K), dim3(256), 0, st, d.fl_slab, blocks, K, out_dev);
    } else {
        HIP_TRY(hipMemsetAsync(out_dev, 0, sizeof(double) * K, st));
    }
    HIP_TRY(hipGetLastError());
    if (h->dd && h->dd->world > 1) MDX_TRY(mdx_dd_allreduce_dev(h, out_dev, K));
    HIP_TRY(hipMemcpyAsync(du, out_dev, sizeof(double) * K, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t k = 0; k < K; ++k) {
        const double dl = h->foreign_lams[k] - h->alch_lambda;
        du[k] += h->pme_on && dl != 0.0 ? dl * h->alch_recip_dudl : 0.0;      // the mesh part: linear in lambda
        if (!std::isfinite(du[k])) FAIL(MDX_ENAN, "non-finite foreign-lambda energy difference");
    }
    return MDX_OK;
}

// ---- C ABI ------------------------------------------------------------------------------------------

extern "C" int mdx_set_foreign_lambdas(mdx_handle* h, uint32_t n, const double* lambdas) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (n > MDX_MAX_FOREIGN_LAMBDAS) FAIL(MDX_EPARAM, "at most MDX_MAX_FOREIGN_LAMBDAS (32) foreign lambdas");
    if (n && !lambdas) FAIL(MDX_EPARAM, "null lambda array");
    for (uint32_t k = 0; k < n; ++k)
        if (!std::isfinite(lambdas[k]) || lambdas[k] < 0.0 || lambdas[k] > 1.0) FAIL(MDX_EPARAM, "foreign lambdas must be finite and lie in [0, 1]");
    h->foreign_lams.assign(lambdas, lambdas + n);
    return MDX_OK;
}

extern "C" int mdx_foreign_energies(mdx_handle* h, double* du, uint32_t n) {
    if (!h || !du) FAIL(MDX_EPARAM, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    if (!h->alch_on) FAIL(MDX_EPARAM, "foreign energies need an active alchemical window (mdx_configure_alchemical_window)");
    if (h->foreign_lams.empty()) FAIL(MDX_EPARAM, "no foreign lambdas are set (mdx_set_foreign_lambdas)");
    if (n != (uint32_t)h->foreign_lams.size()) FAIL(MDX_EPARAM, "n must be the number of foreign lambdas set");
    // the reciprocal dU/dlambda of the current state: the last evaluation's while nothing has moved since (the mesh sums are not
    // bit-reproducible, a repeated call must be), else a fresh one (or the step loop's, through the energy cache)
    const bool recip_current = h->alch_recip_ok && h->alch_recip_step == h->step_count && h->forces_valid && h->list_valid && !h->cons_dirty;
    if (h->pme_on && !recip_current) {
        mdx_energies e;
        MDX_TRY(mdx_energy_impl(h, &e));
    }
    std::vector<double> tmp(n);
    MDX_TRY(mdx_foreign_evaluate(h, tmp.data()));
    std::memcpy(du, tmp.data(), sizeof(double) * n);
    return MDX_OK;
}

extern "C" uint32_t mdx_snapshot_foreign_count(const mdx_handle* h, uint32_t k) {
    return (h && k < h->snapshots.size()) ? (uint32_t)h->snapshots[k].foreign.size() : 0u;
}

extern "C" int mdx_snapshot_read_foreign(mdx_handle* h, uint32_t k, double* du, uint32_t n) {
    if (!h || !du) FAIL(MDX_EPARAM, "null argument");
    if (k >= h->snapshots.size()) FAIL(MDX_EPARAM, "snapshot index out of range");
    const auto& sn = h->snapshots[k];
    if (sn.foreign.empty()) FAIL(MDX_EPARAM, "the snapshot was taken without foreign lambdas (or without an alchemical window)");
    if ((size_t)n != sn.foreign.size()) FAIL(MDX_EPARAM, "n must be the number of foreign lambdas the snapshot was taken with");
    std::memcpy(du, sn.foreign.data(), sizeof(double) * n);
    return MDX_OK;
}
