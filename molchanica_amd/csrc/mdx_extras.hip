// mdx_extras.hip — the callers either side of `step`: energy minimiser,
// velocity initialisation, thermostats, centre-of-mass drift removal and in-memory snapshots.
//
// Reference call sites (the algorithms themselves live in the absent `dynamics` crate):
//   md.minimize_energy(dev, iters, ext)          src/ui/mol_editor.rs:375, src/mol_alignment.rs:356,
//                                                src/properties/sol_shrinking_box.rs:962
//   md.initialize_velocities(TEMP, zero_com)     src/properties/sol_shrinking_box.rs:965
//   VerletVelocity{thermostat: Some(tau)}        src/ui/panels/md.rs:296-305 (CSVR per README.md:237-238)
//   zero_com_drift                               src/properties/water_sol.rs:144
//   snapshot_handlers.memory / md.snapshots /
//   md.flush_snapshot_queues()                   src/properties/water_sol.rs:185-189, src/md/mod.rs:118-122
// All of these reuse the force path; their own kernels are streaming passes (HBM-bound).
#include "mdx_comm.h"
#include <algorithm>
#include <cmath>
#include <cstring>

#define FAIL(code, msg) do { mdx_set_error(msg); return (code); } while (0)
static inline unsigned div_up(unsigned a, unsigned b) { return (a + b - 1) / b; }

// ---- RNG (bit-for-bit the oracle's) -------------------------------------------------------------
static double rng_u01(uint64_t* s) { return ((double)(mdx_splitmix64(s) >> 11) + 0.5) * (1.0 / 9007199254740992.0); }
static double rng_gauss(uint64_t* s) {
#pragma clang fp contract(off)
    const double u1 = rng_u01(s), u2 = rng_u01(s);
    return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
}
static double rng_gamma_int(uint64_t* s, long ia) {   // shape ia >= 1, scale 1 (Marsaglia & Tsang)
    const double d = (double)ia - 1.0 / 3.0, c = 1.0 / std::sqrt(9.0 * d);
    for (;;) {
        const double x = rng_gauss(s), t = 1.0 + c * x;
        if (t <= 0.0) continue;
        const double v = t * t * t, u = rng_u01(s);
        if (std::log(u) < 0.5 * x * x + d - d * v + d * std::log(v)) return d * v;
    }
}
static double rng_sum_noises(uint64_t* s, long nn) {  // sum of nn squared normals
    if (nn <= 0) return 0.0;
    if (nn == 1) { const double g = rng_gauss(s); return g * g; }
    if (nn % 2 == 0) return 2.0 * rng_gamma_int(s, nn / 2);
    const double g = rng_gauss(s);
    return 2.0 * rng_gamma_int(s, (nn - 1) / 2) + g * g;
}

// ---- kernels --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scale_vel_kernel(uint32_t S, float4* __restrict__ vel, float lambda, float cx,
                                                        float cy, float cz) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    float4 v = vel[s];
    if (v.w == 0.f) return;
    v.x = (v.x - cx) * lambda; v.y = (v.y - cy) * lambda; v.z = (v.z - cz) * lambda;
    vel[s] = v;
}

__global__ __launch_bounds__(256) void momentum_kernel(uint32_t S, const float4* __restrict__ vel, double* out) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    double px = 0, py = 0, pz = 0, m = 0;
    if (s < S) {
        const float4 v = vel[s];
        if (v.w != 0.f) {
            m = (double)MDX_ACC_CONV / (double)v.w;
            px = m * v.x; py = m * v.y; pz = m * v.z;
        }
    }
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) {
        px += __shfl_xor(px, k); py += __shfl_xor(py, k); pz += __shfl_xor(pz, k); m += __shfl_xor(m, k);
    }
    if ((threadIdx.x & 63) == 0 && m != 0.0) {
        atomicAdd(&out[0], px); atomicAdd(&out[1], py); atomicAdd(&out[2], pz); atomicAdd(&out[3], m);
    }
}

// x += scale * F for mobile atoms; raises the stale flag like the drift pass
__global__ __launch_bounds__(256) void min_move_kernel(uint32_t S, float4* __restrict__ posq, const float4* __restrict__ force,
                                                       const float4* __restrict__ vel, const float4* __restrict__ ref,
                                                       float scale, uint32_t* flag, uint32_t thr_bits) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    float d2 = 0.f;
    if (s < S && vel[s].w != 0.f) {
        float4 p = posq[s];
        const float4 f = force[s], r = ref[s];
        p.x += scale * f.x; p.y += scale * f.y; p.z += scale * f.z;
        posq[s] = p;
        const float dx = p.x - r.x, dy = p.y - r.y, dz = p.z - r.z;
        d2 = dx * dx + dy * dy + dz * dz;
        if (!(d2 < 1.0e30f)) d2 = 3.0e38f;
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) d2 = fmaxf(d2, __shfl_xor(d2, m));
    if ((threadIdx.x & 63) == 0 && __float_as_uint(d2) > thr_bits) atomicMax(flag, __float_as_uint(d2));
}

// Work the external forces do along a trial move: sum_i F_ext,i . (x_i - x_accepted,i), minimum image per periodic
// dimension (a rebuild between the two may have wrapped an atom).  Caller order on both sides.
__global__ __launch_bounds__(256) void ext_work_kernel(uint32_t N, const uint32_t* __restrict__ slot_of,
                                                       const float4* __restrict__ posq, const float4* __restrict__ accepted,
                                                       const float4* __restrict__ ext, float lx, float ly, float lz,
                                                       double* __restrict__ out, const uint8_t* __restrict__ slot_flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    double w = 0.0;
    if (i < N) {
        const uint32_t s = slot_of[i];
        if (s != MDX_INVALID && (!slot_flags || (slot_flags[s] & 2u))) {      // (decomposed: every atom is counted by its owner)
            const float4 p = posq[s], a = accepted[i], f = ext[i];
            float dx = p.x - a.x, dy = p.y - a.y, dz = p.z - a.z;
            if (lx > 0.f) dx -= rintf(dx / lx) * lx;
            if (ly > 0.f) dy -= rintf(dy / ly) * ly;
            if (lz > 0.f) dz -= rintf(dz / lz) * lz;
            w = (double)f.x * dx + (double)f.y * dy + (double)f.z * dz;
        }
    }
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) w += __shfl_xor(w, k);
    if ((threadIdx.x & 63) == 0 && w != 0.0) atomicAdd(out, w);
}

int mdx_launch_scale_velocities(mdx_handle* h, float lambda, const double* com) {
    hipLaunchKernelGGL(scale_vel_kernel, dim3(div_up(h->S, 256)), dim3(256), 0, h->stream, h->S, h->d.vel, lambda,
                       com ? (float)com[0] : 0.f, com ? (float)com[1] : 0.f, com ? (float)com[2] : 0.f);
    HIP_TRY(hipGetLastError());
    return MDX_OK;
}

int mdx_launch_momentum(mdx_handle* h) {
    HIP_TRY(hipMemsetAsync(h->d.energy + EN_COUNT + 1, 0, sizeof(double) * 4, h->stream));
    hipLaunchKernelGGL(momentum_kernel, dim3(div_up(h->S, 256)), dim3(256), 0, h->stream, h->S, h->d.vel,
                       h->d.energy + EN_COUNT + 1);
    HIP_TRY(hipGetLastError());
    return MDX_OK;
}

// ---- thermostat / COM / snapshots at their cadence ----------------------------------------------------
static double dof(const mdx_handle* h) { return mdx_dof(h); }

static int kinetic_energy(mdx_handle* h, double* ke) {
    HIP_TRY(hipMemsetAsync(h->d.energy + EN_KIN, 0, sizeof(double), h->stream));
    MDX_TRY(mdx_launch_kinetic(h));
    HIP_TRY(hipMemcpyAsync(ke, h->d.energy + EN_KIN, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->dd) MDX_TRY(mdx_dd_allreduce_host(h, ke, 1));   // decomposed: ONE kinetic energy, hence one scale factor, for the whole box
    return MDX_OK;
}

static int remove_com(mdx_handle* h) {
    double p[4];
    MDX_TRY(mdx_launch_momentum(h));
    HIP_TRY(hipMemcpyAsync(p, h->d.energy + EN_COUNT + 1, sizeof(p), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->dd) MDX_TRY(mdx_dd_allreduce_host(h, p, 4));
    if (p[3] <= 0.0) return MDX_OK;
    const double com[3] = {p[0] / p[3], p[1] / p[3], p[2] / p[3]};
    return mdx_launch_scale_velocities(h, 1.0f, com);
}

static int apply_thermostat(mdx_handle* h, double dt_couple) {
    double ke = 0.0;
    MDX_TRY(kinetic_energy(h, &ke));
    if (!(ke > 0.0) || !std::isfinite(ke)) return MDX_OK;
    const double nf = dof(h), k0 = 0.5 * nf * MDX_KB * (double)h->tstat_temp;
    double lambda = 1.0;
    if (h->tstat_kind == MDX_THERMOSTAT_BERENDSEN) {
        const double t = 2.0 * ke / (nf * MDX_KB);
        lambda = std::sqrt(std::max(0.0, 1.0 + dt_couple / (double)h->tstat_tau * ((double)h->tstat_temp / t - 1.0)));
    } else if (h->tstat_kind == MDX_THERMOSTAT_CSVR) {
        // Bussi, Donadio, Parrinello, J. Chem. Phys. 126, 014101 (2007), eq. (A7)
        const double c = h->tstat_tau > 0.f ? std::exp(-dt_couple / (double)h->tstat_tau) : 0.0;
        const double r1 = rng_gauss(&h->rng_state);
        const double s = rng_sum_noises(&h->rng_state, (long)nf - 1);
        const double f = (1.0 - c) * k0 / (nf * ke);
        const double a2 = c + f * (r1 * r1 + s) + 2.0 * r1 * std::sqrt(c * f);
        lambda = std::sqrt(std::max(0.0, a2));
    }
    return mdx_launch_scale_velocities(h, (float)lambda, nullptr);
}

// Weak-coupling barostat: BarostatCfg{tau, pressure_target} (src/ui/panels/md.rs:517-557).  Coordinates
// (caller-order staging, where mdx_set_box expects the state) and the box edges are scaled about
// box_lo; the pair list, the cell grid and the PME mesh follow through mdx_set_box + rebuild.
__global__ void scale_positions_kernel(uint32_t N, float4* __restrict__ pos, float lox, float loy, float loz, float mu) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float4 p = pos[i];
    p.x = lox + mu * (p.x - lox); p.y = loy + mu * (p.y - loy); p.z = loz + mu * (p.z - loz);
    pos[i] = p;
}

static int apply_barostat(mdx_handle* h, double dt_couple) {
    mdx_energies e;
    MDX_TRY(mdx_energy_impl(h, &e));
    if (!std::isfinite(e.pressure)) return MDX_OK;
    const double mu3 = 1.0 - (double)h->baro_beta * dt_couple / (double)h->baro_tau * ((double)h->baro_p0 - e.pressure);
    double mu = std::cbrt(std::max(mu3, 0.5));
    mu = std::min(1.01, std::max(0.99, mu));
    if (mu == 1.0) return MDX_OK;
    float hi[3];
    for (int d = 0; d < 3; ++d) hi[d] = h->box_lo[d] + (float)mu * (h->box_hi[d] - h->box_lo[d]);
    if (h->dd) {      // (the global box is periodic in every dimension whatever the local region is)
        for (int d = 0; d < 3; ++d)
            if (hi[d] - h->box_lo[d] < 2.0f * h->r_list) FAIL(MDX_EPARAM, "box edge shorter than 2*(cutoff+skin): minimum image is not unique");
    } else
    MDX_TRY(mdx_check_box(h, h->box_lo, hi));   // refuse BEFORE touching the state (box < 2 (rc + skin): stop, cf. sol_shrinking_box.rs guards)
    if (h->dd) {      // decomposed: the same mu on every rank (the pressure is all-reduced); scale the gathered state, repartition
        MDX_TRY(mdx_dd_rescale_box(h, hi, (float)mu));
        if (mdx_has_constraints(h)) h->cons_dirty = true;
        h->last_pressure = e.pressure; h->last_mu = mu;
        return MDX_OK;
    }
    MDX_TRY(mdx_unsort_state(h));
    h->vsites_fresh = false;
    hipLaunchKernelGGL(scale_positions_kernel, dim3(div_up(h->n_local, 256)), dim3(256), 0, h->stream, h->n_local,
                       h->d.pos_orig, h->box_lo[0], h->box_lo[1], h->box_lo[2], (float)mu);
    HIP_TRY(hipGetLastError());
    MDX_TRY(mdx_set_box(h, h->box_lo, hi));
    if (mdx_has_constraints(h)) h->cons_dirty = true;   // bonds of constrained clusters were scaled too: project back
    h->last_pressure = e.pressure; h->last_mu = mu;
    return MDX_OK;
}

// `md.shrink_cell_towards(dev, target_cell, ShrinkingBoxCfg{box_shrink_per_step, ..})`
// (/root/reference src/properties/sol_shrinking_box.rs:990, once per MD step of the packing run).  The crate is absent;
// the rule is the one the reference states for its other backend (sol_shrinking_box.rs:765-774, shrink_cell_by_amount):
// every edge shrinks by `shrink_per_step` but not below the target's, the cell keeps its centre; coordinates follow
// affinely (what GROMACS' `deform` does to them in that backend, :1263-1275).  Returns whether any edge changed.
__global__ void scale_positions_about_kernel(uint32_t N, float4* __restrict__ pos, float cx, float cy, float cz,
                                             float mx, float my, float mz) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float4 p = pos[i];
    p.x = cx + mx * (p.x - cx); p.y = cy + my * (p.y - cy); p.z = cz + mz * (p.z - cz);
    pos[i] = p;
}

extern "C" int mdx_shrink_cell_towards(mdx_handle* h, const float target_lo[3], const float target_hi[3],
                                       float shrink_per_step, int* shrank_out) {
    if (!h || !target_lo || !target_hi) FAIL(MDX_EPARAM, "null argument");
    // (a rank of a cut box is not periodic locally in the cut dimensions: a joined handle's box is the global, fully periodic one)
    if (!h->dd && (!h->periodic || !(h->per[0] && h->per[1] && h->per[2]))) FAIL(MDX_EPARAM, "shrink_cell_towards needs a fully periodic box");
    if (!h->dd && h->n_local != h->N) FAIL(MDX_EPARAM, "shrink_cell_towards on a handle narrowed by mdx_set_local_atoms");
    if (!(shrink_per_step >= 0.f) || !std::isfinite(shrink_per_step)) FAIL(MDX_EPARAM, "shrink_per_step must be >= 0");
    float lo[3], hi[3], c[3], mu[3];
    bool shrank = false;
    for (int d = 0; d < 3; ++d) {
        const float e = h->box_hi[d] - h->box_lo[d], te = target_hi[d] - target_lo[d];
        if (!(te > 0.f) || !std::isfinite(te)) FAIL(MDX_EPARAM, "target cell must have positive finite edges");
        const float ne = std::max(e - shrink_per_step, te);
        c[d] = 0.5f * (h->box_lo[d] + h->box_hi[d]);
        lo[d] = c[d] - 0.5f * ne; hi[d] = c[d] + 0.5f * ne;
        mu[d] = ne / e;
        shrank |= ne != e;
    }
    if (shrank_out) *shrank_out = shrank ? 1 : 0;
    if (!shrank) return MDX_OK;
    HIP_TRY(hipSetDevice(h->device));
    if (h->dd) {      // joined handle (collective): the same rule on every rank, the gathered coordinates follow, the ranks repartition
        for (int d = 0; d < 3; ++d)
            if (hi[d] - lo[d] < 2.0f * h->r_list) FAIL(MDX_EPARAM, "box edge shorter than 2*(cutoff+skin): minimum image is not unique");
        h->e_cache_valid = false; h->e_pending = false;
        MDX_TRY(mdx_dd_set_box(h, lo, hi, c, mu));
        if (mdx_has_constraints(h)) h->cons_dirty = true;
        return MDX_OK;
    }
    MDX_TRY(mdx_check_box(h, lo, hi));   // refuse BEFORE touching the state (an edge below 2 (rc + skin))
    MDX_TRY(mdx_unsort_state(h));
    h->vsites_fresh = false;
    hipLaunchKernelGGL(scale_positions_about_kernel, dim3(div_up(h->n_local, 256)), dim3(256), 0, h->stream, h->n_local,
                       h->d.pos_orig, c[0], c[1], c[2], mu[0], mu[1], mu[2]);
    HIP_TRY(hipGetLastError());
    MDX_TRY(mdx_set_box(h, lo, hi));
    if (mdx_has_constraints(h)) h->cons_dirty = true;   // constrained bonds were scaled too: project back
    return MDX_OK;
}

// ---- hydrogen bonds of a configuration (host side: snapshots are rare, the search is linear in N) ----------------------
// Atom references as the reference's (HBondAtomType, index) pairs (src/md/viewer.rs:893-915).
static void hb_ref(const mdx_handle* h, uint32_t atom, uint32_t* idx, uint8_t* type) {
    const uint32_t w0 = h->water_first, w1 = h->water_first + h->n_waters * h->water_sites;
    if (h->n_waters && atom >= w0 && atom < w1) {
        const uint32_t k = (atom - w0) % h->water_sites;
        *idx = (atom - w0) / h->water_sites;
        *type = k == 0 ? MDX_HB_WATER_O : (k == 1 ? MDX_HB_WATER_H0 : (k == 2 ? MDX_HB_WATER_H1 : MDX_HB_WATER_O));
    } else {
        *idx = atom < w0 || !h->n_waters ? atom : atom - h->n_waters * h->water_sites;   // index among the non-water atoms
        *type = MDX_HB_STANDARD;
    }
}

static void detect_hbonds(const mdx_handle* h, const float* pos, std::vector<mdx_hbond>& out) {
    out.clear();
    if (h->hb_heavy.empty()) return;
    const uint32_t N = (uint32_t)h->hb_heavy.size();
    const bool per = h->per[0] || h->per[1] || h->per[2] || (h->dd != nullptr);
    double L[3] = {0, 0, 0}, lo[3] = {0, 0, 0};
    for (int d = 0; d < 3; ++d) { L[d] = (double)h->box_hi[d] - h->box_lo[d]; lo[d] = h->box_lo[d]; }
    auto mimg = [&](double* v) { if (per) for (int d = 0; d < 3; ++d) if (L[d] > 0) v[d] -= std::rint(v[d] / L[d]) * L[d]; };
    // cell grid over the acceptors (cell edge >= max distance)
    const double rc = h->hb_dmax;
    double glo[3] = {1e300, 1e300, 1e300}, ghi[3] = {-1e300, -1e300, -1e300};
    if (per) for (int d = 0; d < 3; ++d) { glo[d] = lo[d]; ghi[d] = lo[d] + L[d]; }
    else for (uint32_t i = 0; i < N; ++i) for (int d = 0; d < 3; ++d) { glo[d] = std::min(glo[d], (double)pos[3 * i + d]); ghi[d] = std::max(ghi[d], (double)pos[3 * i + d] + 1e-3); }
    int nc[3];
    for (int d = 0; d < 3; ++d) nc[d] = std::max(1, std::min(256, (int)std::floor((ghi[d] - glo[d]) / rc)));
    auto cell_of = [&](const float* p, int* c) {
        for (int d = 0; d < 3; ++d) {
            double t = (double)p[d] - glo[d]; const double W = ghi[d] - glo[d];
            if (per) t -= std::floor(t / W) * W;
            c[d] = std::max(0, std::min(nc[d] - 1, (int)(t / W * nc[d])));
        }
    };
    std::vector<uint32_t> start((size_t)nc[0] * nc[1] * nc[2] + 1, 0), items;
    std::vector<uint32_t> acc;
    for (uint32_t i = 0; i < N; ++i) if (h->hb_heavy[i]) acc.push_back(i);
    std::vector<uint32_t> cid(acc.size());
    for (size_t k = 0; k < acc.size(); ++k) { int c[3]; cell_of(pos + 3 * (size_t)acc[k], c); cid[k] = (uint32_t)((c[0] * nc[1] + c[1]) * nc[2] + c[2]); start[cid[k] + 1]++; }
    for (size_t c = 0; c + 1 < start.size(); ++c) start[c + 1] += start[c];
    items.resize(acc.size());
    { std::vector<uint32_t> cur(start.begin(), start.end() - 1); for (size_t k = 0; k < acc.size(); ++k) items[cur[cid[k]]++] = acc[k]; }
    const double cos_min = std::cos(h->hb_angle_min * M_PI / 180.0);
    for (uint32_t hy = 0; hy < N; ++hy) {
        const uint32_t dn = h->hb_donor_of[hy];
        if (dn == MDX_INVALID) continue;
        int c[3]; cell_of(pos + 3 * (size_t)hy, c);
        double dh[3] = {(double)pos[3 * dn] - pos[3 * hy], (double)pos[3 * dn + 1] - pos[3 * hy + 1], (double)pos[3 * dn + 2] - pos[3 * hy + 2]};
        mimg(dh);
        const double rdh = std::sqrt(dh[0] * dh[0] + dh[1] * dh[1] + dh[2] * dh[2]);
        // the distinct neighbour cells per dimension (a box of one or two cells wraps onto itself)
        int nb[3][3], nnb[3];
        for (int d = 0; d < 3; ++d) {
            nnb[d] = 0;
            for (int o = -1; o <= 1; ++o) {
                int q = c[d] + o;
                if (per) q = (q + nc[d]) % nc[d]; else if (q < 0 || q >= nc[d]) continue;
                bool seen = false;
                for (int k = 0; k < nnb[d]; ++k) seen |= nb[d][k] == q;
                if (!seen) nb[d][nnb[d]++] = q;
            }
        }
        for (int ia = 0; ia < nnb[0]; ++ia) for (int ib = 0; ib < nnb[1]; ++ib) for (int ic = 0; ic < nnb[2]; ++ic) {
            const int q[3] = {nb[0][ia], nb[1][ib], nb[2][ic]};
            const size_t cq = ((size_t)q[0] * nc[1] + q[1]) * nc[2] + q[2];
            for (uint32_t k = start[cq]; k < start[cq + 1]; ++k) {
                const uint32_t ac = items[k];
                if (ac == dn) continue;
                double ha[3] = {(double)pos[3 * ac] - pos[3 * hy], (double)pos[3 * ac + 1] - pos[3 * hy + 1], (double)pos[3 * ac + 2] - pos[3 * hy + 2]};
                mimg(ha);
                const double r = std::sqrt(ha[0] * ha[0] + ha[1] * ha[1] + ha[2] * ha[2]);
                if (r > rc || r <= 0.0 || rdh <= 0.0) continue;
                const double cs = (dh[0] * ha[0] + dh[1] * ha[1] + dh[2] * ha[2]) / (rdh * r);   // cos of the angle D-H...A at the hydrogen
                if (cs > cos_min) continue;                                                      // angle below the minimum
                const double ang = std::acos(std::max(-1.0, std::min(1.0, cs))) * 180.0 / M_PI;
                const double sd = std::max(0.0, std::min(1.0, 1.0 - (r - 1.5) / std::max(rc - 1.5, 1e-6)));
                const double sa = std::max(0.0, std::min(1.0, (ang - h->hb_angle_min) / std::max(180.0 - h->hb_angle_min, 1e-6)));
                mdx_hbond hb{};
                hb_ref(h, dn, &hb.donor, &hb.donor_type); hb_ref(h, ac, &hb.acceptor, &hb.acceptor_type); hb_ref(h, hy, &hb.hydrogen, &hb.hydrogen_type);
                hb.strength = (float)(sd * sa);
                out.push_back(hb);
            }
        }
    }
}

// which handlers of mdx_set_snapshot_handlers want the state after `step` (bit i: handler i); the plain cadence is bit 31
static uint32_t snapshot_mask_at(const mdx_handle* h, uint64_t step) {
    uint32_t m = (h->snap_every && step % h->snap_every == 0) ? 0x80000000u : 0u;
    for (int i = 0; i < MDX_SNAP_HANDLERS; ++i) if (h->snap_handlers[i] && step % h->snap_handlers[i] == 0) m |= 1u << i;
    return m;
}
static int take_snapshot(mdx_handle* h) {
    mdx_handle::Snapshot sn;
    sn.time = h->time_ps; sn.step = h->step_count;
    sn.handler_mask = snapshot_mask_at(h, h->step_count);
    const bool want_vel = h->snap_vel || (sn.handler_mask & (1u << MDX_SNAP_NSTVOUT));
    const bool want_frc = (sn.handler_mask & (1u << MDX_SNAP_NSTFOUT)) != 0;
    MDX_TRY(mdx_energy_impl(h, &sn.e));
    const uint32_t n_rows = h->dd ? h->N : h->n_local;     // (a decomposed handle's read-back is the gathered global array)
    sn.pos.resize(3 * (size_t)n_rows);
    MDX_TRY(mdx_download(h, MDX_POS, sn.pos.data()));
    if (want_vel) {
        sn.vel.resize(3 * (size_t)n_rows);
        MDX_TRY(mdx_download(h, MDX_VEL, sn.vel.data()));
    }
    if (want_frc) {
        sn.frc.resize(3 * (size_t)n_rows);
        MDX_TRY(mdx_download(h, MDX_FORCE, sn.frc.data()));
    }
    if (!h->hb_heavy.empty() && n_rows == h->N) detect_hbonds(h, sn.pos.data(), sn.hbonds);
    if (h->n_grp) {      // SnapshotEnergyData.energy_potential_between_mols (src/properties/crystal.rs:533)
        sn.between.resize((size_t)h->n_grp * h->n_grp);
        MDX_TRY(mdx_groups_evaluate(h, sn.between.data()));
    }
    if (mdx_mixing_on(h)) {      // SolubilityMixingDiagnostics (src/properties/sol_shrinking_box.rs:1539), per snapshot
        sn.solubility.resize(1);
        MDX_TRY(mdx_mixing_evaluate(h, sn.solubility.data(), nullptr));
    }
    if (h->alch_on && !h->foreign_lams.empty()) {      // BAR / MBAR inputs (mdx_foreign.hip); the reciprocal part is that of sn.e
        sn.foreign.resize(h->foreign_lams.size());
        MDX_TRY(mdx_foreign_evaluate(h, sn.foreign.data()));
    }
    h->snapshots.push_back(std::move(sn));
    return MDX_OK;
}

uint32_t mdx_steps_to_next_event(const mdx_handle* h) {
    uint32_t n = 0xFFFFFFFFu;
    auto upd = [&](uint32_t every) { if (every) n = std::min<uint32_t>(n, every - (uint32_t)(h->step_count % every)); };
    if (h->tstat_kind) upd(h->tstat_every);
    if (h->zero_com) upd(h->tstat_kind ? h->tstat_every : 100u);
    if (h->baro_kind) upd(h->baro_every);
    upd(h->snap_every);
    for (int i = 0; i < MDX_SNAP_HANDLERS; ++i) upd(h->snap_handlers[i]);
    upd(h->energy_every);
    return n;
}

bool mdx_energy_wanted_at(const mdx_handle* h, uint64_t step) {
    static const bool off = [] { const char* e = std::getenv("MDX_ENERGY_IN_STEP"); return e && e[0] == '0'; }();   // A/B: evaluate afresh when asked
    if (off) return false;
    return (h->energy_every && step % h->energy_every == 0) || snapshot_mask_at(h, step) != 0u ||
           (h->baro_kind && h->baro_every && step % h->baro_every == 0);
}

int mdx_after_steps(mdx_handle* h, float dt, uint32_t done) {
    if (!done) return MDX_OK;
    const uint64_t sc = h->step_count;
    if (h->zero_com && sc % (h->tstat_kind ? h->tstat_every : 100u) == 0) MDX_TRY(remove_com(h));
    if (h->tstat_kind && sc % h->tstat_every == 0) MDX_TRY(apply_thermostat(h, (double)dt * h->tstat_every));
    MDX_TRY(mdx_finalize_energy_cache(h));      // (behind the thermostat: the kinetic energy is the coupled one)
    if (h->baro_kind && sc % h->baro_every == 0) MDX_TRY(apply_barostat(h, (double)dt * h->baro_every));
    if (snapshot_mask_at(h, sc) != 0u) MDX_TRY(take_snapshot(h));
    return MDX_OK;
}

// ---- C ABI ------------------------------------------------------------------------------------------
// The reference reads energies at a cadence (SnapshotHandler ratios, src/md/mod.rs; `energies every 100 steps` in SURVEY 8d):
// told that cadence, the step loop evaluates them as part of the force call that ends such a step instead of a second
// evaluation when mdx_energy is called (at 1 M atoms: +0.35 ms for the energy flavour of that one call instead of +1.1 ms).
extern "C" int mdx_set_energy_cadence(mdx_handle* h, uint32_t every_n_steps) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    h->energy_every = every_n_steps;
    h->e_cache_valid = false;       // (a held evaluation is dropped: the next mdx_energy evaluates afresh)
    return MDX_OK;
}

extern "C" int mdx_set_thermostat(mdx_handle* h, int kind, float temp_target, float tau_ps, uint32_t every_n_steps,
                                  uint64_t seed) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (kind < 0 || kind > 2) FAIL(MDX_EPARAM, "unknown thermostat kind");
    if (kind && (!(temp_target >= 0.f) || !(tau_ps > 0.f) || every_n_steps == 0))
        FAIL(MDX_EPARAM, "thermostat needs temp_target >= 0, tau > 0 and a coupling interval >= 1 step");
    h->tstat_kind = kind; h->tstat_temp = temp_target; h->tstat_tau = tau_ps;
    h->tstat_every = every_n_steps ? every_n_steps : 10; h->rng_state = seed;
    return MDX_OK;
}

extern "C" int mdx_set_integrator(mdx_handle* h, int kind, float gamma_per_ps, float temperature, uint64_t seed) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (kind < 0 || kind > 2) FAIL(MDX_EPARAM, "unknown integrator kind");
    if (kind == MDX_INTEGRATOR_LANGEVIN_MIDDLE && (!(gamma_per_ps >= 0.f) || !(temperature >= 0.f) || !std::isfinite(gamma_per_ps)))
        FAIL(MDX_EPARAM, "Langevin middle needs gamma >= 0 and temperature >= 0");
    if (kind && h->n_local != h->N && !h->dd) FAIL(MDX_EPARAM, "only velocity Verlet is supported on a decomposed handle");
    h->integrator = kind; h->lang_gamma = gamma_per_ps; h->lang_temp = temperature; h->lang_seed = seed;
    return MDX_OK;
}

extern "C" int mdx_set_alchemical_softcore(mdx_handle* h, float alpha, float sigma_min) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (!(alpha >= 0.f) || !std::isfinite(alpha)) FAIL(MDX_EPARAM, "soft-core alpha must be >= 0 (0 = linear coupling)");
    if (!(sigma_min > 0.f) || !std::isfinite(sigma_min)) FAIL(MDX_EPARAM, "soft-core sigma_min must be > 0");
    h->sc_alpha = alpha; h->sc_sigma_min = sigma_min;
    h->forces_valid = false;
    return MDX_OK;
}

extern "C" int mdx_configure_alchemical_window(mdx_handle* h, uint32_t mol_index, double lambda) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    const bool on = lambda >= 0.0;
    if (on) {
        if (!(lambda <= 1.0)) FAIL(MDX_EPARAM, "lambda must lie in [0, 1] (negative switches the window off)");
        if (h->mol_start.empty() || mol_index >= h->mol_start.size()) FAIL(MDX_EPARAM, "molecule index out of range (mol_start missing?)");
        if (!h->dd && h->n_local != h->N) FAIL(MDX_EPARAM, "alchemical windows need the library's own decomposition (mdx_comm_init) on a narrowed handle");
    }
    const uint32_t lo = on ? h->mol_start[mol_index] : 0;
    const uint32_t hi = on ? (mol_index + 1 < h->mol_start.size() ? h->mol_start[mol_index + 1] : h->N) : 0;
    for (uint32_t i = 0; i < h->N; ++i) {
        const float m = std::fabs(h->h_lj[i].y);
        h->h_lj[i].y = (i >= lo && i < hi) ? -m : m;     // -0.0 for eps = 0: the sign bit is the flag
    }
    HIP_TRY(hipMemcpyAsync(h->d.o_lj, h->h_lj.data(), sizeof(float2) * h->N, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    MDX_TRY(mdx_unsort_state(h));       // the per-slot copy of the LJ record is refreshed by the next rebuild
    h->alch_on = on; h->alch_lambda = on ? lambda : 0.0; h->alch_lo = lo; h->alch_hi = hi;
    mdx_refresh_uni_lj(h);      // (a window needs sigma_ij of the pair; switching it off gives the constant-sigma^2 bodies back)
    h->pme_canvas_clean = false; h->pme_canvas2_clean = false;      // (a slab-decomposed mesh keeps only its block clean; the window spreads whole meshes)
    h->list_valid = false; h->forces_valid = false;
    return MDX_OK;
}

extern "C" int mdx_get_box(const mdx_handle* h, float lo[3], float hi[3]) {
    if (!h || !lo || !hi) FAIL(MDX_EPARAM, "null argument");
    for (int d = 0; d < 3; ++d) { lo[d] = h->box_lo[d]; hi[d] = h->box_hi[d]; }
    return MDX_OK;
}

extern "C" int mdx_set_barostat(mdx_handle* h, int kind, float pressure_target_bar, float tau_ps,
                                float compressibility_per_bar, uint32_t every_n_steps) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (kind < 0 || kind > 1) FAIL(MDX_EPARAM, "unknown barostat kind");
    if (kind) {
        // (a decomposed handle is periodic as a whole: only its local region is not, in the cut dimensions)
        if (!h->dd && (!h->periodic || !(h->per[0] && h->per[1] && h->per[2]))) FAIL(MDX_EPARAM, "the barostat needs a fully periodic box");
        if (!h->dd && h->n_local != h->N) FAIL(MDX_EPARAM, "the barostat needs the library's own decomposition (mdx_comm_init) on a narrowed handle");
        if (!(tau_ps > 0.f) || every_n_steps == 0 || !std::isfinite(pressure_target_bar))
            FAIL(MDX_EPARAM, "barostat needs a finite target, tau > 0 and a coupling interval >= 1 step");
    }
    h->baro_kind = kind; h->baro_p0 = pressure_target_bar; h->baro_tau = tau_ps;
    h->baro_beta = compressibility_per_bar > 0.f ? compressibility_per_bar : 4.5e-5f;
    h->baro_every = every_n_steps ? every_n_steps : 25;
    return MDX_OK;
}

extern "C" int mdx_set_zero_com_drift(mdx_handle* h, int enable) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    h->zero_com = enable != 0;
    return MDX_OK;
}

extern "C" int mdx_set_snapshot_cadence(mdx_handle* h, uint32_t every_n, int with_velocities) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    h->snap_every = every_n; h->snap_vel = with_velocities != 0;
    return MDX_OK;
}

extern "C" uint32_t mdx_snapshot_count(const mdx_handle* h) { return h ? (uint32_t)h->snapshots.size() : 0u; }
extern "C" int mdx_snapshot_read_between_mols(mdx_handle* h, uint32_t k, float* out, uint32_t n) {
    if (!h || !out) FAIL(MDX_EPARAM, "null argument");
    if (k >= h->snapshots.size()) FAIL(MDX_EPARAM, "snapshot index out of range");
    const auto& sn = h->snapshots[k];
    if (sn.between.empty()) FAIL(MDX_EPARAM, "the snapshot was taken without energy groups (mdx_set_energy_groups)");
    if ((size_t)n * n != sn.between.size()) FAIL(MDX_EPARAM, "n must be the number of groups the snapshot was taken with");
    std::memcpy(out, sn.between.data(), sizeof(float) * sn.between.size());
    return MDX_OK;
}
extern "C" double mdx_time_ps(const mdx_handle* h) { return h ? h->time_ps : 0.0; }

extern "C" int mdx_set_snapshot_handlers(mdx_handle* h, const uint32_t every_n[MDX_SNAP_HANDLERS]) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    for (int i = 0; i < MDX_SNAP_HANDLERS; ++i) h->snap_handlers[i] = every_n ? every_n[i] : 0u;
    return MDX_OK;
}
extern "C" uint32_t mdx_snapshot_handler_mask(const mdx_handle* h, uint32_t k) {
    return (h && k < h->snapshots.size()) ? h->snapshots[k].handler_mask : 0u;
}
extern "C" int mdx_snapshot_read_forces(mdx_handle* h, uint32_t k, float* frc) {
    if (!h || !frc) FAIL(MDX_EPARAM, "null argument");
    if (k >= h->snapshots.size()) FAIL(MDX_EPARAM, "snapshot index out of range");
    const auto& sn = h->snapshots[k];
    if (sn.frc.empty()) FAIL(MDX_EPARAM, "snapshot was taken without forces (no nstfout handler at its step)");
    std::memcpy(frc, sn.frc.data(), sizeof(float) * sn.frc.size());
    return MDX_OK;
}
extern "C" int mdx_snapshot_read(mdx_handle* h, uint32_t k, double* time_ps, uint64_t* step, mdx_energies* e, float* pos,
                                 float* vel) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (k >= h->snapshots.size()) FAIL(MDX_EPARAM, "snapshot index out of range");
    const auto& sn = h->snapshots[k];
    if (time_ps) *time_ps = sn.time;
    if (step) *step = sn.step;
    if (e) *e = sn.e;
    if (pos) std::memcpy(pos, sn.pos.data(), sizeof(float) * sn.pos.size());
    if (vel) {
        if (sn.vel.empty()) FAIL(MDX_EPARAM, "snapshot was taken without velocities");
        std::memcpy(vel, sn.vel.data(), sizeof(float) * sn.vel.size());
    }
    return MDX_OK;
}

extern "C" int mdx_set_water_layout(mdx_handle* h, uint32_t first_atom, uint32_t n_waters, uint32_t sites_per_water) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (n_waters && sites_per_water != 3 && sites_per_water != 4) FAIL(MDX_EPARAM, "a water record has 3 (O, H0, H1) or 4 (O, H0, H1, M) sites");
    if ((uint64_t)first_atom + (uint64_t)n_waters * sites_per_water > h->N) FAIL(MDX_EPARAM, "water records reach beyond the atom array");
    h->water_first = first_atom; h->n_waters = n_waters; h->water_sites = n_waters ? sites_per_water : 0;
    return MDX_OK;
}

// The engine keeps every atom wrapped into the cell on its own, so a water near a face has its hydrogens on the far side.
// The water views hand molecules out WHOLE: H0, H1 (and M) in the periodic image nearest to their oxygen - what a viewer
// drawing O-H bonds needs (src/md/viewer.rs:378-394) and what a host computing intramolecular geometry expects.
static void water_make_whole(const mdx_handle* h, const float* o, float* const* sites, uint32_t n_sites) {
    const bool per_any = h->dd || h->per[0] || h->per[1] || h->per[2];
    if (!per_any) return;
    for (int d = 0; d < 3; ++d) {
        if (!(h->dd || h->per[d])) continue;
        const float L = h->box_hi[d] - h->box_lo[d];
        if (!(L > 0.f)) continue;
        for (uint32_t k = 0; k < n_sites; ++k) {
            float* s = sites[k];
            if (!s) continue;
            for (uint32_t w = 0; w < h->n_waters; ++w) {
                const float dx = s[3 * (size_t)w + d] - o[3 * (size_t)w + d];
                s[3 * (size_t)w + d] -= L * std::rint(dx / L);
            }
        }
    }
}

extern "C" int mdx_water_download(mdx_handle* h, int which, float* o, float* h0, float* h1, float* m) {
    if (!h || !o || !h0 || !h1) FAIL(MDX_EPARAM, "null argument");
    if (!h->n_waters) FAIL(MDX_EPARAM, "no water layout set (mdx_set_water_layout)");
    if (which != MDX_POS && which != MDX_FORCE) FAIL(MDX_EPARAM, "md.water mirrors posit and force");
    if (m && h->water_sites != 4) FAIL(MDX_EPARAM, "3-site water has no M site");
    std::vector<float> all(3 * (size_t)h->N);
    if (!h->dd && h->n_local != h->N) FAIL(MDX_EPARAM, "mdx_water_download needs the whole system on this handle");
    MDX_TRY(mdx_download(h, which, all.data()));
    float* dst[4] = {o, h0, h1, m};
    for (uint32_t w = 0; w < h->n_waters; ++w)
        for (uint32_t k = 0; k < h->water_sites; ++k)
            if (dst[k]) std::memcpy(dst[k] + 3 * (size_t)w, all.data() + 3 * ((size_t)h->water_first + (size_t)w * h->water_sites + k), 3 * sizeof(float));
    if (which == MDX_POS) water_make_whole(h, o, dst + 1, h->water_sites - 1);
    return MDX_OK;
}

extern "C" int mdx_set_hbond_detection(mdx_handle* h, const uint8_t* is_hbond_heavy, float max_h_acc_dist, float min_angle_deg) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (!is_hbond_heavy) { h->hb_heavy.clear(); h->hb_donor_of.clear(); return MDX_OK; }
    if (!(max_h_acc_dist > 1.5f) || !std::isfinite(max_h_acc_dist)) max_h_acc_dist = 2.5f;
    if (!(min_angle_deg > 0.f && min_angle_deg < 180.f)) min_angle_deg = 120.f;
    h->hb_dmax = max_h_acc_dist; h->hb_angle_min = min_angle_deg;
    h->hb_heavy.assign(is_hbond_heavy, is_hbond_heavy + h->N);
    // donor hydrogens: light atoms (mass < 1.6 Da) bound - bond or constraint - to a flagged heavy atom
    h->hb_donor_of.assign(h->N, MDX_INVALID);
    for (size_t k = 0; k + 1 < h->h_bond_pairs.size(); k += 2) {
        const uint32_t a = h->h_bond_pairs[k], b = h->h_bond_pairs[k + 1];
        const bool ha = h->h_mass[a] > 0.f && h->h_mass[a] < 1.6f, hb = h->h_mass[b] > 0.f && h->h_mass[b] < 1.6f;
        if (ha && !hb && h->hb_heavy[b]) h->hb_donor_of[a] = b;
        else if (hb && !ha && h->hb_heavy[a]) h->hb_donor_of[b] = a;
    }
    return MDX_OK;
}

extern "C" int mdx_snapshot_read_water(mdx_handle* h, uint32_t k, float* o, float* h0, float* h1) {
    if (!h || !o || !h0 || !h1) FAIL(MDX_EPARAM, "null argument");
    if (k >= h->snapshots.size()) FAIL(MDX_EPARAM, "snapshot index out of range");
    if (!h->n_waters) FAIL(MDX_EPARAM, "no water layout set (mdx_set_water_layout)");
    const auto& sn = h->snapshots[k];
    if (sn.pos.size() != 3 * (size_t)h->N) FAIL(MDX_EPARAM, "snapshot does not hold the whole system");
    float* dst[3] = {o, h0, h1};
    for (uint32_t w = 0; w < h->n_waters; ++w)
        for (uint32_t s3 = 0; s3 < 3; ++s3)
            std::memcpy(dst[s3] + 3 * (size_t)w, sn.pos.data() + 3 * ((size_t)h->water_first + (size_t)w * h->water_sites + s3), 3 * sizeof(float));
    water_make_whole(h, o, dst + 1, 2);
    return MDX_OK;
}

extern "C" uint32_t mdx_snapshot_hbond_count(const mdx_handle* h, uint32_t k) {
    return (h && k < h->snapshots.size()) ? (uint32_t)h->snapshots[k].hbonds.size() : 0u;
}

extern "C" int mdx_snapshot_read_hbonds(mdx_handle* h, uint32_t k, mdx_hbond* out, uint32_t capacity) {
    if (!h || (!out && capacity)) FAIL(MDX_EPARAM, "null argument");
    if (k >= h->snapshots.size()) FAIL(MDX_EPARAM, "snapshot index out of range");
    const auto& hb = h->snapshots[k].hbonds;
    if (hb.size() > capacity) FAIL(MDX_EPARAM, "hydrogen-bond buffer too small (mdx_snapshot_hbond_count)");
    if (!hb.empty()) std::memcpy(out, hb.data(), sizeof(mdx_hbond) * hb.size());
    return MDX_OK;
}

extern "C" int mdx_flush_snapshot_queues(mdx_handle* h) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    h->snapshots.clear();
    h->snapshots.shrink_to_fit();
    return MDX_OK;
}

extern "C" int mdx_initialize_velocities(mdx_handle* h, float temperature, int zero_com_drift, uint64_t seed) {
#pragma clang fp contract(off)   // no FMA contraction: the oracle (built -ffp-contract=off) must get the same bits
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (!(temperature >= 0.f) || !std::isfinite(temperature)) FAIL(MDX_EPARAM, "temperature must be >= 0");
    h->e_cache_valid = false; h->e_pending = false;
    // (joined handle: every rank draws the same stream - it is keyed by the seed and the atom's index - and mdx_upload, collective
    // there, hands every owner its rows)
    if (!h->dd && h->n_local != h->N) FAIL(MDX_EPARAM, "initialize_velocities on a handle narrowed by mdx_set_local_atoms");
    const uint32_t N = h->N;
    std::vector<float> v(3 * (size_t)N);
    std::vector<double> vd(3 * (size_t)N);
    uint64_t st = seed;
    double p[3] = {0, 0, 0}, mt = 0;
    for (uint32_t i = 0; i < N; ++i) {
        const bool fixed = (h->flags[i] & (MDX_ATOM_STATIC | MDX_ATOM_GHOST)) != 0;
        const double sig = std::sqrt(MDX_KB * (double)temperature * 418.4 / (double)h->h_mass[i]);
        for (int d = 0; d < 3; ++d) {
            const double g = rng_gauss(&st);          // drawn for every atom: the stream does not depend on flags
            vd[3 * i + d] = fixed ? 0.0 : g * sig;
            if (!fixed) p[d] += (double)h->h_mass[i] * vd[3 * i + d];
        }
        if (!fixed) mt += h->h_mass[i];
    }
    for (uint32_t i = 0; i < N; ++i) {
        const bool fixed = (h->flags[i] & (MDX_ATOM_STATIC | MDX_ATOM_GHOST)) != 0;
        for (int d = 0; d < 3; ++d)
            v[3 * i + d] = (float)((fixed || !zero_com_drift || mt <= 0) ? vd[3 * i + d] : vd[3 * i + d] - p[d] / mt);
    }
    return mdx_upload(h, MDX_VEL, v.data());
}

// The largest displacement one iteration may give the most-forced atom.  Without a ceiling the x1.2 growth reaches
// several A after ~30 accepted steps, and in a 1 M-atom box a step that tears one water apart (+600 kcal/mol) is
// still "downhill" because the other million atoms gain more: one vibrationally hot molecule then triggers a list
// rebuild every 2-3 steps for the rest of the run.
static constexpr double MDX_MIN_MAX_STEP = 0.2;

extern "C" int mdx_minimize_energy(mdx_handle* h, uint32_t max_iters, const float* ext_forces, float f_tol,
                                   mdx_energies* final_e, uint32_t* iters_done) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (!h->dd && h->n_local != h->N) FAIL(MDX_EPARAM, "minimize_energy needs the library's own decomposition (mdx_comm_init) on a narrowed handle");
    h->e_cache_valid = false; h->e_pending = false;
    // Decomposed handle (collective: every rank makes the call; /root/reference src/properties/sol_shrinking_box.rs:962 reaches the
    // minimiser through the same MdState): every rank moves the atoms it owns along their forces with the SAME step length -
    // energies and the largest force are all-reduced, so accept / refuse and the step-length control take the same branch
    // everywhere; ghost positions follow by halo message before each evaluation; "some atom left the list's reach" is an
    // all-reduced word and then handled like a stale list of the step loop (local rebuild or repartition); the accepted state is
    // a copy of the gathered global positions, and a refused move repartitions from it.
    const bool dd = h->dd != nullptr;
    HIP_TRY(hipSetDevice(h->device));
    MDX_TRY(mdx_step(h, 0.f, ext_forces, 0));      // installs / clears the external forces
    hipStream_t st = h->stream;
    float4* backup = nullptr;                          // accepted positions, caller order
    HIP_TRY(hipMalloc((void**)&backup, sizeof(float4) * (size_t)h->N));
    auto done = [&](int rc) { (void)hipFree(backup); return rc; };
    auto evaluate = [&](mdx_energies* e) -> int {
        if (dd && h->dd->world > 1 && h->in_slot_space) { h->dd->halo_pending = true; h->dd->halo_step = -1; }
        return mdx_energy_impl(h, e);
    };
    auto save = [&]() -> int { return dd ? mdx_dd_save_global(h, backup) : mdx_gather_to_orig(h, h->d.posq, backup); };

    mdx_energies cur{};
    int rc = evaluate(&cur);
    if (rc != MDX_OK) return done(rc);
    rc = save();
    if (rc != MDX_OK) return done(rc);
    double hstep = 0.01;
    uint32_t it = 0;
    const float half = 0.5f * h->cfg.skin;
    uint32_t thr; { float t = std::isinf(h->r_list) ? 1.0e29f : half * half; std::memcpy(&thr, &t, 4); }
    while (it < max_iters && cur.max_force >= (double)f_tol && cur.max_force > 0.0) {
        const float scale = (float)(hstep / cur.max_force);
        if (hipMemsetAsync(&h->d.ctl->disp2[1], 0, sizeof(uint32_t), st) != hipSuccess) return done(MDX_EDEVICE);
        h->vsites_fresh = false;
        hipLaunchKernelGGL(min_move_kernel, dim3(div_up(h->S, 256)), dim3(256), 0, st, h->S, h->d.posq, h->d.force,
                           h->d.vel, h->d.ref, scale, &h->d.ctl->disp2[1], thr);
        uint32_t flag = 0;
        if (hipMemcpyAsync(&flag, &h->d.ctl->disp2[1], sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) { mdx_set_error("HIP error in minimiser"); return done(MDX_EDEVICE); }
        if (dd) { double fv = (double)flag; rc = mdx_dd_allreduce_host(h, &fv, 1, true); if (rc != MDX_OK) return done(rc); flag = (uint32_t)fv; }
        h->forces_valid = false; h->moved_outside = true;
        if (flag > thr) {                            // moved more than skin/2 since the last rebuild
            h->list_valid = false;
            if (dd) { rc = mdx_dd_on_stale(h); if (rc != MDX_OK) return done(rc); }
        }
        if (mdx_has_constraints(h)) {                           // keep constrained bonds at their length
            if (!h->list_valid) { rc = mdx_rebuild(h); if (rc != MDX_OK) return done(rc); }
            rc = mdx_launch_constrain_positions(h, 0.f, nullptr, nullptr, 0);
            if (rc != MDX_OK) return done(rc);
        }
        mdx_energies trial{};
        rc = evaluate(&trial);
        ++it;
        if (rc == MDX_ENAN) { trial.potential = INFINITY; rc = MDX_OK; }
        if (rc != MDX_OK) return done(rc);
        // With external forces (the alignment pull, src/mol_alignment.rs:356) the quantity that must drop is
        // U_total = U - sum F_ext . x: a move along the pull raises the internal potential of a relaxed molecule and
        // would otherwise be refused for ever.  The work is measured from the accepted point, so no origin is needed.
        double ext_work = 0.0;
        if (h->have_ext && std::isfinite(trial.potential)) {
            double* wdev = h->d.energy + EN_COUNT + 1;      // the momentum scratch words
            const bool px = dd || h->per[0], py = dd || h->per[1], pz = dd || h->per[2];
            if (hipMemsetAsync(wdev, 0, sizeof(double), st) != hipSuccess) return done(MDX_EDEVICE);
            hipLaunchKernelGGL(ext_work_kernel, dim3(div_up(h->N, 256)), dim3(256), 0, st, h->N, h->d.slot_of, h->d.posq,
                               backup, h->d.ext_orig, px ? h->box_hi[0] - h->box_lo[0] : 0.f,
                               py ? h->box_hi[1] - h->box_lo[1] : 0.f, pz ? h->box_hi[2] - h->box_lo[2] : 0.f, wdev,
                               dd ? h->d.slot_flags : nullptr);
            if (hipMemcpyAsync(&ext_work, wdev, sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess) { mdx_set_error("HIP error in minimiser"); return done(MDX_EDEVICE); }
            if (dd) { rc = mdx_dd_allreduce_host(h, &ext_work, 1); if (rc != MDX_OK) return done(rc); }
        }
        if (trial.potential - ext_work < cur.potential) {
            cur = trial;
            hstep = std::min(hstep * 1.2, MDX_MIN_MAX_STEP);
            rc = save();
            if (rc != MDX_OK) return done(rc);
        } else {
            hstep *= 0.5;
            // undo: accepted positions back into the caller-order staging, velocities kept
            if (dd) {
                rc = mdx_dd_restore_global(h, backup);
                if (rc != MDX_OK) return done(rc);
            } else {
                rc = mdx_unsort_state(h);
                if (rc != MDX_OK) return done(rc);
                if (hipMemcpyAsync(h->d.pos_orig, backup, sizeof(float4) * (size_t)h->N, hipMemcpyDeviceToDevice, st) != hipSuccess)
                    return done(MDX_EDEVICE);
                h->list_valid = false; h->forces_valid = false;
            }
            mdx_energies again{};
            rc = evaluate(&again);          // forces at the accepted point (the sort order changed)
            if (rc != MDX_OK) return done(rc);
            cur.max_force = again.max_force;
        }
    }
    if (final_e) *final_e = cur;
    if (iters_done) *iters_done = it;
    return done(MDX_OK);
}
