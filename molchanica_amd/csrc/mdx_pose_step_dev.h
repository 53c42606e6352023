// mdx_pose_step_dev.h - the device body of the pose refinements' step kernels (mdx_poses.hip states the passes): the unit-order sum of
// a slab, the ligand and the tables of a pose as a step kernel sees them (StepLigand, StepTables), the stages of an evaluation and
// pose_step, the one body of every step kernel.  A header because its kernels stand in two translation units: pose_refine_step_kernel,
// pose_flex_step_kernel and guest_refine_step_kernel in mdx_poses.hip, guest_flex_step_kernel in mdx_guest_flex.hip.  (A second flexible
// instantiation beside pose_flex_step_kernel in one module changed that kernel: the stepper's functions of mdx_refine_step.h /
// mdx_flex_step.h then have two callers each, the inliner takes them in another order and thread 0's decision came out three scalar
// instructions longer - DESIGN.md 7m.  In a module of its own the new kernel leaves the others' instructions as they were.)
#pragma once
#include "mdx_internal.h"
#include "mdx_refine_step.h"
#include "mdx_flex_step.h"
#include "mdx_pose_plan.h"
#include <type_traits>

// one element of a pose's slab, its POSE_UNITS + 1 partial sums added in unit order: the only place that order is written
__device__ __forceinline__ double pose_units_sum(const double* s, size_t stride) {
    double v = 0.0;
    for (uint32_t u = 0; u <= POSE_UNITS; ++u) v += s[(size_t)u * stride];
    return v;
}

// component k of (sum_i f_i, sum_i (x_i - c) x f_i), atoms in order: the one statement both kernels below take rigid from
__device__ __forceinline__ double pose_rigid_component(uint32_t k, uint32_t count, const double (*s_x)[3], const double (*s_v)[3], const double* s_c) {
    const uint32_t d = k % 3u, d1 = (d + 1u) % 3u, d2 = (d + 2u) % 3u;
    double v = 0.0;
    for (uint32_t i = 0; i < count; ++i)
        v += k < 3u ? s_v[i][d] : (s_x[i][d1] - s_c[d1]) * s_v[i][d2] - (s_x[i][d2] - s_c[d2]) * s_v[i][d1];
    return v;
}

// The ligand of a pose as the kernels behind the force pass see it - PoseLigand's counterpart there: its size, where atom i lies in
// every buffer shaped like the coordinates (the staged trial, forces, accepted and input coordinates: at(i), in floats) and where its
// POSE_UNITS + 1 partial forces start in the force slab (units).  Resident: n atoms, the same for every pose.  GUEST: the pose's record,
// uniform over the workgroup and kept in scalar registers; the blocks of partial forces start at double (POSE_UNITS + 1) x xyz.
template <bool GUEST>
struct StepLigand {
    uint32_t count, pose, xoff;
    __device__ __forceinline__ StepLigand(const PoseRec* rec, uint32_t n, uint32_t p) : count(n), pose(p), xoff(0u) {
        if constexpr (GUEST) {
            count = (uint32_t)__builtin_amdgcn_readfirstlane((int)rec[p].count);
            xoff = (uint32_t)__builtin_amdgcn_readfirstlane((int)rec[p].xyz);
        }
    }
    __device__ __forceinline__ size_t at(uint32_t i) const {
        if constexpr (GUEST) return (size_t)xoff + i * 3u;
        else return ((size_t)pose * count + i) * 3u;
    }
    __device__ __forceinline__ const double* units(const double* fslab, uint32_t i) const {
        if constexpr (GUEST) return fslab + (size_t)(POSE_UNITS + 1u) * xoff + i * 3u;
        else return fslab + ((size_t)pose * (POSE_UNITS + 1u) * count + i) * 3u;
    }
};

// The step kernel's arguments, every instantiation; the rigid ones leave T, n_terms, eterm and the table pointers zero.  G is the width
// of a row.  Guests (rec != null): G is the groups + 1, count is unused, and "[..][count][3]" reads "as the chunk's coordinates lie"
// (StepLigand).
struct StepArgs {
    uint32_t count, G, T, n_terms;
    float* stage;                  // [poses of the chunk][count][3]: the trial the force flavour evaluated; receives the next one
    const double* slab; const double* fslab;
    uint32_t* frozen; void* st;    // st: [poses of the chunk] mdx_rf_state (rigid) or mdx_fx_state (flexible)
    float* x0;                     // [..][count][3] the input poses (kept at evaluation 0)
    float* y; float* row; float* rigid;      // the accepted state: coordinates [..][count][3], row [..][G], rigid [..][6]
    double* eterm;                 // [poses of the chunk][n_terms][13]: energy and the four atoms' forces of every term at this evaluation
    const mdx_fx_torsion* tor; const mdx_fx_dihedral* dih; const uint32_t* aoff; const uint32_t* aent;
    double box[3];                 // periodic axes (0: none), as the force pass has them
    mdx_fx_opts o;
    const PoseRec* rec;            // guests: [poses of the chunk] (last: the resident kernels read their arguments where they always did)
    // flexible guests: [poses of the chunk]; T and n_terms are unused, tor, dih, aoff, aent and eterm are the chunk's tables and every
    // pose's record says where its ligand's part and its own terms lie (StepTables)
    const FlexRec* frec;
};
static_assert(sizeof(mdx_fx_torsion) == GUEST_TOR_BYTES && sizeof(mdx_fx_dihedral) == GUEST_DIH_BYTES, "mdx_pose_plan.h sizes the guest tables");

// The torsion and dihedral tables of a pose as the flexible step kernels see them - StepLigand's counterpart for them.  Resident: the one
// table of the call, read from the arguments at every use as the kernel always did (the object is empty), the pose's terms at
// pose x n_terms of eterm.  GUEST: the pose's FlexRec - T and n_terms are uniform over the workgroup and come through readfirstlane, as
// StepLigand's count does, so that they stay in scalar registers.
template <bool GUEST> struct StepTables;
template <>
struct StepTables<false> {
    __device__ __forceinline__ StepTables(const StepArgs&, uint32_t) {}
    __device__ static __forceinline__ uint32_t torsions(const StepArgs& a, uint32_t) { return a.T; }
    __device__ __forceinline__ uint32_t n_terms(const StepArgs& a) const { return a.n_terms; }
    __device__ __forceinline__ const mdx_fx_torsion* tor(const StepArgs& a) const { return a.tor; }
    __device__ __forceinline__ const mdx_fx_dihedral* dih(const StepArgs& a) const { return a.dih; }
    __device__ __forceinline__ const uint32_t* aoff(const StepArgs& a) const { return a.aoff; }
    __device__ __forceinline__ const uint32_t* aent(const StepArgs& a) const { return a.aent; }
    __device__ __forceinline__ double* eterm(const StepArgs& a, uint32_t pose) const { return a.eterm + (size_t)pose * a.n_terms * FLEX_TERM_WORDS; }
};
template <>
struct StepTables<true> {
    uint32_t nt, to, di, ao, ae, et;
    __device__ __forceinline__ StepTables(const StepArgs& a, uint32_t pose) {
        const FlexRec r = a.frec[pose];
        nt = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.n_terms);
        to = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.tor);
        di = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.dih);
        ao = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.aoff);
        ae = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.aent);
        et = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.eterm);
    }
    __device__ static __forceinline__ uint32_t torsions(const StepArgs& a, uint32_t pose) {
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)a.frec[pose].T);
    }
    __device__ __forceinline__ uint32_t n_terms(const StepArgs&) const { return nt; }
    __device__ __forceinline__ const mdx_fx_torsion* tor(const StepArgs& a) const { return a.tor + to; }
    __device__ __forceinline__ const mdx_fx_dihedral* dih(const StepArgs& a) const { return a.dih + di; }
    __device__ __forceinline__ const uint32_t* aoff(const StepArgs& a) const { return a.aoff + ao; }
    __device__ __forceinline__ const uint32_t* aent(const StepArgs& a) const { return a.aent + ae; }
    __device__ __forceinline__ double* eterm(const StepArgs& a, uint32_t) const { return a.eterm + (size_t)et * FLEX_TERM_WORDS; }
};

__device__ __forceinline__ mdx_rf_state& rf_of(mdx_rf_state& s) { return s; }
__device__ __forceinline__ mdx_rf_state& rf_of(mdx_fx_state& s) { return s.rf; }

// ---- the stages of one evaluation (LDS arrays are the caller's) ----
// Rows and forces of the 17 units added in unit order and rounded where pose_sum_kernel / pose_run and pose_force_sum_kernel round
// them, the staged trial in fp64; WITH_F (flexible): s_f takes the fp32 force mdx_pose_forces returns - what a host loop has.
// A non-finite value raises *s_bad.  Ends with a barrier.
template <bool WITH_F, bool GUEST>
__device__ __forceinline__ void step_gather(const StepArgs& a, const StepLigand<GUEST>& lig, uint32_t pose, uint32_t tid, float* s_row,
                                            double (*s_v)[3], double (*s_x)[3], double (*s_f)[3], uint32_t* s_bad) {
    const uint32_t count = lig.count;
    bool bad = false;
    if (tid < a.G) {
        const float r = (float)pose_units_sum(a.slab + (size_t)pose * (POSE_UNITS + 1u) * a.G + tid, a.G);
        s_row[tid] = r;
        bad = !isfinite(r);
    }
    if (tid < count) {
        const double* s = lig.units(a.fslab, tid);
        const size_t at = lig.at(tid);
        for (uint32_t c = 0; c < 3u; ++c) {
            const double v = pose_units_sum(s + c, (size_t)count * 3u);
            s_v[tid][c] = v; s_x[tid][c] = (double)a.stage[at + c];
            if constexpr (WITH_F) s_f[tid][c] = (double)(float)v;
            bad = bad || !isfinite((float)v);
        }
    }
    if (bad) *s_bad = 1u;      // (every writer stores the same word)
    __syncthreads();
}

// the accepted state leaves for the chunk's block: coordinates, row and rigid of a stored trial; the input pose at evaluation 1
template <bool GUEST>
__device__ __forceinline__ void step_store(const StepArgs& a, const StepLigand<GUEST>& lig, uint32_t pose, uint32_t tid, uint32_t fl, bool first,
                                           const float* s_row, const float* s_rigid) {
    const size_t at = lig.at(tid);
    if (fl & MDX_RF_STORE) {
        if (tid < lig.count)
            for (uint32_t c = 0; c < 3u; ++c) a.y[at + c] = a.stage[at + c];
        if (tid < a.G) a.row[(size_t)pose * a.G + tid] = s_row[tid];
        if (tid < 6u) a.rigid[(size_t)pose * 6u + tid] = s_rigid[tid];
    }
    if (first && tid < lig.count)
        for (uint32_t c = 0; c < 3u; ++c) a.x0[at + c] = a.stage[at + c];
}

// the largest atom speed of the new direction (a maximum: exact in any order) from every thread's m; thread 0 hands it to
// rf_set_speed.  Two barriers; returns the flags with rf_set_speed's.
__device__ __forceinline__ uint32_t step_max_speed(double m, uint32_t tid, uint32_t fl, mdx_rf_state& rf, double* s_m, uint32_t* s_flags) {
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) { const double o = __shfl_xor(m, k); m = o > m ? o : m; }
    if ((tid & 63u) == 0u) s_m[tid >> 6] = m;
    __syncthreads();
    if (tid == 0u) {
        double mm = s_m[0];
        for (int k = 1; k < 4; ++k) mm = s_m[k] > mm ? s_m[k] : mm;
        *s_flags = fl | rf_set_speed(rf, mm);
    }
    __syncthreads();
    return *s_flags;
}

// B(theta) in place: s_x holds the pose in fp64; the torsions in order, each a rotation of its moving set about its axis as the
// coordinates then stand (fx_build with the atoms over the threads).  One barrier per non-zero torsion: the axis of torsion k depends on
// the rotations before it, and the axis atoms are not written in their own round.  tor may lie in LDS or in global memory.
__device__ __forceinline__ void pose_build_torsions(double (*s_x)[3], const mdx_fx_torsion* tor, const double* th, const double* cs,
                                                    const double* sn, uint32_t T, uint32_t count, uint32_t tid) {
    for (uint32_t k = 0; k < T; ++k) {
        if (th[k] == 0.0) continue;      // (uniform over the workgroup)
        const mdx_fx_torsion& t = tor[k];
        double u[3];
        const bool turns = fx_axis(&s_x[0][0], t, u);
        if (turns && tid < count && tid != t.b && fx_member(t.mask, tid)) {
            const double b[3] = {s_x[t.b][0], s_x[t.b][1], s_x[t.b][2]};
            fx_rotate(u, b, cs[k], sn[k], s_x[tid]);
        }
        __syncthreads();
    }
}

// One evaluation of every live pose ends here: gather, frame, then the stepper of mdx_refine_step.h (FLEX: mdx_flex_step.h).  Thread 0
// takes the decisions (a few dozen fp64 operations); the sums over atoms run one component per thread, in atom order.
// FLEX adds the dihedral terms (thread t: term t, its energy and four forces through eterm; one thread adds the energies in list order
// while thread i gathers the forces of the terms that name atom i, in list order), g_k / J_k (thread k, members in atom order), the
// torsion part of the atom field, and the trial builder: B(theta) in LDS from the input pose, then the rigid image of it.  The rigid
// instantiation names none of the FLEX arrays (they take no LDS there) and forms the next trial from x0 by rf_coords.
template <bool FLEX, bool GUEST = false>
__device__ __forceinline__ void pose_step(const StepArgs& a) {
    using State = typename std::conditional<FLEX, mdx_fx_state, mdx_rf_state>::type;
    // s_f, s_g .. s_bc, s_edih and s_tor are FLEX only.  The rigid instantiation must read and write none of them (s_f is handed to
    // step_gather<false>, which does not touch it): an array nobody uses takes no LDS, and that is all that keeps the rigid kernel at
    // 13,752 B and 8 workgroups per CU.  After a change here, read "LDS Size" of both instantiations in the
    // -Rpass-analysis=kernel-resource-usage remarks (13,752 / 26,088 B).  The order of the declarations is the LDS layout's.
    __shared__ double s_x[MDX_POSE_MAX_ATOMS][3], s_v[MDX_POSE_MAX_ATOMS][3], s_f[MDX_POSE_MAX_ATOMS][3], s_c[3], s_I[6], s_R[9], s_m[4];
    __shared__ double s_g[MDX_FX_MAX_TORSIONS], s_J[MDX_FX_MAX_TORSIONS], s_A[MDX_FX_MAX_TORSIONS][3], s_u[MDX_FX_MAX_TORSIONS][3],
                      s_sh[MDX_FX_MAX_TORSIONS][3], s_wk[MDX_FX_MAX_TORSIONS], s_cs[MDX_FX_MAX_TORSIONS], s_sn[MDX_FX_MAX_TORSIONS], s_bc[3];
    __shared__ float s_row[256], s_rigid[6], s_edih;
    __shared__ State s_st;
    __shared__ mdx_fx_torsion s_tor[MDX_FX_MAX_TORSIONS];
    __shared__ uint32_t s_bad, s_flags;
    const uint32_t tid = threadIdx.x, pose = blockIdx.x, T = StepTables<FLEX && GUEST>::torsions(a, pose);
    if (a.frozen[pose] != 0u) return;      // (uniform over the workgroup, before any barrier)
    const StepLigand<GUEST> lig(a.rec, a.count, pose);
    const StepTables<FLEX && GUEST> tab(a, pose);      // (FLEX only: the rigid instantiations use nothing of it)
    const uint32_t count = lig.count;
    uint32_t* const rec = (uint32_t*)((State*)a.st + pose);
    for (uint32_t i = tid; i < sizeof(State) / 4u; i += 256u) ((uint32_t*)&s_st)[i] = rec[i];
    if constexpr (FLEX)
        for (uint32_t i = tid; i < T * (uint32_t)(sizeof(mdx_fx_torsion) / 4u); i += 256u) ((uint32_t*)s_tor)[i] = ((const uint32_t*)tab.tor(a))[i];
    if (tid == 0u) s_bad = 0u;
    __syncthreads();
    mdx_rf_state& rf = rf_of(s_st);
    step_gather<FLEX>(a, lig, pose, tid, s_row, s_v, s_x, s_f, &s_bad);      // (s_f: written under FLEX only)
    // centroid | barrier | rigid by the statement of pose_force_sum_kernel beside the six inertia sums on a wave of their own; the
    // FLEX parts share those two intervals, so the three statements stand here and not in a helper
    if (tid < 3u) s_c[tid] = rf_mean(&s_x[0][0], count, tid);
    double* eterm = nullptr;
    if constexpr (FLEX) {
        // the ligand's dihedral terms, one term per thread: its energy and its four forces go through eterm
        eterm = tab.eterm(a, pose);
        const double box[3] = {a.box[0], a.box[1], a.box[2]};
        for (uint32_t t = tid; t < tab.n_terms(a); t += 256u) {
            double f[4][3];
            double* o = eterm + (size_t)t * FLEX_TERM_WORDS;
            o[0] = fx_dihedral(&s_x[0][0], tab.dih(a)[t], box, f);
#pragma unroll
            for (int r = 0; r < 4; ++r) { o[1 + 3 * r] = f[r][0]; o[2 + 3 * r] = f[r][1]; o[3 + 3 * r] = f[r][2]; }
        }
    }
    __syncthreads();
    if (tid < 6u) s_rigid[tid] = (float)pose_rigid_component(tid, count, s_x, s_v, s_c);
    if (tid >= 64u && tid < 70u) s_I[tid - 64u] = rf_inertia(&s_x[0][0], count, s_c, tid - 64u);
    if constexpr (FLEX) {
        if (tid == 128u) {      // the energies in list order
            double e = 0.0;
            for (uint32_t t = 0; t < tab.n_terms(a); ++t) e += eterm[(size_t)t * FLEX_TERM_WORDS];
            s_edih = (float)e;
        }
        if (tid < count && tab.n_terms(a)) {
            // thread i: the forces of the terms that name atom i, in list order - the atom-owned gather
            double f0 = 0.0, f1 = 0.0, f2 = 0.0;
            for (uint32_t e = tab.aoff(a)[tid]; e < tab.aoff(a)[tid + 1u]; ++e) {
                const uint32_t w = tab.aent(a)[e];
                const double* o = eterm + (size_t)(w >> 2) * FLEX_TERM_WORDS + 1u + 3u * (w & 3u);
                f0 += o[0]; f1 += o[1]; f2 += o[2];
            }
            if (!isfinite(f0) || !isfinite(f1) || !isfinite(f2)) s_bad = 1u;
            s_f[tid][0] += f0; s_f[tid][1] += f1; s_f[tid][2] += f2;
        }
        __syncthreads();
        if (tid < T) {
            const double n = (double)count;
            const double v[3] = {(double)s_rigid[0] / n, (double)s_rigid[1] / n, (double)s_rigid[2] / n};
            fx_gradient(&s_x[0][0], &s_f[0][0], count, v, s_tor[tid], s_u[tid], s_g[tid], s_J[tid], s_A[tid]);
        }
    }
    __syncthreads();
    if (tid == 0u) {
        bool finite = s_bad == 0u;
        for (int k = 0; k < 6; ++k) finite = finite && isfinite(s_rigid[k]);
        double S = 0.0;
        for (uint32_t b = 0; b < a.G; ++b) S += (double)s_row[b];
        uint32_t fl;
        if constexpr (FLEX) {
            double gmax = 0.0;
            finite = finite && isfinite(s_edih);      // (here: read ahead of the row sum, the evaluation measured 0.3 us slower)
            S += (double)s_edih;
            for (uint32_t k = 0; k < T; ++k) {
                const double g = fabs(s_g[k]);
                finite = finite && isfinite(g);
                gmax = g > gmax ? g : gmax;
            }
            if (rf.evals == 0u) fx_start(s_st, s_c, a.o.rf.h_start);      // (the record was zeroed: the trial is the input pose)
            fl = fx_decide(s_st, a.o, T, S, finite, s_rigid, gmax);
            if (fl & MDX_RF_STORE) {
                s_st.edih = s_edih;
                for (uint32_t k = 0; k < T; ++k) s_st.g[k] = s_g[k];
            }
        } else {
            if (rf.evals == 0u) rf_start(rf, s_c, a.o.rf.h_start);        // (likewise)
            fl = rf_decide(rf, a.o.rf, S, finite, s_rigid);
        }
        if (fl == MDX_RF_STORE) rf_direction(rf, count, s_rigid, s_I);
        s_flags = fl;
    }
    if constexpr (FLEX)
        if (tid >= 64u && tid < 64u + T) {      // (a wave beside thread 0's: used only if the trial is stored and the pose goes on)
            const uint32_t k = tid - 64u;
            s_wk[k] = fx_omega(s_g[k], s_J[k]);
            fx_shift(s_wk[k], s_A[k], count, s_sh[k]);
        }
    __syncthreads();
    if constexpr (FLEX)
        if (s_flags == MDX_RF_STORE && tid < T) s_st.wk[tid] = s_wk[tid];      // (read again only after the next barrier)
    uint32_t fl = s_flags;
    step_store(a, lig, pose, tid, fl, rf.evals == 1u, s_row, s_rigid);
    if (fl == MDX_RF_STORE) {
        double m = 0.0;
        if (tid < count) {
            if constexpr (FLEX) m = fx_speed(rf.v, rf.w, s_c, &s_x[0][0], tid, T, s_tor, s_u, s_wk, s_sh);
            else {
                const double r[3] = {s_x[tid][0] - s_c[0], s_x[tid][1] - s_c[1], s_x[tid][2] - s_c[2]};
                m = rf_speed(rf.v, rf.w, r);
            }
        }
        fl = step_max_speed(m, tid, fl, rf, s_m, &s_flags);
    }
    const size_t at = lig.at(tid);
    if (!(fl & MDX_RF_FROZEN)) {
        if (tid == 0u) {
            if constexpr (FLEX) fx_trial(s_st, T); else rf_trial(rf);
            rf_rotation(rf.qt, s_R);
        }
        if constexpr (FLEX) {
            // B(theta_try) from the input pose: s_x is free now
            if (tid < count)
                for (uint32_t c = 0; c < 3u; ++c) s_x[tid][c] = (double)a.x0[at + c];
            __syncthreads();
            if (tid < T) { s_cs[tid] = cos(s_st.tht[tid]); s_sn[tid] = sin(s_st.tht[tid]); }
            __syncthreads();
            pose_build_torsions(s_x, s_tor, s_st.tht, s_cs, s_sn, T, count, tid);
            if (tid < 3u) s_bc[tid] = rf_mean(&s_x[0][0], count, tid);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < sizeof(State) / 4u; i += 256u) rec[i] = ((const uint32_t*)&s_st)[i];
    if (fl & MDX_RF_FROZEN) {
        if (tid == 0u) a.frozen[pose] = 1u;
        return;
    }
    if (tid < count) {
        float y[3];
        if constexpr (FLEX) fx_coords(rf.c0, rf.tt, s_R, s_x[tid], s_bc, y);
        else {
            const float x0[3] = {a.x0[at], a.x0[at + 1u], a.x0[at + 2u]};
            rf_coords(rf.c0, rf.tt, s_R, x0, y);
        }
        for (uint32_t c = 0; c < 3u; ++c) a.stage[at + c] = y[c];
    }
}

// mdx_guest_flex.hip: guest_flex_step_kernel on n poses (pose_step<true, true>)
void mdx_launch_guest_flex_step(hipStream_t st, uint32_t n, const StepArgs& a);
