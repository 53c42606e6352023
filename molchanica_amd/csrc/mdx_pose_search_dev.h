// mdx_pose_search_dev.h - the device body of the search kernels (mdx_search_step.h holds the rule, mdx_poses.hip states the passes):
// pose_search<GUEST>, the one body of pose_search_kernel (mdx_poses.hip, a resident ligand) and guest_search_kernel
// (mdx_guest_search.hip, a library of guests).  A header for the reason mdx_pose_step_dev.h is one: the guest kernel calls the stepper's
// inline functions (rf_mean, rf_rotation, fx_coords, sr_xform -> rf_trial), and a second caller of them inside mdx_poses.hip changes how
// the inliner treats the resident kernels.
#pragma once
#include "mdx_pose_step_dev.h"
#include "mdx_search_step.h"

static_assert(sizeof(mdx_sr_record) == SEARCH_REC_BYTES, "mdx_pose_plan.h sizes the search records");

// Resident: count atoms and T torsions of the one table `tor` for every walker, the coordinate-shaped buffers walker-major.  Guests:
// count and T are unused, G is the groups + 1, stage is the chunk's staged coordinates (the xyz block of GuestLayout: the guest force
// pass reads it, the step kernel writes it), tor the chunk's torsion tables, and every walker's PoseRec / FlexRec - two further kernel
// arguments, so that the resident kernel's stay where they were - say where its stretch of the coordinates and its ligand's table lie
// (StepLigand<true>, StepTables<true>).
struct SearchArgs {
    uint32_t count, G, T, pad;
    float* stage; uint32_t* frozen; mdx_fx_state* st;              // what the refinement starts from: staged pose, frozen word, state record
    const float* y; const float* row; const float* rigid;          // what it ended with: its accepted coordinates, row and rigid
    const mdx_fx_torsion* tor;
    const uint64_t* streams; mdx_sr_record* rec;
    float* cur_y; float* best_y; float* best_row; float* best_rigid;
    mdx_sr_opts o;
};

// Launched with round index r between two refinements, one workgroup per walker: it decides round r - 1 (r >= 1) from what the
// refinement left - thread 0 takes the decision, the threads copy the accepted coordinates (and, for a new best, row and rigid) into the
// walker's search record - and, for r < n_rounds, starts round r: thread 0 draws the move and forms (dq, dt), B(dtheta) is built in LDS
// from the current pose by pose_build_torsions, the loop the flexible step kernels build a trial with, every thread writes its atom of
// X0' into the staging buffer, and the walker's state record and frozen word are zeroed ("evaluation 0: the trial is the input").
// Round 0 has no move: the staged pose is the caller's.  Plain stores only: one workgroup owns a walker.
template <bool GUEST>
__device__ __forceinline__ void pose_search(const SearchArgs& a, uint32_t r, const PoseRec* prec = nullptr, const FlexRec* frec = nullptr) {
    __shared__ double s_x[MDX_POSE_MAX_ATOMS][3], s_c[3], s_bc[3], s_R[9], s_t[3], s_th[MDX_FX_MAX_TORSIONS], s_cs[MDX_FX_MAX_TORSIONS],
                      s_sn[MDX_FX_MAX_TORSIONS];
    __shared__ uint32_t s_fl;
    const uint32_t tid = threadIdx.x, walker = blockIdx.x;
    const StepLigand<GUEST> lig(prec, a.count, walker);
    const uint32_t count = lig.count;
    // the walker's torsions: the call's table, or its ligand's part of the chunk's (the record's words through readfirstlane)
    uint32_t T = a.T;
    const mdx_fx_torsion* tor = a.tor;
    if constexpr (GUEST) {
        StepArgs sa{};
        sa.frec = frec; sa.tor = a.tor;
        T = StepTables<true>::torsions(sa, walker);
        tor = StepTables<true>(sa, walker).tor(sa);
    }
    const size_t at = lig.at(tid);
    uint32_t fl = 0u;
    if (r >= 1u) {
        if (tid == 0u) {
            const mdx_fx_state* s = a.st + walker;
            mdx_sr_record rec = a.rec[walker];
            const bool finite = !(s->rf.frozen != 0u && s->rf.status == MDX_RF_NONFINITE);
            s_fl = sr_decide(rec, a.o, r - 1u, s->rf.S, finite, s->edih, s->rf.evals, sr_stream(a.o.seed, a.streams[walker], r - 1u));
            a.rec[walker] = rec;
        }
        __syncthreads();
        fl = s_fl;
        if (fl & MDX_SR_BEST) {
            if (tid < count)
                for (uint32_t c = 0; c < 3u; ++c) a.best_y[at + c] = a.y[at + c];
            if (tid < a.G) a.best_row[(size_t)walker * a.G + tid] = a.row[(size_t)walker * a.G + tid];
            if (tid < 6u) a.best_rigid[(size_t)walker * 6u + tid] = a.rigid[(size_t)walker * 6u + tid];
        }
    }
    if (r >= a.o.n_rounds) {      // (uniform over the grid: the last launch only decides)
        if ((fl & MDX_SR_ACCEPT) && tid < count)
            for (uint32_t c = 0; c < 3u; ++c) a.cur_y[at + c] = a.y[at + c];
        return;
    }
    if (r >= 1u) {
        // the current pose: the round just accepted, or the record's
        const float* src = (fl & MDX_SR_ACCEPT) ? a.y : a.cur_y;
        if (tid < count)
            for (uint32_t c = 0; c < 3u; ++c) {
                const float v = src[at + c];
                s_x[tid][c] = (double)v;
                if (fl & MDX_SR_ACCEPT) a.cur_y[at + c] = v;
            }
        if (tid < MDX_FX_MAX_TORSIONS) s_th[tid] = 0.0;
        __syncthreads();
        if (tid < 3u) s_c[tid] = rf_mean(&s_x[0][0], count, tid);
        if (tid == 64u) {      // (a wave beside the centroid's)
            mdx_sr_move mv;
            double q[4];
            sr_move(a.o, T, sr_stream(a.o.seed, a.streams[walker], r), mv);
            sr_xform(mv, q, s_t);
            rf_rotation(q, s_R);
            if (mv.kind == MDX_SR_TORSION) { s_th[mv.torsion] = mv.dtheta; s_cs[mv.torsion] = cos(mv.dtheta); s_sn[mv.torsion] = sin(mv.dtheta); }
        }
        __syncthreads();
        pose_build_torsions(s_x, tor, s_th, s_cs, s_sn, T, count, tid);      // (the table where it lies: at most one torsion turns per round)
        if (tid < 3u) s_bc[tid] = rf_mean(&s_x[0][0], count, tid);
        __syncthreads();
        if (tid < count) {
            float y[3];
            fx_coords(s_c, s_t, s_R, s_x[tid], s_bc, y);
            for (uint32_t c = 0; c < 3u; ++c) a.stage[at + c] = y[c];
        }
    }
    uint32_t* dst = (uint32_t*)(a.st + walker);
    for (uint32_t i = tid; i < sizeof(mdx_fx_state) / 4u; i += 256u) dst[i] = 0u;
    if (tid == 0u) a.frozen[walker] = 0u;
}

// mdx_guest_search.hip: guest_search_kernel on the n walkers of a chunk with round index r (pose_search<true>)
// prec, frec: [n] the walkers' records
void mdx_launch_guest_search(hipStream_t st, uint32_t n, const SearchArgs& a, uint32_t r, const PoseRec* prec, const FlexRec* frec);
