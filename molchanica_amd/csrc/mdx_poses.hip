// mdx_poses.hip - mdx_score_poses: the ligand row of `energy_potential_between_mols` for a BATCH of alternative placements of one
// group of atoms (the docking scorer of BASELINE config 3, /root/reference src/docking/mod.rs:81-154 "a binding energy computation each
// step"; src/screening wants the same), in one pass that leaves the handle as it found it.
//
// Per pose only ~count x a few thousand pairs depend on the pose; mdx_upload_range + mdx_energy_between_mols pays a pass over the whole
// pair list of the complex for them.  Here the environment stays where it is - slot-space posq / lj of the current state, the column /
// tile structure of the last rebuild - and a pose is the ligand's rows in LDS:
//
//   grid (POSE_UNITS + 1, poses of the chunk), 256 threads.  Every workgroup stages its pose (xyz from the batch, charge and LJ record
//   from the ligand's own slots) and takes the pose's bounding box.
//   units 0 .. POSE_UNITS-1  the environment.  The columns whose atoms can lie within r_list of the box (periodic axes wrap, a
//       non-periodic grid clamps), their tiles, of those the tiles with t mod POSE_UNITS = unit; the tile's eight cluster boxes are tested by
//       eight lanes at once - the boxes were taken at the rebuild, so the test radius is r_list = cutoff + skin, twice the drift the list
//       allows - and the clusters that pass go round the four waves.  Lane = (environment atom ii of the cluster, ligand atom jj of a
//       strip of 8), looping over the ligand in strips: the 8 x 8 shape of the pair kernels.  The minimum image is taken per pair
//       (d - rint(d / L) L, as the bonded gather and the oracle take it), then the SAME pair_eval (mdx_pair_dev.h) in its energy flavour:
//       a row is made of the pair terms mdx_energy sums.  Slots of the ligand's own group and dummy slots are skipped.
//       fp64 per lane, keyed by the environment atom's group; when a key changes the wave folds its sums - shuffles over jj, then the
//       eight ii in lane order - into its own LDS row.  At the end the four rows are added in wave order.
//   unit POSE_UNITS  the ligand's own pairs from the class map (plain: pair_eval; excluded: nothing; 1-4: the scaled records, the
//       arithmetic of group_pairs14_kernel), one fixed share per thread, folded in lane and wave order.
//   Every unit writes its partial row into slab[pose][unit][group]; pose_sum_kernel adds the units in order.  Which tiles a unit
//   takes, which cluster a wave takes and the order of every sum depend on the pose and the resident structure alone - not on the
//   batch, its size or timing - so a pose gives the same bits alone or among 4096, anywhere in the batch.  No atomics.
//
// mdx_pose_forces: the same pass in its force flavour (FORCE = true; the energy flavour is the parent's code) - per pose the force on
// every ligand atom, -d(sum of the row)/dx_i, and their net force and torque about the pose's centroid.
//   environment units  pair_eval hands back the force on the environment atom; minus it is the force on ligand atom ja.  The eight ii
//       lanes of a jj fold it with three fp32 shuffle-adds (eight pair forces: 3 roundings of 2^-24 of their gross sum, below what the
//       fp32 pair arithmetic itself leaves), and lane ii = 0 adds the sum into the wave's own fp64 LDS accumulator [wave][xyz][ja]:
//       the eight ja of a strip are distinct and the accumulator belongs to one wave - plain read-modify-write, no atomics.  fp64
//       there because a ligand atom collects thousands of pair forces that largely cancel.  Dynamic LDS, 96 B per ligand atom (rounded
//       up to whole strips): 5.4 kB for 50 atoms, 24 kB for 256.  At the end the four waves' sums are added in wave order.
//   ligand unit  thread ia owns ligand atom ia: it walks ib in order over the class map (each plain pair is evaluated from both sides;
//       d and -d give forces that are exact negatives) and the 1-4 records that name ia, fp64 in registers.  The energy part is the
//       energy flavour's, statement by statement: the rows are the bits mdx_score_poses returns.
//   Every unit writes fslab[pose][unit][count][3]; pose_force_sum_kernel adds the units in order, rounds to fp32 and forms the net
//   force and the torque in fp64 in atom order.
//
// mdx_refine_poses: a rigid-body steepest descent of every pose of the batch with its own adaptive step length (the rule of
// mdx_minimize_energy carried over to rigid motions; mdx_refine_step.h holds its arithmetic), max_evals x (the force flavour,
// pose_refine_step_kernel) per chunk on the stream, one read-back and one wait at the end.
//   pose_step<FLEX>  the body of both step kernels, one workgroup per pose (pose_refine_step_kernel is pose_step<false>,
//       pose_flex_step_kernel is pose_step<true>: two plain kernels, one body).  It adds the units' rows and forces as the two sum kernels do, forms rigid as
//       pose_force_sum_kernel does, accepts or rejects the trial from the pose's state record, and writes the next trial into the
//       staging buffer the force flavour reads.  A pose that has finished sets its word in frozen[]; the REFINE instantiation of
//       pose_score_kernel reads it before anything else and the whole workgroup returns, as the step kernel's does.
//
// mdx_refine_poses_flex: the same loop with the ligand's torsion angles as further coordinates (pose_flex_step_kernel,
// mdx_flex_step.h): the torsion and dihedral parts of pose_step, compiled in by `if constexpr (FLEX)`.
//
// mdx_search_poses: n_rounds of that loop per walker with pose_search_kernel between two of them (mdx_search_step.h): it decides the
// round that ended - Metropolis on the refinement's objective, current and best pose in the walker's search record - and perturbs the
// current pose into the staging buffer for the next; n_rounds x (1 + 2 max_evals) + 1 launches per chunk, one read-back, one wait.
//
// mdx_screen_ligands: the energy flavour for GUEST ligands - described by the caller, never entered into the handle (src/screening: one
// receptor, a library of candidates).  The same kernel body under GUEST = true: PoseLigand<GUEST> is the one place the two ligand
// sources differ - a resident ligand is a range of the handle's atoms, the same for every pose of the launch, with its rows behind
// slot_of and its own pairs in the handle's table; a guest pose carries a PoseRec into the chunk's staged tables, so one launch holds
// ligands of different sizes.  The environment walk, the strips, the fold, the own-pair loops and the slab are the resident ones; a
// guest skips no group, and its slab rows have one more column for its own pairs.  guest_best_kernel picks the best pose per ligand
// from the chunk's summed rows and carries it across chunks.
//
// mdx_guest_forces, mdx_refine_guests: the force flavour and the rigid refinement for guests.  One launch holds poses of different
// sizes, so what the force flavour sized by the ligand's count comes from the pose's record: the unit's block of the force slab
// (PoseLigand::fslab - a pose's POSE_UNITS + 1 blocks start at (POSE_UNITS + 1) x the offset of its coordinates), fstride and the
// own-pair unit's tid < count; the launch's dynamic LDS is sized by the chunk's largest ligand and every workgroup lays its own
// [wave][xyz][fstride] inside it.  Behind the force pass StepLigand<GUEST> mirrors PoseLigand: pose_force_sum and pose_step index every
// coordinate-shaped buffer through it (guest_force_sum_kernel, guest_refine_step_kernel: further plain kernels over the one body),
// the stage buffer is the chunk's coordinate block, rows are G + 1 wide, and guest_best reads the accepted fp32 rows.
//
// mdx_refine_guests_flex: the flexible refinement for guests - the GUEST REFINE force pass as it is, then guest_flex_step_kernel,
// pose_step<true, true>.  A pose's torsion table, dihedral terms, gather tables and its stretch of the terms' energies and forces come
// from a FlexRec beside its PoseRec (StepTables<GUEST> is to them what StepLigand is to the coordinates): T and n_terms differ from
// ligand to ligand within one launch, the tables are staged once per ligand of the chunk behind its class map, and eterm is as long as
// the chunk's poses have terms.  guest_best_flex_kernel is guest_best over the flexible records: S with the accepted E_dih.  The body of
// the step kernels stands in mdx_pose_step_dev.h and the new kernel in mdx_guest_flex.hip, for the reason given there.
//
// mdx_search_guests: the search for guests - the loop of mdx_refine_guests_flex run n_rounds times per chunk with guest_search_kernel
// between two of them: pose_search<true>, the body of pose_search_kernel (mdx_pose_search_dev.h) with the walker's size and stretch of
// the coordinates from its PoseRec and its torsion table from its FlexRec; the kernel stands in mdx_guest_search.hip.  The chunk's
// search block (SearchLayout, the same struct for both tracks) lies behind its step block in gs_blk (GUEST_SEARCH), the stream ids go
// up with the chunk, and guest_best_search_kernel is guest_best over the walkers' search records: S_best as it is.
//
// What is written once: the unit-order sum of a slab (pose_units_sum: the four kernels that add the 17 units take it from there, which
// is why rows_out / rigid_out of a refinement are the bits mdx_score_poses / mdx_pose_forces return), the stages of an evaluation
// (step_gather, step_store, step_max_speed; centroid, rigid and inertia stand once in pose_step), the B(theta) loop
// (pose_build_torsions: the flexible step kernel and the search kernel), and on the host the Coulomb dispatch (pose_launch),
// buffer growth (pose_grow), the block of a chunk (StepLayout), the option checks (refine_opts_check) and the chunk loop with its
// unpacker (refine_chunks, refine_unpack); for guests the checks, the plan (mdx_pose_plan.h), the arguments and the staging of a chunk
// (guest_check, guest_plan / guest_slots / guest_records, guest_ready, guest_stage), shared by the three guest entry points.
#include "mdx_bonded_dev.h"
#include "mdx_pair_dev.h"
#include "mdx_refine_step.h"
#include "mdx_flex_step.h"
#include "mdx_search_step.h"
#include "mdx_pose_plan.h"
#include "mdx_pose_step_dev.h"
#include "mdx_pose_search_dev.h"
#include <cmath>
#include <cstring>
#include <type_traits>

#define FAIL(code, msg) do { mdx_set_error(msg); return (code); } while (0)

// (POSE_UNITS, POSE_CHUNK, Pose14 and PoseRec - the record of a guest pose - stand in mdx_pose_plan.h beside the layouts made of them)

struct PoseArgs {
    NbParams p;
    GridParams g;
    const float4* posq; const float2* lj;
    const uint32_t* orig_of; const uint32_t* gid; const uint8_t* grp; const uint32_t* slot_of;
    const uint32_t* tile_start; const float4* cl_lo; const float4* cl_hi;
    uint32_t G, L, first, count;
    const float* poses;            // [poses of the chunk][count][3]
    double* slab;                  // [poses of the chunk][POSE_UNITS + 1][G]
    double* fslab;                 // force flavour: [poses of the chunk][POSE_UNITS + 1][count][3]
    float r_cull;                  // r_list (+ rounding room); not finite: no cutoff, everything is a candidate
    float box[3], inv_box[3];      // periodic axes (0: none)
    const uint8_t* cls; const Pose14* p14; uint32_t n14;
    const uint32_t* frozen;        // REFINE: [poses of the chunk], non-zero = the pose has finished, its workgroups return at once
    // GUEST: the ligand is the caller's, not the handle's.  first / L are unused and count is the host's alone (the chunk's largest
    // ligand: it sizes the force flavour's dynamic LDS); cls and p14 are the chunk's tables, poses its coordinates, and the slab rows
    // are G + 1 wide (column G: the ligand's own pairs)
    const PoseRec* rec;            // [poses of the chunk]
    const float* gq; const float2* glj;      // [ligand atoms of the chunk]: q sqrt(k_e), the packed LJ record (mdx_pack_lj)
};

__device__ __forceinline__ float pose_mimg(float d, float box, float inv) { return box > 0.f ? d - rintf(d * inv) * box : d; }

// the wave's per-lane sums leave for its LDS row: lanes of equal ii hold the same key
__device__ __forceinline__ void pose_fold(double& dacc, uint32_t key, double* row, int lane) {
    double v = dacc;
    v += __shfl_xor(v, 8); v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
#pragma unroll 1
    for (int k = 0; k < 8; ++k)
        if (lane == k && v != 0.0) row[key] += v;
    dacc = 0.0;
}

// The ligand of a pose: its size, where its coordinates and its own-pair tables lie, its charge and LJ rows.  Resident (GUEST = false): a
// range of the handle's atoms, the same for every pose of the launch, rows through slot_of.  GUEST: the pose's record - one launch
// carries ligands of different sizes - and rows from the chunk's guest tables.  Every member but the rows is uniform over the
// workgroup; the guest's come through readfirstlane so that count and the strip count stay in scalar registers, as `wave` does.
template <bool GUEST>
struct PoseLigand {
    uint32_t count, n14, W;        // W: width of a slab row
    const float* xyz; const uint8_t* cls; const Pose14* p14;
    uint32_t atom, xoff;           // xoff (GUEST): the record's xyz
    __device__ __forceinline__ PoseLigand(const PoseArgs& a, uint32_t pose) {
        if constexpr (GUEST) {
            const PoseRec r = a.rec[pose];
            xoff = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.xyz);
            count = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.count);
            n14 = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.n14);
            atom = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.atom);
            xyz = a.poses + xoff;
            cls = a.cls + (uint32_t)__builtin_amdgcn_readfirstlane((int)r.cls);
            p14 = a.p14 + (uint32_t)__builtin_amdgcn_readfirstlane((int)r.p14);
            W = a.G + 1u;
        } else {
            count = a.count; n14 = a.n14; atom = a.first; W = a.G; xoff = 0u;
            xyz = a.poses + (size_t)pose * count * 3;
            cls = a.cls; p14 = a.p14;
        }
    }
    // the unit's partial forces [count][3] of the force slab: the poses of a guest chunk differ in size, and a pose's POSE_UNITS + 1
    // blocks start where its coordinates do, scaled
    __device__ __forceinline__ double* fslab(const PoseArgs& a, uint32_t pose, uint32_t unit) const {
        if constexpr (GUEST) return a.fslab + (size_t)(POSE_UNITS + 1u) * xoff + (size_t)unit * count * 3u;
        else return a.fslab + ((size_t)pose * (POSE_UNITS + 1u) + unit) * count * 3u;
    }
    // charge (q sqrt(k_e)) and packed LJ record of ligand atom i
    __device__ __forceinline__ void row(const PoseArgs& a, uint32_t i, float& q, float2& lj) const {
        if constexpr (GUEST) { q = a.gq[atom + i]; lj = a.glj[atom + i]; }
        else {
            const uint32_t s = a.slot_of[atom + i];
            if (s != MDX_INVALID) { q = a.posq[s].w; lj = a.lj[s]; }
        }
    }
};

template <int COUL, bool GEOM, bool FORCE, bool REFINE = false, bool GUEST = false>
__global__ __launch_bounds__(256) void pose_score_kernel(PoseArgs a) {
    extern __shared__ double s_f[];      // FORCE: [4 waves][xyz][fstride] of this pose (the launch sizes it by its largest; nothing otherwise)
    if (REFINE && a.frozen[blockIdx.y] != 0u) return;      // (uniform over the workgroup, before any barrier)
    __shared__ float4 s_xyzq[MDX_POSE_MAX_ATOMS];
    __shared__ float2 s_lj[MDX_POSE_MAX_ATOMS];
    __shared__ double s_row[4][256];
    __shared__ float s_bb[4][6];
    const uint32_t tid = threadIdx.x, unit = blockIdx.x, pose = blockIdx.y;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const PoseLigand<GUEST> lig(a, pose);
    const uint32_t count = lig.count;

    // ---- the pose: rows in LDS, bounding box ----
    float4 me = make_float4(0.f, 0.f, 0.f, 0.f); float2 mlj = make_float2(0.f, 0.f);
    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    if (tid < count) {
        const float* x = lig.xyz + (size_t)tid * 3;
        me = make_float4(x[0], x[1], x[2], 0.f);
        lig.row(a, tid, me.w, mlj);
        lo[0] = hi[0] = me.x; lo[1] = hi[1] = me.y; lo[2] = hi[2] = me.z;
    }
    s_xyzq[tid] = me; s_lj[tid] = mlj;
#pragma unroll
    for (int w = 0; w < 4; ++w) s_row[w][tid] = 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) { lo[d] = fminf(lo[d], __shfl_xor(lo[d], m)); hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], m)); }
    if (lane == 0)
#pragma unroll
        for (int d = 0; d < 3; ++d) { s_bb[wave][d] = lo[d]; s_bb[wave][3 + d] = hi[d]; }
    __syncthreads();
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        lo[d] = fminf(fminf(s_bb[0][d], s_bb[1][d]), fminf(s_bb[2][d], s_bb[3][d]));
        hi[d] = fmaxf(fmaxf(s_bb[0][3 + d], s_bb[1][3 + d]), fmaxf(s_bb[2][3 + d], s_bb[3][3 + d]));
    }
    double* out = a.slab + ((size_t)pose * (POSE_UNITS + 1u) + unit) * lig.W;
    const uint32_t fstride = ((count + 7u) >> 3) << 3;
    double* fout = FORCE ? lig.fslab(a, pose, unit) : nullptr;

    if (unit == POSE_UNITS) {
        // ---- the ligand's own pairs ----
        double acc = 0.0;
        const uint32_t n2 = count * count;
        for (uint32_t i = tid; i < n2; i += 256u) {
            const uint32_t ia = i / count, ib = i - ia * count;
            if (ia >= ib || lig.cls[i] != 0) continue;
            const float4 pa = s_xyzq[ia], pb = s_xyzq[ib];
            const float2 la = s_lj[ia];
            const float dx = pose_mimg(pa.x - pb.x, a.box[0], a.inv_box[0]), dy = pose_mimg(pa.y - pb.y, a.box[1], a.inv_box[1]),
                        dz = pose_mimg(pa.z - pb.z, a.box[2], a.inv_box[2]);
            float fx = 0.f, fy = 0.f, fz = 0.f, e1 = 0.f, e2 = 0.f;
            pair_eval<true, COUL, GEOM, false, true, false, false, true>(dx, dy, dz, pa.w, la.x, la.y, make_float4(0.f, 0.f, 0.f, pb.w), s_lj[ib], true, a.p,
                                                                       fx, fy, fz, e1, e2, nullptr, nullptr, nullptr, 0.f);
            acc += (double)(e1 + e2);
        }
        for (uint32_t k = tid; k < lig.n14; k += 256u) {
            const Pose14 r = lig.p14[k];
            const float4 pa = s_xyzq[r.a], pb = s_xyzq[r.b];
            const float dx = pose_mimg(pa.x - pb.x, a.box[0], a.inv_box[0]), dy = pose_mimg(pa.y - pb.y, a.box[1], a.inv_box[1]),
                        dz = pose_mimg(pa.z - pb.z, a.box[2], a.inv_box[2]);
            const float r2 = dx * dx + dy * dy + dz * dz, rinv = rsqrtf(r2), rinv2 = rinv * rinv;
            const float s2 = r.sig * r.sig * rinv2, s6 = s2 * s2 * s2;
            acc += (double)(r.e4 * s6 * (s6 - 1.0f)) + (double)(r.qq * rinv);
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m);
        if (lane == 0) s_row[wave][0] = acc;
        __syncthreads();
        // the ligand's element: column L of a resident ligand's row, the column behind the groups of a guest's
        const uint32_t own = GUEST ? a.G : a.L;
        if (tid < lig.W) out[tid] = tid == own ? ((s_row[0][0] + s_row[1][0]) + s_row[2][0]) + s_row[3][0] : 0.0;
        if (FORCE && tid < count) {
            // thread ia: the force on ligand atom ia from the ligand's other atoms, ib in order, then the 1-4 records that name it
            const uint32_t ia = tid;
            const float4 pa = s_xyzq[ia];
            const float2 la = s_lj[ia];
            double f0 = 0.0, f1 = 0.0, f2 = 0.0;
            for (uint32_t ib = 0; ib < count; ++ib) {
                if (ib == ia || lig.cls[ib * count + ia] != 0) continue;      // (the map is symmetric: this row is read coalesced)
                const float4 pb = s_xyzq[ib];
                const float dx = pose_mimg(pa.x - pb.x, a.box[0], a.inv_box[0]), dy = pose_mimg(pa.y - pb.y, a.box[1], a.inv_box[1]),
                            dz = pose_mimg(pa.z - pb.z, a.box[2], a.inv_box[2]);
                float fx = 0.f, fy = 0.f, fz = 0.f, e1 = 0.f, e2 = 0.f;
                pair_eval<false, COUL, GEOM, false, true, false, false, true>(dx, dy, dz, pa.w, la.x, la.y, make_float4(0.f, 0.f, 0.f, pb.w), s_lj[ib], true, a.p,
                                                                            fx, fy, fz, e1, e2, nullptr, nullptr, nullptr, 0.f);
                f0 += (double)fx; f1 += (double)fy; f2 += (double)fz;
            }
            for (uint32_t k = 0; k < lig.n14; ++k) {
                const Pose14 r = lig.p14[k];
                if (r.a != ia && r.b != ia) continue;
                const float4 p0 = s_xyzq[r.a], p1 = s_xyzq[r.b];
                const float dx = pose_mimg(p0.x - p1.x, a.box[0], a.inv_box[0]), dy = pose_mimg(p0.y - p1.y, a.box[1], a.inv_box[1]),
                            dz = pose_mimg(p0.z - p1.z, a.box[2], a.inv_box[2]);
                const float r2 = dx * dx + dy * dy + dz * dz, rinv = rsqrtf(r2), rinv2 = rinv * rinv;
                const float s2 = r.sig * r.sig * rinv2, s6 = s2 * s2 * s2;
                // -dE/dr / r of E = e4 s6 (s6 - 1) + qq / r, on atom r.a; r.b takes minus it
                float fs = (6.0f * r.e4 * s6 * (2.0f * s6 - 1.0f) + r.qq * rinv) * rinv2;
                if (r.b == ia) fs = -fs;
                f0 += (double)(fs * dx); f1 += (double)(fs * dy); f2 += (double)(fs * dz);
            }
            fout[ia * 3u] = f0; fout[ia * 3u + 1u] = f1; fout[ia * 3u + 2u] = f2;
        }
        return;
    }
    if (FORCE) {
        for (uint32_t i = tid; i < 12u * fstride; i += 256u) s_f[i] = 0.0;
        __syncthreads();
    }
    double* facc = s_f + (size_t)wave * 3u * fstride;

    // ---- the environment ----
    const GridParams& g = a.g;
    const float r = a.r_cull;
    const bool all = !(r < 1.0e30f);
    int ix0 = 0, ix1 = g.ncx - 1, iy0 = 0, iy1 = g.ncy - 1;
    if (!all) {
        ix0 = mdx_col_of(g, 0, lo[0] - r); ix1 = mdx_col_of(g, 0, hi[0] + r);
        iy0 = mdx_col_of(g, 1, lo[1] - r); iy1 = mdx_col_of(g, 1, hi[1] + r);
        if (!g.per[0]) { ix0 = max(ix0, 0); ix1 = min(ix1, g.ncx - 1); }
        else if ((long long)ix1 - ix0 + 1 >= g.ncx) { ix0 = 0; ix1 = g.ncx - 1; }
        if (!g.per[1]) { iy0 = max(iy0, 0); iy1 = min(iy1, g.ncy - 1); }
        else if ((long long)iy1 - iy0 + 1 >= g.ncy) { iy0 = 0; iy1 = g.ncy - 1; }
    }
    const int nxr = max(ix1 - ix0 + 1, 0), nyr = max(iy1 - iy0 + 1, 0), ncr = nxr * nyr;
    const float r2cull = r * r;
    const float bcx = 0.5f * (lo[0] + hi[0]), bcy = 0.5f * (lo[1] + hi[1]), bcz = 0.5f * (lo[2] + hi[2]);
    const float bhx = 0.5f * (hi[0] - lo[0]), bhy = 0.5f * (hi[1] - lo[1]), bhz = 0.5f * (hi[2] - lo[2]);
    const int ii = lane & 7, jj = lane >> 3;
    const uint32_t nstrip = (count + 7u) >> 3;
    uint32_t cur_g = 0xFFFFFFFFu;
    double dacc = 0.0;
    double* row = s_row[wave];
    for (int base = 0; base < ncr; base += 64) {
        uint32_t t0 = 0, t1 = 0;
        const int q = base + lane;
        if (q < ncr) {
            int cx = ix0 + q / nyr, cy = iy0 + q % nyr;
            cx %= g.ncx; if (cx < 0) cx += g.ncx;       // (periodic axes; the others were clamped)
            cy %= g.ncy; if (cy < 0) cy += g.ncy;
            const uint32_t c = (uint32_t)(cx * g.ncy + cy);
            t0 = a.tile_start[c]; t1 = a.tile_start[c + 1];
        }
        const int nq = min(64, ncr - base);
        for (int l = 0; l < nq; ++l) {
            const uint32_t a0 = (uint32_t)__builtin_amdgcn_readlane((int)t0, l), a1 = (uint32_t)__builtin_amdgcn_readlane((int)t1, l);
            for (uint32_t t = a0 + ((unit + POSE_UNITS - (a0 % POSE_UNITS)) % POSE_UNITS); t < a1; t += POSE_UNITS) {
                // eight lanes, eight cluster boxes (as the rebuild left them: r_cull covers the drift since)
                bool near = false;
                if (lane < 8) {
                    const float4 l4 = a.cl_lo[t * MDX_CL_PER_TILE + lane], h4 = a.cl_hi[t * MDX_CL_PER_TILE + lane];
                    if (l4.w > 0.f) {
                        const float gx = fmaxf(0.f, fabsf(pose_mimg(0.5f * (l4.x + h4.x) - bcx, a.box[0], a.inv_box[0])) - (0.5f * (h4.x - l4.x) + bhx));
                        const float gy = fmaxf(0.f, fabsf(pose_mimg(0.5f * (l4.y + h4.y) - bcy, a.box[1], a.inv_box[1])) - (0.5f * (h4.y - l4.y) + bhy));
                        const float gz = fmaxf(0.f, fabsf(pose_mimg(0.5f * (l4.z + h4.z) - bcz, a.box[2], a.inv_box[2])) - (0.5f * (h4.z - l4.z) + bhz));
                        near = all || gx * gx + gy * gy + gz * gz <= r2cull;
                    }
                }
                uint32_t mask = (uint32_t)(__ballot(near) & 0xFFull);
                for (uint32_t turn = 0; mask; ++turn) {
                    const uint32_t ci = (uint32_t)__ffs((int)mask) - 1u;
                    mask &= mask - 1u;
                    if ((turn & 3u) != (uint32_t)wave) continue;
                    const uint32_t s = (t * MDX_CL_PER_TILE + ci) * MDX_CLUSTER + (uint32_t)ii;
                    const uint32_t o = a.orig_of[s];
                    const uint32_t ge = o == MDX_INVALID ? 0xFFFFFFFFu : (uint32_t)a.grp[a.gid[o]];
                    const bool live = o != MDX_INVALID && (GUEST || ge != a.L);      // (a guest skips no group: every resident atom is environment)
                    if (!__ballot(live)) continue;
                    if (__ballot(live && ge != cur_g && dacc != 0.0)) pose_fold(dacc, cur_g, row, lane);
                    if (live && dacc == 0.0) cur_g = ge;
                    const float4 pi = a.posq[s];
                    const float2 li = a.lj[s];
#pragma unroll 1
                    for (uint32_t k = 0; k < nstrip; ++k) {
                        const uint32_t ja = k * 8u + (uint32_t)jj;
                        const float4 pj = s_xyzq[ja];
                        const float2 lj = s_lj[ja];
                        const float dx = pose_mimg(pi.x - pj.x, a.box[0], a.inv_box[0]), dy = pose_mimg(pi.y - pj.y, a.box[1], a.inv_box[1]),
                                    dz = pose_mimg(pi.z - pj.z, a.box[2], a.inv_box[2]);
                        const float bias = (live && ja < count) ? 0.f : __builtin_nanf("");
                        float fx = 0.f, fy = 0.f, fz = 0.f, e1 = 0.f, e2 = 0.f;
                        pair_eval<true, COUL, GEOM, false, true, false, false, true>(dx, dy, dz, pi.w, li.x, li.y, make_float4(0.f, 0.f, 0.f, pj.w), lj, true, a.p,
                                                                                   fx, fy, fz, e1, e2, nullptr, nullptr, nullptr, bias);
                        dacc += (double)(e1 + e2);
                        if (FORCE) {
                            // fx is the force on the environment atom: the ligand atom takes minus it, summed over the eight ii
                            float lx = -fx, ly = -fy, lz = -fz;
                            lx += __shfl_xor(lx, 1); ly += __shfl_xor(ly, 1); lz += __shfl_xor(lz, 1);
                            lx += __shfl_xor(lx, 2); ly += __shfl_xor(ly, 2); lz += __shfl_xor(lz, 2);
                            lx += __shfl_xor(lx, 4); ly += __shfl_xor(ly, 4); lz += __shfl_xor(lz, 4);
                            if (ii == 0 && (lx != 0.f || ly != 0.f || lz != 0.f)) {
                                facc[ja] += (double)lx; facc[fstride + ja] += (double)ly; facc[2u * fstride + ja] += (double)lz;
                            }
                        }
                    }
                }
            }
        }
    }
    pose_fold(dacc, cur_g, row, lane);
    __syncthreads();
    if (tid < a.G) out[tid] = ((s_row[0][tid] + s_row[1][tid]) + s_row[2][tid]) + s_row[3][tid];
    if (GUEST && tid == 0u) out[a.G] = 0.0;
    if (FORCE)
        for (uint32_t i = tid; i < count * 3u; i += 256u) {
            const uint32_t ia = i / 3u, k = (i - ia * 3u) * fstride + ia;
            fout[i] = ((s_f[k] + s_f[3u * fstride + k]) + s_f[6u * fstride + k]) + s_f[9u * fstride + k];
        }
}

__global__ __launch_bounds__(256) void pose_sum_kernel(uint32_t n, uint32_t G, const double* __restrict__ slab, double* __restrict__ rows) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * G) return;
    const uint32_t pose = i / G, b = i - pose * G;
    rows[i] = pose_units_sum(slab + (size_t)pose * (POSE_UNITS + 1u) * G + b, G);
}

// forces[pose][atom] = the units' partial forces added in unit order (fp64, rounded once); rigid[pose] = (sum_i f_i, sum_i (x_i - c) x f_i),
// c the unweighted mean of the pose's coordinates as the caller gave them - fp64, atom order, of the unrounded forces.
template <bool GUEST>
__device__ __forceinline__ void pose_force_sum(const PoseRec* rec, uint32_t n, const float* __restrict__ poses, const double* __restrict__ fslab,
                                               float* __restrict__ forces, float* __restrict__ rigid) {
    __shared__ double s_x[MDX_POSE_MAX_ATOMS][3], s_v[MDX_POSE_MAX_ATOMS][3], s_c[3];
    const uint32_t tid = threadIdx.x, pose = blockIdx.x;
    const StepLigand<GUEST> lig(rec, n, pose);
    const uint32_t count = lig.count;
    if (tid < count) {
        const double* s = lig.units(fslab, tid);
        const size_t at = lig.at(tid);
        for (uint32_t c = 0; c < 3u; ++c) {
            const double v = pose_units_sum(s + c, (size_t)count * 3u);
            s_v[tid][c] = v; s_x[tid][c] = (double)poses[at + c];
            forces[at + c] = (float)v;
        }
    }
    __syncthreads();
    if (tid < 3u) {
        double c = 0.0;
        for (uint32_t i = 0; i < count; ++i) c += s_x[i][tid];
        s_c[tid] = c / (double)count;
    }
    __syncthreads();
    if (tid < 6u) rigid[(size_t)pose * 6u + tid] = (float)pose_rigid_component(tid, count, s_x, s_v, s_c);
}
// one body, two plain kernels (as the step kernels below)
__global__ __launch_bounds__(256) void pose_force_sum_kernel(uint32_t count, const float* __restrict__ poses, const double* __restrict__ fslab,
                                                             float* __restrict__ forces, float* __restrict__ rigid) {
    pose_force_sum<false>(nullptr, count, poses, fslab, forces, rigid);
}
__global__ __launch_bounds__(256) void guest_force_sum_kernel(const PoseRec* __restrict__ rec, const float* __restrict__ poses,
                                                              const double* __restrict__ fslab, float* __restrict__ forces, float* __restrict__ rigid) {
    pose_force_sum<true>(rec, 0u, poses, fslab, forces, rigid);
}

// The two step kernels: one body, two plain kernels under the names they had as separate copies.  (A kernel template
// pose_step_kernel<FLEX> gave the same instructions but left its instantiations behind the 24 pose_score_kernel ones in the code
// object; it measured 0.5 % slower in the flexible arm and no cause was found in the instructions - DESIGN.md 7h.)
__global__ __launch_bounds__(256) void pose_refine_step_kernel(StepArgs a) { pose_step<false>(a); }
__global__ __launch_bounds__(256) void pose_flex_step_kernel(StepArgs a) { pose_step<true>(a); }
__global__ __launch_bounds__(256) void guest_refine_step_kernel(StepArgs a) { pose_step<false, true>(a); }
// (guest_flex_step_kernel, pose_step<true, true>, stands in mdx_guest_flex.hip: see mdx_pose_step_dev.h)

template <int COUL>
static void launch_poses(mdx_handle* h, const PoseArgs& a, bool geom, uint32_t n, bool force, bool refine = false, bool guest = false) {
    const dim3 g(POSE_UNITS + 1u, n), b(256);
    if (guest && (force || refine)) {
        const size_t lds = sizeof(double) * 12u * (((a.count + 7u) >> 3) << 3);      // (a.count: the chunk's largest ligand)
        if (refine) {
            if (geom) hipLaunchKernelGGL((pose_score_kernel<COUL, true, true, true, true>), g, b, lds, h->stream, a);
            else hipLaunchKernelGGL((pose_score_kernel<COUL, false, true, true, true>), g, b, lds, h->stream, a);
        } else if (geom) hipLaunchKernelGGL((pose_score_kernel<COUL, true, true, false, true>), g, b, lds, h->stream, a);
        else hipLaunchKernelGGL((pose_score_kernel<COUL, false, true, false, true>), g, b, lds, h->stream, a);
    } else if (guest) {
        if (geom) hipLaunchKernelGGL((pose_score_kernel<COUL, true, false, false, true>), g, b, 0, h->stream, a);
        else hipLaunchKernelGGL((pose_score_kernel<COUL, false, false, false, true>), g, b, 0, h->stream, a);
    } else if (refine) {
        const size_t lds = sizeof(double) * 12u * (((a.count + 7u) >> 3) << 3);
        if (geom) hipLaunchKernelGGL((pose_score_kernel<COUL, true, true, true>), g, b, lds, h->stream, a);
        else hipLaunchKernelGGL((pose_score_kernel<COUL, false, true, true>), g, b, lds, h->stream, a);
    } else if (force) {
        const size_t lds = sizeof(double) * 12u * (((a.count + 7u) >> 3) << 3);
        if (geom) hipLaunchKernelGGL((pose_score_kernel<COUL, true, true>), g, b, lds, h->stream, a);
        else hipLaunchKernelGGL((pose_score_kernel<COUL, false, true>), g, b, lds, h->stream, a);
    } else if (geom) hipLaunchKernelGGL((pose_score_kernel<COUL, true, false>), g, b, 0, h->stream, a);
    else hipLaunchKernelGGL((pose_score_kernel<COUL, false, false>), g, b, 0, h->stream, a);
}

// the pose pass of n poses under the handle's Coulomb treatment
static void pose_launch(mdx_handle* h, const PoseArgs& a, int mode, bool geom, uint32_t n, bool force, bool refine, bool guest = false) {
    switch (mode) {
    case CM_SHIFTED: launch_poses<CM_SHIFTED>(h, a, geom, n, force, refine, guest); break;
    case CM_SOFT: launch_poses<CM_SOFT>(h, a, geom, n, force, refine, guest); break;
    case CM_RF: launch_poses<CM_RF>(h, a, geom, n, force, refine, guest); break;
    default: launch_poses<CM_EWALD>(h, a, geom, n, force, refine, guest); break;
    }
}

// A device buffer grows to `need` bytes: free, zero the capacity, hipMalloc, set the capacity - a failure leaves the capacity 0 and the
// pointer null, so the next call starts over.  Buffers that share a capacity: the followers grow on a zero capacity of their own
// behind the test of the shared one, the leader last with the shared one.
static int pose_grow(void** p, size_t& cap, size_t need) {
    if (cap >= need) return MDX_OK;
    if (*p) { (void)hipFree(*p); *p = nullptr; }
    cap = 0;
    HIP_TRY(hipMalloc(p, need));
    cap = need;
    return MDX_OK;
}

// The ligand's own pairs, once per (range, group map): who is excluded, who is a scaled 1-4 pair and with what parameters - from the
// handle's merged exclusion / 1-4 CSR and the 1-4 roles of the bonded gather.  Refuses a range that is tied to the outside.
static int pose_table(mdx_handle* h, const std::string& who, uint32_t first, uint32_t count) {
    DeviceState& d = h->d;
    hipStream_t st = h->stream;
    const uint32_t last = first + count;
    auto inside = [&](uint32_t i) { return i >= first && i < last; };
    for (size_t k = 0; k + 1 < h->h_bond_pairs.size(); k += 2)
        if (inside(h->h_bond_pairs[k]) != inside(h->h_bond_pairs[k + 1]))
            FAIL(MDX_EPARAM, who + ": a bond or constraint links the range to an atom outside it");
    for (const VSite& v : h->h_vsites) {
        const bool in = inside(v.site);
        if (inside(v.p0) != in || inside(v.p1) != in || inside(v.p2) != in)
            FAIL(MDX_EPARAM, who + ": a virtual site links the range to an atom outside it");
    }
    std::vector<uint32_t> off(count + 1), idx;
    HIP_TRY(hipMemcpyAsync(off.data(), d.excl_off + first, sizeof(uint32_t) * (count + 1), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    idx.resize(off[count] - off[0]);
    if (!idx.empty()) HIP_TRY(hipMemcpyAsync(idx.data(), d.excl_idx + off[0], sizeof(uint32_t) * idx.size(), hipMemcpyDeviceToHost, st));
    std::vector<uint32_t> roff(count + 1, 0);
    std::vector<RoleRec> recs;
    std::vector<float4> prm(h->n_prm_base);
    if (h->n_roles) {
        HIP_TRY(hipMemcpyAsync(roff.data(), d.role_off_o + first, sizeof(uint32_t) * (count + 1), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        recs.resize(roff[count] - roff[0]);
        if (!recs.empty()) HIP_TRY(hipMemcpyAsync(recs.data(), d.role_rec_o + roff[0], sizeof(RoleRec) * recs.size(), hipMemcpyDeviceToHost, st));
        if (!prm.empty()) HIP_TRY(hipMemcpyAsync(prm.data(), d.role_prm, sizeof(float4) * prm.size(), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<uint8_t> cls((size_t)count * count, 0);
    for (uint32_t i = 0; i < count; ++i)
        for (uint32_t k = off[i] - off[0]; k < off[i + 1] - off[0]; ++k) {
            if (!inside(idx[k])) FAIL(MDX_EPARAM, who + ": an exclusion or 1-4 pair links the range to an atom outside it");
            cls[(size_t)i * count + (idx[k] - first)] = 1;      // (the CSR is symmetric)
        }
    std::vector<Pose14> p14;
    const bool skip14 = (h->cfg.overrides & MDX_OVR_BONDED_DISABLED) != 0;
    for (uint32_t i = 0; i < count; ++i)
        for (uint32_t k = roff[i] - roff[0]; k < roff[i + 1] - roff[0] && k < recs.size(); ++k) {
            const RoleRec& r = recs[k];
            if ((r.meta & 0xFu) != ROLE_PAIR14 || ((r.meta >> 4) & 0xFu) != 0u) continue;
            if (!inside(r.p[0])) FAIL(MDX_EPARAM, who + ": an exclusion or 1-4 pair links the range to an atom outside it");
            const uint32_t b = r.p[0] - first, pi = r.meta >> 8;
            cls[(size_t)i * count + b] = 2; cls[(size_t)b * count + i] = 2;
            if (skip14 || pi >= prm.size()) continue;      // (bonded terms disabled: the matrix leaves the scaled pairs out too)
            p14.push_back(Pose14{i, b, prm[pi].x, prm[pi].y, prm[pi].z});
        }
    size_t c0 = 0, c1 = 0;      // (a new table: both buffers are made anew)
    MDX_TRY(pose_grow((void**)&d.ps_cls, c0, cls.size()));
    MDX_TRY(pose_grow(&d.ps_p14, c1, sizeof(Pose14) * std::max<size_t>(p14.size(), 1)));
    HIP_TRY(hipMemcpyAsync(d.ps_cls, cls.data(), cls.size(), hipMemcpyHostToDevice, st));
    if (!p14.empty()) HIP_TRY(hipMemcpyAsync(d.ps_p14, p14.data(), sizeof(Pose14) * p14.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    h->ps_n14 = (uint32_t)p14.size();
    return MDX_OK;
}

// What the three entry points share: the refusals, the intra-ligand table, the buffers of a chunk and the kernel's arguments
static int pose_setup(mdx_handle* h, const std::string& who, uint32_t first, uint32_t count, uint32_t n_poses, const float* poses,
                      uint32_t n_groups, bool force, PoseArgs& a, int& mode, bool& geom) {
    const uint32_t G = h->n_grp;
    if (!G) FAIL(MDX_EPARAM, "no energy groups are set (mdx_set_energy_groups)");
    if (n_groups != G) FAIL(MDX_EPARAM, "n_groups must be the number of groups (mdx_energy_group_count)");
    if (count == 0 || count > MDX_POSE_MAX_ATOMS) FAIL(MDX_EPARAM, who + ": count must be in 1..MDX_POSE_MAX_ATOMS (256)");
    if ((uint64_t)first + count > h->N) FAIL(MDX_EPARAM, "atom range out of bounds");
    if (h->dd || h->n_local != h->N) FAIL(MDX_EPARAM, who + " on a decomposed handle (single-device handles only)");
    if (h->alch_on) FAIL(MDX_EPARAM, who + " while an alchemical window is active");
    const bool fresh = !h->ps_valid || h->ps_first != first || h->ps_count != count || h->ps_epoch != h->grp_epoch;
    uint32_t L = h->ps_group;
    if (fresh) {
        L = h->grp_host[first];
        uint32_t members = 0;
        for (uint32_t i = 0; i < h->N; ++i) members += h->grp_host[i] == L ? 1u : 0u;
        bool whole = members == count;
        for (uint32_t i = first; i < first + count && whole; ++i) whole = h->grp_host[i] == L;
        if (!whole) FAIL(MDX_EPARAM, who + ": the range must be exactly one energy group");
    }
    const size_t per_pose = 3 * (size_t)count;
    for (size_t k = 0; k < per_pose * n_poses; ++k)
        if (!std::isfinite(poses[k])) FAIL(MDX_EPARAM, who + ": non-finite pose coordinate");
    HIP_TRY(hipSetDevice(h->device));
    if (fresh) {
        h->ps_valid = false;
        MDX_TRY(pose_table(h, who, first, count));
        h->ps_valid = true; h->ps_first = first; h->ps_count = count; h->ps_group = L; h->ps_epoch = h->grp_epoch;
    }
    MDX_TRY(mdx_ensure_ready(h));          // what the matrix would see: list, constraints and virtual sites of the current state
    DeviceState& d = h->d;
    // capacities in bytes, every buffer for a whole chunk; ps_rows shares ps_slab's, ps_fout and ps_rigid share ps_fslab's
    const size_t slab = sizeof(double) * (size_t)POSE_CHUNK * (POSE_UNITS + 1u) * G, fslab = sizeof(double) * (size_t)POSE_CHUNK * (POSE_UNITS + 1u) * per_pose;
    MDX_TRY(pose_grow((void**)&d.ps_stage, h->ps_cap_stage, sizeof(float) * per_pose * POSE_CHUNK));
    if (h->ps_cap_slab < slab) {
        size_t c = 0;
        h->ps_cap_slab = 0;
        MDX_TRY(pose_grow((void**)&d.ps_rows, c, sizeof(double) * (size_t)POSE_CHUNK * G));
        MDX_TRY(pose_grow((void**)&d.ps_slab, h->ps_cap_slab, slab));
    }
    if (force && h->ps_cap_fslab < fslab) {
        size_t c0 = 0, c1 = 0;
        h->ps_cap_fslab = 0;
        MDX_TRY(pose_grow((void**)&d.ps_fout, c0, sizeof(float) * (size_t)POSE_CHUNK * per_pose));
        MDX_TRY(pose_grow((void**)&d.ps_rigid, c1, sizeof(float) * (size_t)POSE_CHUNK * 6u));
        MDX_TRY(pose_grow((void**)&d.ps_fslab, h->ps_cap_fslab, fslab));
    }
    a = PoseArgs{};
    bool samecut = false;
    mdx_fill_nb_params(h, a.p, &mode, &geom, &samecut);
    a.g = h->grid;
    a.posq = d.posq; a.lj = d.lj; a.orig_of = d.orig_of; a.gid = d.gid; a.grp = d.grp; a.slot_of = d.slot_of;
    a.tile_start = d.tile_start; a.cl_lo = d.cl_lo; a.cl_hi = d.cl_hi;
    a.G = G; a.L = L; a.first = first; a.count = count;
    a.poses = d.ps_stage; a.slab = d.ps_slab; a.fslab = d.ps_fslab;
    a.r_cull = std::isfinite(h->r_list) ? h->r_list + 0.01f : INFINITY;
    for (int k = 0; k < 3; ++k) {
        a.box[k] = h->per[k] ? h->box_hi[k] - h->box_lo[k] : 0.f;
        a.inv_box[k] = h->per[k] ? 1.0f / a.box[k] : 0.f;
    }
    a.cls = d.ps_cls; a.p14 = (const Pose14*)d.ps_p14; a.n14 = h->ps_n14;
    return MDX_OK;
}

// mdx_score_poses (forces == nullptr: the energy flavour, rows only) and mdx_pose_forces (the force flavour; out / rigid may be null)
static int pose_run(mdx_handle* h, const std::string& who, uint32_t first, uint32_t count, uint32_t n_poses, const float* poses, float* out,
                    uint32_t n_groups, float* forces, float* rigid) {
    const bool force = forces != nullptr;
    PoseArgs a{};
    int mode = 0; bool geom = false;
    MDX_TRY(pose_setup(h, who, first, count, n_poses, poses, n_groups, force, a, mode, geom));
    DeviceState& d = h->d;
    hipStream_t st = h->stream;
    const uint32_t G = h->n_grp, chunk = std::min(n_poses, POSE_CHUNK);
    const size_t per_pose = 3 * (size_t)count;
    std::vector<double> rows((size_t)chunk * G);
    std::vector<float> res((size_t)n_poses * G), fres(force ? per_pose * n_poses : 0), rres(force ? 6u * (size_t)n_poses : 0);
    for (uint32_t p0 = 0; p0 < n_poses; p0 += POSE_CHUNK) {
        const uint32_t n = std::min(POSE_CHUNK, n_poses - p0);
        HIP_TRY(hipMemcpyAsync(d.ps_stage, poses + per_pose * p0, sizeof(float) * per_pose * n, hipMemcpyHostToDevice, st));
        mdx_prof_begin(h, 0);
        pose_launch(h, a, mode, geom, n, force, false);
        hipLaunchKernelGGL(pose_sum_kernel, dim3((n * G + 255u) / 256u), dim3(256), 0, st, n, G, d.ps_slab, d.ps_rows);
        if (force) hipLaunchKernelGGL(pose_force_sum_kernel, dim3(n), dim3(256), 0, st, count, d.ps_stage, d.ps_fslab, d.ps_fout, d.ps_rigid);
        mdx_prof_end(h);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(rows.data(), d.ps_rows, sizeof(double) * (size_t)n * G, hipMemcpyDeviceToHost, st));
        if (force) {
            HIP_TRY(hipMemcpyAsync(fres.data() + per_pose * p0, d.ps_fout, sizeof(float) * per_pose * n, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(rres.data() + 6u * (size_t)p0, d.ps_rigid, sizeof(float) * 6u * n, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t k = 0; force && k < per_pose * n; ++k)
            if (!std::isfinite(fres[per_pose * p0 + k])) FAIL(MDX_ENAN, who + ": non-finite force");
        for (size_t k = 0; force && k < 6u * (size_t)n; ++k)
            if (!std::isfinite(rres[6u * (size_t)p0 + k])) FAIL(MDX_ENAN, who + ": non-finite net force or torque");
        for (size_t k = 0; k < (size_t)n * G; ++k) {
            if (!std::isfinite(rows[k])) FAIL(MDX_ENAN, who + ": non-finite energy in a row");
            res[(size_t)p0 * G + k] = (float)rows[k];
        }
    }
    if (out) std::memcpy(out, res.data(), sizeof(float) * res.size());
    if (force) std::memcpy(forces, fres.data(), sizeof(float) * fres.size());
    if (force && rigid) std::memcpy(rigid, rres.data(), sizeof(float) * rres.size());
    return MDX_OK;
}

extern "C" int mdx_score_poses(mdx_handle* h, uint32_t first, uint32_t count, uint32_t n_poses, const float* poses, float* out,
                               uint32_t n_groups) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (n_poses == 0) return MDX_OK;
    if (!poses || !out) FAIL(MDX_EPARAM, "null argument");
    return pose_run(h, "mdx_score_poses", first, count, n_poses, poses, out, n_groups, nullptr, nullptr);
}

extern "C" int mdx_pose_forces(mdx_handle* h, uint32_t first, uint32_t count, uint32_t n_poses, const float* poses, float* rows_or_null,
                               uint32_t n_groups, float* forces, float* rigid_or_null) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (n_poses == 0) return MDX_OK;
    if (!poses || !forces) FAIL(MDX_EPARAM, "null argument");
    return pose_run(h, "mdx_pose_forces", first, count, n_poses, poses, rows_or_null, n_groups, forces, rigid_or_null);
}

// ---- mdx_refine_poses and mdx_refine_poses_flex: one loop, the rigid and the flexible state record ---------------------------------------
// (StepLayout - the refinement's device block of a chunk - stands in mdx_pose_plan.h)

// The table of one (range, torsion list, flags): the torsions with their moving-set masks, the ligand's dihedral terms in the system's
// list order, and per ligand atom the (term, role) entries that name it, in list order too - the atom-owned gather.
struct FlexTable {
    size_t tor, dih, aoff, aent, end;
    FlexTable(uint32_t count, uint32_t n_terms) {
        tor = 0;
        dih = sizeof(mdx_fx_torsion) * MDX_FX_MAX_TORSIONS;
        aoff = dih + sizeof(mdx_fx_dihedral) * n_terms;
        aent = aoff + sizeof(uint32_t) * (count + 1u);
        end = aent + sizeof(uint32_t) * 4u * (size_t)n_terms;
    }
};

// the options of a refinement: the refusals, then the stepper's options with the defaults filled in (the rigid entry point has neither
// tors_tol nor flags: it passes 0 for both)
static int refine_opts_check(const std::string& who, const mdx_flex_opts& opts, mdx_fx_opts& o) {
    if (opts.max_evals == 0 || opts.max_evals > MDX_REFINE_MAX_EVALS_CAP) FAIL(MDX_EPARAM, who + ": max_evals must be in 1..MDX_REFINE_MAX_EVALS_CAP (4096)");
    for (float v : {opts.f_tol, opts.tau_tol, opts.tors_tol, opts.h_start, opts.h_max})
        if (!std::isfinite(v) || v < 0.f) FAIL(MDX_EPARAM, who + ": a tolerance or step length is negative or not finite");
    if (opts.flags & ~MDX_FLEX_DIHEDRALS) FAIL(MDX_EPARAM, who + ": unknown flag bits");
    o = mdx_fx_opts{{(double)opts.f_tol, (double)opts.tau_tol, opts.h_start > 0.f ? (double)opts.h_start : 0.01,
                     opts.h_max > 0.f ? (double)opts.h_max : 0.2}, (double)opts.tors_tol};
    if (o.rf.h_start > o.rf.h_max) FAIL(MDX_EPARAM, who + ": h_start exceeds h_max");
    return MDX_OK;
}

// the step kernel's arguments for a chunk laid out by `lay` at blk, behind the force pass of `a` (it evaluates the staged trial a.poses
// into a.slab and a.fslab; W: the width of its rows); flex: with the torsion table of flex_table (T torsions, n_terms terms)
static StepArgs step_args(mdx_handle* h, const PoseArgs& a, unsigned char* blk, uint32_t count, uint32_t W, bool flex, uint32_t T,
                          uint32_t n_terms, const StepLayout& lay, const mdx_fx_opts& o) {
    DeviceState& d = h->d;
    StepArgs r{};
    r.count = count; r.G = W; r.T = T; r.n_terms = n_terms; r.stage = const_cast<float*>(a.poses); r.slab = a.slab; r.fslab = a.fslab;
    r.frozen = (uint32_t*)(blk + lay.frozen); r.st = blk + lay.state;
    r.y = (float*)(blk + lay.y); r.row = (float*)(blk + lay.row); r.rigid = (float*)(blk + lay.rigid); r.x0 = (float*)(blk + lay.x0);
    if (flex) {
        const FlexTable tab(count, n_terms);
        const unsigned char* tb = (const unsigned char*)d.ps_flex_tab;
        r.eterm = (double*)(blk + lay.eterm);
        r.tor = (const mdx_fx_torsion*)(tb + tab.tor); r.dih = (const mdx_fx_dihedral*)(tb + tab.dih);
        r.aoff = (const uint32_t*)(tb + tab.aoff); r.aent = (const uint32_t*)(tb + tab.aent);
    }
    for (int k = 0; k < 3; ++k) r.box[k] = (double)a.box[k];
    r.o = o;
    return r;
}

// one evaluation of a chunk: the REFINE force pass, then the step kernel (guests: r.rec is set)
template <bool FLEX>
static void step_evaluate(mdx_handle* h, const PoseArgs& a, int mode, bool geom, uint32_t n, const StepArgs& r) {
    pose_launch(h, a, mode, geom, n, true, true, r.rec != nullptr);
    if (r.rec && FLEX) mdx_launch_guest_flex_step(h->stream, n, r);
    else if (r.rec) hipLaunchKernelGGL(guest_refine_step_kernel, dim3(n), dim3(256), 0, h->stream, r);
    else if (FLEX) hipLaunchKernelGGL(pose_flex_step_kernel, dim3(n), dim3(256), 0, h->stream, r);
    else hipLaunchKernelGGL(pose_refine_step_kernel, dim3(n), dim3(256), 0, h->stream, r);
}

// where a refinement's results go; the rigid entry point has no dih / tgrad, and its xform ends with t
struct RefineOut { float* poses; float* rows; float* rigid; float* xform; float* dih; float* tgrad; uint32_t* status; uint32_t* evals; };

// one pose's record as it came back: status, evaluations, (q, t) and - flexible - theta behind them, E_dih and g
static void refine_unpack(const mdx_rf_state& s, uint32_t* status, uint32_t* evals, float* x) {
    *status = s.frozen ? s.status : MDX_REFINE_MAX_EVALS;
    *evals = s.evals;
    for (int c = 0; c < 4; ++c) x[c] = (float)s.q[c];
    for (int c = 0; c < 3; ++c) x[4 + c] = (float)s.t[c];
}
static void refine_unpack(const mdx_fx_state& s, uint32_t T, uint32_t* status, uint32_t* evals, float* x, float* dih, float* tgrad) {
    refine_unpack(s.rf, status, evals, x);
    for (uint32_t c = 0; c < T; ++c) { x[7u + c] = (float)s.th[c]; tgrad[c] = (float)s.g[c]; }
    *dih = s.edih;
}

// The loop of both refinements over the chunks of a batch, State = mdx_rf_state (T = n_terms = 0) or mdx_fx_state: upload, zero the
// frozen words and records, max_evals x (force pass, step kernel), one read-back, one wait; the outputs are written once all chunks
// have run.  pose_setup (and, flexible, flex_table) have passed.
template <class State>
static int refine_chunks(mdx_handle* h, PoseArgs& a, int mode, bool geom, uint32_t count, uint32_t n_poses, const float* poses, uint32_t T,
                         uint32_t n_terms, uint32_t max_evals, const mdx_fx_opts& o, const RefineOut& out) {
    constexpr bool FLEX = std::is_same<State, mdx_fx_state>::value;
    DeviceState& d = h->d;
    hipStream_t st = h->stream;
    const uint32_t G = h->n_grp, X = 7u + T;
    const size_t per_pose = 3 * (size_t)count;
    MDX_TRY(pose_grow(&d.ps_flex, h->ps_cap_flex, StepLayout(POSE_CHUNK, per_pose * POSE_CHUNK, G, sizeof(State), n_terms).end));
    std::vector<float> yres(per_pose * n_poses), rres((size_t)n_poses * G), gres(6u * (size_t)n_poses), xres((size_t)X * n_poses),
        dres(FLEX ? n_poses : 0u), tres((size_t)T * n_poses);
    std::vector<uint32_t> sres(n_poses), eres(n_poses);
    std::vector<unsigned char> back;
    for (uint32_t p0 = 0; p0 < n_poses; p0 += POSE_CHUNK) {
        const uint32_t n = std::min(POSE_CHUNK, n_poses - p0);
        const StepLayout lay(n, per_pose * n, G, sizeof(State), n_terms);
        unsigned char* blk = (unsigned char*)d.ps_flex;
        const StepArgs r = step_args(h, a, blk, count, G, FLEX, T, n_terms, lay, o);
        a.frozen = r.frozen;
        HIP_TRY(hipMemcpyAsync(d.ps_stage, poses + per_pose * p0, sizeof(float) * per_pose * n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(blk, 0, lay.y, st));
        mdx_prof_begin(h, 0);
        for (uint32_t k = 0; k < max_evals; ++k) step_evaluate<FLEX>(h, a, mode, geom, n, r);
        mdx_prof_end(h);
        HIP_TRY(hipGetLastError());
        back.resize(lay.x0 - lay.state);
        HIP_TRY(hipMemcpyAsync(back.data(), blk + lay.state, back.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const unsigned char* b0 = back.data() - lay.state;
        std::memcpy(yres.data() + per_pose * p0, b0 + lay.y, sizeof(float) * per_pose * n);
        std::memcpy(rres.data() + (size_t)p0 * G, b0 + lay.row, sizeof(float) * (size_t)G * n);
        std::memcpy(gres.data() + 6u * (size_t)p0, b0 + lay.rigid, sizeof(float) * 6u * n);
        for (uint32_t k = 0; k < n; ++k) {
            State s;
            std::memcpy(&s, b0 + lay.state + sizeof(State) * k, sizeof(s));
            const size_t p = p0 + k;
            if constexpr (FLEX) refine_unpack(s, T, &sres[p], &eres[p], xres.data() + X * p, &dres[p], tres.data() + (size_t)T * p);
            else refine_unpack(s, &sres[p], &eres[p], xres.data() + X * p);
        }
    }
    std::memcpy(out.poses, yres.data(), sizeof(float) * yres.size());
    if (out.rows) std::memcpy(out.rows, rres.data(), sizeof(float) * rres.size());
    if (out.rigid) std::memcpy(out.rigid, gres.data(), sizeof(float) * gres.size());
    if (out.xform) std::memcpy(out.xform, xres.data(), sizeof(float) * xres.size());
    if (out.dih) std::memcpy(out.dih, dres.data(), sizeof(float) * dres.size());
    if (out.tgrad && T) std::memcpy(out.tgrad, tres.data(), sizeof(float) * tres.size());
    if (out.status) std::memcpy(out.status, sres.data(), sizeof(uint32_t) * sres.size());
    if (out.evals) std::memcpy(out.evals, eres.data(), sizeof(uint32_t) * eres.size());
    return MDX_OK;
}

extern "C" int mdx_refine_poses(mdx_handle* h, uint32_t first, uint32_t count, uint32_t n_poses, const float* poses,
                                const mdx_refine_opts* opts, float* poses_out, float* rows_out_or_null, uint32_t n_groups,
                                float* rigid_out_or_null, float* xform_out_or_null, uint32_t* status_out_or_null,
                                uint32_t* evals_out_or_null) {
    const std::string who = "mdx_refine_poses";
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (n_poses == 0) return MDX_OK;
    if (!poses || !poses_out || !opts) FAIL(MDX_EPARAM, "null argument");
    mdx_fx_opts o{};
    MDX_TRY(refine_opts_check(who, mdx_flex_opts{opts->max_evals, opts->f_tol, opts->tau_tol, 0.f, opts->h_start, opts->h_max, 0u}, o));
    PoseArgs a{};
    int mode = 0; bool geom = false;
    MDX_TRY(pose_setup(h, who, first, count, n_poses, poses, n_groups, true, a, mode, geom));
    return refine_chunks<mdx_rf_state>(h, a, mode, geom, count, n_poses, poses, 0u, 0u, opts->max_evals, o,
                                       RefineOut{poses_out, rows_out_or_null, rigid_out_or_null, xform_out_or_null, nullptr, nullptr,
                                                 status_out_or_null, evals_out_or_null});
}

// ---- the flexible refinement's own: the torsion list and its table -----------------------------------------------------------------------

// The moving sides of a torsion list over a ligand-local bond graph, with the refusals in words - what does not depend on where the
// graph comes from (the handle's topology: flex_graph; the caller's: guest_check).  tor: [MDX_FX_MAX_TORSIONS]
static int flex_sides(const std::string& who, uint32_t count, uint32_t n_bonds, const uint32_t* bonds, uint32_t root, uint32_t n_torsions,
                      const uint32_t* tb, std::vector<mdx_fx_torsion>& tor) {
    tor.assign(MDX_FX_MAX_TORSIONS, mdx_fx_torsion{});
    uint32_t bad = 0;
    const int rc = fx_moving_sides(count, n_bonds, bonds, root, n_torsions, tb, tor.data(), &bad);
    const std::string t = who + ": torsion " + std::to_string(bad);
    switch (rc) {
    case MDX_FX_OK: return MDX_OK;
    case MDX_FX_E_ROOT: FAIL(MDX_EPARAM, who + ": root must be an atom of the range (root < count)");
    case MDX_FX_E_INDEX: FAIL(MDX_EPARAM, t + " names an atom index >= count");
    case MDX_FX_E_SELF: FAIL(MDX_EPARAM, t + " names the same atom twice");
    case MDX_FX_E_NOT_BONDED: FAIL(MDX_EPARAM, t + ": the two atoms are not bonded");
    case MDX_FX_E_TWICE: FAIL(MDX_EPARAM, t + ": the bond is listed twice");
    case MDX_FX_E_RING: FAIL(MDX_EPARAM, t + ": removing the bond leaves its ends connected (a ring bond)");
    case MDX_FX_E_LEAF: FAIL(MDX_EPARAM, t + ": one side of the bond is a single atom (a leaf bond: the torsion moves nothing)");
    default: FAIL(MDX_EPARAM, who + ": the bond graph of the range is not connected");
    }
}

// What can be refused of a torsion list on the host's copy of the topology alone: the range's bonds, the moving sides
static int flex_graph(mdx_handle* h, const std::string& who, uint32_t first, uint32_t count, uint32_t root, uint32_t n_torsions,
                      const uint32_t* tb, std::vector<mdx_fx_torsion>& tor) {
    std::vector<uint32_t> bonds;
    for (size_t k = 0; k + 1 < h->h_bond_pairs.size(); k += 2) {
        const uint32_t p = h->h_bond_pairs[k], q = h->h_bond_pairs[k + 1];
        if (p >= first && p - first < count && q >= first && q - first < count) { bonds.push_back(p - first); bonds.push_back(q - first); }
    }
    return flex_sides(who, count, (uint32_t)(bonds.size() / 2), bonds.data(), root, n_torsions, tb, tor);
}

// the atom-owned gather of a ligand's terms: aoff [count + 1], aent [4 n_terms] = per atom the (term << 2 | role) words that name it, in
// list order
static void flex_gather(uint32_t count, const std::vector<mdx_fx_dihedral>& dih, std::vector<uint32_t>& aoff, std::vector<uint32_t>& aent) {
    const uint32_t n_terms = (uint32_t)dih.size();
    aoff.assign(count + 1u, 0u); aent.assign(4u * (size_t)n_terms, 0u);
    for (const mdx_fx_dihedral& t : dih)
        for (int r = 0; r < 4; ++r) aoff[t.at[r] + 1u]++;
    for (uint32_t i = 0; i < count; ++i) aoff[i + 1u] += aoff[i];
    std::vector<uint32_t> cur(aoff.begin(), aoff.end() - 1);
    for (uint32_t k = 0; k < n_terms; ++k)
        for (uint32_t r = 0; r < 4u; ++r) aent[cur[dih[k].at[r]]++] = (k << 2) | r;
}

// The table on the device, once per (range, group epoch, root, torsion list, flags)
static int flex_table(mdx_handle* h, const std::string& who, uint32_t first, uint32_t count, uint32_t root, uint32_t n_torsions,
                      const uint32_t* tb, uint32_t flags, const std::vector<mdx_fx_torsion>& tor) {
    DeviceState& d = h->d;
    const std::vector<uint32_t> key(tb, tb + 2 * (size_t)n_torsions);
    if (h->fx_valid && h->fx_first == first && h->fx_count == count && h->fx_epoch == h->grp_epoch && h->fx_root == root &&
        h->fx_flags == flags && h->fx_bonds == key) return MDX_OK;
    h->fx_valid = false;
    std::vector<mdx_fx_dihedral> dih;
    const bool on = (flags & MDX_FLEX_DIHEDRALS) != 0u && (h->cfg.overrides & MDX_OVR_BONDED_DISABLED) == 0u;
    for (size_t k = 0; on && k < h->h_dih_v.size(); ++k) {
        const uint32_t* at = h->h_dih_idx.data() + 4 * k;
        uint32_t in = 0;
        for (int r = 0; r < 4; ++r) in += (at[r] >= first && at[r] - first < count) ? 1u : 0u;
        if (in == 0u) continue;
        if (in != 4u) FAIL(MDX_EPARAM, who + ": a dihedral term links the range to an atom outside it");
        dih.push_back(mdx_fx_dihedral{{at[0] - first, at[1] - first, at[2] - first, at[3] - first}, (double)h->h_dih_v[k],
                                      (double)h->h_dih_phase[k], (double)h->h_dih_n[k]});
    }
    const uint32_t n_terms = (uint32_t)dih.size();
    if (n_terms >= (1u << 30)) FAIL(MDX_EPARAM, who + ": too many dihedral terms in the range");
    std::vector<uint32_t> aoff, aent;
    flex_gather(count, dih, aoff, aent);
    const FlexTable lay(count, n_terms);
    std::vector<unsigned char> img(lay.end, 0);
    std::memcpy(img.data() + lay.tor, tor.data(), sizeof(mdx_fx_torsion) * MDX_FX_MAX_TORSIONS);
    if (n_terms) std::memcpy(img.data() + lay.dih, dih.data(), sizeof(mdx_fx_dihedral) * n_terms);
    std::memcpy(img.data() + lay.aoff, aoff.data(), sizeof(uint32_t) * aoff.size());
    if (n_terms) std::memcpy(img.data() + lay.aent, aent.data(), sizeof(uint32_t) * aent.size());
    MDX_TRY(pose_grow(&d.ps_flex_tab, h->ps_cap_flex_tab, lay.end));
    HIP_TRY(hipMemcpyAsync(d.ps_flex_tab, img.data(), lay.end, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->fx_valid = true; h->fx_first = first; h->fx_count = count; h->fx_epoch = h->grp_epoch; h->fx_root = root; h->fx_flags = flags;
    h->fx_bonds = key; h->fx_terms = n_terms;
    return MDX_OK;
}

// What mdx_refine_poses_flex and mdx_search_poses share ahead of their loops: the checks of the torsion list and the options, the
// refusals and buffers of pose_setup, the table
static int flex_begin(mdx_handle* h, const std::string& who, uint32_t first, uint32_t count, uint32_t n_poses, const float* poses, uint32_t root,
                      uint32_t n_torsions, const uint32_t* torsion_bonds, const mdx_flex_opts* opts, uint32_t n_groups, PoseArgs& a, int& mode,
                      bool& geom, mdx_fx_opts& o) {
    if (n_torsions > MDX_POSE_MAX_TORSIONS) FAIL(MDX_EPARAM, who + ": n_torsions exceeds MDX_POSE_MAX_TORSIONS (32)");
    if (n_torsions && !torsion_bonds) FAIL(MDX_EPARAM, who + ": null torsion_bonds with n_torsions > 0");
    MDX_TRY(refine_opts_check(who, *opts, o));
    // the torsion list against the host's copy of the bonds - once the range itself has passed the checks pose_setup opens with
    if (count == 0 || count > MDX_POSE_MAX_ATOMS) FAIL(MDX_EPARAM, who + ": count must be in 1..MDX_POSE_MAX_ATOMS (256)");
    if ((uint64_t)first + count > h->N) FAIL(MDX_EPARAM, "atom range out of bounds");
    std::vector<mdx_fx_torsion> tor;
    MDX_TRY(flex_graph(h, who, first, count, root, n_torsions, torsion_bonds, tor));
    MDX_TRY(pose_setup(h, who, first, count, n_poses, poses, n_groups, true, a, mode, geom));
    return flex_table(h, who, first, count, root, n_torsions, torsion_bonds, opts->flags, tor);
}

extern "C" int mdx_refine_poses_flex(mdx_handle* h, uint32_t first, uint32_t count, uint32_t n_poses, const float* poses, uint32_t root,
                                     uint32_t n_torsions, const uint32_t* torsion_bonds, const mdx_flex_opts* opts, float* poses_out,
                                     float* rows_out_or_null, uint32_t n_groups, float* rigid_out_or_null, float* xform_out_or_null,
                                     float* dih_out_or_null, float* tgrad_out_or_null, uint32_t* status_out_or_null,
                                     uint32_t* evals_out_or_null) {
    const std::string who = "mdx_refine_poses_flex";
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (n_poses == 0) return MDX_OK;
    if (!poses || !poses_out || !opts) FAIL(MDX_EPARAM, "null argument");
    PoseArgs a{};
    int mode = 0; bool geom = false;
    mdx_fx_opts o{};
    MDX_TRY(flex_begin(h, who, first, count, n_poses, poses, root, n_torsions, torsion_bonds, opts, n_groups, a, mode, geom, o));
    return refine_chunks<mdx_fx_state>(h, a, mode, geom, count, n_poses, poses, n_torsions, h->fx_terms, opts->max_evals, o,
                                       RefineOut{poses_out, rows_out_or_null, rigid_out_or_null, xform_out_or_null, dih_out_or_null,
                                                 tgrad_out_or_null, status_out_or_null, evals_out_or_null});
}

// ---- mdx_search_poses: an iterated local search per walker around the loop above (mdx_search_step.h) ------------------------------------
// (SearchLayout - the search block of a chunk - stands in mdx_pose_plan.h; SearchArgs and the body of the search kernels, pose_search,
// in mdx_pose_search_dev.h: one body, two plain kernels - this one and guest_search_kernel of mdx_guest_search.hip)
__global__ __launch_bounds__(256) void pose_search_kernel(SearchArgs a, uint32_t r) { pose_search<false>(a, r); }

// The search kernel's arguments for a chunk whose refinement runs with r and whose search block lies at sb, laid out by sl (W: the width
// of a row; resident: count and T of the call, guests: 0 - the records say)
static SearchArgs search_args(const StepArgs& r, unsigned char* sb, const SearchLayout& sl, uint32_t count, uint32_t W, uint32_t T, const mdx_sr_opts& so) {
    SearchArgs s{};
    s.count = count; s.G = W; s.T = T; s.stage = r.stage; s.frozen = r.frozen; s.st = (mdx_fx_state*)r.st; s.y = r.y; s.row = r.row; s.rigid = r.rigid;
    s.tor = r.tor; s.streams = (const uint64_t*)(sb + sl.streams); s.rec = (mdx_sr_record*)(sb + sl.rec);
    s.cur_y = (float*)(sb + sl.cur_y); s.best_y = (float*)(sb + sl.best_y); s.best_row = (float*)(sb + sl.best_row);
    s.best_rigid = (float*)(sb + sl.best_rigid);
    s.o = so;
    return s;
}

// What a search returns per walker beside coordinates and rows, on the host until every chunk has run: take() reads the n records of a
// chunk as they came back (walkers p0 ..), write() fills the caller's optional outputs
struct SearchOut {
    std::vector<double> score; std::vector<float> dih; std::vector<uint32_t> round, stats;
    explicit SearchOut(size_t n) : score(n), dih(n), round(n), stats(4u * n) {}
    void take(const unsigned char* recs, uint32_t n, size_t p0) {
        for (uint32_t k = 0; k < n; ++k) {
            mdx_sr_record rec;
            std::memcpy(&rec, recs + sizeof(mdx_sr_record) * k, sizeof(rec));
            score[p0 + k] = rec.S_best; dih[p0 + k] = rec.edih_best; round[p0 + k] = rec.best_round;
            uint32_t* c = stats.data() + 4u * (p0 + k);
            c[0] = rec.accepted; c[1] = rec.uphill; c[2] = rec.nonfinite; c[3] = rec.evals;
        }
    }
    void write(double* score_out, float* dih_out, uint32_t* round_out, uint32_t* stats_out) const {
        if (score_out) std::memcpy(score_out, score.data(), sizeof(double) * score.size());
        if (dih_out) std::memcpy(dih_out, dih.data(), sizeof(float) * dih.size());
        if (round_out) std::memcpy(round_out, round.data(), sizeof(uint32_t) * round.size());
        if (stats_out) std::memcpy(stats_out, stats.data(), sizeof(uint32_t) * stats.size());
    }
};

extern "C" int mdx_search_poses(mdx_handle* h, uint32_t first, uint32_t count, uint32_t n_walkers, const float* starts,
                                const uint64_t* streams_or_null, uint32_t root, uint32_t n_torsions, const uint32_t* torsion_bonds,
                                const mdx_search_opts* opts, float* best_out, float* best_rows_out_or_null, uint32_t n_groups,
                                double* best_score_out_or_null, float* best_dih_out_or_null, uint32_t* best_round_out_or_null,
                                uint32_t* stats_out_or_null) {
    const std::string who = "mdx_search_poses";
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (n_walkers == 0) return MDX_OK;
    if (!starts || !best_out || !opts) FAIL(MDX_EPARAM, "null argument");
    if (opts->n_rounds == 0 || opts->n_rounds > MDX_SEARCH_MAX_ROUNDS) FAIL(MDX_EPARAM, who + ": n_rounds must be in 1..MDX_SEARCH_MAX_ROUNDS (1024)");
    if ((uint64_t)opts->n_rounds * opts->refine.max_evals > 65536u) FAIL(MDX_EPARAM, who + ": n_rounds x max_evals exceeds 65536");
    for (float v : {opts->trans_amp, opts->rot_amp, opts->tors_amp, opts->kT})
        if (!std::isfinite(v) || v < 0.f) FAIL(MDX_EPARAM, who + ": an amplitude or kT is negative or not finite");
    if (opts->tors_amp > 3.14159265358979323846f) FAIL(MDX_EPARAM, who + ": tors_amp exceeds pi");      // (the fp32 nearest to pi passes)
    mdx_sr_opts so{(double)opts->trans_amp, (double)opts->rot_amp, (double)opts->tors_amp, (double)opts->kT, opts->seed, opts->n_rounds, 0u};
    if (n_torsions <= MDX_POSE_MAX_TORSIONS && sr_choices(so, n_torsions) == 0u)
        FAIL(MDX_EPARAM, who + ": no move is enabled (every amplitude is 0, or only tors_amp with no torsion)");
    PoseArgs a{};
    int mode = 0; bool geom = false;
    mdx_fx_opts o{};
    MDX_TRY(flex_begin(h, who, first, count, n_walkers, starts, root, n_torsions, torsion_bonds, &opts->refine, n_groups, a, mode, geom, o));
    DeviceState& d = h->d;
    hipStream_t st = h->stream;
    const uint32_t G = h->n_grp, T = n_torsions, n_terms = h->fx_terms;
    const size_t per_pose = 3 * (size_t)count;
    MDX_TRY(pose_grow(&d.ps_flex, h->ps_cap_flex, StepLayout(POSE_CHUNK, per_pose * POSE_CHUNK, G, sizeof(mdx_fx_state), n_terms).end));
    MDX_TRY(pose_grow(&d.ps_search, h->ps_cap_search, SearchLayout(POSE_CHUNK, per_pose, G).end));
    std::vector<float> yres(per_pose * n_walkers), rres((size_t)n_walkers * G);
    SearchOut res(n_walkers);
    std::vector<uint64_t> ids(std::min(n_walkers, POSE_CHUNK));
    std::vector<unsigned char> back;
    for (uint32_t p0 = 0; p0 < n_walkers; p0 += POSE_CHUNK) {
        const uint32_t n = std::min(POSE_CHUNK, n_walkers - p0);
        const StepLayout lay(n, per_pose * n, G, sizeof(mdx_fx_state), n_terms);
        const SearchLayout sl(n, per_pose, G);
        unsigned char* sb = (unsigned char*)d.ps_search;
        const StepArgs r = step_args(h, a, (unsigned char*)d.ps_flex, count, G, true, T, n_terms, lay, o);
        a.frozen = r.frozen;
        const SearchArgs s = search_args(r, sb, sl, count, G, T, so);      // (r.stage is ps_stage: the force pass reads what the kernels stage)
        for (uint32_t k = 0; k < n; ++k) ids[k] = streams_or_null ? streams_or_null[p0 + k] : (uint64_t)(p0 + k);
        HIP_TRY(hipMemcpyAsync(d.ps_stage, starts + per_pose * p0, sizeof(float) * per_pose * n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(sb + sl.streams, ids.data(), sizeof(uint64_t) * n, hipMemcpyHostToDevice, st));
        mdx_prof_begin(h, 0);
        for (uint32_t rd = 0; rd < opts->n_rounds; ++rd) {
            hipLaunchKernelGGL(pose_search_kernel, dim3(n), dim3(256), 0, st, s, rd);
            for (uint32_t k = 0; k < opts->refine.max_evals; ++k) step_evaluate<true>(h, a, mode, geom, n, r);
        }
        hipLaunchKernelGGL(pose_search_kernel, dim3(n), dim3(256), 0, st, s, opts->n_rounds);
        mdx_prof_end(h);
        HIP_TRY(hipGetLastError());
        back.resize(sl.cur_y - sl.rec);
        HIP_TRY(hipMemcpyAsync(back.data(), sb + sl.rec, back.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));      // (ids is free again: the upload above has completed)
        const unsigned char* b0 = back.data();
        std::memcpy(yres.data() + per_pose * p0, b0 + sl.best_y, sizeof(float) * per_pose * n);
        std::memcpy(rres.data() + (size_t)p0 * G, b0 + sl.best_row, sizeof(float) * (size_t)G * n);
        res.take(b0 + sl.rec, n, p0);
    }
    std::memcpy(best_out, yres.data(), sizeof(float) * yres.size());
    if (best_rows_out_or_null) std::memcpy(best_rows_out_or_null, rres.data(), sizeof(float) * rres.size());
    res.write(best_score_out_or_null, best_dih_out_or_null, best_round_out_or_null, stats_out_or_null);
    return MDX_OK;
}

// ---- guest ligands: mdx_screen_ligands, mdx_guest_forces, mdx_refine_guests -------------------------------------------------------------------
// A guest is described by the caller and never enters the handle: its charge / LJ rows, class map and 1-4 records are staged per chunk
// beside its poses (GuestLayout), a PoseRec per pose says where, and the GUEST instantiations of pose_score_kernel read them where the
// resident ones go through slot_of and the handle's table.  Rows are n_groups + 1 wide: every resident group, then the ligand's own
// pairs.  Nothing of the handle's state or of the resident-pose cache (ps_*) is written: a chunk's whole block - staged tables, slabs,
// sums and, for a refinement, its StepLayout - lies in gs_blk.  The three entry points share the checks (guest_check), the plan
// (mdx_pose_plan.h), the kernel arguments (guest_ready) and the staging of a chunk (guest_stage).
struct GuestBest { double score; uint32_t pose, pad; };      // smallest row sum of a ligand so far and its ligand-local pose

// The best pose of every ligand that has poses in the chunk: the thread of the first such pose walks the ligand's run in pose order
// (lig_of[p] = (ligand, ligand-local pose); a ligand's poses are consecutive), S = the fp32-rounded row added in column order in fp64 -
// what a host gets from the returned rows - and a strictly smaller S replaces the carried one: the lowest index wins a tie, also
// across chunks.  One writer per ligand, no atomics.  Row: double (the summed rows of mdx_screen_ligands) or float (the accepted rows
// of a refinement; st: its state records - a pose that ended MDX_REFINE_NONFINITE is passed over whatever its row holds; the flexible
// refinement's records add their accepted E_dih behind the columns); or none at all and st the walkers' search records
// (mdx_search_guests): S is the record's S_best, read as it is.
__device__ __forceinline__ const mdx_rf_state& rf_of(const mdx_rf_state& s) { return s; }
__device__ __forceinline__ const mdx_rf_state& rf_of(const mdx_fx_state& s) { return s.rf; }
template <class Row, class State>
__device__ __forceinline__ void guest_best(uint32_t n, uint32_t W, const Row* __restrict__ rows, const uint2* __restrict__ lig_of,
                                           const State* __restrict__ st, GuestBest* __restrict__ best) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t m = lig_of[p].x;
    if (p > 0u && lig_of[p - 1u].x == m) return;
    GuestBest b = best[m];
    for (uint32_t k = p; k < n && lig_of[k].x == m; ++k) {
        double S = 0.0;
        if constexpr (std::is_same<State, mdx_sr_record>::value) S = st[k].S_best;      // (as it is; +inf - no finite round - never wins)
        else {
            if (st && rf_of(st[k]).frozen != 0u && rf_of(st[k]).status == MDX_RF_NONFINITE) continue;
            for (uint32_t c = 0; c < W; ++c) S += (double)(float)rows[(size_t)k * W + c];
            if constexpr (std::is_same<State, mdx_fx_state>::value) S += (double)st[k].edih;
        }
        if (S < b.score) { b.score = S; b.pose = lig_of[k].y; }
    }
    best[m] = b;
}
__global__ __launch_bounds__(256) void guest_best_kernel(uint32_t n, uint32_t W, const double* __restrict__ rows, const uint2* __restrict__ lig_of,
                                                         GuestBest* __restrict__ best) {
    guest_best(n, W, rows, lig_of, (const mdx_rf_state*)nullptr, best);
}
__global__ __launch_bounds__(256) void guest_best_refined_kernel(uint32_t n, uint32_t W, const float* __restrict__ rows,
                                                                 const uint2* __restrict__ lig_of, const mdx_rf_state* __restrict__ st,
                                                                 GuestBest* __restrict__ best) {
    guest_best(n, W, rows, lig_of, st, best);
}
__global__ __launch_bounds__(256) void guest_best_flex_kernel(uint32_t n, uint32_t W, const float* __restrict__ rows,
                                                              const uint2* __restrict__ lig_of, const mdx_fx_state* __restrict__ st,
                                                              GuestBest* __restrict__ best) {
    guest_best(n, W, rows, lig_of, st, best);
}
__global__ __launch_bounds__(256) void guest_best_search_kernel(uint32_t n, const uint2* __restrict__ lig_of, const mdx_sr_record* __restrict__ rec,
                                                                GuestBest* __restrict__ best) {
    guest_best(n, 0u, (const float*)nullptr, lig_of, rec, best);
}

// A guest's own pairs: the class map [count^2] (0 plain, 1 excluded, 2 scaled 1-4) of its two pair lists; null, or why the lists are refused
static const char* guest_class_map(const mdx_guest_ligand& g, std::vector<uint8_t>& cls) {
    const uint32_t n = g.count;
    cls.assign((size_t)n * n, 0);
    for (int list = 0; list < 2; ++list) {
        const uint32_t np = list ? g.n_pairs14 : g.n_excl;
        const uint32_t* pr = list ? g.pairs14 : g.excl_pairs;
        const uint8_t mine = list ? 2 : 1;
        for (uint32_t k = 0; k < np; ++k) {
            const uint32_t a = pr[2 * (size_t)k], b = pr[2 * (size_t)k + 1];
            if (a >= n || b >= n) return "a pair names an atom outside the ligand";
            if (a == b) return "a pair of an atom with itself";
            uint8_t& c = cls[(size_t)a * n + b];
            if (c != 0 && c != mine) return "a pair is in both the exclusion and the 1-4 list";
            c = mine; cls[(size_t)b * n + a] = mine;
        }
    }
    return nullptr;
}

// What mdx_guest_flex adds to a ligand, as the kernels take it: the torsions with their moving sets, the terms that count (none without
// MDX_FLEX_DIHEDRALS or under MDX_OVR_BONDED_DISABLED) and their gather tables
struct GuestFlexTables { std::vector<mdx_fx_torsion> tor; std::vector<mdx_fx_dihedral> dih; std::vector<uint32_t> aoff, aent; };

// the refusals of one ligand's mdx_guest_flex (who: the call and the ligand), then its tables
static int guest_flex_check(const std::string& who, uint32_t count, const mdx_guest_flex& f, bool dihedrals, GuestFlexTables& t) {
    if (f.n_torsions > MDX_POSE_MAX_TORSIONS) FAIL(MDX_EPARAM, who + ": n_torsions exceeds MDX_POSE_MAX_TORSIONS (32)");
    if ((f.n_bonds && !f.bonds) || (f.n_torsions && !f.torsion_bonds) ||
        (f.n_dihedrals && (!f.dihedral_idx || !f.dihedral_v || !f.dihedral_phase || !f.dihedral_n)))
        FAIL(MDX_EPARAM, who + ": null argument (a list of the flexible record with a non-zero count)");
    if (f.n_dihedrals >= (1u << 20)) FAIL(MDX_EPARAM, who + ": too many dihedral terms");
    for (uint32_t k = 0; k < f.n_bonds; ++k) {
        const uint32_t a = f.bonds[2 * (size_t)k], b = f.bonds[2 * (size_t)k + 1];
        if (a >= count || b >= count) FAIL(MDX_EPARAM, who + ": bond " + std::to_string(k) + " names an atom index >= count");
        if (a == b) FAIL(MDX_EPARAM, who + ": bond " + std::to_string(k) + " names the same atom twice");
    }
    MDX_TRY(flex_sides(who, count, f.n_bonds, f.bonds, f.root, f.n_torsions, f.torsion_bonds, t.tor));
    t.tor.resize(f.n_torsions);
    t.dih.clear();
    for (uint32_t k = 0; k < f.n_dihedrals; ++k) {
        const uint32_t* at = f.dihedral_idx + 4 * (size_t)k;
        for (int r = 0; r < 4; ++r)
            if (at[r] >= count) FAIL(MDX_EPARAM, who + ": dihedral term " + std::to_string(k) + " names an atom index >= count");
        if (!std::isfinite(f.dihedral_v[k]) || !std::isfinite(f.dihedral_phase[k]))
            FAIL(MDX_EPARAM, who + ": dihedral term " + std::to_string(k) + ": v or phase is not finite");
        if (dihedrals)
            t.dih.push_back(mdx_fx_dihedral{{at[0], at[1], at[2], at[3]}, (double)f.dihedral_v[k], (double)f.dihedral_phase[k], (double)f.dihedral_n[k]});
    }
    flex_gather(count, t.dih, t.aoff, t.aent);
    return MDX_OK;
}

// A call on a library: its plan, the kernel arguments, the staging buffer
struct GuestRun {
    std::vector<GuestFlexTables> fx;      // mdx_refine_guests_flex: [n_ligands]
    std::vector<GuestShape> shapes;
    std::vector<size_t> pstart;
    std::vector<GuestChunk> chunks;
    std::vector<GuestSlot> slots;
    std::vector<unsigned char> up;
    std::vector<uint64_t> ids;            // mdx_search_guests: the stream ids of the chunk in flight
    std::vector<GuestBest> best;
    size_t total = 0;
    PoseArgs a{};
    int mode = 0; bool geom = false;
};

// the refusals that need no device, then the plan; flex (mdx_refine_guests_flex alone): the ligands' flexible records under `flags`
static int guest_check(mdx_handle* h, const std::string& who, uint32_t n_ligands, const mdx_guest_ligand* ligs, uint32_t n_groups, GuestRun& run,
                       const mdx_guest_flex* flex = nullptr, uint32_t flags = 0u) {
    const uint32_t G = h->n_grp;
    if (!G) FAIL(MDX_EPARAM, "no energy groups are set (mdx_set_energy_groups)");
    if (n_groups != G) FAIL(MDX_EPARAM, "n_groups must be the number of groups (mdx_energy_group_count)");
    if (h->dd || h->n_local != h->N) FAIL(MDX_EPARAM, who + " on a decomposed handle (single-device handles only)");
    if (h->alch_on) FAIL(MDX_EPARAM, who + " while an alchemical window is active");
    const bool skip14 = (h->cfg.overrides & MDX_OVR_BONDED_DISABLED) != 0;
    std::vector<uint8_t> cls;
    run.shapes.resize(n_ligands);
    run.fx.resize(flex ? n_ligands : 0u);
    for (uint32_t m = 0; m < n_ligands; ++m) {
        const mdx_guest_ligand& g = ligs[m];
        const std::string lig = who + ": ligand " + std::to_string(m) + ": ";
        if (g.count == 0 || g.count > MDX_POSE_MAX_ATOMS) FAIL(MDX_EPARAM, lig + "count must be in 1..MDX_POSE_MAX_ATOMS (256)");
        if (!g.charge || !g.lj_sigma || !g.lj_eps || (g.n_excl && !g.excl_pairs) || (g.n_pairs14 && !g.pairs14) || (g.n_poses && !g.poses))
            FAIL(MDX_EPARAM, lig + "null argument");
        for (uint32_t i = 0; i < g.count; ++i) {
            if (!std::isfinite(g.charge[i]) || !std::isfinite(g.lj_sigma[i]) || !std::isfinite(g.lj_eps[i]))
                FAIL(MDX_EPARAM, lig + "non-finite charge, sigma or eps");
            if (g.lj_sigma[i] < 0.f || g.lj_eps[i] < 0.f) FAIL(MDX_EPARAM, lig + "negative sigma or eps");
        }
        if (const char* why = guest_class_map(g, cls)) FAIL(MDX_EPARAM, lig + why);
        const size_t nx = 3 * (size_t)g.count * g.n_poses;
        for (size_t k = 0; k < nx; ++k)
            if (!std::isfinite(g.poses[k])) FAIL(MDX_EPARAM, lig + "non-finite pose coordinate");
        run.shapes[m] = GuestShape{g.count, g.n_poses, skip14 ? 0u : g.n_pairs14, 0u, 0u};
        if (flex) {
            MDX_TRY(guest_flex_check(who + ": ligand " + std::to_string(m), g.count, flex[m], (flags & MDX_FLEX_DIHEDRALS) != 0u && !skip14, run.fx[m]));
            run.shapes[m].T = (uint32_t)run.fx[m].tor.size(); run.shapes[m].n_terms = (uint32_t)run.fx[m].dih.size();
        }
    }
    guest_plan(run.shapes, run.pstart, run.chunks);
    run.total = run.pstart[n_ligands];
    return MDX_OK;
}

static GuestLayout guest_layout(const GuestChunk& c, uint32_t W, int gmode) {
    const bool flex = gmode == GUEST_FLEX || gmode == GUEST_SEARCH;
    return GuestLayout(c.n, c.atoms, c.n14, c.nxyz, c.ncls, W, gmode, flex ? sizeof(mdx_fx_state) : sizeof(mdx_rf_state), c.fx);
}

// the device side of a call that has work: the list of the current state, the block (it follows the largest chunk), the carried best
// poses, the kernel's arguments but for the chunk's pointers
static int guest_ready(mdx_handle* h, uint32_t n_ligands, int gmode, bool want_best, GuestRun& run) {
    HIP_TRY(hipSetDevice(h->device));
    MDX_TRY(mdx_ensure_ready(h));          // what the matrix would see: list, constraints and virtual sites of the current state
    DeviceState& d = h->d;
    const uint32_t G = h->n_grp;
    size_t need = 0;
    for (const GuestChunk& c : run.chunks) need = std::max(need, guest_layout(c, G + 1u, gmode).end);
    MDX_TRY(pose_grow(&d.gs_blk, h->gs_cap_blk, need));
    if (want_best) {
        run.best.assign(n_ligands, GuestBest{INFINITY, 0xFFFFFFFFu, 0u});
        MDX_TRY(pose_grow(&d.gs_best, h->gs_cap_best, sizeof(GuestBest) * run.best.size()));
        HIP_TRY(hipMemcpyAsync(d.gs_best, run.best.data(), sizeof(GuestBest) * run.best.size(), hipMemcpyHostToDevice, h->stream));
    }
    PoseArgs& a = run.a;
    a = PoseArgs{};
    bool samecut = false;
    mdx_fill_nb_params(h, a.p, &run.mode, &run.geom, &samecut);
    a.g = h->grid;
    a.posq = d.posq; a.lj = d.lj; a.orig_of = d.orig_of; a.gid = d.gid; a.grp = d.grp; a.slot_of = d.slot_of;
    a.tile_start = d.tile_start; a.cl_lo = d.cl_lo; a.cl_hi = d.cl_hi;
    a.G = G; a.L = 0xFFFFFFFFu;
    a.r_cull = std::isfinite(h->r_list) ? h->r_list + 0.01f : INFINITY;
    for (int k = 0; k < 3; ++k) {
        a.box[k] = h->per[k] ? h->box_hi[k] - h->box_lo[k] : 0.f;
        a.inv_box[k] = h->per[k] ? 1.0f / a.box[k] : 0.f;
    }
    return MDX_OK;
}

// a chunk goes up: records, tables and coordinates in one copy; the kernel's arguments point into its block.  search (mdx_search_guests:
// the layout is GUEST_SEARCH's): the walkers' stream ids follow into the search block - the caller's, in library pose order, or the
// walker's ligand-local pose index
static int guest_stage(mdx_handle* h, const mdx_guest_ligand* ligs, const GuestChunk& c, const GuestLayout& lay, GuestRun& run,
                       bool search = false, const uint64_t* streams_or_null = nullptr) {
    const mdx_config& cfg = h->cfg;
    const bool lj_off = (cfg.overrides & MDX_OVR_LJ_DISABLED) != 0, coul_off = (cfg.overrides & MDX_OVR_COULOMB_DISABLED) != 0;
    const bool geometric = cfg.combining_rule == MDX_COMBINE_GEOMETRIC;
    const float sqrt_ke = std::sqrt(cfg.coulomb_k);
    std::vector<unsigned char>& up = run.up;
    up.assign(lay.up_end, 0);
    float* gq = (float*)(up.data() + lay.q);
    float2* glj = (float2*)(up.data() + lay.lj);
    Pose14* p14 = (Pose14*)(up.data() + lay.p14);
    float* xyz = (float*)(up.data() + lay.xyz);
    guest_slots(run.shapes, run.pstart, c, run.slots);
    guest_records(run.shapes, run.slots, (PoseRec*)(up.data() + lay.rec), (uint32_t*)(up.data() + lay.ligof));
    const bool flex = !run.fx.empty();      // (the layout is GUEST_FLEX's or GUEST_SEARCH's then)
    if (flex) guest_flex_records(run.shapes, run.slots, (FlexRec*)(up.data() + lay.frec));
    std::vector<uint8_t> cls;
    for (const GuestSlot& s : run.slots) {
        const mdx_guest_ligand& g = ligs[s.m];
        const uint32_t cnt = g.count;
        // rows and records as mdx_create makes a resident atom's: the overrides zero eps and charge first
        std::vector<float2> raw(cnt);
        std::vector<float> q(cnt);
        for (uint32_t i = 0; i < cnt; ++i) {
            raw[i] = make_float2(g.lj_sigma[i], lj_off ? 0.f : g.lj_eps[i]);
            q[i] = coul_off ? 0.f : g.charge[i];
            gq[s.atom + i] = q[i] * sqrt_ke;
            glj[s.atom + i] = mdx_pack_lj(geometric, raw[i].x, raw[i].y);
        }
        (void)guest_class_map(g, cls);
        std::memcpy(up.data() + lay.cls + s.cls, cls.data(), cls.size());
        for (uint32_t k = 0; k < s.n14; ++k) {      // (0 with the bonded terms disabled)
            const uint32_t i = g.pairs14[2 * (size_t)k], j = g.pairs14[2 * (size_t)k + 1];
            const float4 prm = mdx_pair14_params(cfg, raw[i], raw[j], q[i], q[j]);
            p14[s.p14 + k] = Pose14{i, j, prm.x, prm.y, prm.z};
        }
        std::memcpy(xyz + s.xyz, g.poses + 3 * (size_t)cnt * s.l0, sizeof(float) * 3 * cnt * (s.l1 - s.l0));
        if (flex) {      // the ligand's flexible tables, once, as its rows above
            const GuestFlexTables& t = run.fx[s.m];
            if (!t.tor.empty()) std::memcpy(up.data() + lay.tor + sizeof(mdx_fx_torsion) * s.tor, t.tor.data(), sizeof(mdx_fx_torsion) * t.tor.size());
            if (!t.dih.empty()) {
                std::memcpy(up.data() + lay.dih + sizeof(mdx_fx_dihedral) * s.dih, t.dih.data(), sizeof(mdx_fx_dihedral) * t.dih.size());
                std::memcpy(up.data() + lay.aent + sizeof(uint32_t) * 4u * s.dih, t.aent.data(), sizeof(uint32_t) * t.aent.size());
            }
            std::memcpy(up.data() + lay.aoff + sizeof(uint32_t) * s.aoff, t.aoff.data(), sizeof(uint32_t) * t.aoff.size());
        }
    }
    unsigned char* blk = (unsigned char*)h->d.gs_blk;
    HIP_TRY(hipMemcpyAsync(blk, up.data(), lay.up_end, hipMemcpyHostToDevice, h->stream));
    if (search) {
        run.ids.resize(c.n);      // (free again: the chunk before this one has been waited for)
        for (const GuestSlot& s : run.slots)
            for (size_t l = s.l0; l < s.l1; ++l)
                run.ids[s.p + (l - s.l0)] = streams_or_null ? streams_or_null[run.pstart[s.m] + l] : (uint64_t)l;
        const SearchLayout ssl = SearchLayout::guest(c.n, c.nxyz, h->n_grp + 1u);
        HIP_TRY(hipMemcpyAsync(blk + lay.search + ssl.streams, run.ids.data(), sizeof(uint64_t) * c.n, hipMemcpyHostToDevice, h->stream));
    }
    PoseArgs& a = run.a;
    a.count = c.max_count;
    a.rec = (const PoseRec*)(blk + lay.rec);
    a.gq = (const float*)(blk + lay.q); a.glj = (const float2*)(blk + lay.lj);
    a.cls = blk + lay.cls; a.p14 = (const Pose14*)(blk + lay.p14);
    a.poses = (const float*)(blk + lay.xyz);
    a.slab = (double*)(blk + lay.slab);
    a.fslab = (double*)(blk + lay.fslab);
    return MDX_OK;
}

// mdx_screen_ligands (forces == nullptr: the energy flavour) and mdx_guest_forces (the force flavour; rows_out / rigid may be null)
static int guest_run(mdx_handle* h, const std::string& who, bool force, uint32_t n_ligands, const mdx_guest_ligand* ligs, float* rows_out,
                     uint32_t n_groups, float* forces, float* rigid, uint32_t* best_pose, double* best_score) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (n_ligands == 0) return MDX_OK;
    if (!ligs) FAIL(MDX_EPARAM, "null argument");
    const int gmode = force ? GUEST_FORCES : GUEST_ROWS;
    GuestRun run;
    MDX_TRY(guest_check(h, who, n_ligands, ligs, n_groups, run));
    const size_t total = run.total;
    if (total == 0) return MDX_OK;
    if (force ? !forces : !rows_out) FAIL(MDX_EPARAM, "null argument");
    const bool want_best = best_pose || best_score;
    MDX_TRY(guest_ready(h, n_ligands, gmode, want_best, run));
    DeviceState& d = h->d;
    hipStream_t st = h->stream;
    const uint32_t W = h->n_grp + 1u;
    size_t nxyz = 0;
    for (const GuestChunk& c : run.chunks) nxyz += c.nxyz;
    std::vector<float> res(total * W), fres(force ? nxyz : 0), rres(force ? 6u * total : 0);
    std::vector<double> rows((size_t)std::min<size_t>(total, POSE_CHUNK) * W);
    unsigned char* blk = (unsigned char*)d.gs_blk;
    size_t x0 = 0;      // first float of the chunk in `forces`
    for (const GuestChunk& c : run.chunks) {
        const GuestLayout lay = guest_layout(c, W, gmode);
        MDX_TRY(guest_stage(h, ligs, c, lay, run));
        const PoseArgs& a = run.a;
        double* drows = (double*)(blk + lay.rows);
        mdx_prof_begin(h, 0);
        pose_launch(h, a, run.mode, run.geom, c.n, force, false, true);
        hipLaunchKernelGGL(pose_sum_kernel, dim3((c.n * W + 255u) / 256u), dim3(256), 0, st, c.n, W, a.slab, drows);
        if (force)
            hipLaunchKernelGGL(guest_force_sum_kernel, dim3(c.n), dim3(256), 0, st, a.rec, a.poses, a.fslab, (float*)(blk + lay.fout),
                               (float*)(blk + lay.rigid));
        if (want_best)
            hipLaunchKernelGGL(guest_best_kernel, dim3((c.n + 255u) / 256u), dim3(256), 0, st, c.n, W, drows, (const uint2*)(blk + lay.ligof),
                               (GuestBest*)d.gs_best);
        mdx_prof_end(h);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(rows.data(), drows, sizeof(double) * (size_t)c.n * W, hipMemcpyDeviceToHost, st));
        if (force) {
            HIP_TRY(hipMemcpyAsync(fres.data() + x0, blk + lay.fout, sizeof(float) * c.nxyz, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(rres.data() + 6u * c.p0, blk + lay.rigid, sizeof(float) * 6u * c.n, hipMemcpyDeviceToHost, st));
        }
        if (want_best && &c == &run.chunks.back())
            HIP_TRY(hipMemcpyAsync(run.best.data(), d.gs_best, sizeof(GuestBest) * run.best.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t k = 0; force && k < c.nxyz; ++k)
            if (!std::isfinite(fres[x0 + k])) FAIL(MDX_ENAN, who + ": non-finite force");
        for (size_t k = 0; force && k < 6u * (size_t)c.n; ++k)
            if (!std::isfinite(rres[6u * c.p0 + k])) FAIL(MDX_ENAN, who + ": non-finite net force or torque");
        for (size_t k = 0; k < (size_t)c.n * W; ++k) {
            if (!std::isfinite(rows[k])) FAIL(MDX_ENAN, who + ": non-finite energy in a row");
            res[c.p0 * W + k] = (float)rows[k];
        }
        x0 += c.nxyz;
    }
    if (rows_out) std::memcpy(rows_out, res.data(), sizeof(float) * res.size());
    if (force) std::memcpy(forces, fres.data(), sizeof(float) * fres.size());
    if (force && rigid) std::memcpy(rigid, rres.data(), sizeof(float) * rres.size());
    for (uint32_t m = 0; want_best && m < n_ligands; ++m) {
        if (best_pose) best_pose[m] = run.best[m].pose;
        if (best_score) best_score[m] = run.best[m].score;
    }
    return MDX_OK;
}

extern "C" int mdx_screen_ligands(mdx_handle* h, uint32_t n_ligands, const mdx_guest_ligand* ligs, float* rows_out, uint32_t n_groups,
                                  uint32_t* best_pose, double* best_score) {
    return guest_run(h, "mdx_screen_ligands", false, n_ligands, ligs, rows_out, n_groups, nullptr, nullptr, best_pose, best_score);
}

extern "C" int mdx_guest_forces(mdx_handle* h, uint32_t n_ligands, const mdx_guest_ligand* ligs, float* rows_or_null, uint32_t n_groups,
                                float* forces, float* rigid_or_null) {
    return guest_run(h, "mdx_guest_forces", true, n_ligands, ligs, rows_or_null, n_groups, forces, rigid_or_null, nullptr, nullptr);
}

// the step kernel's arguments for a staged chunk of guests (guest_stage has set run.a) whose step block, laid out by sl, lies at
// lay.step; flex: with the chunk's flexible records and tables.  The force pass's frozen words are the step block's.
static StepArgs guest_step_args(mdx_handle* h, GuestRun& run, const GuestLayout& lay, const StepLayout& sl, uint32_t W, bool flex, const mdx_fx_opts& o) {
    unsigned char* blk = (unsigned char*)h->d.gs_blk;
    unsigned char* sb = blk + lay.step;
    StepArgs r = step_args(h, run.a, sb, 0u, W, false, 0u, 0u, sl, o);
    r.rec = run.a.rec;
    if (flex) {
        r.frec = (const FlexRec*)(blk + lay.frec);
        r.eterm = (double*)(sb + sl.eterm);
        r.tor = (const mdx_fx_torsion*)(blk + lay.tor); r.dih = (const mdx_fx_dihedral*)(blk + lay.dih);
        r.aoff = (const uint32_t*)(blk + lay.aoff); r.aent = (const uint32_t*)(blk + lay.aent);
    }
    run.a.frozen = r.frozen;
    return r;
}

// The loop of refine_chunks over the chunks of a library, State = mdx_rf_state (mdx_refine_guests: flex == null) or mdx_fx_state
// (mdx_refine_guests_flex): per chunk one upload, the frozen words and records zeroed, max_evals x (the GUEST REFINE force pass, the guest
// step kernel of the state), the best kernel on the accepted rows, one read-back, one wait.  The staged coordinates are the stage
// buffer: the step kernel writes the next trial where the force pass reads the pose.  xform and tgrad have the ligand's own width.
template <class State>
static int guest_refine(mdx_handle* h, const std::string& who, uint32_t n_ligands, const mdx_guest_ligand* ligs, const mdx_guest_flex* flex,
                        const mdx_flex_opts& fo, uint32_t n_groups, const RefineOut& out, uint32_t* best_pose_or_null, double* best_score_or_null) {
    constexpr bool FLEX = std::is_same<State, mdx_fx_state>::value;
    constexpr int gmode = FLEX ? GUEST_FLEX : GUEST_REFINE;
    mdx_fx_opts o{};
    MDX_TRY(refine_opts_check(who, fo, o));
    GuestRun run;
    MDX_TRY(guest_check(h, who, n_ligands, ligs, n_groups, run, flex, fo.flags));
    const size_t total = run.total;
    if (total == 0) return MDX_OK;
    if (!out.poses) FAIL(MDX_EPARAM, "null argument");
    const bool want_best = best_pose_or_null || best_score_or_null;
    MDX_TRY(guest_ready(h, n_ligands, gmode, want_best, run));
    DeviceState& d = h->d;
    hipStream_t st = h->stream;
    const uint32_t W = h->n_grp + 1u;
    size_t nxyz = 0;
    for (const GuestChunk& c : run.chunks) nxyz += c.nxyz;
    // where pose p's (q, t, theta) and g start: the ligands one behind the other, each with its own width
    std::vector<size_t> xat(total + 1, 0), tat(total + 1, 0);
    std::vector<uint32_t> Tof(total, 0);
    for (uint32_t m = 0; m < n_ligands; ++m)
        for (size_t p = run.pstart[m]; p < run.pstart[m + 1]; ++p) Tof[p] = run.shapes[m].T;
    for (size_t p = 0; p < total; ++p) { xat[p + 1] = xat[p] + 7u + Tof[p]; tat[p + 1] = tat[p] + Tof[p]; }
    std::vector<float> yres(nxyz), rres(total * W), gres(6u * total), xres(xat[total]), dres(FLEX ? total : 0u), tres(tat[total]);
    std::vector<uint32_t> sres(total), eres(total);
    std::vector<unsigned char> back;
    unsigned char* blk = (unsigned char*)d.gs_blk;
    size_t x0 = 0;      // first float of the chunk in poses_out
    for (const GuestChunk& c : run.chunks) {
        const GuestLayout lay = guest_layout(c, W, gmode);
        const StepLayout sl = StepLayout::guest(c.n, c.nxyz, W, sizeof(State), c.fx.terms);
        MDX_TRY(guest_stage(h, ligs, c, lay, run));
        PoseArgs& a = run.a;
        unsigned char* sb = blk + lay.step;
        const StepArgs r = guest_step_args(h, run, lay, sl, W, FLEX, o);
        HIP_TRY(hipMemsetAsync(sb, 0, sl.y, st));
        mdx_prof_begin(h, 0);
        for (uint32_t k = 0; k < fo.max_evals; ++k) step_evaluate<FLEX>(h, a, run.mode, run.geom, c.n, r);
        if (want_best) {
            const dim3 g((c.n + 255u) / 256u), b(256);
            const uint2* ligof = (const uint2*)(blk + lay.ligof);
            if constexpr (FLEX) hipLaunchKernelGGL(guest_best_flex_kernel, g, b, 0, st, c.n, W, (const float*)r.row, ligof, (const mdx_fx_state*)r.st, (GuestBest*)d.gs_best);
            else hipLaunchKernelGGL(guest_best_refined_kernel, g, b, 0, st, c.n, W, (const float*)r.row, ligof, (const mdx_rf_state*)r.st, (GuestBest*)d.gs_best);
        }
        mdx_prof_end(h);
        HIP_TRY(hipGetLastError());
        back.resize(sl.x0 - sl.state);
        HIP_TRY(hipMemcpyAsync(back.data(), sb + sl.state, back.size(), hipMemcpyDeviceToHost, st));
        if (want_best && &c == &run.chunks.back())
            HIP_TRY(hipMemcpyAsync(run.best.data(), d.gs_best, sizeof(GuestBest) * run.best.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const unsigned char* b0 = back.data() - sl.state;
        std::memcpy(yres.data() + x0, b0 + sl.y, sizeof(float) * c.nxyz);
        std::memcpy(rres.data() + c.p0 * W, b0 + sl.row, sizeof(float) * (size_t)W * c.n);
        std::memcpy(gres.data() + 6u * c.p0, b0 + sl.rigid, sizeof(float) * 6u * c.n);
        for (uint32_t k = 0; k < c.n; ++k) {
            State s;
            std::memcpy(&s, b0 + sl.state + sizeof(s) * k, sizeof(s));
            const size_t p = c.p0 + k;
            if constexpr (FLEX) refine_unpack(s, Tof[p], &sres[p], &eres[p], xres.data() + xat[p], &dres[p], tres.data() + tat[p]);
            else refine_unpack(s, &sres[p], &eres[p], xres.data() + xat[p]);
        }
        x0 += c.nxyz;
    }
    std::memcpy(out.poses, yres.data(), sizeof(float) * yres.size());
    if (out.rows) std::memcpy(out.rows, rres.data(), sizeof(float) * rres.size());
    if (out.rigid) std::memcpy(out.rigid, gres.data(), sizeof(float) * gres.size());
    if (out.xform) std::memcpy(out.xform, xres.data(), sizeof(float) * xres.size());
    if (out.dih) std::memcpy(out.dih, dres.data(), sizeof(float) * dres.size());
    if (out.tgrad && !tres.empty()) std::memcpy(out.tgrad, tres.data(), sizeof(float) * tres.size());
    if (out.status) std::memcpy(out.status, sres.data(), sizeof(uint32_t) * sres.size());
    if (out.evals) std::memcpy(out.evals, eres.data(), sizeof(uint32_t) * eres.size());
    for (uint32_t m = 0; want_best && m < n_ligands; ++m) {
        if (best_pose_or_null) best_pose_or_null[m] = run.best[m].pose;
        if (best_score_or_null) best_score_or_null[m] = run.best[m].score;
    }
    return MDX_OK;
}

extern "C" int mdx_refine_guests(mdx_handle* h, uint32_t n_ligands, const mdx_guest_ligand* ligs, const mdx_refine_opts* opts, float* poses_out,
                                 float* rows_out_or_null, uint32_t n_groups, float* rigid_out_or_null, float* xform_out_or_null,
                                 uint32_t* status_out_or_null, uint32_t* evals_out_or_null, uint32_t* best_pose_or_null,
                                 double* best_score_or_null) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (n_ligands == 0) return MDX_OK;
    if (!ligs || !opts) FAIL(MDX_EPARAM, "null argument");
    return guest_refine<mdx_rf_state>(h, "mdx_refine_guests", n_ligands, ligs, nullptr,
                                      mdx_flex_opts{opts->max_evals, opts->f_tol, opts->tau_tol, 0.f, opts->h_start, opts->h_max, 0u}, n_groups,
                                      RefineOut{poses_out, rows_out_or_null, rigid_out_or_null, xform_out_or_null, nullptr, nullptr,
                                                status_out_or_null, evals_out_or_null},
                                      best_pose_or_null, best_score_or_null);
}

extern "C" int mdx_refine_guests_flex(mdx_handle* h, uint32_t n_ligands, const mdx_guest_ligand* ligs, const mdx_guest_flex* flex,
                                      const mdx_flex_opts* opts, float* poses_out, float* rows_out_or_null, uint32_t n_groups,
                                      float* rigid_out_or_null, float* xform_out_or_null, float* dih_out_or_null, float* tgrad_out_or_null,
                                      uint32_t* status_out_or_null, uint32_t* evals_out_or_null, uint32_t* best_pose_or_null,
                                      double* best_score_or_null) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (n_ligands == 0) return MDX_OK;
    if (!ligs || !flex || !opts) FAIL(MDX_EPARAM, "null argument");
    return guest_refine<mdx_fx_state>(h, "mdx_refine_guests_flex", n_ligands, ligs, flex, *opts, n_groups,
                                      RefineOut{poses_out, rows_out_or_null, rigid_out_or_null, xform_out_or_null, dih_out_or_null,
                                                tgrad_out_or_null, status_out_or_null, evals_out_or_null},
                                      best_pose_or_null, best_score_or_null);
}

// ---- mdx_search_guests: the search of mdx_search_poses for a library - the loop of guest_refine<mdx_fx_state> run n_rounds times per
// chunk with guest_search_kernel between two of them.  Per chunk: one staging (the stream ids with it), the step block's head and the
// search records zeroed, n_rounds x (search kernel, max_evals x (the GUEST REFINE force pass, guest_flex_step_kernel)), the search kernel
// once more to decide the last round, guest_best_search_kernel on the records, one read-back of records .. best rigid, one wait.
extern "C" int mdx_search_guests(mdx_handle* h, uint32_t n_ligands, const mdx_guest_ligand* ligs, const mdx_guest_flex* flex,
                                 const uint64_t* streams_or_null, const mdx_search_opts* opts, float* best_out, float* best_rows_out_or_null,
                                 uint32_t n_groups, double* best_score_out_or_null, float* best_dih_out_or_null,
                                 uint32_t* best_round_out_or_null, uint32_t* stats_out_or_null, uint32_t* best_walker_or_null,
                                 double* best_ligand_score_or_null) {
    const std::string who = "mdx_search_guests";
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (n_ligands == 0) return MDX_OK;
    if (!ligs || !flex || !opts) FAIL(MDX_EPARAM, who + ": null argument");
    if (opts->n_rounds == 0 || opts->n_rounds > MDX_SEARCH_MAX_ROUNDS) FAIL(MDX_EPARAM, who + ": n_rounds must be in 1..MDX_SEARCH_MAX_ROUNDS (1024)");
    if ((uint64_t)opts->n_rounds * opts->refine.max_evals > 65536u) FAIL(MDX_EPARAM, who + ": n_rounds x max_evals exceeds 65536");
    for (float v : {opts->trans_amp, opts->rot_amp, opts->tors_amp, opts->kT})
        if (!std::isfinite(v) || v < 0.f) FAIL(MDX_EPARAM, who + ": an amplitude or kT is negative or not finite");
    if (opts->tors_amp > 3.14159265358979323846f) FAIL(MDX_EPARAM, who + ": tors_amp exceeds pi");      // (the fp32 nearest to pi passes)
    const mdx_sr_opts so{(double)opts->trans_amp, (double)opts->rot_amp, (double)opts->tors_amp, (double)opts->kT, opts->seed, opts->n_rounds, 0u};
    if (sr_choices(so, MDX_POSE_MAX_TORSIONS) == 0u) FAIL(MDX_EPARAM, who + ": no move is enabled (every amplitude is 0)");
    const mdx_flex_opts& fo = opts->refine;
    mdx_fx_opts o{};
    MDX_TRY(refine_opts_check(who, fo, o));
    GuestRun run;
    MDX_TRY(guest_check(h, who, n_ligands, ligs, n_groups, run, flex, fo.flags));
    for (uint32_t m = 0; m < n_ligands; ++m)
        if (run.shapes[m].n_poses && sr_choices(so, run.shapes[m].T) == 0u)
            FAIL(MDX_EPARAM, who + ": ligand " + std::to_string(m) + ": no move is enabled (only tors_amp with no torsion)");
    const size_t total = run.total;
    if (total == 0) return MDX_OK;
    if (!best_out) FAIL(MDX_EPARAM, who + ": null argument");
    const bool want_best = best_walker_or_null || best_ligand_score_or_null;
    MDX_TRY(guest_ready(h, n_ligands, GUEST_SEARCH, want_best, run));
    DeviceState& d = h->d;
    hipStream_t st = h->stream;
    const uint32_t W = h->n_grp + 1u;
    size_t nxyz = 0;
    for (const GuestChunk& c : run.chunks) nxyz += c.nxyz;
    std::vector<float> yres(nxyz), rres(total * W);
    SearchOut res(total);
    std::vector<unsigned char> back;
    unsigned char* blk = (unsigned char*)d.gs_blk;
    size_t x0 = 0;      // first float of the chunk in best_out
    for (const GuestChunk& c : run.chunks) {
        const GuestLayout lay = guest_layout(c, W, GUEST_SEARCH);
        const StepLayout sl = StepLayout::guest(c.n, c.nxyz, W, sizeof(mdx_fx_state), c.fx.terms);
        const SearchLayout ssl = SearchLayout::guest(c.n, c.nxyz, W);
        MDX_TRY(guest_stage(h, ligs, c, lay, run, true, streams_or_null));
        PoseArgs& a = run.a;
        unsigned char* sb = blk + lay.step;
        unsigned char* qb = blk + lay.search;
        const StepArgs r = guest_step_args(h, run, lay, sl, W, true, o);
        const SearchArgs s = search_args(r, qb, ssl, 0u, W, 0u, so);
        HIP_TRY(hipMemsetAsync(sb, 0, sl.y, st));
        HIP_TRY(hipMemsetAsync(qb + ssl.rec, 0, ssl.best_y - ssl.rec, st));
        mdx_prof_begin(h, 0);
        for (uint32_t rd = 0; rd < opts->n_rounds; ++rd) {
            mdx_launch_guest_search(st, c.n, s, rd, a.rec, r.frec);
            for (uint32_t k = 0; k < fo.max_evals; ++k) step_evaluate<true>(h, a, run.mode, run.geom, c.n, r);
        }
        mdx_launch_guest_search(st, c.n, s, opts->n_rounds, a.rec, r.frec);
        if (want_best)
            hipLaunchKernelGGL(guest_best_search_kernel, dim3((c.n + 255u) / 256u), dim3(256), 0, st, c.n, (const uint2*)(blk + lay.ligof),
                               (const mdx_sr_record*)s.rec, (GuestBest*)d.gs_best);
        mdx_prof_end(h);
        HIP_TRY(hipGetLastError());
        back.resize(ssl.cur_y - ssl.rec);
        HIP_TRY(hipMemcpyAsync(back.data(), qb + ssl.rec, back.size(), hipMemcpyDeviceToHost, st));
        if (want_best && &c == &run.chunks.back())
            HIP_TRY(hipMemcpyAsync(run.best.data(), d.gs_best, sizeof(GuestBest) * run.best.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const unsigned char* b0 = back.data();
        std::memcpy(yres.data() + x0, b0 + ssl.best_y, sizeof(float) * c.nxyz);
        std::memcpy(rres.data() + c.p0 * W, b0 + ssl.best_row, sizeof(float) * (size_t)W * c.n);
        res.take(b0 + ssl.rec, c.n, c.p0);
        x0 += c.nxyz;
    }
    std::memcpy(best_out, yres.data(), sizeof(float) * yres.size());
    if (best_rows_out_or_null) std::memcpy(best_rows_out_or_null, rres.data(), sizeof(float) * rres.size());
    res.write(best_score_out_or_null, best_dih_out_or_null, best_round_out_or_null, stats_out_or_null);
    for (uint32_t m = 0; want_best && m < n_ligands; ++m) {
        if (best_walker_or_null) best_walker_or_null[m] = run.best[m].pose;
        if (best_ligand_score_or_null) best_ligand_score_or_null[m] = run.best[m].score;
    }
    return MDX_OK;
}
