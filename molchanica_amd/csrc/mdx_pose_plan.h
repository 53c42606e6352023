// mdx_pose_plan.h - the host arithmetic of the pose passes' device blocks: which poses a chunk holds and where everything in its block
// lies.  Plain C++ (no device code, no runtime call): mdx_poses.hip lays its chunks out with it, and a stand-alone program can call it
// (tests/cpp/guest_plan_driver.cpp).
//   StepLayout   the refinement's block of a chunk (mdx_refine_poses, mdx_refine_poses_flex, mdx_search_poses, mdx_refine_guests)
//   GuestLayout  the block of one chunk of guest poses: what the host stages, then what the kernels write
//   guest_plan   the chunks of a library (POSE_CHUNK consecutive poses each) and, per chunk, the ligands it holds poses of
//   guest_slots  where every such ligand's tables and poses lie in the chunk; guest_records makes the per-pose records from them
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#define POSE_UNITS 16u     // environment units per pose: a batch of one pose still spreads over 17 workgroups
#define POSE_CHUNK 256u    // poses staged per launch (host staging only: it does not enter the arithmetic)
#define FLEX_TERM_WORDS 13u      // per dihedral term and evaluation: energy, then the forces on its four atoms

struct Pose14 { uint32_t a, b; float sig, e4, qq; };      // ligand-local atoms; sigma_ij, 4 scale eps_ij, scale k_e q_i q_j

// A guest pose: where its ligand lies in the chunk's tables.  atom: first row of the charge / LJ tables; cls: first byte of its class
// map [count^2]; p14, n14: its 1-4 records; xyz: first float of the pose's coordinates - and of everything shaped like them: forces,
// accepted coordinates, input poses; the pose's partial forces start at double (POSE_UNITS + 1) x xyz of the force slab.
struct PoseRec { uint32_t atom, count, cls, p14, n14, xyz; };

// The refinement's device block of a chunk of n poses with nxyz coordinates in all (n x count x 3 of a resident ligand): [frozen words |
// state records | accepted coordinates | rows | rigid | input poses | the dihedral terms' energies and forces]; the first two are
// zeroed at the start of the chunk, records .. rigid come back in one copy at its end.  W is the width of a row; state_bytes is
// sizeof(mdx_rf_state) or sizeof(mdx_fx_state); the rigid refinement has no terms.
struct StepLayout {
    size_t frozen, state, y, row, rigid, x0, eterm, end;
    StepLayout(uint32_t n, size_t nxyz, uint32_t W, size_t state_bytes, uint32_t n_terms) {
        frozen = 0;
        state = ((sizeof(uint32_t) * n + 15u) / 16u) * 16u;
        y = state + state_bytes * n;
        row = y + sizeof(float) * nxyz;
        rigid = row + sizeof(float) * (size_t)W * n;
        x0 = rigid + sizeof(float) * 6u * n;
        eterm = ((x0 + sizeof(float) * nxyz + 15u) / 16u) * 16u;
        end = eterm + sizeof(double) * FLEX_TERM_WORDS * (size_t)n_terms * n;
    }
};

enum GuestMode { GUEST_ROWS = 0, GUEST_FORCES = 1, GUEST_REFINE = 2 };      // mdx_screen_ligands, mdx_guest_forces, mdx_refine_guests

// The device block of one chunk of n guest poses: what the host stages ([0, up_end): records, (ligand, pose) words, charge and LJ rows
// of the chunk's ligands, their 1-4 records, the coordinates, the class maps), then the units' slab and the summed rows; with forces
// the units' force slab, the summed forces and rigid; for a refinement the force slab and a StepLayout at `step` (state_bytes > 0).
struct GuestLayout {
    size_t rec, ligof, q, lj, p14, xyz, cls, up_end, slab, rows, fslab, fout, rigid, step, end;
    GuestLayout(size_t n, size_t atoms, size_t n14, size_t nxyz, size_t ncls, uint32_t W, int mode = GUEST_ROWS, size_t state_bytes = 0) {
        auto al = [](size_t x) { return (x + 15u) / 16u * 16u; };
        rec = 0;
        ligof = al(rec + sizeof(PoseRec) * n);
        q = al(ligof + 2u * sizeof(uint32_t) * n);
        lj = al(q + sizeof(float) * atoms);
        p14 = al(lj + 2u * sizeof(float) * atoms);
        xyz = al(p14 + sizeof(Pose14) * n14);
        cls = al(xyz + sizeof(float) * nxyz);
        up_end = cls + ncls;
        slab = al(up_end);
        rows = slab + sizeof(double) * n * (POSE_UNITS + 1u) * W;
        end = rows + sizeof(double) * n * W;
        fslab = fout = rigid = step = end;
        if (mode == GUEST_ROWS) return;
        fslab = end;
        fout = fslab + sizeof(double) * (POSE_UNITS + 1u) * nxyz;
        rigid = fout + sizeof(float) * nxyz;
        step = al(rigid + sizeof(float) * 6u * n);
        end = mode == GUEST_REFINE ? step + StepLayout((uint32_t)n, nxyz, W, state_bytes, 0u).end : step;
    }
};

struct GuestShape { uint32_t count, n_poses, n14; };      // a ligand as the planner sees it; n14: the 1-4 records it stages

// POSE_CHUNK consecutive poses of the library: p0, n; the ligands it holds poses of (m0 .. m1; empty ligands between them are skipped);
// the sums its layout is made from, and its largest ligand (the force flavour's dynamic LDS)
struct GuestChunk { size_t p0; uint32_t n, m0, m1; size_t atoms, n14, nxyz, ncls; uint32_t max_count; };

// -> pstart [n_ligands + 1] (first pose of every ligand in the library's pose order) and the chunks, in order
inline void guest_plan(const std::vector<GuestShape>& ligs, std::vector<size_t>& pstart, std::vector<GuestChunk>& chunks) {
    const uint32_t M = (uint32_t)ligs.size();
    pstart.assign((size_t)M + 1, 0);
    for (uint32_t m = 0; m < M; ++m) pstart[m + 1] = pstart[m] + ligs[m].n_poses;
    const size_t total = pstart[M];
    chunks.clear();
    uint32_t m = 0;
    for (size_t p0 = 0; p0 < total; p0 += POSE_CHUNK) {
        GuestChunk c{p0, (uint32_t)std::min<size_t>(POSE_CHUNK, total - p0), 0, 0, 0, 0, 0, 0, 0};
        while (pstart[m + 1] <= p0) ++m;
        c.m0 = m;
        for (uint32_t k = m; k < M && pstart[k] < p0 + c.n; ++k) {
            if (ligs[k].n_poses == 0) continue;
            const size_t cnt = ligs[k].count, np = std::min(pstart[k + 1], p0 + c.n) - std::max(pstart[k], p0);
            c.m1 = k; c.atoms += cnt; c.ncls += cnt * cnt; c.nxyz += 3 * cnt * np; c.n14 += ligs[k].n14;
            c.max_count = std::max(c.max_count, ligs[k].count);
        }
        chunks.push_back(c);
    }
}

// A ligand with poses in a chunk: its first rows in the chunk's tables, its poses [l0, l1) (ligand-local) as the chunk's poses
// p .. p + (l1 - l0), the first of them at float xyz of the coordinates
struct GuestSlot { uint32_t m, atom, cls, p14, n14, p, xyz; size_t l0, l1; };

inline void guest_slots(const std::vector<GuestShape>& ligs, const std::vector<size_t>& pstart, const GuestChunk& c, std::vector<GuestSlot>& slots) {
    slots.clear();
    uint32_t atom = 0, n14 = 0, nx = 0, ncls = 0, p = 0;
    for (uint32_t m = c.m0; m <= c.m1; ++m) {
        const GuestShape& g = ligs[m];
        if (g.n_poses == 0) continue;
        const size_t l0 = std::max(pstart[m], c.p0) - pstart[m], l1 = std::min(pstart[m + 1], c.p0 + c.n) - pstart[m];
        slots.push_back(GuestSlot{m, atom, ncls, n14, g.n14, p, nx, l0, l1});
        atom += g.count; ncls += g.count * g.count; n14 += g.n14;
        p += (uint32_t)(l1 - l0); nx += 3u * g.count * (uint32_t)(l1 - l0);
    }
}

// the records of the chunk's poses and their (ligand, ligand-local pose) words: rec [c.n], ligof [c.n][2]
inline void guest_records(const std::vector<GuestShape>& ligs, const std::vector<GuestSlot>& slots, PoseRec* rec, uint32_t* ligof) {
    for (const GuestSlot& s : slots) {
        const uint32_t cnt = ligs[s.m].count;
        for (size_t l = s.l0; l < s.l1; ++l) {
            const uint32_t p = s.p + (uint32_t)(l - s.l0);
            rec[p] = PoseRec{s.atom, cnt, s.cls, s.p14, s.n14, s.xyz + 3u * cnt * (uint32_t)(l - s.l0)};
            ligof[2u * p] = s.m; ligof[2u * p + 1u] = (uint32_t)l;
        }
    }
}
