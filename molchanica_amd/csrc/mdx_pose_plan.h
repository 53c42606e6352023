// mdx_pose_plan.h - the host arithmetic of the pose passes' device blocks: which poses a chunk holds and where everything in its block
// lies.  Plain C++ (no device code, no runtime call): mdx_poses.hip lays its chunks out with it, and a stand-alone program can call it
// (tests/cpp/guest_plan_driver.cpp).
//   StepLayout   the refinement's block of a chunk (mdx_refine_poses, mdx_refine_poses_flex, mdx_search_poses, mdx_refine_guests)
//   SearchLayout the search's block of a chunk behind it (mdx_search_poses, mdx_search_guests): one struct, two forms
//   GuestLayout  the block of one chunk of guest poses: what the host stages, then what the kernels write
//   guest_plan   the chunks of a library (POSE_CHUNK consecutive poses each) and, per chunk, the ligands it holds poses of
//   guest_slots  where every such ligand's tables and poses lie in the chunk; guest_records makes the per-pose records from them
//   (the flexible guest refinement: per ligand the torsion table, the dihedral terms and their gather tables - FlexRec per pose,
//   guest_flex_records - and per pose its own stretch of the terms' energies and forces)
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

// What a guest pose adds for the flexible refinement, parallel to PoseRec: its ligand's torsion table (first mdx_fx_torsion of the chunk's
// and T), its dihedral terms (first mdx_fx_dihedral and n_terms), the gather tables (first word of aoff [count + 1] and of aent
// [4 n_terms]), and the pose's own first term of the chunk's eterm [terms of all poses][FLEX_TERM_WORDS].
struct FlexRec { uint32_t tor, T, dih, n_terms, aoff, aent, eterm, pad; };
#define GUEST_TOR_BYTES 48u     // sizeof(mdx_fx_torsion), sizeof(mdx_fx_dihedral) (mdx_flex_step.h; mdx_poses.hip asserts both)
#define GUEST_DIH_BYTES 40u

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
    // a chunk of guest poses: every pose has its ligand's number of terms, `terms` in all
    static StepLayout guest(uint32_t n, size_t nxyz, uint32_t W, size_t state_bytes, size_t terms) {
        StepLayout l(n, nxyz, W, state_bytes, 0u);
        l.end = l.eterm + sizeof(double) * FLEX_TERM_WORDS * terms;
        return l;
    }
};

// The search block of a chunk of n walkers with nxyz coordinates in all and rows W wide: [records | best coordinates | best rows | best
// rigid | current coordinates | stream ids], every part on 16 bytes; records .. best rigid come back in one copy at the chunk's end.
// A walker's stretch of the best and the current coordinates is its stretch of the refinement's coordinate-shaped buffers (resident:
// walker x count x 3; guests: PoseRec.xyz).  The resident form takes the ligand's per_pose = 3 count floats.
#define SEARCH_REC_BYTES 40u    // sizeof(mdx_sr_record) (mdx_search_step.h; mdx_pose_search_dev.h asserts it)
struct SearchLayout {
    size_t rec, best_y, best_row, best_rigid, cur_y, streams, end;
    SearchLayout(uint32_t n, size_t per_pose, uint32_t G) { lay(n, per_pose * n, G); }
    static SearchLayout guest(uint32_t n, size_t nxyz, uint32_t W) {
        SearchLayout l;
        l.lay(n, nxyz, W);
        return l;
    }
private:
    SearchLayout() {}
    void lay(uint32_t n, size_t nxyz, uint32_t W) {
        auto al = [](size_t x) { return (x + 15u) / 16u * 16u; };
        rec = 0;
        best_y = al(SEARCH_REC_BYTES * (size_t)n);
        best_row = al(best_y + sizeof(float) * nxyz);
        best_rigid = al(best_row + sizeof(float) * (size_t)W * n);
        cur_y = al(best_rigid + sizeof(float) * 6u * n);
        streams = al(cur_y + sizeof(float) * nxyz);
        end = streams + sizeof(uint64_t) * n;
    }
};

// mdx_screen_ligands, mdx_guest_forces, mdx_refine_guests, mdx_refine_guests_flex, mdx_search_guests
enum GuestMode { GUEST_ROWS = 0, GUEST_FORCES = 1, GUEST_REFINE = 2, GUEST_FLEX = 3, GUEST_SEARCH = 4 };

// the flexible tables of a chunk, in elements: torsions, dihedral terms (every ligand's rounded up to an even number: its table starts
// on 16 bytes), words of aoff (every ligand's count + 1 rounded up to 4) and the terms of all poses (eterm)
struct GuestFlexSums { size_t tor = 0, dih = 0, aoff = 0, terms = 0; };
inline size_t guest_dih_room(uint32_t n_terms) { return ((size_t)n_terms + 1u) / 2u * 2u; }
inline size_t guest_aoff_room(uint32_t count) { return ((size_t)count + 1u + 3u) / 4u * 4u; }

// The device block of one chunk of n guest poses: what the host stages ([0, up_end): records, (ligand, pose) words, charge and LJ rows
// of the chunk's ligands, their 1-4 records, the coordinates, the class maps), then the units' slab and the summed rows; with forces
// the units' force slab, the summed forces and rigid; for a refinement the force slab and a StepLayout at `step` (state_bytes > 0).
// GUEST_FLEX stages, behind the class maps, the FlexRec records and the ligands' flexible tables (fx), each on 16 bytes, and its
// StepLayout ends with the terms of all poses.  GUEST_SEARCH is GUEST_FLEX with a SearchLayout at `search` behind the step block.
struct GuestLayout {
    size_t rec, ligof, q, lj, p14, xyz, cls, frec, tor, dih, aoff, aent, up_end, slab, rows, fslab, fout, rigid, step, end, search;
    GuestLayout(size_t n, size_t atoms, size_t n14, size_t nxyz, size_t ncls, uint32_t W, int mode = GUEST_ROWS, size_t state_bytes = 0,
                const GuestFlexSums& fx = GuestFlexSums()) {
        auto al = [](size_t x) { return (x + 15u) / 16u * 16u; };
        rec = 0;
        ligof = al(rec + sizeof(PoseRec) * n);
        q = al(ligof + 2u * sizeof(uint32_t) * n);
        lj = al(q + sizeof(float) * atoms);
        p14 = al(lj + 2u * sizeof(float) * atoms);
        xyz = al(p14 + sizeof(Pose14) * n14);
        cls = al(xyz + sizeof(float) * nxyz);
        up_end = cls + ncls;
        frec = tor = dih = aoff = aent = up_end;
        if (mode == GUEST_FLEX || mode == GUEST_SEARCH) {
            frec = al(up_end);
            tor = al(frec + sizeof(FlexRec) * n);
            dih = al(tor + GUEST_TOR_BYTES * fx.tor);
            aoff = al(dih + GUEST_DIH_BYTES * fx.dih);
            aent = al(aoff + sizeof(uint32_t) * fx.aoff);
            up_end = aent + sizeof(uint32_t) * 4u * fx.dih;
        }
        slab = al(up_end);
        rows = slab + sizeof(double) * n * (POSE_UNITS + 1u) * W;
        end = rows + sizeof(double) * n * W;
        fslab = fout = rigid = step = search = end;
        if (mode == GUEST_ROWS) return;
        fslab = end;
        fout = fslab + sizeof(double) * (POSE_UNITS + 1u) * nxyz;
        rigid = fout + sizeof(float) * nxyz;
        step = al(rigid + sizeof(float) * 6u * n);
        end = step;
        if (mode == GUEST_REFINE) end = step + StepLayout((uint32_t)n, nxyz, W, state_bytes, 0u).end;
        if (mode == GUEST_FLEX || mode == GUEST_SEARCH) end = step + StepLayout::guest((uint32_t)n, nxyz, W, state_bytes, fx.terms).end;
        search = end;
        if (mode == GUEST_SEARCH) {
            search = al(end);
            end = search + SearchLayout::guest((uint32_t)n, nxyz, W).end;
        }
    }
};

// a ligand as the planner sees it; n14: the 1-4 records it stages; T, n_terms: its torsions and dihedral terms (flexible refinement)
struct GuestShape { uint32_t count, n_poses, n14, T, n_terms; };

// POSE_CHUNK consecutive poses of the library: p0, n; the ligands it holds poses of (m0 .. m1; empty ligands between them are skipped);
// the sums its layout is made from, and its largest ligand (the force flavour's dynamic LDS)
struct GuestChunk { size_t p0; uint32_t n, m0, m1; size_t atoms, n14, nxyz, ncls; uint32_t max_count; GuestFlexSums fx; };

// -> pstart [n_ligands + 1] (first pose of every ligand in the library's pose order) and the chunks, in order
inline void guest_plan(const std::vector<GuestShape>& ligs, std::vector<size_t>& pstart, std::vector<GuestChunk>& chunks) {
    const uint32_t M = (uint32_t)ligs.size();
    pstart.assign((size_t)M + 1, 0);
    for (uint32_t m = 0; m < M; ++m) pstart[m + 1] = pstart[m] + ligs[m].n_poses;
    const size_t total = pstart[M];
    chunks.clear();
    uint32_t m = 0;
    for (size_t p0 = 0; p0 < total; p0 += POSE_CHUNK) {
        GuestChunk c{p0, (uint32_t)std::min<size_t>(POSE_CHUNK, total - p0), 0, 0, 0, 0, 0, 0, 0, GuestFlexSums()};
        while (pstart[m + 1] <= p0) ++m;
        c.m0 = m;
        for (uint32_t k = m; k < M && pstart[k] < p0 + c.n; ++k) {
            if (ligs[k].n_poses == 0) continue;
            const size_t cnt = ligs[k].count, np = std::min(pstart[k + 1], p0 + c.n) - std::max(pstart[k], p0);
            c.m1 = k; c.atoms += cnt; c.ncls += cnt * cnt; c.nxyz += 3 * cnt * np; c.n14 += ligs[k].n14;
            c.max_count = std::max(c.max_count, ligs[k].count);
            c.fx.tor += ligs[k].T; c.fx.dih += guest_dih_room(ligs[k].n_terms); c.fx.aoff += guest_aoff_room(ligs[k].count);
            c.fx.terms += (size_t)ligs[k].n_terms * np;
        }
        chunks.push_back(c);
    }
}

// A ligand with poses in a chunk: its first rows in the chunk's tables, its poses [l0, l1) (ligand-local) as the chunk's poses
// p .. p + (l1 - l0), the first of them at float xyz of the coordinates; its flexible tables (tor, dih, aoff; aent starts at word
// 4 dih) and the first term of its first pose in the chunk's eterm
struct GuestSlot { uint32_t m, atom, cls, p14, n14, p, xyz; size_t l0, l1; uint32_t tor, dih, aoff, eterm; };

inline void guest_slots(const std::vector<GuestShape>& ligs, const std::vector<size_t>& pstart, const GuestChunk& c, std::vector<GuestSlot>& slots) {
    slots.clear();
    uint32_t atom = 0, n14 = 0, nx = 0, ncls = 0, p = 0, tor = 0, dih = 0, aoff = 0, eterm = 0;
    for (uint32_t m = c.m0; m <= c.m1; ++m) {
        const GuestShape& g = ligs[m];
        if (g.n_poses == 0) continue;
        const size_t l0 = std::max(pstart[m], c.p0) - pstart[m], l1 = std::min(pstart[m + 1], c.p0 + c.n) - pstart[m];
        slots.push_back(GuestSlot{m, atom, ncls, n14, g.n14, p, nx, l0, l1, tor, dih, aoff, eterm});
        atom += g.count; ncls += g.count * g.count; n14 += g.n14;
        tor += g.T; dih += (uint32_t)guest_dih_room(g.n_terms); aoff += (uint32_t)guest_aoff_room(g.count);
        eterm += g.n_terms * (uint32_t)(l1 - l0);
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

// the flexible records of the chunk's poses: frec [c.n]
inline void guest_flex_records(const std::vector<GuestShape>& ligs, const std::vector<GuestSlot>& slots, FlexRec* frec) {
    for (const GuestSlot& s : slots) {
        const GuestShape& g = ligs[s.m];
        for (size_t l = s.l0; l < s.l1; ++l)
            frec[s.p + (uint32_t)(l - s.l0)] = FlexRec{s.tor, g.T, s.dih, g.n_terms, s.aoff, 4u * s.dih, s.eterm + g.n_terms * (uint32_t)(l - s.l0), 0u};
    }
}
