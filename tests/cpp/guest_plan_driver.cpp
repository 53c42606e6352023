// The chunk planner of the guest-ligand calls (molchanica_amd/csrc/mdx_pose_plan.h) on one host thread, for tests/test_guest_refine_host.py:
// built with the address and undefined-behaviour sanitizers.  stdin: the number of ligands, then per ligand "count n_poses n14".  For each of
// the three modes it plans the library, lays out every chunk, writes the records into a buffer of exactly the staged size and checks what
// a kernel relies on; the first violated condition is printed and the exit status is 1.  stdout: "ok <chunks> <poses> <largest block>".
#include "mdx_pose_plan.h"
#include <cstdio>
#include <cstdlib>
#include <string>

static int fail(const std::string& what, size_t chunk, size_t pose) {
    std::printf("FAIL chunk %zu pose %zu: %s\n", chunk, pose, what.c_str());
    return 1;
}

int main() {
    unsigned M = 0;
    if (std::scanf("%u", &M) != 1) return 2;
    std::vector<GuestShape> ligs(M);
    for (GuestShape& g : ligs)
        if (std::scanf("%u %u %u", &g.count, &g.n_poses, &g.n14) != 3) return 2;
    const uint32_t W = 3;
    const size_t state_bytes = 216;      // (any multiple of 8: the layouts take it as a parameter)
    size_t largest = 0, n_chunks = 0, total = 0;
    for (int mode = GUEST_ROWS; mode <= GUEST_REFINE; ++mode) {
        std::vector<size_t> pstart;
        std::vector<GuestChunk> chunks;
        std::vector<GuestSlot> slots;
        guest_plan(ligs, pstart, chunks);
        total = pstart[M];
        n_chunks = chunks.size();
        size_t next = 0;                 // the library's pose the next record must be
        std::vector<size_t> lig_next(M, 0);
        for (size_t ci = 0; ci < chunks.size(); ++ci) {
            const GuestChunk& c = chunks[ci];
            if (c.p0 != next || c.n == 0 || c.n > POSE_CHUNK) return fail("the chunks do not tile the pose range", ci, 0);
            if (ci + 1 < chunks.size() && c.n != POSE_CHUNK) return fail("a chunk before the last is not full", ci, 0);
            const GuestLayout lay(c.n, c.atoms, c.n14, c.nxyz, c.ncls, W, mode, state_bytes);
            largest = std::max(largest, lay.end);
            // the staged part: ascending, 16-byte aligned but for the byte-sized class maps' end, inside the block
            const size_t off[] = {lay.rec, lay.ligof, lay.q, lay.lj, lay.p14, lay.xyz, lay.cls};
            const size_t len[] = {sizeof(PoseRec) * c.n, 8u * c.n, 4u * c.atoms, 8u * c.atoms, sizeof(Pose14) * c.n14, 4u * c.nxyz, c.ncls};
            for (int k = 0; k < 7; ++k) {
                if (off[k] % 16u) return fail("a staged table is not 16-byte aligned", ci, (size_t)k);
                const size_t end = k < 6 ? off[k + 1] : lay.up_end;
                if (off[k] + len[k] > end) return fail("staged tables overlap", ci, (size_t)k);
            }
            if (lay.slab % 16u || lay.slab < lay.up_end) return fail("the slab overlaps the staged part", ci, 0);
            if (lay.rows != lay.slab + 8u * c.n * (POSE_UNITS + 1u) * W) return fail("rows overlap the slab", ci, 0);
            size_t end = lay.rows + 8u * c.n * W;
            if (mode != GUEST_ROWS) {
                if (lay.fslab % 8u || lay.fslab < end) return fail("the force slab overlaps the rows", ci, 0);
                if (lay.fout < lay.fslab + 8u * (POSE_UNITS + 1u) * c.nxyz || lay.fout % 4u) return fail("forces overlap the force slab", ci, 0);
                if (lay.rigid < lay.fout + 4u * c.nxyz || lay.rigid % 4u) return fail("rigid overlaps the forces", ci, 0);
                if (lay.step % 16u || lay.step < lay.rigid + 24u * c.n) return fail("the step block overlaps rigid", ci, 0);
                end = lay.step;
            }
            if (mode == GUEST_REFINE) {
                const StepLayout sl(c.n, c.nxyz, W, state_bytes, 0u);
                if (sl.frozen != 0 || sl.state % 16u || sl.state < 4u * c.n) return fail("state records overlap the frozen words", ci, 0);
                if (sl.y != sl.state + state_bytes * c.n || sl.row != sl.y + 4u * c.nxyz || sl.rigid != sl.row + 4u * W * c.n ||
                    sl.x0 != sl.rigid + 24u * c.n || sl.eterm < sl.x0 + 4u * c.nxyz || sl.end != sl.eterm)
                    return fail("the step block's parts are not one behind the other", ci, 0);
                end = lay.step + sl.end;
            }
            if (lay.end != end) return fail("the block does not end where its last part does", ci, 0);
            // the records: written into buffers of exactly the staged size (the sanitizer watches their ends)
            std::vector<PoseRec> rec(c.n, PoseRec{~0u, ~0u, ~0u, ~0u, ~0u, ~0u});
            std::vector<uint32_t> ligof(2u * c.n, ~0u);
            guest_slots(ligs, pstart, c, slots);
            guest_records(ligs, slots, rec.data(), ligof.data());
            size_t atoms = 0, n14 = 0, ncls = 0;
            for (const GuestSlot& s : slots) {
                if (s.m < c.m0 || s.m > c.m1 || ligs[s.m].n_poses == 0) return fail("a slot names a ligand outside the chunk", ci, s.m);
                if (s.atom != atoms || s.p14 != n14 || s.cls != ncls) return fail("the ligands' tables are not one behind the other", ci, s.m);
                atoms += ligs[s.m].count; n14 += ligs[s.m].n14; ncls += (size_t)ligs[s.m].count * ligs[s.m].count;
            }
            if (atoms != c.atoms || n14 != c.n14 || ncls != c.ncls) return fail("the chunk's sums are not those of its ligands", ci, 0);
            size_t nx = 0;
            uint32_t max_count = 0;
            for (uint32_t p = 0; p < c.n; ++p) {
                const PoseRec& r = rec[p];
                const uint32_t m = ligof[2u * p], l = ligof[2u * p + 1u];
                if (m >= M) return fail("a pose without a record", ci, p);
                if (pstart[m] + l != next) return fail("the records do not follow the library's pose order", ci, p);
                if (l != lig_next[m]++) return fail("a ligand's poses are not consecutive", ci, p);
                if (r.count != ligs[m].count || r.n14 != ligs[m].n14) return fail("a record's size is not its ligand's", ci, p);
                if (r.xyz != nx) return fail("the poses' coordinates are not one behind the other", ci, p);
                if ((size_t)r.atom + r.count > c.atoms || (size_t)r.cls + (size_t)r.count * r.count > c.ncls || (size_t)r.p14 + r.n14 > c.n14)
                    return fail("a record points outside the chunk's tables", ci, p);
                // the force slab of the pose: POSE_UNITS + 1 blocks from (POSE_UNITS + 1) x xyz on, inside the slab and clear of the next pose's
                if ((size_t)(POSE_UNITS + 1u) * (r.xyz + 3u * (size_t)r.count) > (size_t)(POSE_UNITS + 1u) * c.nxyz)
                    return fail("a pose's partial forces leave the force slab", ci, p);
                nx += 3u * (size_t)r.count;
                max_count = std::max(max_count, r.count);
                ++next;
            }
            if (nx != c.nxyz) return fail("the coordinates do not fill the chunk's block", ci, 0);
            if (max_count != c.max_count) return fail("max_count is not the chunk's largest ligand", ci, 0);
        }
        if (next != total) return fail("poses left over", chunks.size(), next);
        for (uint32_t m = 0; m < M; ++m)
            if (lig_next[m] != ligs[m].n_poses) return fail("a ligand's poses were not all placed", chunks.size(), m);
    }
    std::printf("ok %zu %zu %zu\n", n_chunks, total, largest);
    return 0;
}
