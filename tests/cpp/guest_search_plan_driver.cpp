// The search block of the guest pose search in the chunk planner (molchanica_amd/csrc/mdx_pose_plan.h: SearchLayout, GUEST_SEARCH) on one
// host thread, for tests/test_guest_search_host.py: built plain and with the address and undefined-behaviour sanitizers.  stdin: the
// number of ligands, then per ligand "count n_poses n14 T n_terms".  It plans the library, lays out every chunk in GUEST_SEARCH mode and
// checks what guest_search_kernel and the driver rely on: the staged part and the step block are GUEST_FLEX's, the parts of the search
// block are 16-byte aligned, overlap neither each other nor the step block, and hold every walker's stretch - written here, walker by
// walker, into buffers of exactly the parts' sizes; the four older modes lie where the layout before the search block put them (Before:
// that layout restated).  The first violated condition is printed and the exit status is 1.
// stdout: "ok <chunks> <walkers> <largest block>", then per chunk "chunk <i> walkers <n> search <offset> <bytes>".
#include "mdx_pose_plan.h"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>

static int fail(const std::string& what, size_t chunk, size_t at) {
    std::printf("FAIL chunk %zu at %zu: %s\n", chunk, at, what.c_str());
    return 1;
}

static size_t al(size_t x) { return (x + 15u) / 16u * 16u; }

// GuestLayout as it was before GUEST_SEARCH: the offsets of the four older modes, from the sizes alone
struct Before {
    size_t rec, ligof, q, lj, p14, xyz, cls, frec, tor, dih, aoff, aent, up_end, slab, rows, fslab, fout, rigid, step, end;
    Before(size_t n, size_t atoms, size_t n14, size_t nxyz, size_t ncls, uint32_t W, int mode, size_t state_bytes, const GuestFlexSums& fx) {
        rec = 0;
        ligof = al(24u * n);
        q = al(ligof + 8u * n);
        lj = al(q + 4u * atoms);
        p14 = al(lj + 8u * atoms);
        xyz = al(p14 + 20u * n14);
        cls = al(xyz + 4u * nxyz);
        up_end = cls + ncls;
        frec = tor = dih = aoff = aent = up_end;
        if (mode == GUEST_FLEX) {
            frec = al(up_end);
            tor = al(frec + 32u * n);
            dih = al(tor + 48u * fx.tor);
            aoff = al(dih + 40u * fx.dih);
            aent = al(aoff + 4u * fx.aoff);
            up_end = aent + 16u * fx.dih;
        }
        slab = al(up_end);
        rows = slab + 8u * n * 17u * W;
        end = rows + 8u * n * W;
        fslab = fout = rigid = step = end;
        if (mode == GUEST_ROWS) return;
        fout = fslab + 8u * 17u * nxyz;
        rigid = fout + 4u * nxyz;
        step = al(rigid + 24u * n);
        end = step;
        if (mode == GUEST_FORCES) return;
        const size_t state = al(4u * n), x0 = state + state_bytes * n + 4u * nxyz + 4u * (size_t)W * n + 24u * n, eterm = al(x0 + 4u * nxyz);
        end = step + eterm + (mode == GUEST_FLEX ? 8u * 13u * fx.terms : 0u);
    }
};

int main() {
    unsigned M = 0;
    if (std::scanf("%u", &M) != 1) return 2;
    std::vector<GuestShape> ligs(M);
    for (GuestShape& g : ligs)
        if (std::scanf("%u %u %u %u %u", &g.count, &g.n_poses, &g.n14, &g.T, &g.n_terms) != 5) return 2;
    const uint32_t W = 3;
    const size_t state_bytes = 1248;      // (any multiple of 8: the layouts take it as a parameter)
    std::vector<size_t> pstart;
    std::vector<GuestChunk> chunks;
    std::vector<GuestSlot> slots;
    guest_plan(ligs, pstart, chunks);
    size_t largest = 0;
    std::string lines;
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
        const GuestChunk& c = chunks[ci];
        // the four older modes, field by field
        for (int mode = GUEST_ROWS; mode <= GUEST_FLEX; ++mode) {
            const size_t sb = mode == GUEST_FLEX ? state_bytes : mode == GUEST_REFINE ? 328u : 0u;
            const GuestFlexSums fx = mode == GUEST_FLEX ? c.fx : GuestFlexSums();
            const GuestLayout l(c.n, c.atoms, c.n14, c.nxyz, c.ncls, W, mode, sb, fx);
            const Before b(c.n, c.atoms, c.n14, c.nxyz, c.ncls, W, mode, sb, fx);
            const size_t mine[] = {l.rec, l.ligof, l.q, l.lj, l.p14, l.xyz, l.cls, l.frec, l.tor, l.dih, l.aoff, l.aent, l.up_end, l.slab, l.rows,
                                   l.fslab, l.fout, l.rigid, l.step, l.end};
            const size_t was[] = {b.rec, b.ligof, b.q, b.lj, b.p14, b.xyz, b.cls, b.frec, b.tor, b.dih, b.aoff, b.aent, b.up_end, b.slab, b.rows,
                                  b.fslab, b.fout, b.rigid, b.step, b.end};
            for (size_t k = 0; k < sizeof(mine) / sizeof(mine[0]); ++k)
                if (mine[k] != was[k]) return fail("an older mode's layout moved (mode " + std::to_string(mode) + ")", ci, k);
            if (l.search != l.end) return fail("an older mode has a search block", ci, (size_t)mode);
        }
        // GUEST_SEARCH: GUEST_FLEX, then the search block
        const GuestLayout flex(c.n, c.atoms, c.n14, c.nxyz, c.ncls, W, GUEST_FLEX, state_bytes, c.fx);
        const GuestLayout lay(c.n, c.atoms, c.n14, c.nxyz, c.ncls, W, GUEST_SEARCH, state_bytes, c.fx);
        const size_t a[] = {lay.rec, lay.ligof, lay.q, lay.lj, lay.p14, lay.xyz, lay.cls, lay.frec, lay.tor, lay.dih, lay.aoff, lay.aent, lay.up_end,
                            lay.slab, lay.rows, lay.fslab, lay.fout, lay.rigid, lay.step};
        const size_t f[] = {flex.rec, flex.ligof, flex.q, flex.lj, flex.p14, flex.xyz, flex.cls, flex.frec, flex.tor, flex.dih, flex.aoff, flex.aent,
                            flex.up_end, flex.slab, flex.rows, flex.fslab, flex.fout, flex.rigid, flex.step};
        for (size_t k = 0; k < sizeof(a) / sizeof(a[0]); ++k)
            if (a[k] != f[k]) return fail("the search mode moves a part of the flexible one", ci, k);
        const StepLayout sl = StepLayout::guest(c.n, c.nxyz, W, state_bytes, c.fx.terms);
        const SearchLayout ss = SearchLayout::guest(c.n, c.nxyz, W);
        if (lay.search % 16u) return fail("the search block is not 16-byte aligned", ci, 0);
        if (lay.search < lay.step + sl.end) return fail("the search block overlaps the step block", ci, 0);
        if (lay.end != lay.search + ss.end) return fail("the block does not end where the search block does", ci, 0);
        largest = std::max(largest, lay.end);
        const size_t off[] = {ss.rec, ss.best_y, ss.best_row, ss.best_rigid, ss.cur_y, ss.streams, ss.end};
        const size_t len[] = {SEARCH_REC_BYTES * (size_t)c.n, 4u * c.nxyz, 4u * (size_t)W * c.n, 24u * (size_t)c.n, 4u * c.nxyz, 8u * (size_t)c.n};
        if (ss.rec != 0) return fail("the records do not open the search block", ci, 0);
        for (int k = 0; k < 6; ++k) {
            if (off[k] % 16u) return fail("a part of the search block is not 16-byte aligned", ci, (size_t)k);
            if (off[k] + len[k] > off[k + 1]) return fail("parts of the search block overlap", ci, (size_t)k);
        }
        // the resident form is the same struct: n walkers of per_pose floats each
        if (c.nxyz % c.n == 0) {
            const SearchLayout r(c.n, c.nxyz / c.n, W);
            if (r.rec != ss.rec || r.best_y != ss.best_y || r.best_row != ss.best_row || r.best_rigid != ss.best_rigid || r.cur_y != ss.cur_y ||
                r.streams != ss.streams || r.end != ss.end)
                return fail("the resident and the guest form of SearchLayout differ", ci, 0);
        }
        // every walker writes its stretch of best / current coordinates, its row, rigid, record and stream id into buffers of exactly the
        // parts' sizes (the sanitizer watches their ends): the stretch is its PoseRec's, and no two walkers share a float
        std::vector<PoseRec> rec(c.n, PoseRec{~0u, ~0u, ~0u, ~0u, ~0u, ~0u});
        std::vector<uint32_t> ligof(2u * c.n, ~0u);
        guest_slots(ligs, pstart, c, slots);
        guest_records(ligs, slots, rec.data(), ligof.data());
        std::vector<unsigned char> recs(len[0], 0), rows(len[2], 0), rigid(len[3], 0), ids(len[5], 0);
        std::vector<float> best(c.nxyz, 0.f), cur(c.nxyz, 0.f);
        std::vector<std::pair<size_t, size_t>> stretch;
        for (uint32_t p = 0; p < c.n; ++p) {
            const PoseRec& r = rec[p];
            if (r.count == ~0u) return fail("a walker without a record", ci, p);
            if (ligs[ligof[2u * p]].count != r.count) return fail("a walker's record is not its ligand's", ci, p);
            if ((size_t)r.xyz + 3u * (size_t)r.count > c.nxyz) return fail("a walker's coordinates leave the chunk's", ci, p);
            stretch.push_back({r.xyz, (size_t)r.xyz + 3u * r.count});
            for (uint32_t i = 0; i < 3u * r.count; ++i) { best[r.xyz + i] += 1.f; cur[r.xyz + i] += 1.f; }
            for (uint32_t i = 0; i < SEARCH_REC_BYTES; ++i) recs[(size_t)p * SEARCH_REC_BYTES + i]++;
            for (uint32_t i = 0; i < 4u * W; ++i) rows[(size_t)p * 4u * W + i]++;
            for (uint32_t i = 0; i < 24u; ++i) rigid[(size_t)p * 24u + i]++;
            for (uint32_t i = 0; i < 8u; ++i) ids[(size_t)p * 8u + i]++;
        }
        std::sort(stretch.begin(), stretch.end());
        size_t at = 0;
        for (const auto& s : stretch) {
            if (s.first != at) return fail("the walkers' stretches do not tile the coordinates", ci, s.first);
            at = s.second;
        }
        if (at != c.nxyz) return fail("the walkers' stretches do not sum to the chunk's coordinates", ci, at);
        for (size_t k = 0; k < c.nxyz; ++k)
            if (best[k] != 1.f || cur[k] != 1.f) return fail("a coordinate of the search block is written twice or never", ci, k);
        for (unsigned char v : recs) if (v != 1) return fail("a record byte is written twice or never", ci, 0);
        for (unsigned char v : rows) if (v != 1) return fail("a row byte is written twice or never", ci, 0);
        for (unsigned char v : rigid) if (v != 1) return fail("a rigid byte is written twice or never", ci, 0);
        for (unsigned char v : ids) if (v != 1) return fail("a stream id byte is written twice or never", ci, 0);
        lines += "chunk " + std::to_string(ci) + " walkers " + std::to_string(c.n) + " search " + std::to_string(lay.search) + " " + std::to_string(ss.end) + "\n";
    }
    std::printf("ok %zu %zu %zu\n%s", chunks.size(), pstart[M], largest, lines.c_str());
    return 0;
}
