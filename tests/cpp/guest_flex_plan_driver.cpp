// The flexible additions to the chunk planner of the guest-ligand calls (molchanica_amd/csrc/mdx_pose_plan.h) on one host thread, for
// tests/test_guest_flex_host.py: built plain and with the address and undefined-behaviour sanitizers.  stdin: the number of ligands,
// then per ligand "count n_poses n14 T n_terms".  It plans the library in GUEST_FLEX mode, lays out every chunk, writes the records
// into buffers of exactly the staged size and checks what guest_flex_step_kernel relies on; the first violated condition is printed
// and the exit status is 1.  stdout: "ok <chunks> <poses> <largest block>", then per chunk "chunk <i> ligands <m> <m> ...".
#include "mdx_pose_plan.h"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>

static int fail(const std::string& what, size_t chunk, size_t at) {
    std::printf("FAIL chunk %zu at %zu: %s\n", chunk, at, what.c_str());
    return 1;
}

// [lo, hi) byte intervals must not overlap
static bool disjoint(std::vector<std::pair<size_t, size_t>> v) {
    std::sort(v.begin(), v.end());
    for (size_t k = 0; k + 1 < v.size(); ++k)
        if (v[k].second > v[k + 1].first) return false;
    return true;
}

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
        const GuestLayout lay(c.n, c.atoms, c.n14, c.nxyz, c.ncls, W, GUEST_FLEX, state_bytes, c.fx);
        const GuestLayout rigid(c.n, c.atoms, c.n14, c.nxyz, c.ncls, W, GUEST_REFINE, state_bytes);
        largest = std::max(largest, lay.end);
        // the staged part: what the rigid refinement stages lies where it did; the flexible tables behind it, ascending, 16-byte aligned
        if (lay.rec != rigid.rec || lay.ligof != rigid.ligof || lay.q != rigid.q || lay.lj != rigid.lj || lay.p14 != rigid.p14 ||
            lay.xyz != rigid.xyz || lay.cls != rigid.cls)
            return fail("the flexible mode moves a table of the rigid one", ci, 0);
        if (rigid.up_end != rigid.cls + c.ncls || rigid.frec != rigid.up_end) return fail("the rigid mode stages flexible tables", ci, 0);
        const size_t off[] = {lay.frec, lay.tor, lay.dih, lay.aoff, lay.aent, lay.up_end};
        const size_t len[] = {sizeof(FlexRec) * c.n, GUEST_TOR_BYTES * c.fx.tor, GUEST_DIH_BYTES * c.fx.dih, 4u * c.fx.aoff, 16u * c.fx.dih};
        if (lay.frec < lay.cls + c.ncls) return fail("the flexible records overlap the class maps", ci, 0);
        for (int k = 0; k < 5; ++k) {
            if (off[k] % 16u) return fail("a flexible table is not 16-byte aligned", ci, (size_t)k);
            if (off[k] + len[k] > off[k + 1]) return fail("flexible tables overlap", ci, (size_t)k);
        }
        if (lay.slab % 16u || lay.slab < lay.up_end) return fail("the slab overlaps the staged part", ci, 0);
        const StepLayout sl = StepLayout::guest(c.n, c.nxyz, W, state_bytes, c.fx.terms);
        if (sl.eterm % 16u || sl.eterm < sl.x0 + 4u * c.nxyz || sl.end != sl.eterm + 8u * FLEX_TERM_WORDS * c.fx.terms)
            return fail("eterm does not close the step block", ci, 0);
        if (lay.step % 16u || lay.end != lay.step + sl.end) return fail("the block does not end where eterm does", ci, 0);
        // the records, written into buffers of exactly the staged size (the sanitizer watches their ends)
        std::vector<PoseRec> rec(c.n, PoseRec{~0u, ~0u, ~0u, ~0u, ~0u, ~0u});
        std::vector<uint32_t> ligof(2u * c.n, ~0u);
        std::vector<FlexRec> frec(c.n, FlexRec{~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u});
        guest_slots(ligs, pstart, c, slots);
        guest_records(ligs, slots, rec.data(), ligof.data());
        guest_flex_records(ligs, slots, frec.data());
        // per ligand with poses in the chunk: its four tables disjoint from every other ligand's, each starting on 16 bytes
        std::vector<std::pair<size_t, size_t>> tor, dih, aoff, aent;
        lines += "chunk " + std::to_string(ci) + " ligands";
        for (const GuestSlot& s : slots) {
            const GuestShape& g = ligs[s.m];
            lines += " " + std::to_string(s.m);
            const size_t t0 = lay.tor + (size_t)GUEST_TOR_BYTES * s.tor, d0 = lay.dih + (size_t)GUEST_DIH_BYTES * s.dih,
                         a0 = lay.aoff + 4u * (size_t)s.aoff, e0 = lay.aent + 16u * (size_t)s.dih;
            if (t0 % 16u || d0 % 16u || a0 % 16u || e0 % 16u) return fail("a ligand's table does not start on 16 bytes", ci, s.m);
            tor.push_back({t0, t0 + (size_t)GUEST_TOR_BYTES * g.T}); dih.push_back({d0, d0 + (size_t)GUEST_DIH_BYTES * g.n_terms});
            aoff.push_back({a0, a0 + 4u * ((size_t)g.count + 1u)}); aent.push_back({e0, e0 + 16u * (size_t)g.n_terms});
            if (tor.back().second > lay.dih || dih.back().second > lay.aoff || aoff.back().second > lay.aent || aent.back().second > lay.up_end)
                return fail("a ligand's table leaves its part of the block", ci, s.m);
        }
        lines += "\n";
        if (!disjoint(tor) || !disjoint(dih) || !disjoint(aoff) || !disjoint(aent)) return fail("two ligands' tables overlap", ci, 0);
        // per pose: the record is its ligand's, and its stretch of eterm is its own; the stretches tile [0, terms)
        std::vector<std::pair<size_t, size_t>> et;
        size_t terms = 0;
        for (uint32_t p = 0; p < c.n; ++p) {
            const uint32_t m = ligof[2u * p];
            if (m >= M) return fail("a pose without a record", ci, p);
            const GuestShape& g = ligs[m];
            const FlexRec& f = frec[p];
            const GuestSlot* mine = nullptr;
            for (const GuestSlot& s : slots)
                if (s.m == m) mine = &s;
            if (!mine) return fail("a pose of a ligand without a slot", ci, p);
            if (f.T != g.T || f.n_terms != g.n_terms || f.pad != 0u) return fail("a flexible record's sizes are not its ligand's", ci, p);
            if (f.tor != mine->tor || f.dih != mine->dih || f.aoff != mine->aoff || f.aent != 4u * mine->dih)
                return fail("a flexible record does not point at its ligand's tables", ci, p);
            if ((size_t)f.eterm + f.n_terms > c.fx.terms) return fail("a pose's terms leave eterm", ci, p);
            et.push_back({f.eterm, (size_t)f.eterm + f.n_terms});
            terms += f.n_terms;
        }
        if (!disjoint(et)) return fail("two poses share a stretch of eterm", ci, 0);
        if (terms != c.fx.terms) return fail("the poses' terms do not sum to the chunk's", ci, 0);
    }
    std::printf("ok %zu %zu %zu\n%s", chunks.size(), pstart[M], largest, lines.c_str());
    return 0;
}
