// mdx_set_solute_copies / mdx_solubility_mixing / mdx_snapshot_read_solubility: the solubility mixing diagnostics of the resident state
// (include/mdx.h states the rule; mdx_mixing_rule.h is its arithmetic, shared with stand-alone host programs).  The handle's positions
// are read where they lie; nothing of its state is written.  One call enqueues everything and waits once.
//
//   mx_gather_kernel   one thread per gathered atom: the selected atoms of every copy as float4 {x, y, z, copy id}, copy by copy, then -
//                      from the next multiple of MX_TILE on, so that no tile mixes the two kinds - the water oxygens tagged MDX_MX_WATER.
//                      Positions come through the index map mdx_download uses (slot order while the step loop owns the state).  A
//                      non-finite coordinate sets the one flag word.
//   mx_pair_kernel     the hot path: one row (selected solute atom) per thread, 256 rows per workgroup, the partners staged through LDS
//                      in tiles of MX_TILE; blockIdx.y walks one slab of the partner range.  Per pair one d2 and three v_exp_f32 (the
//                      factors -log2(e) / 2 sigma^2 are kernel arguments: SGPRs), six fp64 accumulators per row.  A solute partner of
//                      another copy within the cutoff sets bit (own copy, partner copy) by a vector atomicOr.  Every (slab, row) stores
//                      its six partial sums.
//   mx_reduce_kernel   adds the slabs in slab order: no floating-point atomics anywhere, the same state gives the same bits.
// The tail (scores, union-find over the bit matrix, centres, dispersion, scalars) is mx_tail of the rule header, on the host, from one
// read-back of the flag, the sums, the bit matrix and the gathered solute atoms.
#include "mdx_internal.h"
#include "mdx_mixing_rule.h"
#include <cmath>
#include <cstring>

#define FAIL(code, msg) do { mdx_set_error(msg); return (code); } while (0)

#define MX_ROWS 256u      // rows per workgroup
#define MX_TILE 256u      // partners staged per step: 4 KiB of LDS, occupancy is bounded by registers, not by LDS
#define MX_GRID_TARGET 1024u      // workgroups the slabs aim at: four per compute unit
#define MX_SLAB_MIN_TILES 2u      // ... but a slab is never shorter than this: 131 k pairs per workgroup

struct MxGatherArgs {
    const float4* src;             // slot order (slot_of != nullptr) or caller order
    const uint32_t* gid; const uint32_t* slot_of;
    const uint32_t* sel;           // [n_sel] indices inside a copy
    uint32_t first, apc, n_sel, n_rows, row_pad, water_first, water_sites, n_waters;
    float4* g;                     // [row_pad + n_waters]
    uint32_t* flag;
};

__global__ __launch_bounds__(256) void mx_gather_kernel(MxGatherArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n_rows + a.n_waters) return;
    uint32_t atom, dst, tag;
    if (i < a.n_rows) {
        tag = i / a.n_sel;
        atom = a.first + tag * a.apc + a.sel[i - tag * a.n_sel];
        dst = i;
    } else {
        tag = MDX_MX_WATER;
        atom = a.water_first + (i - a.n_rows) * a.water_sites;
        dst = a.row_pad + (i - a.n_rows);
    }
    const float4 x = a.src[a.slot_of ? a.slot_of[a.gid[atom]] : atom];
    if (!(isfinite(x.x) && isfinite(x.y) && isfinite(x.z))) atomicOr(a.flag, 1u);
    a.g[dst] = make_float4(x.x, x.y, x.z, __uint_as_float(tag));
}

struct MxPairArgs {
    const float4* g;
    uint32_t n_rows, row_pad, n_end, n_tiles, tiles_per_slab, w32;
    mx_params p;
    uint32_t* bits;                // [n_copies][w32]
    double* part;                  // [n_slabs][n_rows][6]
};

__global__ __launch_bounds__(256) void mx_pair_kernel(MxPairArgs a) {
    __shared__ float4 s_t[MX_TILE];
    const uint32_t tid = threadIdx.x, row = blockIdx.x * MX_ROWS + tid;
    const bool valid = row < a.n_rows;
    const float4 me = a.g[valid ? row : a.n_rows - 1u];      // (a tail row: computed, never written)
    const uint32_t own = __float_as_uint(me.w);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, w0 = 0.0, w1 = 0.0, w2 = 0.0;
    uint32_t last = MDX_MX_WATER;                             // the partner copy whose bit this row set last
    const uint32_t t0 = blockIdx.y * a.tiles_per_slab, t1 = min(t0 + a.tiles_per_slab, a.n_tiles);
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t j0 = t * MX_TILE;
        const bool water = j0 >= a.row_pad;                   // uniform: a tile holds one kind
        const uint32_t kc = min(MX_TILE, (water ? a.n_end : a.n_rows) - j0);
        __syncthreads();      // the reads of the tile before are done
        if (tid < kc) s_t[tid] = a.g[j0 + tid];
        __syncthreads();
        if (water) {
            for (uint32_t j = 0; j < kc; ++j) {
                const float4 b = s_t[j];
                const float d2 = mx_d2(me.x, me.y, me.z, b.x, b.y, b.z, a.p);
                w0 += (double)mx_weight(d2, a.p.k2[0]);
                w1 += (double)mx_weight(d2, a.p.k2[1]);
                w2 += (double)mx_weight(d2, a.p.k2[2]);
            }
        } else {
            for (uint32_t j = 0; j < kc; ++j) {
                const float4 b = s_t[j];
                const uint32_t pc = __float_as_uint(b.w);
                const bool other = pc != own;
                const float d2 = mx_d2(me.x, me.y, me.z, b.x, b.y, b.z, a.p);
                s0 += other ? (double)mx_weight(d2, a.p.k2[0]) : 0.0;
                s1 += other ? (double)mx_weight(d2, a.p.k2[1]) : 0.0;
                s2 += other ? (double)mx_weight(d2, a.p.k2[2]) : 0.0;
                if (valid && other && d2 <= a.p.cut2 && pc != last) {
                    atomicOr(&a.bits[(size_t)own * a.w32 + (pc >> 5)], 1u << (pc & 31u));
                    last = pc;
                }
            }
        }
    }
    if (valid) {
        double* o = a.part + ((size_t)blockIdx.y * a.n_rows + row) * 6u;
        o[0] = s0; o[1] = w0; o[2] = s1; o[3] = w1; o[4] = s2; o[5] = w2;
    }
}

__global__ __launch_bounds__(256) void mx_reduce_kernel(const double* __restrict__ part, uint32_t n_slabs, uint32_t n_vals, double* __restrict__ sums) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_vals) return;
    double s = 0.0;
    for (uint32_t k = 0; k < n_slabs; ++k) s += part[(size_t)k * n_vals + i];
    sums[i] = s;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// the block of one call in mx_blk: byte offsets, every part 256-byte aligned; [flag, sums, bits, g rows] is read back in one copy
struct MxLayout {
    size_t sel, part, flag, sums, bits, g, g_rows_end, end;
    MxLayout(uint32_t n_sel, uint32_t n_rows, uint32_t row_pad, uint32_t n_waters, uint32_t n_copies, uint32_t w32, uint32_t n_slabs) {
        size_t o = 0;
        auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255u) & ~(size_t)255u; return at; };
        sel = take(sizeof(uint32_t) * n_sel);
        part = take(sizeof(double) * 6 * (size_t)n_rows * n_slabs);
        flag = take(sizeof(uint32_t));
        sums = take(sizeof(double) * 6 * (size_t)n_rows);
        bits = take(sizeof(uint32_t) * (size_t)n_copies * w32);
        g = take(sizeof(float4) * ((size_t)row_pad + n_waters));
        g_rows_end = g + sizeof(float4) * (size_t)n_rows;
        end = o;
    }
};

// what a layout is refused for; the same list at mdx_set_solute_copies and at every evaluation (the water layout and the box can change
// in between)
static int mx_check(const mdx_handle* h, uint32_t first, uint32_t n_copies, uint32_t apc) {
    if (h->dd || h->n_local != h->N) FAIL(MDX_EPARAM, "solubility mixing on a decomposed handle (single-device handles only)");
    if (!(h->per[0] && h->per[1] && h->per[2])) FAIL(MDX_EPARAM, "solubility mixing on a non-periodic handle: the score needs a cell");
    if (!n_copies) FAIL(MDX_EPARAM, "no solute layout set (mdx_set_solute_copies)");
    if (!h->n_waters) FAIL(MDX_EPARAM, "no water layout set (mdx_set_water_layout): the waters of the score are its oxygens");
    const uint64_t s0 = first, s1 = (uint64_t)first + (uint64_t)n_copies * apc;
    const uint64_t w0 = h->water_first, w1 = w0 + (uint64_t)h->n_waters * h->water_sites;
    if (s1 > h->N) FAIL(MDX_EPARAM, "solute copies reach beyond the atom array");
    if (s0 < w1 && w0 < s1) FAIL(MDX_EPARAM, "the solute range overlaps the water range");
    return MDX_OK;
}

extern "C" int mdx_set_solute_copies(mdx_handle* h, uint32_t first_atom, uint32_t n_copies, uint32_t atoms_per_copy, const uint32_t* sel,
                                     uint32_t n_sel) {
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (n_copies == 0) { h->mx_first = h->mx_copies = h->mx_apc = 0; h->mx_sel.clear(); return MDX_OK; }
    if (n_copies > MDX_MX_MAX_COPIES) FAIL(MDX_EPARAM, "more than MDX_SOLUTE_MAX_COPIES (4096) solute copies");
    if (atoms_per_copy == 0) FAIL(MDX_EPARAM, "atoms_per_copy must be positive");
    MDX_TRY(mx_check(h, first_atom, n_copies, atoms_per_copy));
    if (n_sel > 0 && !sel) FAIL(MDX_EPARAM, "null sel with n_sel > 0");
    std::vector<uint32_t> s;
    if (n_sel == 0) {
        s.resize(atoms_per_copy);
        for (uint32_t k = 0; k < atoms_per_copy; ++k) s[k] = k;
    } else {
        std::vector<uint8_t> seen(atoms_per_copy, 0);
        for (uint32_t k = 0; k < n_sel; ++k) {
            if (sel[k] >= atoms_per_copy) FAIL(MDX_EPARAM, "sel[" + std::to_string(k) + "] is not an index inside a copy (>= atoms_per_copy)");
            if (seen[sel[k]]) FAIL(MDX_EPARAM, "sel[" + std::to_string(k) + "] repeats an index");
            seen[sel[k]] = 1;
        }
        s.assign(sel, sel + n_sel);
    }
    h->mx_first = first_atom; h->mx_copies = n_copies; h->mx_apc = atoms_per_copy; h->mx_sel = std::move(s);
    return MDX_OK;
}

bool mdx_mixing_on(const mdx_handle* h) {
    if (!h->mx_copies || !h->n_waters || h->dd || h->n_local != h->N || !(h->per[0] && h->per[1] && h->per[2])) return false;
    const uint64_t s0 = h->mx_first, s1 = s0 + (uint64_t)h->mx_copies * h->mx_apc, w0 = h->water_first, w1 = w0 + (uint64_t)h->n_waters * h->water_sites;
    return s1 <= h->N && !(s0 < w1 && w0 < s1);
}

int mdx_mixing_evaluate(mdx_handle* h, mdx_solubility* out, double* atom_sums) {
    MDX_TRY(mx_check(h, h->mx_first, h->mx_copies, h->mx_apc));
    HIP_TRY(hipSetDevice(h->device));
    const uint32_t n_copies = h->mx_copies, n_sel = (uint32_t)h->mx_sel.size(), n_rows = n_copies * n_sel, n_waters = h->n_waters;
    const uint32_t row_pad = (n_rows + MX_TILE - 1u) / MX_TILE * MX_TILE, n_end = row_pad + n_waters;
    const uint32_t n_tiles = (n_end + MX_TILE - 1u) / MX_TILE, row_blocks = (n_rows + MX_ROWS - 1u) / MX_ROWS;
    const uint32_t want_slabs = std::min(n_tiles, std::max(1u, (MX_GRID_TARGET + row_blocks - 1u) / row_blocks));
    const uint32_t tiles_per_slab = std::max(MX_SLAB_MIN_TILES, (n_tiles + want_slabs - 1u) / want_slabs), n_slabs = (n_tiles + tiles_per_slab - 1u) / tiles_per_slab;
    const uint32_t w32 = (n_copies + 31u) / 32u;
    const MxLayout lay(n_sel, n_rows, row_pad, n_waters, n_copies, w32, n_slabs);
    DeviceState& d = h->d;
    hipStream_t st = h->stream;
    if (h->mx_cap < lay.end) {
        if (d.mx_blk) { HIP_TRY(hipStreamSynchronize(st)); (void)hipFree(d.mx_blk); d.mx_blk = nullptr; }
        h->mx_cap = 0;
        HIP_TRY(hipMalloc(&d.mx_blk, lay.end));
        h->mx_cap = lay.end;
    }
    unsigned char* b0 = (unsigned char*)d.mx_blk;
    mx_params p;
    mx_setup(h->box_lo, h->box_hi, p);
    HIP_TRY(hipMemcpyAsync(b0 + lay.sel, h->mx_sel.data(), sizeof(uint32_t) * n_sel, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(b0 + lay.flag, 0, lay.g - lay.flag, st));      // the flag word and the bit matrix (the sums between them are overwritten)
    const bool slots = h->in_slot_space;
    MxGatherArgs ga{slots ? d.posq : d.pos_orig, slots ? d.gid : nullptr, slots ? d.slot_of : nullptr, (const uint32_t*)(b0 + lay.sel),
                    h->mx_first, h->mx_apc, n_sel, n_rows, row_pad, h->water_first, h->water_sites, n_waters, (float4*)(b0 + lay.g),
                    (uint32_t*)(b0 + lay.flag)};
    mdx_prof_begin(h, 1);
    hipLaunchKernelGGL(mx_gather_kernel, dim3((n_rows + n_waters + 255u) / 256u), dim3(256), 0, st, ga);
    mdx_prof_end(h);
    MxPairArgs pa{(const float4*)(b0 + lay.g), n_rows, row_pad, n_end, n_tiles, tiles_per_slab, w32, p, (uint32_t*)(b0 + lay.bits), (double*)(b0 + lay.part)};
    mdx_prof_begin(h, 0);
    hipLaunchKernelGGL(mx_pair_kernel, dim3(row_blocks, n_slabs), dim3(MX_ROWS), 0, st, pa);
    mdx_prof_end(h);
    mdx_prof_begin(h, 2);
    hipLaunchKernelGGL(mx_reduce_kernel, dim3((6u * n_rows + 255u) / 256u), dim3(256), 0, st, (const double*)(b0 + lay.part), n_slabs, 6u * n_rows,
                       (double*)(b0 + lay.sums));
    mdx_prof_end(h);
    HIP_TRY(hipGetLastError());
    std::vector<unsigned char> back(lay.g_rows_end - lay.flag);
    HIP_TRY(hipMemcpyAsync(back.data(), b0 + lay.flag, back.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    auto at = [&](size_t off) { return back.data() + (off - lay.flag); };
    uint32_t flag = 0;
    std::memcpy(&flag, at(lay.flag), sizeof(flag));
    if (flag) FAIL(MDX_ENAN, "non-finite coordinate among the solute copies or the water oxygens (mdx_solubility_mixing)");
    const double* sums = (const double*)at(lay.sums);
    float f[10];
    mx_tail(n_copies, n_sel, n_waters, (const float*)at(lay.g), sums, (const uint32_t*)at(lay.bits), w32, p, f);
    std::memcpy(out, f, sizeof(f));
    if (atom_sums) std::memcpy(atom_sums, sums, sizeof(double) * 6 * (size_t)n_rows);
    return MDX_OK;
}

extern "C" int mdx_solubility_mixing(mdx_handle* h, mdx_solubility* out, double* atom_sums_or_null) {
    if (!h || !out) FAIL(MDX_EPARAM, "null argument");
    return mdx_mixing_evaluate(h, out, atom_sums_or_null);
}

extern "C" int mdx_snapshot_read_solubility(mdx_handle* h, uint32_t k, mdx_solubility* out) {
    if (!h || !out) FAIL(MDX_EPARAM, "null argument");
    if (k >= h->snapshots.size()) FAIL(MDX_EPARAM, "snapshot index out of range");
    const auto& sn = h->snapshots[k];
    if (sn.solubility.empty()) FAIL(MDX_EPARAM, "the snapshot was taken without a solute layout (mdx_set_solute_copies)");
    *out = sn.solubility[0];
    return MDX_OK;
}
