// mdx_pose_rmsd / mdx_cluster_poses: the symmetry-aware distance of pose pairs and the greedy leader clustering of a pose batch by it
// (include/mdx.h states the rule; mdx_cluster_rule.h is its arithmetic, shared with stand-alone host programs).  The handle gives its
// device, stream, box and scratch; nothing of its state is read or written.  One call enqueues everything and waits once.
//
//   cl_gather_kernel   one thread per pose: the masked atoms of pose order[r] into the fp32 layout [masked atom][xyz][pose] (the lanes
//                      of a wave walk over poses, so every later read is contiguous) and the pose's fp64 centroid.
//   cl_tile_kernel     the hot path: 256 threads own 64 x 64 pose pairs, 4 x 4 per thread, fp64 accumulators in registers.  The atoms
//                      are walked in the rule's order in chunks of CL_CHUNK staged in LDS, the permuted side staged anew per perm,
//                      the perms in the outer loop with the minimum.  One body, two epilogues: BITS = false writes fp32 rmsd for
//                      every tile (mdx_pose_rmsd); BITS = true runs the lower triangle in rank order and writes one bit per pair,
//                      D <= T, into the N x N-bit matrix.  PERIODIC = false leaves the image shift out: s = 0 changes a difference by
//                      the sign of a zero at most, which its square does not see.
//   cl_scan_kernel     one workgroup resolves the leaders from the bit matrix, 64 ranks per step: the 64 rows against the leaders
//                      already known in parallel (16 threads per row), then the 64 x 64 block inside wave 0 with ballots.
//   cl_assign_kernel   one thread per pose: D(leader, pose) by the rule again, rmsd_to_leader, and the cluster sizes by vector atomics.
#include "mdx_internal.h"
#include "mdx_cluster_rule.h"
#include <cmath>
#include <cstring>
#include <numeric>

#define FAIL(code, msg) do { mdx_set_error(msg); return (code); } while (0)

#define CL_TILE 64u       // poses per tile side
#define CL_CHUNK 32u      // masked atoms staged per step: 2 sides x 32 x 3 x 64 fp32 = 48 KiB of LDS, three workgroups per CU

typedef unsigned long long cl_u64;

struct ClGatherArgs {
    const float* poses;        // [n][count][3], caller order
    const uint32_t* order;     // [n] rank -> caller index (nullptr: the identity)
    const uint32_t* atoms;     // [n_m] the masked atoms in atom order
    float* g;                  // [n_m][3][n]
    double* c;                 // [n][3]
    uint32_t n, count, n_m;
};

struct ClGView {               // pose r of a gathered batch, as the rule's functions index it
    const float* g; uint32_t n, r;
    __device__ float operator()(uint32_t k, uint32_t axis) const { return g[(size_t)(3u * k + axis) * n + r]; }
};

__global__ __launch_bounds__(256) void cl_gather_kernel(ClGatherArgs a) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.n) return;
    const float* p = a.poses + 3 * (size_t)a.count * (a.order ? a.order[r] : r);
    for (uint32_t k = 0; k < a.n_m; ++k) {
        const float* x = p + 3u * a.atoms[k];
        for (uint32_t axis = 0; axis < 3u; ++axis) a.g[(size_t)(3u * k + axis) * a.n + r] = x[axis];
    }
    double c[3];
    cl_centroid(ClGView{a.g, a.n, r}, a.n_m, c);      // (this thread's own stores)
    for (int d = 0; d < 3; ++d) a.c[3 * (size_t)r + d] = c[d];
}

struct ClTileArgs {
    const float* ga; const float* gb;      // [n_m][3][na], [n_m][3][nb]
    const double* ca; const double* cb;    // centroids
    const uint16_t* perms;                 // [n_perms][n_m], masked-atom index space
    uint32_t na, nb, n_m, n_perms;
    double L[3], T;
    float* out;                            // BITS = false: [na][nb]
    cl_u64* bits;                          // BITS = true: [na][w64]
    uint32_t w64;
};

template <bool PERIODIC, bool BITS>
__global__ __launch_bounds__(256) void cl_tile_kernel(ClTileArgs a) {
    __shared__ __attribute__((aligned(16))) float s_a[CL_CHUNK * 3u][CL_TILE];
    __shared__ __attribute__((aligned(16))) float s_b[CL_CHUNK * 3u][CL_TILE];
    __shared__ uint32_t s_bits[CL_TILE][2];
    const uint32_t ti = blockIdx.y, tj = blockIdx.x;
    if (BITS && tj > ti) return;      // the lower triangle in rank order (uniform over the workgroup, before any barrier)
    const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
    const uint32_t i0 = ti * CL_TILE, j0 = tj * CL_TILE;
    if (BITS && tid < 2u * CL_TILE) s_bits[tid >> 1][tid & 1u] = 0u;
    double s[PERIODIC ? 16 : 1][3];
    if (PERIODIC) {
#pragma unroll
        for (uint32_t ii = 0; ii < 4u; ++ii)
#pragma unroll
            for (uint32_t jj = 0; jj < 4u; ++jj) {
                const uint32_t i = min(i0 + 4u * ty + ii, a.na - 1u), j = min(j0 + 4u * tx + jj, a.nb - 1u);      // (a tail pair: computed, never written)
                for (int d = 0; d < 3; ++d) s[PERIODIC ? 4u * ii + jj : 0u][d] = cl_shift(a.ca[3 * (size_t)i + d], a.cb[3 * (size_t)j + d], a.L[d]);
            }
    }
    double best[4][4];
    const uint32_t nq = a.n_perms ? a.n_perms : 1u;
    for (uint32_t q = 0; q < nq; ++q) {
        double acc[4][4];
        for (int ii = 0; ii < 4; ++ii)
            for (int jj = 0; jj < 4; ++jj) acc[ii][jj] = 0.0;
        for (uint32_t k0 = 0; k0 < a.n_m; k0 += CL_CHUNK) {
            const uint32_t kc = min(CL_CHUNK, a.n_m - k0);
            __syncthreads();      // the reads of the chunk before are done
            for (uint32_t e = tid; e < kc * 3u * CL_TILE; e += 256u) {
                const uint32_t row = e >> 6, col = e & 63u, k = k0 + row / 3u, axis = row % 3u;
                if (q == 0u || a.n_m > CL_CHUNK)      // (a single chunk: the row side stays as perm 0 staged it)
                    s_a[row][col] = i0 + col < a.na ? a.ga[(size_t)(3u * k + axis) * a.na + i0 + col] : 0.f;
                const uint32_t pk = a.n_perms ? (uint32_t)a.perms[(size_t)q * a.n_m + k] : k;
                s_b[row][col] = j0 + col < a.nb ? a.gb[(size_t)(3u * pk + axis) * a.nb + j0 + col] : 0.f;
            }
            __syncthreads();
            for (uint32_t kl = 0; kl < kc; ++kl) {      // atom order, then x, y, z
#pragma unroll
                for (int axis = 0; axis < 3; ++axis) {
                    const float4 av = *(const float4*)&s_a[3u * kl + axis][4u * ty], bv = *(const float4*)&s_b[3u * kl + axis][4u * tx];
                    const float af[4] = {av.x, av.y, av.z, av.w}, bf[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                    for (int ii = 0; ii < 4; ++ii)
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj)
                            acc[ii][jj] = PERIODIC ? cl_term(acc[ii][jj], af[ii], bf[jj], s[PERIODIC ? 4 * ii + jj : 0][axis])
                                                   : cl_term0(acc[ii][jj], af[ii], bf[jj]);
                }
            }
        }
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) best[ii][jj] = (q == 0u || acc[ii][jj] < best[ii][jj]) ? acc[ii][jj] : best[ii][jj];
    }
#pragma unroll
    for (uint32_t ii = 0; ii < 4u; ++ii)
#pragma unroll
        for (uint32_t jj = 0; jj < 4u; ++jj) {
            const uint32_t ri = 4u * ty + ii, cj = 4u * tx + jj, i = i0 + ri, j = j0 + cj;
            if (BITS) {
                if (i < a.na && j < i && best[ii][jj] <= a.T) atomicOr(&s_bits[ri][cj >> 5], 1u << (cj & 31u));
            } else if (i < a.na && j < a.nb) {
                a.out[(size_t)i * a.nb + j] = cl_rmsd(best[ii][jj], a.n_m);
            }
        }
    if (BITS) {
        __syncthreads();
        if (tid < CL_TILE && i0 + tid < a.na) a.bits[(size_t)(i0 + tid) * a.w64 + tj] = (cl_u64)s_bits[tid][0] | ((cl_u64)s_bits[tid][1] << 32);
    }
}

struct ClScanArgs {
    const cl_u64* bits; uint32_t w64, n;
    uint32_t* lead_of;       // [n] the rank of every rank's leader
    uint32_t* cid;           // [n] cluster of every rank
    uint32_t* lead_list;     // [n_clusters] rank of cluster c's leader
    uint32_t* n_clusters;
};

// Pose i in rank order is a leader iff no leader of a rank < i has its bit in row i; otherwise its leader is the lowest such bit.
__global__ __launch_bounds__(1024) void cl_scan_kernel(ClScanArgs a) {
    __shared__ cl_u64 s_lm[MDX_CL_MAX_POSES / 64u];      // the leaders' bits, block by block
    __shared__ uint32_t s_pre[MDX_CL_MAX_POSES / 64u];   // leaders before the block
    __shared__ uint32_t s_ext[64];
    __shared__ uint16_t s_lead[MDX_CL_MAX_POSES];
    const uint32_t tid = threadIdx.x, nblk = (a.n + 63u) / 64u;
    for (uint32_t b = 0; b < nblk; ++b) {
        {   // the block's 64 rows against the leaders of the blocks before: 16 threads per row, the first hit of each in ascending words
            const uint32_t r = tid >> 4, sub = tid & 15u, i = 64u * b + r;
            uint32_t first = MDX_CL_NONE;
            if (i < a.n)
                for (uint32_t w = sub; w < b; w += 16u) {
                    const cl_u64 v = a.bits[(size_t)i * a.w64 + w] & s_lm[w];
                    if (v) { first = 64u * w + (uint32_t)__builtin_ctzll(v); break; }
                }
            for (int off = 8; off >= 1; off >>= 1) first = min(first, (uint32_t)__shfl_xor((int)first, off));
            if (sub == 0u) s_ext[r] = first;
        }
        __syncthreads();
        if (tid < 64u) {      // wave 0 settles the block: lane = rank 64 b + lane
            const uint32_t i = 64u * b + tid;
            const bool valid = i < a.n;
            const uint32_t ext = s_ext[tid];
            const cl_u64 w = valid ? a.bits[(size_t)i * a.w64 + b] : 0ull;      // (the tile kernel left only bits of lower ranks)
            cl_u64 cand = __ballot(valid && ext == MDX_CL_NONE), lm = 0ull;
            while (cand) {      // uniform over the wave: candidates in rank order against the block's leaders so far
                const int t = __builtin_ctzll(cand);
                cand &= cand - 1ull;
                const cl_u64 wt = __shfl(w, t);
                if ((wt & lm) == 0ull) lm |= 1ull << t;
            }
            if (valid) s_lead[i] = (uint16_t)(ext != MDX_CL_NONE ? ext : ((lm >> tid) & 1ull) ? i : 64u * b + (uint32_t)__builtin_ctzll(w & lm));
            if (tid == 0u) s_lm[b] = lm;
        }
        __syncthreads();
    }
    if (tid == 0u) {
        uint32_t run = 0;
        for (uint32_t b = 0; b < nblk; ++b) { s_pre[b] = run; run += (uint32_t)__popcll(s_lm[b]); }
        *a.n_clusters = run;
    }
    __syncthreads();
    for (uint32_t i = tid; i < a.n; i += 1024u) {
        const uint32_t lr = s_lead[i];
        const uint32_t c = s_pre[lr >> 6] + (uint32_t)__popcll(s_lm[lr >> 6] & ((1ull << (lr & 63u)) - 1ull));
        a.lead_of[i] = lr; a.cid[i] = c;
        if (lr == i) a.lead_list[c] = i;
    }
}

struct ClAssignArgs {
    const float* g; const double* c; const uint16_t* perms;
    uint32_t n, n_m, n_perms;
    double L[3];
    const uint32_t* lead_of; const uint32_t* cid;
    float* rmsd;          // [n] rank order
    uint32_t* size;       // [n_clusters], zeroed
};

__global__ __launch_bounds__(256) void cl_assign_kernel(ClAssignArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t lr = a.lead_of[i];
    atomicAdd(&a.size[a.cid[i]], 1u);
    if (lr == i) { a.rmsd[i] = 0.f; return; }
    double s[3];
    for (int d = 0; d < 3; ++d) s[d] = cl_shift(a.c[3 * (size_t)lr + d], a.c[3 * (size_t)i + d], a.L[d]);
    a.rmsd[i] = cl_rmsd(cl_distance(ClGView{a.g, a.n, lr}, ClGView{a.g, a.n, i}, a.perms, a.n_perms, a.n_m, s), a.n_m);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static int cl_grow(void** p, size_t& cap, size_t need) {      // (pose_grow of mdx_poses.hip)
    if (cap >= need) return MDX_OK;
    if (*p) { (void)hipFree(*p); *p = nullptr; }
    cap = 0;
    HIP_TRY(hipMalloc(p, need));
    cap = need;
    return MDX_OK;
}

// What the two entry points refuse on their arguments alone (the handle is not followed), and the tables they share: the masked atoms
// in atom order and the perms in masked-atom index space.
static int cl_check(const std::string& who, uint32_t count, const uint8_t* mask, uint32_t n_perms, const uint32_t* perms,
                    std::vector<uint32_t>& atoms, std::vector<uint16_t>& ptab) {
    if (count == 0 || count > MDX_POSE_MAX_ATOMS) FAIL(MDX_EPARAM, who + ": count must be in 1..MDX_POSE_MAX_ATOMS (256)");
    if (n_perms > MDX_CLUSTER_MAX_PERMS) FAIL(MDX_EPARAM, who + ": n_perms exceeds MDX_CLUSTER_MAX_PERMS (64)");
    if (n_perms > 0 && !perms) FAIL(MDX_EPARAM, who + ": null perms with n_perms > 0");
    std::vector<uint32_t> slot(count, MDX_CL_NONE);
    atoms.clear();
    for (uint32_t i = 0; i < count; ++i)
        if (!mask || mask[i]) { slot[i] = (uint32_t)atoms.size(); atoms.push_back(i); }
    if (atoms.empty()) FAIL(MDX_EPARAM, who + ": the mask selects no atom");
    const uint32_t n_m = (uint32_t)atoms.size();
    std::vector<uint8_t> seen(count);
    for (uint32_t q = 0; q < n_perms; ++q) {
        const uint32_t* p = perms + (size_t)q * count;
        std::fill(seen.begin(), seen.end(), 0);
        for (uint32_t i = 0; i < count; ++i) {
            if (p[i] >= count || seen[p[i]]) FAIL(MDX_EPARAM, who + ": perm " + std::to_string(q) + " is not a bijection of 0..count-1");
            seen[p[i]] = 1;
        }
        if (q == 0)
            for (uint32_t i = 0; i < count; ++i)
                if (p[i] != i) FAIL(MDX_EPARAM, who + ": perm 0 must be the identity");
        for (uint32_t k = 0; k < n_m; ++k)
            if (slot[p[atoms[k]]] == MDX_CL_NONE)
                FAIL(MDX_EPARAM, who + ": perm " + std::to_string(q) + " maps a masked atom to an unmasked one");
    }
    ptab.assign((size_t)n_perms * n_m, 0);
    for (uint32_t q = 0; q < n_perms; ++q)
        for (uint32_t k = 0; k < n_m; ++k) ptab[(size_t)q * n_m + k] = (uint16_t)slot[perms[(size_t)q * count + atoms[k]]];
    return MDX_OK;
}

static int cl_finite(const std::string& who, const float* poses, size_t n_values) {
    for (size_t k = 0; k < n_values; ++k)
        if (!std::isfinite(poses[k])) FAIL(MDX_EPARAM, who + ": non-finite pose coordinate");
    return MDX_OK;
}

static int cl_handle(mdx_handle* h, const std::string& who, double L[3]) {
    if (h->dd || h->n_local != h->N) FAIL(MDX_EPARAM, who + " on a decomposed handle (single-device handles only)");
    for (int d = 0; d < 3; ++d) L[d] = h->per[d] ? (double)h->box_hi[d] - (double)h->box_lo[d] : 0.0;
    HIP_TRY(hipSetDevice(h->device));
    return MDX_OK;
}

// the block of one call in ps_cl: byte offsets, every part 256-byte aligned
struct ClLayout {
    size_t raw_a, raw_b, order, atoms, perms, ga, gb, ca, cb, res, lead_of, cid, lead_list, rmsd, size, end;
    // res: [n_clusters, pad] then lead_of, cid, lead_list, rmsd, size [nr] each - the read-back of a clustering in one copy
    ClLayout(uint32_t count, uint32_t na, uint32_t nb, uint32_t n_m, uint32_t n_perms, uint32_t nr) {
        size_t o = 0;
        auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255u) & ~(size_t)255u; return at; };
        raw_a = take(sizeof(float) * 3 * (size_t)count * na); raw_b = take(sizeof(float) * 3 * (size_t)count * nb);
        order = take(sizeof(uint32_t) * nr); atoms = take(sizeof(uint32_t) * n_m); perms = take(sizeof(uint16_t) * (size_t)n_perms * n_m);
        ga = take(sizeof(float) * 3 * (size_t)n_m * na); gb = take(sizeof(float) * 3 * (size_t)n_m * nb);
        ca = take(sizeof(double) * 3 * (size_t)na); cb = take(sizeof(double) * 3 * (size_t)nb);
        res = take(256);
        lead_of = take(sizeof(uint32_t) * nr); cid = take(sizeof(uint32_t) * nr); lead_list = take(sizeof(uint32_t) * nr);
        rmsd = take(sizeof(float) * nr); size = take(sizeof(uint32_t) * nr);
        end = o;
    }
};

static void cl_gather(hipStream_t st, const float* poses, const uint32_t* order, const uint32_t* atoms, float* g, double* c, uint32_t n,
                      uint32_t count, uint32_t n_m) {
    ClGatherArgs ga{poses, order, atoms, g, c, n, count, n_m};
    hipLaunchKernelGGL(cl_gather_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, ga);
}

template <bool BITS>
static void cl_tiles(hipStream_t st, const ClTileArgs& t, bool periodic) {
    const dim3 grid((t.nb + CL_TILE - 1u) / CL_TILE, (t.na + CL_TILE - 1u) / CL_TILE);
    if (periodic) hipLaunchKernelGGL((cl_tile_kernel<true, BITS>), grid, dim3(256), 0, st, t);
    else hipLaunchKernelGGL((cl_tile_kernel<false, BITS>), grid, dim3(256), 0, st, t);
}

extern "C" int mdx_pose_rmsd(mdx_handle* h, uint32_t count, uint32_t n_a, const float* poses_a, uint32_t n_b, const float* poses_b_or_null,
                             const uint8_t* mask_or_null, uint32_t n_perms, const uint32_t* perms_or_null, float* out) {
    const std::string who = "mdx_pose_rmsd";
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (n_a > MDX_CLUSTER_MAX_POSES || n_b > MDX_CLUSTER_MAX_POSES) FAIL(MDX_EPARAM, who + ": more than MDX_CLUSTER_MAX_POSES (16384) poses");
    std::vector<uint32_t> atoms;
    std::vector<uint16_t> ptab;
    MDX_TRY(cl_check(who, count, mask_or_null, n_perms, perms_or_null, atoms, ptab));
    const bool self = !poses_b_or_null;
    const uint32_t nb = self ? n_a : n_b;
    if (n_a == 0 || nb == 0) return MDX_OK;
    if (!poses_a || !out) FAIL(MDX_EPARAM, "null argument");
    const size_t per_pose = 3 * (size_t)count;
    MDX_TRY(cl_finite(who, poses_a, per_pose * n_a));
    if (!self) MDX_TRY(cl_finite(who, poses_b_or_null, per_pose * nb));
    ClTileArgs t{};
    MDX_TRY(cl_handle(h, who, t.L));
    DeviceState& d = h->d;
    hipStream_t st = h->stream;
    const uint32_t n_m = (uint32_t)atoms.size();
    const ClLayout lay(count, n_a, self ? 0u : nb, n_m, n_perms, 0u);
    MDX_TRY(cl_grow(&d.ps_cl, h->ps_cap_cl, lay.end));
    MDX_TRY(cl_grow(&d.ps_cl_mat, h->ps_cap_cl_mat, sizeof(float) * (size_t)n_a * nb));
    unsigned char* b0 = (unsigned char*)d.ps_cl;
    HIP_TRY(hipMemcpyAsync(b0 + lay.raw_a, poses_a, sizeof(float) * per_pose * n_a, hipMemcpyHostToDevice, st));
    if (!self) HIP_TRY(hipMemcpyAsync(b0 + lay.raw_b, poses_b_or_null, sizeof(float) * per_pose * nb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b0 + lay.atoms, atoms.data(), sizeof(uint32_t) * n_m, hipMemcpyHostToDevice, st));
    if (n_perms) HIP_TRY(hipMemcpyAsync(b0 + lay.perms, ptab.data(), sizeof(uint16_t) * ptab.size(), hipMemcpyHostToDevice, st));
    mdx_prof_begin(h, 1);
    cl_gather(st, (const float*)(b0 + lay.raw_a), nullptr, (const uint32_t*)(b0 + lay.atoms), (float*)(b0 + lay.ga), (double*)(b0 + lay.ca), n_a, count, n_m);
    if (!self) cl_gather(st, (const float*)(b0 + lay.raw_b), nullptr, (const uint32_t*)(b0 + lay.atoms), (float*)(b0 + lay.gb), (double*)(b0 + lay.cb), nb, count, n_m);
    mdx_prof_end(h);
    t.ga = (const float*)(b0 + lay.ga); t.gb = self ? t.ga : (const float*)(b0 + lay.gb);
    t.ca = (const double*)(b0 + lay.ca); t.cb = self ? t.ca : (const double*)(b0 + lay.cb);
    t.perms = (const uint16_t*)(b0 + lay.perms);
    t.na = n_a; t.nb = nb; t.n_m = n_m; t.n_perms = n_perms; t.T = 0.0;
    t.out = (float*)d.ps_cl_mat; t.bits = nullptr; t.w64 = 0;
    mdx_prof_begin(h, 0);
    cl_tiles<false>(st, t, t.L[0] > 0.0 || t.L[1] > 0.0 || t.L[2] > 0.0);
    mdx_prof_end(h);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d.ps_cl_mat, sizeof(float) * (size_t)n_a * nb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MDX_OK;
}

extern "C" int mdx_cluster_poses(mdx_handle* h, uint32_t count, uint32_t n_poses, const float* poses, const double* scores,
                                 const uint8_t* mask_or_null, uint32_t n_perms, const uint32_t* perms_or_null, float rmsd_cut,
                                 uint32_t* n_clusters_out, uint32_t* leader_out_or_null, uint32_t* cluster_of_out_or_null,
                                 float* rmsd_to_leader_out_or_null, uint32_t* size_out_or_null) {
    const std::string who = "mdx_cluster_poses";
    if (!h) FAIL(MDX_EPARAM, "null handle");
    if (!n_clusters_out) FAIL(MDX_EPARAM, "null argument");
    if (n_poses > MDX_CLUSTER_MAX_POSES) FAIL(MDX_EPARAM, who + ": more than MDX_CLUSTER_MAX_POSES (16384) poses");
    std::vector<uint32_t> atoms;
    std::vector<uint16_t> ptab;
    MDX_TRY(cl_check(who, count, mask_or_null, n_perms, perms_or_null, atoms, ptab));
    if (!std::isfinite(rmsd_cut) || rmsd_cut < 0.f) FAIL(MDX_EPARAM, who + ": rmsd_cut is negative or not finite");
    const uint32_t n = n_poses;
    if (n > 0 && (!poses || !scores)) FAIL(MDX_EPARAM, "null argument");
    const size_t per_pose = 3 * (size_t)count;
    MDX_TRY(cl_finite(who, poses, per_pose * n));
    for (uint32_t p = 0; p < n; ++p)
        if (std::isnan(scores[p])) FAIL(MDX_EPARAM, who + ": a score is NaN");
    ClTileArgs t{};
    MDX_TRY(cl_handle(h, who, t.L));
    if (n == 0) { *n_clusters_out = 0u; return MDX_OK; }
    // rank: score ascending, index ascending
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return scores[x] < scores[y]; });
    DeviceState& d = h->d;
    hipStream_t st = h->stream;
    const uint32_t n_m = (uint32_t)atoms.size(), w64 = (n + 63u) / 64u;
    const ClLayout lay(count, n, 0u, n_m, n_perms, n);
    MDX_TRY(cl_grow(&d.ps_cl, h->ps_cap_cl, lay.end));
    MDX_TRY(cl_grow(&d.ps_cl_mat, h->ps_cap_cl_mat, sizeof(cl_u64) * (size_t)n * w64));
    unsigned char* b0 = (unsigned char*)d.ps_cl;
    HIP_TRY(hipMemcpyAsync(b0 + lay.raw_a, poses, sizeof(float) * per_pose * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b0 + lay.order, order.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b0 + lay.atoms, atoms.data(), sizeof(uint32_t) * n_m, hipMemcpyHostToDevice, st));
    if (n_perms) HIP_TRY(hipMemcpyAsync(b0 + lay.perms, ptab.data(), sizeof(uint16_t) * ptab.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(b0 + lay.size, 0, sizeof(uint32_t) * n, st));
    mdx_prof_begin(h, 1);
    cl_gather(st, (const float*)(b0 + lay.raw_a), (const uint32_t*)(b0 + lay.order), (const uint32_t*)(b0 + lay.atoms), (float*)(b0 + lay.ga),
              (double*)(b0 + lay.ca), n, count, n_m);
    mdx_prof_end(h);
    t.ga = t.gb = (const float*)(b0 + lay.ga); t.ca = t.cb = (const double*)(b0 + lay.ca);
    t.perms = (const uint16_t*)(b0 + lay.perms);
    t.na = t.nb = n; t.n_m = n_m; t.n_perms = n_perms; t.T = cl_threshold(rmsd_cut, n_m);
    t.out = nullptr; t.bits = (cl_u64*)d.ps_cl_mat; t.w64 = w64;
    mdx_prof_begin(h, 0);
    cl_tiles<true>(st, t, t.L[0] > 0.0 || t.L[1] > 0.0 || t.L[2] > 0.0);
    mdx_prof_end(h);
    ClScanArgs sc{t.bits, w64, n, (uint32_t*)(b0 + lay.lead_of), (uint32_t*)(b0 + lay.cid), (uint32_t*)(b0 + lay.lead_list), (uint32_t*)(b0 + lay.res)};
    mdx_prof_begin(h, 2);
    hipLaunchKernelGGL(cl_scan_kernel, dim3(1), dim3(1024), 0, st, sc);
    mdx_prof_end(h);
    ClAssignArgs as{t.ga, t.ca, t.perms, n, n_m, n_perms, {t.L[0], t.L[1], t.L[2]}, sc.lead_of, sc.cid, (float*)(b0 + lay.rmsd), (uint32_t*)(b0 + lay.size)};
    mdx_prof_begin(h, 5);
    hipLaunchKernelGGL(cl_assign_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, as);
    mdx_prof_end(h);
    HIP_TRY(hipGetLastError());
    std::vector<unsigned char> back(lay.end - lay.res);
    HIP_TRY(hipMemcpyAsync(back.data(), b0 + lay.res, back.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    auto at = [&](size_t off) { return back.data() + (off - lay.res); };
    uint32_t K = 0;
    std::memcpy(&K, at(lay.res), sizeof(K));
    if (K == 0 || K > n) FAIL(MDX_EDEVICE, "internal: " + who + " read back an impossible cluster count");
    const uint32_t* cid = (const uint32_t*)at(lay.cid);
    const uint32_t* lead = (const uint32_t*)at(lay.lead_list);
    const float* rm = (const float*)at(lay.rmsd);
    // rank order -> caller order
    *n_clusters_out = K;
    if (leader_out_or_null) for (uint32_t c = 0; c < K; ++c) leader_out_or_null[c] = order[lead[c]];
    if (cluster_of_out_or_null) for (uint32_t r = 0; r < n; ++r) cluster_of_out_or_null[order[r]] = cid[r];
    if (rmsd_to_leader_out_or_null) for (uint32_t r = 0; r < n; ++r) rmsd_to_leader_out_or_null[order[r]] = rm[r];
    if (size_out_or_null) std::memcpy(size_out_or_null, at(lay.size), sizeof(uint32_t) * K);
    return MDX_OK;
}
