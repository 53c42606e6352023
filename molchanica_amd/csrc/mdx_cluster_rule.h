// mdx_cluster_rule.h - the rule of mdx_pose_rmsd and mdx_cluster_poses (include/mdx.h states it): the symmetry-aware distance of two
// poses in the receptor's frame and the greedy leader clustering by it.  Plain C++ in fp64, no HIP types: the kernels of
// mdx_pose_cluster.hip call the distance functions on the device, and a stand-alone host program can include this file and call the
// same ones, with the host clustering beside them (tests/cpp/pose_cluster_driver.cpp, tools/pose_cluster_rates.py).
//
// Fixed order of every sum, contraction off, so that the device, a host compiler and the numpy restatement in
// tests/pose_cluster_ref.py round alike up to the last bit of the one sqrt.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MDX_CL_HD __host__ __device__
#else
#define MDX_CL_HD
#endif
#if defined(__clang__)
#define MDX_CL_EXACT _Pragma("clang fp contract(off)")
#else
#define MDX_CL_EXACT
#endif

#define MDX_CL_MAX_POSES 16384u      // MDX_CLUSTER_MAX_POSES of include/mdx.h
#define MDX_CL_MAX_PERMS 64u         // MDX_CLUSTER_MAX_PERMS
#define MDX_CL_NONE 0xFFFFFFFFu      // "no leader within the cutoff"

// c(p): the fp64 mean over the masked atoms, in atom order.  x(k, axis) is the k-th MASKED atom's fp32 coordinate.
template <class X>
MDX_CL_HD inline void cl_centroid(const X& x, uint32_t n_m, double c[3]) {
    MDX_CL_EXACT
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (uint32_t k = 0; k < n_m; ++k) {
        s0 = s0 + (double)x(k, 0u);
        s1 = s1 + (double)x(k, 1u);
        s2 = s2 + (double)x(k, 2u);
    }
    c[0] = s0 / (double)n_m; c[1] = s1 / (double)n_m; c[2] = s2 / (double)n_m;
}

// the image shift of one axis: L rint((c(b) - c(a)) / L); 0 on an axis that is not periodic (L == 0)
MDX_CL_HD inline double cl_shift(double ca, double cb, double L) {
    MDX_CL_EXACT
    return L > 0.0 ? L * rint((cb - ca) / L) : 0.0;
}

// one term of acc_pi: acc + d d, d = ((double) a - (double) b) + s
MDX_CL_HD inline double cl_term(double acc, float a, float b, double s) {
    MDX_CL_EXACT
    const double d = ((double)a - (double)b) + s;
    return acc + d * d;
}

// ... with s = 0 left out: (a - b) + 0 differs from a - b in the sign of a zero at most, which d d does not see
MDX_CL_HD inline double cl_term0(double acc, float a, float b) {
    MDX_CL_EXACT
    const double d = (double)a - (double)b;
    return acc + d * d;
}

// acc_pi(a, b): the masked atoms in atom order, then x, y, z.  a(k, axis) and b(k, axis) index MASKED atoms; perm is the permutation
// in masked-atom index space (nullptr: the identity).
template <class A, class B, class P>
MDX_CL_HD inline double cl_acc(const A& a, const B& b, const P* perm, uint32_t n_m, const double s[3]) {
    double acc = 0.0;
    for (uint32_t k = 0; k < n_m; ++k) {
        const uint32_t pk = perm ? (uint32_t)perm[k] : k;
        acc = cl_term(acc, a(k, 0u), b(pk, 0u), s[0]);
        acc = cl_term(acc, a(k, 1u), b(pk, 1u), s[1]);
        acc = cl_term(acc, a(k, 2u), b(pk, 2u), s[2]);
    }
    return acc;
}

// D(a, b) = the minimum over the perms, in caller order; perms [n_perms][n_m] in masked-atom index space, n_perms == 0: the identity only
template <class A, class B, class P>
MDX_CL_HD inline double cl_distance(const A& a, const B& b, const P* perms, uint32_t n_perms, uint32_t n_m, const double s[3]) {
    if (n_perms == 0u) return cl_acc(a, b, (const P*)nullptr, n_m, s);
    double D = cl_acc(a, b, perms, n_m, s);
    for (uint32_t q = 1; q < n_perms; ++q) {
        const double v = cl_acc(a, b, perms + (size_t)q * n_m, n_m, s);
        D = v < D ? v : D;
    }
    return D;
}

// T = (cut cut) n_m, once per call; a pair is within the cutoff when D <= T
MDX_CL_HD inline double cl_threshold(float cut, uint32_t n_m) {
    MDX_CL_EXACT
    return ((double)cut * (double)cut) * (double)n_m;
}

// rmsd = sqrt(D / n_m), rounded to fp32
MDX_CL_HD inline float cl_rmsd(double D, uint32_t n_m) {
    MDX_CL_EXACT
    return (float)sqrt(D / (double)n_m);
}

#include <algorithm>
#include <numeric>
#include <vector>

// The whole rule on the host, single thread: what a caller without the device path would run, and what the stand-alone driver prints.
// poses [n][count][3]; mask (nullptr: all atoms); perms [n_perms][count] in ATOM index space, validated by the caller; L[3] the box
// edges (0: not periodic).  Ranks are (score ascending, index ascending).
struct mdx_cl_host {
    uint32_t count = 0, n_m = 0, n_perms = 0;
    std::vector<uint32_t> atoms;       // [n_m] the masked atoms in atom order
    std::vector<uint16_t> perms;       // [n_perms][n_m] in masked-atom index space
    double L[3] = {0.0, 0.0, 0.0};

    void setup(uint32_t count_, const uint8_t* mask, uint32_t n_perms_, const uint32_t* perms_atom, const double L_[3]) {
        count = count_; n_perms = n_perms_;
        atoms.clear();
        std::vector<uint32_t> slot(count, 0u);
        for (uint32_t i = 0; i < count; ++i)
            if (!mask || mask[i]) { slot[i] = (uint32_t)atoms.size(); atoms.push_back(i); }
        n_m = (uint32_t)atoms.size();
        perms.assign((size_t)n_perms * n_m, 0);
        for (uint32_t q = 0; q < n_perms; ++q)
            for (uint32_t k = 0; k < n_m; ++k) perms[(size_t)q * n_m + k] = (uint16_t)slot[perms_atom[(size_t)q * count + atoms[k]]];
        for (int d = 0; d < 3; ++d) L[d] = L_[d];
    }
    struct View {
        const float* p; const uint32_t* atoms;
        float operator()(uint32_t k, uint32_t axis) const { return p[3u * atoms[k] + axis]; }
    };
    View view(const float* pose) const { return View{pose, atoms.data()}; }
    void shift(const float* a, const float* b, double s[3]) const {
        double ca[3], cb[3];
        cl_centroid(view(a), n_m, ca);
        cl_centroid(view(b), n_m, cb);
        for (int d = 0; d < 3; ++d) s[d] = cl_shift(ca[d], cb[d], L[d]);
    }
    double distance(const float* a, const float* b) const {
        double s[3];
        shift(a, b, s);
        return cl_distance(view(a), view(b), perms.data(), n_perms, n_m, s);
    }
    // greedy leader clustering -> the number of clusters; leader [n_clusters], cluster_of [n], rmsd_to_leader [n], size [n_clusters]
    uint32_t cluster(uint32_t n, const float* poses, const double* scores, float cut, std::vector<uint32_t>& leader,
                     std::vector<uint32_t>& cluster_of, std::vector<float>& rmsd_to_leader, std::vector<uint32_t>& size) const {
        std::vector<uint32_t> order(n);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return scores[x] < scores[y]; });
        const double T = cl_threshold(cut, n_m);
        const size_t per_pose = 3 * (size_t)count;
        leader.clear(); size.clear();
        cluster_of.assign(n, 0u); rmsd_to_leader.assign(n, 0.f);
        for (uint32_t r = 0; r < n; ++r) {
            const uint32_t p = order[r];
            uint32_t c = MDX_CL_NONE;
            double D = 0.0;
            for (uint32_t k = 0; k < leader.size() && c == MDX_CL_NONE; ++k) {
                D = distance(poses + per_pose * leader[k], poses + per_pose * p);
                if (D <= T) c = k;
            }
            if (c == MDX_CL_NONE) { c = (uint32_t)leader.size(); leader.push_back(p); size.push_back(0u); D = 0.0; }
            cluster_of[p] = c; size[c] += 1u;
            rmsd_to_leader[p] = leader[c] == p ? 0.f : cl_rmsd(D, n_m);
        }
        return (uint32_t)leader.size();
    }
};
