// Stand-alone host program around molchanica_amd/csrc/mdx_cluster_rule.h: the rule of mdx_pose_rmsd / mdx_cluster_poses on the host,
// single thread.  tests/test_pose_cluster_host.py holds it against the numpy restatement; tools/pose_cluster_rates.py times it as the
// baseline a caller has without the device path.
//
//   pose_cluster_driver <file>
// file (binary, little endian): u32 mode, count, n, n_perms, has_mask; f64 L[3]; f32 cut; u8 mask[count] (if has_mask);
// u32 perms[n_perms][count]; f32 poses[n][count][3]; f64 scores[n].
//   mode 0   "T <hex>" then n lines of n "<D hex>:<rmsd bits hex>" - every pair, a the row
//   mode 1   "K <n_clusters>", then the leaders, cluster_of, the bits of rmsd_to_leader and the sizes, one line each
//   mode 2   the clustering of mode 1, timed: "S <seconds> <n_clusters>"
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mdx_cluster_rule.h"

template <class T>
static bool take(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: pose_cluster_driver <file>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t head[5];
    double L[3];
    float cut;
    if (fread(head, sizeof(uint32_t), 5, f) != 5 || fread(L, sizeof(double), 3, f) != 3 || fread(&cut, sizeof(float), 1, f) != 1) return 3;
    const uint32_t mode = head[0], count = head[1], n = head[2], n_perms = head[3], has_mask = head[4];
    if (count == 0 || count > 256u || n > MDX_CL_MAX_POSES || n_perms > MDX_CL_MAX_PERMS) return 3;
    std::vector<uint8_t> mask;
    std::vector<uint32_t> perms;
    std::vector<float> poses;
    std::vector<double> scores;
    if (!take(f, mask, has_mask ? count : 0u) || !take(f, perms, (size_t)n_perms * count) || !take(f, poses, 3 * (size_t)count * n) ||
        !take(f, scores, n)) return 3;
    fclose(f);
    for (uint32_t v : perms)
        if (v >= count) return 3;
    mdx_cl_host R;
    R.setup(count, has_mask ? mask.data() : nullptr, n_perms, perms.data(), L);
    if (R.n_m == 0) return 3;
    const size_t per_pose = 3 * (size_t)count;
    if (mode == 0) {
        printf("T %a\n", cl_threshold(cut, R.n_m));
        for (uint32_t i = 0; i < n; ++i) {
            for (uint32_t j = 0; j < n; ++j) {
                const double D = R.distance(poses.data() + per_pose * i, poses.data() + per_pose * j);
                const float r = cl_rmsd(D, R.n_m);
                uint32_t bits;
                memcpy(&bits, &r, sizeof(bits));
                printf("%a:%08x%c", D, bits, j + 1 == n ? '\n' : ' ');
            }
        }
        return 0;
    }
    std::vector<uint32_t> leader, cluster_of, size;
    std::vector<float> rm;
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t K = R.cluster(n, poses.data(), scores.data(), cut, leader, cluster_of, rm, size);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (mode == 2) { printf("S %.9f %u\n", sec, K); return 0; }
    printf("K %u\n", K);
    for (uint32_t c = 0; c < K; ++c) printf("%u%c", leader[c], c + 1 == K ? '\n' : ' ');
    for (uint32_t p = 0; p < n; ++p) printf("%u%c", cluster_of[p], p + 1 == n ? '\n' : ' ');
    for (uint32_t p = 0; p < n; ++p) {
        uint32_t bits;
        memcpy(&bits, &rm[p], sizeof(bits));
        printf("%08x%c", bits, p + 1 == n ? '\n' : ' ');
    }
    for (uint32_t c = 0; c < K; ++c) printf("%u%c", size[c], c + 1 == K ? '\n' : ' ');
    return 0;
}
