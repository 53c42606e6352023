// The stepper of mdx_refine_poses_flex on the host: molchanica_amd/csrc/mdx_flex_step.h - the functions pose_flex_step_kernel calls on
// the device and the moving-side derivation of the host entry - so that tests/test_pose_flex_host.py can hold it against the numpy
// restatement of tests/pose_flex_ref.py without a GPU.  Every real number is read and written as a C hexadecimal float.
//
// stdin, first word = the mode:
//   G count root n_bonds T, then n_bonds lines "p q" and T lines "a b"
//       -> "M rc torsion"; for rc = 0, T lines "a b w0 .. w7" (axis atoms, the moving set's mask words in hex)
//   D n n_terms box_x box_y box_z, then n lines "x y z" (fp32 coordinates) and n_terms lines "i j k l v phase n"
//       -> "E energy" (terms added in list order), then n lines "fx fy fz" (per atom, the terms that name it in list order)
//   S n k max_evals f_tol tau_tol tors_tol h_start h_max root n_bonds T, then n lines "x y z" (the pose, fp32), n lines "x y z" (the
//     targets, fp64), the bonds and the torsions as for G
//       -> "I d" - d atoms whose coords(identity, 0, 0) are not the input's bits -, then per evaluation "E flags h" and, unless the pose
//          is finished, n lines with the bits of the next trial's coordinates; at the end "R status evals" and the accepted
//          (q, t, theta) on one line.
// The field of S: S = k/2 sum |Y_i - T_i|^2 as a one-group row, f_i = fp32(-k (Y_i - T_i)), rigid about the mean of Y of the unrounded
// forces - sums in atom order (tests/pose_refine_ref.py: synthetic_evaluate).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mdx_flex_step.h"

static bool read_graph(uint32_t n_bonds, uint32_t T, std::vector<uint32_t>& bonds, std::vector<uint32_t>& tb) {
    bonds.resize(2 * (size_t)n_bonds); tb.resize(2 * (size_t)T);
    for (uint32_t& v : bonds) if (std::scanf("%u", &v) != 1) return false;
    for (uint32_t& v : tb) if (std::scanf("%u", &v) != 1) return false;
    return true;
}

static int graph_mode() {
    uint32_t count = 0, root = 0, n_bonds = 0, T = 0;
    if (std::scanf("%u %u %u %u", &count, &root, &n_bonds, &T) != 4 || count == 0 || count > MDX_FX_MAX_ATOMS || T > MDX_FX_MAX_TORSIONS) return 2;
    std::vector<uint32_t> bonds, tb;
    if (!read_graph(n_bonds, T, bonds, tb)) return 2;
    std::vector<mdx_fx_torsion> tor(MDX_FX_MAX_TORSIONS);
    uint32_t bad = 0;
    const int rc = fx_moving_sides(count, n_bonds, bonds.data(), root, T, tb.data(), tor.data(), &bad);
    std::printf("M %d %u\n", rc, bad);
    for (uint32_t k = 0; rc == MDX_FX_OK && k < T; ++k) {
        std::printf("%u %u", tor[k].a, tor[k].b);
        for (uint32_t w = 0; w < MDX_FX_MASK_WORDS; ++w) std::printf(" %08x", tor[k].mask[w]);
        std::printf("\n");
    }
    return 0;
}

static int dihedral_mode() {
    uint32_t n = 0, nt = 0;
    double box[3];
    if (std::scanf("%u %u %la %la %la", &n, &nt, &box[0], &box[1], &box[2]) != 5 || n == 0) return 2;
    std::vector<double> x(3 * (size_t)n);
    for (double& v : x) { double r; if (std::scanf("%la", &r) != 1) return 2; v = (double)(float)r; }
    std::vector<mdx_fx_dihedral> terms(nt);
    for (mdx_fx_dihedral& t : terms)
        if (std::scanf("%u %u %u %u %la %la %la", &t.at[0], &t.at[1], &t.at[2], &t.at[3], &t.v, &t.phase, &t.n) != 7) return 2;
    double E = 0.0;
    std::vector<double> f(3 * (size_t)n, 0.0);
    for (const mdx_fx_dihedral& t : terms) {      // (term by term: every atom meets the terms that name it in list order)
        double g[4][3];
        E += fx_dihedral(x.data(), t, box, g);
        for (uint32_t r = 0; r < 4u; ++r)
            for (int d = 0; d < 3; ++d) f[3 * (size_t)t.at[r] + d] += g[r][d];
    }
    std::printf("E %a\n", E);
    for (uint32_t i = 0; i < n; ++i) std::printf("%a %a %a\n", f[3 * (size_t)i], f[3 * (size_t)i + 1], f[3 * (size_t)i + 2]);
    return 0;
}

static void evaluate(const std::vector<float>& Y, const std::vector<double>& T, double k, float& row, float rigid[6], std::vector<double>& f32) {
    const uint32_t n = (uint32_t)(Y.size() / 3);
    std::vector<double> y(Y.begin(), Y.end());
    double c[3];
    for (uint32_t d = 0; d < 3; ++d) c[d] = rf_mean(y.data(), n, d);
    double S = 0.0, net[3] = {0, 0, 0}, tau[3] = {0, 0, 0};
    for (uint32_t i = 0; i < n; ++i) {
        double dd[3], f[3], r[3];
        for (int d = 0; d < 3; ++d) {
            dd[d] = y[3 * i + d] - T[3 * i + d];
            const double kd = k * dd[d];
            f[d] = -kd; r[d] = y[3 * i + d] - c[d];
            f32[3 * (size_t)i + d] = (double)(float)f[d];
        }
        const double s0 = dd[0] * dd[0], s1 = dd[1] * dd[1], s2 = dd[2] * dd[2];
        S += (s0 + s1) + s2;
        for (int d = 0; d < 3; ++d) {
            const int d1 = (d + 1) % 3, d2 = (d + 2) % 3;
            const double p = r[d1] * f[d2], q = r[d2] * f[d1];
            net[d] += f[d];
            tau[d] += p - q;
        }
    }
    const double hk = 0.5 * k;
    row = (float)(hk * S);
    for (int d = 0; d < 3; ++d) { rigid[d] = (float)net[d]; rigid[3 + d] = (float)tau[d]; }
}

static int stepper_mode() {
    uint32_t n = 0, max_evals = 0, root = 0, n_bonds = 0, T = 0;
    double k = 0.0;
    mdx_fx_opts o{};
    if (std::scanf("%u %la %u %la %la %la %la %la %u %u %u", &n, &k, &max_evals, &o.rf.f_tol, &o.rf.tau_tol, &o.tors_tol, &o.rf.h_start,
                   &o.rf.h_max, &root, &n_bonds, &T) != 11 || n == 0 || n > MDX_FX_MAX_ATOMS || T > MDX_FX_MAX_TORSIONS) return 2;
    std::vector<float> x0(3 * (size_t)n), Y;
    std::vector<double> Tg(3 * (size_t)n), y(3 * (size_t)n), B(3 * (size_t)n), f(3 * (size_t)n);
    for (size_t i = 0; i < x0.size(); ++i) { double v; if (std::scanf("%la", &v) != 1) return 2; x0[i] = (float)v; }
    for (size_t i = 0; i < Tg.size(); ++i) if (std::scanf("%la", &Tg[i]) != 1) return 2;
    std::vector<uint32_t> bonds, tb;
    if (!read_graph(n_bonds, T, bonds, tb)) return 2;
    std::vector<mdx_fx_torsion> tor(MDX_FX_MAX_TORSIONS);
    uint32_t bad = 0;
    if (fx_moving_sides(n, n_bonds, bonds.data(), root, T, tb.data(), tor.data(), &bad) != MDX_FX_OK) return 3;
    mdx_fx_state s;
    std::memset(&s, 0, sizeof(s));
    // the trial builder: B(theta) from the input, its mean, the rigid image
    auto trial_coords = [&](const double c0[3], const double t[3], const double q[4], const double* theta, std::vector<float>& out) {
        double R[9], mean[3];
        rf_rotation(q, R);
        for (size_t i = 0; i < B.size(); ++i) B[i] = (double)x0[i];
        fx_build(B.data(), n, T, tor.data(), theta);
        for (uint32_t d = 0; d < 3; ++d) mean[d] = rf_mean(B.data(), n, d);
        for (uint32_t i = 0; i < n; ++i) fx_coords(c0, t, R, &B[3 * (size_t)i], mean, &out[3 * (size_t)i]);
    };
    Y = x0;
    {   // coords(identity, 0, 0) must give the input back bit for bit
        for (size_t i = 0; i < Y.size(); ++i) y[i] = (double)x0[i];
        const double qi[4] = {1.0, 0.0, 0.0, 0.0}, t0[3] = {0.0, 0.0, 0.0};
        double c[3], zero[MDX_FX_MAX_TORSIONS] = {};
        for (uint32_t d = 0; d < 3; ++d) c[d] = rf_mean(y.data(), n, d);
        std::vector<float> z(x0.size());
        trial_coords(c, t0, qi, zero, z);
        uint32_t differ = 0;
        for (uint32_t i = 0; i < n; ++i) differ += std::memcmp(&z[3 * (size_t)i], &x0[3 * (size_t)i], 3 * sizeof(float)) != 0;
        std::printf("I %u\n", differ);
    }
    for (uint32_t e = 0; e < max_evals; ++e) {
        float row, rigid[6];
        evaluate(Y, Tg, k, row, rigid, f);
        bool finite = std::isfinite(row);
        for (int d = 0; d < 6; ++d) finite = finite && std::isfinite(rigid[d]);
        for (size_t i = 0; i < Y.size(); ++i) { y[i] = (double)Y[i]; finite = finite && std::isfinite(f[i]); }
        double c[3], I[6], g[MDX_FX_MAX_TORSIONS], J[MDX_FX_MAX_TORSIONS], A[MDX_FX_MAX_TORSIONS][3], U[MDX_FX_MAX_TORSIONS][3],
            sh[MDX_FX_MAX_TORSIONS][3];
        for (uint32_t d = 0; d < 3; ++d) c[d] = rf_mean(y.data(), n, d);
        const double v[3] = {(double)rigid[0] / (double)n, (double)rigid[1] / (double)n, (double)rigid[2] / (double)n};
        double gmax = 0.0;
        for (uint32_t t = 0; t < T; ++t) {
            fx_gradient(y.data(), f.data(), n, v, tor[t], U[t], g[t], J[t], A[t]);
            finite = finite && std::isfinite(g[t]);
            gmax = std::fabs(g[t]) > gmax ? std::fabs(g[t]) : gmax;
        }
        if (s.rf.evals == 0) fx_start(s, c, o.rf.h_start);
        uint32_t fl = fx_decide(s, o, T, (double)row, finite, rigid, gmax);
        if (fl & MDX_RF_STORE) for (uint32_t t = 0; t < T; ++t) s.g[t] = g[t];
        if (fl == MDX_RF_STORE) {
            for (uint32_t j = 0; j < 6; ++j) I[j] = rf_inertia(y.data(), n, c, j);
            rf_direction(s.rf, n, rigid, I);
            for (uint32_t t = 0; t < T; ++t) { s.wk[t] = fx_omega(g[t], J[t]); fx_shift(s.wk[t], A[t], n, sh[t]); }
            double m = 0.0;
            for (uint32_t i = 0; i < n; ++i) {
                const double u = fx_speed(s.rf.v, s.rf.w, c, y.data(), i, T, tor.data(), U, s.wk, sh);
                m = u > m ? u : m;
            }
            fl |= rf_set_speed(s.rf, m);
        }
        std::printf("E %u %a\n", fl, s.rf.h);
        if (fl & MDX_RF_FROZEN) break;
        fx_trial(s, T);
        trial_coords(s.rf.c0, s.rf.tt, s.rf.qt, s.tht, Y);
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t b[3];
            std::memcpy(b, &Y[3 * (size_t)i], sizeof(b));
            std::printf("%08x %08x %08x\n", b[0], b[1], b[2]);
        }
    }
    std::printf("R %u %u\n", s.rf.frozen ? s.rf.status : MDX_RF_MAX_EVALS, s.rf.evals);
    std::printf("%a %a %a %a %a %a %a", s.rf.q[0], s.rf.q[1], s.rf.q[2], s.rf.q[3], s.rf.t[0], s.rf.t[1], s.rf.t[2]);
    for (uint32_t t = 0; t < T; ++t) std::printf(" %a", s.th[t]);
    std::printf("\n");
    return 0;
}

int main() {
    char mode = 0;
    if (std::scanf(" %c", &mode) != 1) return 2;
    if (mode == 'G') return graph_mode();
    if (mode == 'D') return dihedral_mode();
    if (mode == 'S') return stepper_mode();
    return 2;
}
