// The stepper of mdx_refine_poses on the host: molchanica_amd/csrc/mdx_refine_step.h - the functions pose_refine_step_kernel calls on
// the device - driven by a synthetic quadratic field, so that tests/test_pose_refine_host.py can hold it against the numpy stepper
// of tests/pose_refine_ref.py without a GPU.
//
// stdin:  n k max_evals f_tol tau_tol h_start h_max, then n lines "x y z" (the pose, fp32) and n lines "x y z" (the targets, fp64),
//         every number as a C hexadecimal float.
// stdout: "I d" - d atoms whose coords(identity, 0) are not the input's bits -, then per evaluation "E flags h" and, unless the pose is finished, n lines with the bits of the next trial's coordinates;
//         at the end "R status evals" and the accepted (q, t) as hexadecimal floats.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mdx_refine_step.h"

// The field: S = k/2 sum |Y_i - T_i|^2 as a one-group row, f_i = -k (Y_i - T_i), rigid about the mean of Y - sums in atom order
static void evaluate(const std::vector<float>& Y, const std::vector<double>& T, double k, float& row, float rigid[6]) {
    const uint32_t n = (uint32_t)(Y.size() / 3);
    std::vector<double> y(Y.begin(), Y.end());
    double c[3];
    for (uint32_t d = 0; d < 3; ++d) c[d] = rf_mean(y.data(), n, d);
    double S = 0.0, net[3] = {0, 0, 0}, tau[3] = {0, 0, 0};
    for (uint32_t i = 0; i < n; ++i) {
        double dd[3], f[3], r[3];
        for (int d = 0; d < 3; ++d) { dd[d] = y[3 * i + d] - T[3 * i + d]; const double kd = k * dd[d]; f[d] = -kd; r[d] = y[3 * i + d] - c[d]; }
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

int main() {
    uint32_t n = 0, max_evals = 0;
    double k = 0.0;
    mdx_rf_opts o{};
    if (std::scanf("%u %la %u %la %la %la %la", &n, &k, &max_evals, &o.f_tol, &o.tau_tol, &o.h_start, &o.h_max) != 7 || n == 0) return 2;
    std::vector<float> x0(3 * (size_t)n), Y;
    std::vector<double> T(3 * (size_t)n), y(3 * (size_t)n);
    for (size_t i = 0; i < x0.size(); ++i) { double v; if (std::scanf("%la", &v) != 1) return 2; x0[i] = (float)v; }
    for (size_t i = 0; i < T.size(); ++i) if (std::scanf("%la", &T[i]) != 1) return 2;
    mdx_rf_state s;
    std::memset(&s, 0, sizeof(s));
    Y = x0;
    {   // coords(identity, 0) must give the input back bit for bit
        for (size_t i = 0; i < Y.size(); ++i) y[i] = (double)x0[i];
        const double qi[4] = {1.0, 0.0, 0.0, 0.0}, t0[3] = {0.0, 0.0, 0.0};
        double c[3], R[9];
        for (uint32_t d = 0; d < 3; ++d) c[d] = rf_mean(y.data(), n, d);
        rf_rotation(qi, R);
        uint32_t differ = 0;
        for (uint32_t i = 0; i < n; ++i) {
            float z[3];
            rf_coords(c, t0, R, &x0[3 * i], z);
            differ += std::memcmp(z, &x0[3 * i], sizeof(z)) != 0;
        }
        std::printf("I %u\n", differ);
    }
    for (uint32_t e = 0; e < max_evals; ++e) {
        float row, rigid[6];
        evaluate(Y, T, k, row, rigid);
        bool finite = std::isfinite(row);
        for (int d = 0; d < 6; ++d) finite = finite && std::isfinite(rigid[d]);
        for (size_t i = 0; i < Y.size(); ++i) y[i] = (double)Y[i];
        double c[3], I[6];
        for (uint32_t d = 0; d < 3; ++d) c[d] = rf_mean(y.data(), n, d);
        if (s.evals == 0) rf_start(s, c, o.h_start);
        uint32_t fl = rf_decide(s, o, (double)row, finite, rigid);
        if (fl == MDX_RF_STORE) {
            for (uint32_t j = 0; j < 6; ++j) I[j] = rf_inertia(y.data(), n, c, j);
            rf_direction(s, n, rigid, I);
            double m = 0.0;
            for (uint32_t i = 0; i < n; ++i) {
                const double r[3] = {y[3 * i] - c[0], y[3 * i + 1] - c[1], y[3 * i + 2] - c[2]};
                const double u = rf_speed(s.v, s.w, r);
                m = u > m ? u : m;
            }
            fl |= rf_set_speed(s, m);
        }
        std::printf("E %u %a\n", fl, s.h);
        if (fl & MDX_RF_FROZEN) break;
        rf_trial(s);
        double R[9];
        rf_rotation(s.qt, R);
        for (uint32_t i = 0; i < n; ++i) {
            rf_coords(s.c0, s.tt, R, &x0[3 * i], &Y[3 * i]);
            uint32_t b[3];
            std::memcpy(b, &Y[3 * i], sizeof(b));
            std::printf("%08x %08x %08x\n", b[0], b[1], b[2]);
        }
    }
    std::printf("R %u %u\n", s.frozen ? s.status : MDX_RF_MAX_EVALS, s.evals);
    std::printf("%a %a %a %a %a %a %a\n", s.q[0], s.q[1], s.q[2], s.q[3], s.t[0], s.t[1], s.t[2]);
    return 0;
}
