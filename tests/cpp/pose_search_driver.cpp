// The rule of mdx_search_poses on the host: molchanica_amd/csrc/mdx_search_step.h with the two steppers it builds on - the functions
// pose_search_kernel and pose_flex_step_kernel call on the device - so that tests/test_pose_search_host.py can hold it against the numpy
// restatement of tests/pose_search_ref.py without a GPU.  Every real number is read and written as a C hexadecimal float.
//
// stdin, first word = the mode:
//   V seed id n_rounds
//       -> per round "S s0" (hex), then 51 lines "bits u01": the round's draws in their places
//   M n trans_amp rot_amp tors_amp seed id n_rounds root n_bonds T, then n lines "x y z" (the pose, fp32), n_bonds lines "p q", T lines "a b"
//       -> per round r = 1 .. n_rounds "M kind torsion choice tries v0 v1 v2 w0 w1 w2 dtheta" and n lines with the bits of X0'; the
//          X0' of a round is the input of the next
//   W n k d1 d2 hole hx hy hz max_evals f_tol tau_tol tors_tol h_start h_max trans_amp rot_amp tors_amp kT seed id n_rounds root n_bonds T,
//     then n lines "x y z" (the start, fp32), n lines (the targets of well 1, fp64), n lines (those of well 2), the bonds, the torsions
//       -> per round "D flags S finite evals"; at the end "B best_round accepted uphill nonfinite evals S_best" and n lines with the
//          bits of the best pose.
// The field of W: two quadratic wells, e_w = (double) fp32(k/2 sum |Y_i - T_w,i|^2) + d_w; the lower one (well 1 on a tie) gives the
// one-group row fp32(e_w), f_i = fp32(-k (Y_i - T_w,i)) and rigid as tests/cpp/pose_flex_driver.cpp takes them.  With hole > 0 the row is
// NaN while atom 0 lies closer than `hole` to (hx, hy, hz).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mdx_search_step.h"

static bool read_graph(uint32_t n_bonds, uint32_t T, std::vector<uint32_t>& bonds, std::vector<uint32_t>& tb) {
    bonds.resize(2 * (size_t)n_bonds); tb.resize(2 * (size_t)T);
    for (uint32_t& v : bonds) if (std::scanf("%u", &v) != 1) return false;
    for (uint32_t& v : tb) if (std::scanf("%u", &v) != 1) return false;
    return true;
}

static void print_bits(const std::vector<float>& Y) {
    for (size_t i = 0; i + 2 < Y.size(); i += 3) {
        uint32_t b[3];
        std::memcpy(b, &Y[i], sizeof(b));
        std::printf("%08x %08x %08x\n", b[0], b[1], b[2]);
    }
}

static int variates_mode() {
    unsigned long long seed = 0, id = 0;
    uint32_t n_rounds = 0;
    if (std::scanf("%llu %llu %u", &seed, &id, &n_rounds) != 3) return 2;
    for (uint32_t r = 0; r < n_rounds; ++r) {
        const uint64_t s0 = sr_stream(seed, id, r);
        std::printf("S %016llx\n", (unsigned long long)s0);
        for (uint32_t k = 0; k <= MDX_SR_DRAW_ACCEPT; ++k) {
            const uint64_t x = sr_bits(s0, k);
            std::printf("%016llx %a\n", (unsigned long long)x, sr_u01(x));
        }
    }
    return 0;
}

static int move_mode() {
    uint32_t n = 0, n_rounds = 0, root = 0, n_bonds = 0, T = 0;
    unsigned long long seed = 0, id = 0;
    mdx_sr_opts o{};
    if (std::scanf("%u %la %la %la %llu %llu %u %u %u %u", &n, &o.trans_amp, &o.rot_amp, &o.tors_amp, &seed, &id, &n_rounds, &root, &n_bonds,
                   &T) != 10 || n == 0 || n > MDX_FX_MAX_ATOMS || T > MDX_FX_MAX_TORSIONS) return 2;
    o.seed = seed; o.n_rounds = n_rounds + 1u;
    std::vector<float> Y(3 * (size_t)n), out(3 * (size_t)n);
    std::vector<double> work(3 * (size_t)n);
    for (float& v : Y) { double r; if (std::scanf("%la", &r) != 1) return 2; v = (float)r; }
    std::vector<uint32_t> bonds, tb;
    if (!read_graph(n_bonds, T, bonds, tb)) return 2;
    std::vector<mdx_fx_torsion> tor(MDX_FX_MAX_TORSIONS);
    uint32_t bad = 0;
    if (fx_moving_sides(n, n_bonds, bonds.data(), root, T, tb.data(), tor.data(), &bad) != MDX_FX_OK) return 3;
    if (sr_choices(o, T) == 0u) return 4;
    for (uint32_t r = 1; r <= n_rounds; ++r) {
        mdx_sr_move mv;
        sr_move(o, T, sr_stream(o.seed, id, r), mv);
        std::printf("M %u %u %u %u %a %a %a %a %a %a %a\n", mv.kind, mv.torsion, mv.choice, mv.tries, mv.v[0], mv.v[1], mv.v[2], mv.w[0], mv.w[1],
                    mv.w[2], mv.dtheta);
        sr_perturb(Y.data(), n, T, tor.data(), mv, work.data(), out.data());
        print_bits(out);
        Y = out;
    }
    return 0;
}

struct Field {
    uint32_t n; double k, d[2], hole, hp[3];
    std::vector<double> T[2];
};

static void evaluate(const Field& F, const std::vector<float>& Y, float& row, float rigid[6], std::vector<double>& f32) {
    const uint32_t n = F.n;
    std::vector<double> y(Y.begin(), Y.end());
    double c[3];
    for (uint32_t d = 0; d < 3; ++d) c[d] = rf_mean(y.data(), n, d);
    double e[2];
    const double hk = 0.5 * F.k;
    for (int w = 0; w < 2; ++w) {
        double S = 0.0;
        for (uint32_t i = 0; i < n; ++i) {
            const double a = y[3 * i] - F.T[w][3 * i], b = y[3 * i + 1] - F.T[w][3 * i + 1], g = y[3 * i + 2] - F.T[w][3 * i + 2];
            const double s0 = a * a, s1 = b * b, s2 = g * g;
            S += (s0 + s1) + s2;
        }
        e[w] = (double)(float)(hk * S) + F.d[w];
    }
    const int w = e[0] <= e[1] ? 0 : 1;
    double net[3] = {0, 0, 0}, tau[3] = {0, 0, 0};
    for (uint32_t i = 0; i < n; ++i) {
        double f[3], r[3];
        for (int d = 0; d < 3; ++d) {
            const double kd = F.k * (y[3 * i + d] - F.T[w][3 * i + d]);
            f[d] = -kd; r[d] = y[3 * i + d] - c[d];
            f32[3 * (size_t)i + d] = (double)(float)f[d];
        }
        for (int d = 0; d < 3; ++d) {
            const int d1 = (d + 1) % 3, d2 = (d + 2) % 3;
            const double p = r[d1] * f[d2], q = r[d2] * f[d1];
            net[d] += f[d];
            tau[d] += p - q;
        }
    }
    row = (float)e[w];
    if (F.hole > 0.0 && rf_norm(y[0] - F.hp[0], y[1] - F.hp[1], y[2] - F.hp[2]) < F.hole) row = NAN;
    for (int d = 0; d < 3; ++d) { rigid[d] = (float)net[d]; rigid[3 + d] = (float)tau[d]; }
}

// the refinement of one round: the stepper loop of tests/cpp/pose_flex_driver.cpp from x0 -> its accepted pose, S, status, evaluations
static void refine(const Field& F, const mdx_fx_opts& o, uint32_t max_evals, uint32_t T, const std::vector<mdx_fx_torsion>& tor,
                   const std::vector<float>& x0, std::vector<float>& acc, mdx_fx_state& s) {
    const uint32_t n = F.n;
    std::vector<float> Y = x0;
    std::vector<double> y(3 * (size_t)n), B(3 * (size_t)n), f(3 * (size_t)n);
    std::memset(&s, 0, sizeof(s));
    acc = x0;
    for (uint32_t e = 0; e < max_evals; ++e) {
        float row, rigid[6];
        evaluate(F, Y, row, rigid, f);
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
        if (fl & MDX_RF_STORE) { acc = Y; for (uint32_t t = 0; t < T; ++t) s.g[t] = g[t]; }
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
        if (fl & MDX_RF_FROZEN) break;
        fx_trial(s, T);
        double R[9], mean[3];
        rf_rotation(s.rf.qt, R);
        for (size_t i = 0; i < B.size(); ++i) B[i] = (double)x0[i];
        fx_build(B.data(), n, T, tor.data(), s.tht);
        for (uint32_t d = 0; d < 3; ++d) mean[d] = rf_mean(B.data(), n, d);
        for (uint32_t i = 0; i < n; ++i) fx_coords(s.rf.c0, s.rf.tt, R, &B[3 * (size_t)i], mean, &Y[3 * (size_t)i]);
    }
}

static int search_mode() {
    Field F{};
    mdx_fx_opts o{};
    mdx_sr_opts so{};
    uint32_t max_evals = 0, root = 0, n_bonds = 0, T = 0;
    unsigned long long seed = 0, id = 0;
    if (std::scanf("%u %la %la %la %la %la %la %la %u %la %la %la %la %la %la %la %la %la %llu %llu %u %u %u %u", &F.n, &F.k, &F.d[0], &F.d[1],
                   &F.hole, &F.hp[0], &F.hp[1], &F.hp[2], &max_evals, &o.rf.f_tol, &o.rf.tau_tol, &o.tors_tol, &o.rf.h_start, &o.rf.h_max,
                   &so.trans_amp, &so.rot_amp, &so.tors_amp, &so.kT, &seed, &id, &so.n_rounds, &root, &n_bonds, &T) != 24 ||
        F.n == 0 || F.n > MDX_FX_MAX_ATOMS || T > MDX_FX_MAX_TORSIONS || so.n_rounds == 0) return 2;
    so.seed = seed;
    const uint32_t n = F.n;
    std::vector<float> start(3 * (size_t)n);
    for (float& v : start) { double r; if (std::scanf("%la", &r) != 1) return 2; v = (float)r; }
    for (int w = 0; w < 2; ++w) {
        F.T[w].resize(3 * (size_t)n);
        for (double& v : F.T[w]) if (std::scanf("%la", &v) != 1) return 2;
    }
    std::vector<uint32_t> bonds, tb;
    if (!read_graph(n_bonds, T, bonds, tb)) return 2;
    std::vector<mdx_fx_torsion> tor(MDX_FX_MAX_TORSIONS);
    uint32_t bad = 0;
    if (fx_moving_sides(n, n_bonds, bonds.data(), root, T, tb.data(), tor.data(), &bad) != MDX_FX_OK) return 3;
    if (so.n_rounds > 1u && sr_choices(so, T) == 0u) return 4;
    mdx_sr_record rec{};
    std::vector<float> cur = start, best = start, x0 = start, acc;
    std::vector<double> work(3 * (size_t)n);
    for (uint32_t r = 0; r < so.n_rounds; ++r) {
        const uint64_t s0 = sr_stream(so.seed, id, r);
        if (r > 0) {
            mdx_sr_move mv;
            sr_move(so, T, s0, mv);
            sr_perturb(cur.data(), n, T, tor.data(), mv, work.data(), x0.data());
        }
        mdx_fx_state s;
        refine(F, o, max_evals, T, tor, x0, acc, s);
        const bool finite = !(s.rf.frozen != 0u && s.rf.status == MDX_RF_NONFINITE);
        const uint32_t fl = sr_decide(rec, so, r, s.rf.S, finite, s.edih, s.rf.evals, s0);
        if (fl & MDX_SR_ACCEPT) cur = acc;
        if (fl & MDX_SR_BEST) best = acc;
        std::printf("D %u %a %d %u\n", fl, s.rf.S, finite ? 1 : 0, s.rf.evals);
    }
    std::printf("B %u %u %u %u %u %a\n", rec.best_round, rec.accepted, rec.uphill, rec.nonfinite, rec.evals, rec.S_best);
    print_bits(best);
    return 0;
}

int main() {
    char mode = 0;
    if (std::scanf(" %c", &mode) != 1) return 2;
    if (mode == 'V') return variates_mode();
    if (mode == 'M') return move_mode();
    if (mode == 'W') return search_mode();
    return 2;
}
