// mdx_flex_step.h - the stepper of mdx_refine_poses_flex (include/mdx.h states the rule): the rigid-body descent of mdx_refine_step.h
// with the ligand's torsion angles as further coordinates.  Plain C++ in fp64, no HIP types: pose_flex_step_kernel (mdx_poses.hip)
// calls these functions on the device, and a stand-alone host program can include this file and call the same ones
// (tests/cpp/pose_flex_driver.cpp).  Where the rule is the rigid stepper's, the function is the rigid stepper's.
//
// As there: fixed order of every sum, contraction off, so that the device, a host compiler and the numpy restatement in
// tests/pose_flex_ref.py round alike up to the last bit of sqrt / sin / cos / atan2.
#pragma once
#include "mdx_refine_step.h"

#define MDX_FX_MAX_TORSIONS 32u    // MDX_POSE_MAX_TORSIONS of include/mdx.h
#define MDX_FX_MAX_ATOMS 256u      // MDX_POSE_MAX_ATOMS
#define MDX_FX_MASK_WORDS 8u       // a moving set: one bit per ligand atom

struct mdx_fx_opts { mdx_rf_opts rf; double tors_tol; };

struct mdx_fx_state {
    mdx_rf_state rf;                            // the rigid record: q, t, their trials, c0, v, w, m, h, S, status, evals
    double th[MDX_FX_MAX_TORSIONS];             // accepted torsion angles (rad)
    double tht[MDX_FX_MAX_TORSIONS];            // those of the trial being evaluated
    double wk[MDX_FX_MAX_TORSIONS];             // torsion speeds omega_k of the accepted state's direction
    double g[MDX_FX_MAX_TORSIONS];              // torsion gradient g_k = -dS/dtheta_k of the accepted state
    float edih; uint32_t pad;                   // its dihedral energy
};

// one torsion as the kernels see it: the axis runs from atom a (fixed side) to atom b (moving side), mask = the moving set M_k
struct mdx_fx_torsion { uint32_t a, b, pad[2]; uint32_t mask[MDX_FX_MASK_WORDS]; };

// one dihedral term of the ligand, atoms ligand-local: E = v (1 + cos(n phi - phase))
struct mdx_fx_dihedral { uint32_t at[4]; double v, phase, n; };

MDX_HD inline bool fx_member(const uint32_t* mask, uint32_t i) { return (mask[i >> 5] >> (i & 31u)) & 1u; }

MDX_HD inline void fx_start(mdx_fx_state& s, const double c0[3], double h_start) {
    rf_start(s.rf, c0, h_start);
    for (uint32_t k = 0; k < MDX_FX_MAX_TORSIONS; ++k) s.th[k] = s.tht[k] = s.wk[k] = s.g[k] = 0.0;
    s.edih = 0.f; s.pad = 0u;
}

// ---- the moving sides (host only: it runs once per torsion list) ----------------------------------------------------------------------
#define MDX_FX_OK 0
#define MDX_FX_E_ROOT 1            // root >= count
#define MDX_FX_E_INDEX 2           // an atom index >= count
#define MDX_FX_E_SELF 3            // a == b
#define MDX_FX_E_NOT_BONDED 4
#define MDX_FX_E_TWICE 5           // the bond is listed twice
#define MDX_FX_E_RING 6            // removing the bond leaves its ends connected
#define MDX_FX_E_LEAF 7            // one side is a single atom
#define MDX_FX_E_DISCONNECTED 8    // the range's bond graph is not connected (*bad_torsion is not set)

// atoms reachable from `from` over bonds[n_bonds][2] (ligand-local pairs) without crossing the bond {skip_a, skip_b}; -> their number
inline uint32_t fx_reach(uint32_t count, uint32_t n_bonds, const uint32_t* bonds, uint32_t from, uint32_t skip_a, uint32_t skip_b,
                         uint32_t* mask) {
    uint32_t stack[MDX_FX_MAX_ATOMS], top = 0, seen = 1;
    for (uint32_t w = 0; w < MDX_FX_MASK_WORDS; ++w) mask[w] = 0u;
    mask[from >> 5] |= 1u << (from & 31u);
    stack[top++] = from;
    while (top) {
        const uint32_t i = stack[--top];
        for (uint32_t e = 0; e < n_bonds; ++e) {
            const uint32_t p = bonds[2 * e], q = bonds[2 * e + 1];
            if (p >= count || q >= count || (p != i && q != i)) continue;
            if ((p == skip_a && q == skip_b) || (p == skip_b && q == skip_a)) continue;
            const uint32_t j = p == i ? q : p;
            if (fx_member(mask, j)) continue;
            mask[j >> 5] |= 1u << (j & 31u);
            stack[top++] = j; ++seen;
        }
    }
    return seen;
}

// Torsion k names the bond {tb[2k], tb[2k+1]}: removing it must split the ligand in two; the side without `root` is the moving set,
// its end of the bond is out[k].b.  -> MDX_FX_OK or the first rule broken (*bad_torsion = k)
inline int fx_moving_sides(uint32_t count, uint32_t n_bonds, const uint32_t* bonds, uint32_t root, uint32_t n_torsions,
                           const uint32_t* tb, mdx_fx_torsion* out, uint32_t* bad_torsion) {
    const uint32_t none = 0xFFFFFFFFu;
    uint32_t mask[MDX_FX_MASK_WORDS];
    *bad_torsion = 0;
    if (root >= count) return MDX_FX_E_ROOT;
    for (uint32_t k = 0; k < n_torsions; ++k) {
        const uint32_t a = tb[2 * k], b = tb[2 * k + 1];
        *bad_torsion = k;
        if (a >= count || b >= count) return MDX_FX_E_INDEX;
        if (a == b) return MDX_FX_E_SELF;
        bool bonded = false;
        for (uint32_t e = 0; e < n_bonds && !bonded; ++e)
            bonded = (bonds[2 * e] == a && bonds[2 * e + 1] == b) || (bonds[2 * e] == b && bonds[2 * e + 1] == a);
        if (!bonded) return MDX_FX_E_NOT_BONDED;
        for (uint32_t j = 0; j < k; ++j)
            if ((tb[2 * j] == a && tb[2 * j + 1] == b) || (tb[2 * j] == b && tb[2 * j + 1] == a)) return MDX_FX_E_TWICE;
    }
    *bad_torsion = 0;
    if (n_torsions && fx_reach(count, n_bonds, bonds, root, none, none, mask) != count) return MDX_FX_E_DISCONNECTED;
    for (uint32_t k = 0; k < n_torsions; ++k) {
        const uint32_t a = tb[2 * k], b = tb[2 * k + 1];
        *bad_torsion = k;
        const uint32_t fixed = fx_reach(count, n_bonds, bonds, root, a, b, mask);      // the root's side once the bond is gone
        if (fx_member(mask, a) && fx_member(mask, b)) return MDX_FX_E_RING;
        if (fixed == 1u || count - fixed == 1u) return MDX_FX_E_LEAF;
        out[k].a = fx_member(mask, a) ? a : b;
        out[k].b = fx_member(mask, a) ? b : a;
        out[k].pad[0] = out[k].pad[1] = 0u;
        for (uint32_t w = 0; w < MDX_FX_MASK_WORDS; ++w) out[k].mask[w] = ~mask[w];
        for (uint32_t i = count; i < 32u * MDX_FX_MASK_WORDS; ++i) out[k].mask[i >> 5] &= ~(1u << (i & 31u));
    }
    *bad_torsion = 0;
    return MDX_FX_OK;
}

// ---- the ligand's dihedral terms, fp64 of the fp32 trial ------------------------------------------------------------------------------
MDX_HD inline double fx_mimg(double d, double box) {
    MDX_RF_EXACT
    return box > 0.0 ? d - rint(d / box) * box : d;
}

// One term at x[n][3] (phi as the fp64 oracle defines it, Blondel & Karplus): -> its energy, and in f[r] the force on the atom in
// position r of the term.  A term whose geometry leaves phi undefined (the oracle's guards) contributes nothing.
MDX_HD inline double fx_dihedral(const double* x, const mdx_fx_dihedral& t, const double box[3], double f[4][3]) {
    MDX_RF_EXACT
    const double* xi = x + 3u * t.at[0]; const double* xj = x + 3u * t.at[1]; const double* xk = x + 3u * t.at[2];
    const double* xl = x + 3u * t.at[3];
    double F[3], G[3], H[3];
    for (int d = 0; d < 3; ++d) {
        F[d] = fx_mimg(xi[d] - xj[d], box[d]); G[d] = fx_mimg(xj[d] - xk[d], box[d]); H[d] = fx_mimg(xl[d] - xk[d], box[d]);
    }
    double A[3], B[3];
    for (int d = 0; d < 3; ++d) {
        const int d1 = (d + 1) % 3, d2 = (d + 2) % 3;
        const double p0 = F[d1] * G[d2], p1 = F[d2] * G[d1], p2 = H[d1] * G[d2], p3 = H[d2] * G[d1];
        A[d] = p0 - p1; B[d] = p2 - p3;
    }
    for (int r = 0; r < 4; ++r) f[r][0] = f[r][1] = f[r][2] = 0.0;
    const double a0 = A[0] * A[0], a1 = A[1] * A[1], a2 = A[2] * A[2], b0 = B[0] * B[0], b1 = B[1] * B[1], b2 = B[2] * B[2];
    const double A2 = (a0 + a1) + a2, B2 = (b0 + b1) + b2, Gn = rf_norm(G[0], G[1], G[2]);
    if (A2 < 1e-24 || B2 < 1e-24 || Gn < 1e-12) return 0.0;
    const double c0 = A[0] * B[0], c1 = A[1] * B[1], c2 = A[2] * B[2];
    const double cosphi = (c0 + c1) + c2;
    double BxA[3];
    for (int d = 0; d < 3; ++d) {
        const int d1 = (d + 1) % 3, d2 = (d + 2) % 3;
        const double p0 = B[d1] * A[d2], p1 = B[d2] * A[d1];
        BxA[d] = p0 - p1;
    }
    const double s0 = BxA[0] * G[0], s1 = BxA[1] * G[1], s2 = BxA[2] * G[2];
    const double sinphi = ((s0 + s1) + s2) / Gn;
    const double phi = atan2(sinphi, cosphi);
    const double arg = t.n * phi - t.phase;
    const double E = t.v * (1.0 + cos(arg));
    const double dE = -(t.v * t.n) * sin(arg);
    const double fg0 = F[0] * G[0], fg1 = F[1] * G[1], fg2 = F[2] * G[2], hg0 = H[0] * G[0], hg1 = H[1] * G[1], hg2 = H[2] * G[2];
    const double FG = (fg0 + fg1) + fg2, HG = (hg0 + hg1) + hg2;
    const double ca = Gn / A2, cb = Gn / B2, ta = FG / (A2 * Gn), tb = HG / (B2 * Gn);
    // dphi/dx of the four atoms = wa A + wb B
    const double wa[4] = {-ca, ca + ta, -ta, 0.0}, wb[4] = {0.0, -tb, tb - cb, cb};
    for (int r = 0; r < 4; ++r)
        for (int d = 0; d < 3; ++d) { const double pa = wa[r] * A[d], pb = wb[r] * B[d]; f[r][d] = -(dE * (pa + pb)); }
    return E;
}

// ---- torsion gradient ------------------------------------------------------------------------------------------------------------------
// u = (Y_b - Y_a) / |Y_b - Y_a|; false (u = 0) where the two atoms coincide: such a torsion neither pulls nor turns
MDX_HD inline bool fx_axis(const double* y, const mdx_fx_torsion& t, double u[3]) {
    MDX_RF_EXACT
    const double d0 = y[3u * t.b] - y[3u * t.a], d1 = y[3u * t.b + 1u] - y[3u * t.a + 1u], d2 = y[3u * t.b + 2u] - y[3u * t.a + 2u];
    const double len = rf_norm(d0, d1, d2);
    if (!(len > 0.0)) { u[0] = u[1] = u[2] = 0.0; return false; }
    u[0] = d0 / len; u[1] = d1 / len; u[2] = d2 / len;
    return true;
}

// arm = u x (y_i - y_b)
MDX_HD inline void fx_arm(const double u[3], const double* yi, const double* yb, double arm[3]) {
    MDX_RF_EXACT
    const double r0 = yi[0] - yb[0], r1 = yi[1] - yb[1], r2 = yi[2] - yb[2];
    const double a0 = u[1] * r2, b0 = u[2] * r1, a1 = u[2] * r0, b1 = u[0] * r2, a2 = u[0] * r1, b2 = u[1] * r0;
    arm[0] = a0 - b0; arm[1] = a1 - b1; arm[2] = a2 - b2;
}

// g = sum_{i in M} arm_i . (f_i - v), J = sum |arm_i|^2, A = sum arm_i - members in atom order; y, f: [n][3]
MDX_HD inline void fx_gradient(const double* y, const double* f, uint32_t n, const double v[3], const mdx_fx_torsion& t, double u[3],
                               double& g, double& J, double A[3]) {
    MDX_RF_EXACT
    g = 0.0; J = 0.0; A[0] = A[1] = A[2] = 0.0;
    if (!fx_axis(y, t, u)) return;
    for (uint32_t i = 0; i < n; ++i) {
        if (!fx_member(t.mask, i)) continue;
        double arm[3];
        fx_arm(u, y + 3u * i, y + 3u * t.b, arm);
        const double m0 = f[3u * i] - v[0], m1 = f[3u * i + 1u] - v[1], m2 = f[3u * i + 2u] - v[2];
        const double p0 = arm[0] * m0, p1 = arm[1] * m1, p2 = arm[2] * m2;
        g += (p0 + p1) + p2;
        const double q0 = arm[0] * arm[0], q1 = arm[1] * arm[1], q2 = arm[2] * arm[2];
        J += (q0 + q1) + q2;
        A[0] += arm[0]; A[1] += arm[1]; A[2] += arm[2];
    }
}

// omega_k = g / (J + 1e-6 J + 1e-12): the regularisation of rf_solve carried over to one axis
MDX_HD inline double fx_omega(double g, double J) {
    MDX_RF_EXACT
    const double lam = MDX_RF_LAMBDA_REL * J;
    return g / ((J + lam) + MDX_RF_LAMBDA_ABS);
}

// shift_k = omega_k A_k / n: what recentring takes from every atom
MDX_HD inline void fx_shift(double wk, const double A[3], uint32_t n, double sh[3]) {
    MDX_RF_EXACT
    for (int d = 0; d < 3; ++d) { const double p = wk * A[d]; sh[d] = p / (double)n; }
}

// |u_i|, u_i = v + w x r_i + sum_k ([i in M_k] omega_k arm_ki - shift_k), torsions in order; with no torsion this is rf_speed
MDX_HD inline double fx_speed(const double v[3], const double w[3], const double c[3], const double* y, uint32_t i, uint32_t n_torsions,
                              const mdx_fx_torsion* tor, const double (*axis)[3], const double* wk, const double (*shift)[3]) {
    MDX_RF_EXACT
    const double* yi = y + 3u * i;
    const double r[3] = {yi[0] - c[0], yi[1] - c[1], yi[2] - c[2]};
    const double a0 = w[1] * r[2], b0 = w[2] * r[1], a1 = w[2] * r[0], b1 = w[0] * r[2], a2 = w[0] * r[1], b2 = w[1] * r[0];
    double u[3] = {v[0] + (a0 - b0), v[1] + (a1 - b1), v[2] + (a2 - b2)};
    for (uint32_t k = 0; k < n_torsions; ++k) {
        if (fx_member(tor[k].mask, i)) {
            double arm[3];
            fx_arm(axis[k], yi, y + 3u * tor[k].b, arm);
            for (int d = 0; d < 3; ++d) { const double p = wk[k] * arm[d]; u[d] += p - shift[k][d]; }
        } else
            for (int d = 0; d < 3; ++d) u[d] -= shift[k][d];
    }
    return rf_norm(u[0], u[1], u[2]);
}

// ---- decision and next trial -----------------------------------------------------------------------------------------------------------
// rf_decide with one more condition for MDX_RF_CONVERGED: gmax = max_k |g_k| <= tors_tol.  While a torsion still pulls, the rigid
// tolerances are withheld (no norm is <= -1); everything else is the rigid rule.  On MDX_RF_STORE the trial's angles are accepted.
MDX_HD inline uint32_t fx_decide(mdx_fx_state& s, const mdx_fx_opts& o, uint32_t n_torsions, double S, bool finite, const float* rigid,
                                 double gmax) {
    mdx_rf_opts r = o.rf;
    if (!(gmax <= o.tors_tol)) r.f_tol = -1.0;
    const uint32_t fl = rf_decide(s.rf, r, S, finite, rigid);
    if (fl & MDX_RF_STORE)
        for (uint32_t k = 0; k < n_torsions; ++k) s.th[k] = s.tht[k];
    return fl;
}

// rf_trial, and theta_try = theta + (h / m) omega_k
MDX_HD inline void fx_trial(mdx_fx_state& s, uint32_t n_torsions) {
    MDX_RF_EXACT
    rf_trial(s.rf);
    const double sc = s.rf.h / s.rf.m;
    for (uint32_t k = 0; k < n_torsions; ++k) { const double p = sc * s.wk[k]; s.tht[k] = s.th[k] + p; }
}

// Rodrigues: p <- b + r cos + (u x r) sin + u (u . r)(1 - cos), r = p - b; the axis atom itself (r = 0) stays where it is
MDX_HD inline void fx_rotate(const double u[3], const double b[3], double cs, double sn, double p[3]) {
    MDX_RF_EXACT
    const double r[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
    const double a0 = u[1] * r[2], b0 = u[2] * r[1], a1 = u[2] * r[0], b1 = u[0] * r[2], a2 = u[0] * r[1], b2 = u[1] * r[0];
    const double cr[3] = {a0 - b0, a1 - b1, a2 - b2};
    const double d0 = u[0] * r[0], d1 = u[1] * r[1], d2 = u[2] * r[2];
    const double dt = (d0 + d1) + d2, oc = 1.0 - cs;
    for (int d = 0; d < 3; ++d) {
        const double p0 = r[d] * cs, p1 = cr[d] * sn, p2 = (u[d] * dt) * oc;
        p[d] = b[d] + ((p0 + p1) + p2);
    }
}

// coords(q, t, theta)_i = fp32(c0 + t + R(q) b_i), b_i = B_i(theta) - mean(B(theta)): rf_coords with b given.  With theta = 0, B is the
// input and its mean is c0, so this is rf_coords bit for bit.
MDX_HD inline void fx_coords(const double c0[3], const double t[3], const double R[9], const double B[3], const double mean[3], float y[3]) {
    MDX_RF_EXACT
    const double b0 = B[0] - mean[0], b1 = B[1] - mean[1], b2 = B[2] - mean[2];
    for (int d = 0; d < 3; ++d) {
        const double p0 = R[3 * d] * b0, p1 = R[3 * d + 1] * b1, p2 = R[3 * d + 2] * b2;
        y[d] = (float)((c0[d] + t[d]) + ((p0 + p1) + p2));
    }
}

// B(theta) in place (x: [n][3], the input pose in fp64 on entry): the torsions in caller order, each about its axis as the coordinates then
// stand; theta_k == 0 and a zero-length axis are skipped.  (The kernel runs the same statements with one barrier per torsion.)
MDX_HD inline void fx_build(double* x, uint32_t n, uint32_t n_torsions, const mdx_fx_torsion* tor, const double* theta) {
    for (uint32_t k = 0; k < n_torsions; ++k) {
        if (theta[k] == 0.0) continue;
        double u[3];
        if (!fx_axis(x, tor[k], u)) continue;
        const double cs = cos(theta[k]), sn = sin(theta[k]);
        const double b[3] = {x[3u * tor[k].b], x[3u * tor[k].b + 1u], x[3u * tor[k].b + 2u]};
        for (uint32_t i = 0; i < n; ++i)
            if (i != tor[k].b && fx_member(tor[k].mask, i)) fx_rotate(u, b, cs, sn, x + 3u * i);
    }
}
