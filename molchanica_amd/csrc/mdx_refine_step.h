// mdx_refine_step.h - the stepper of mdx_refine_poses (include/mdx.h states the rule): a rigid-body steepest descent with an adaptive
// step length, one state record per pose.  Plain C++ in fp64, no HIP types: pose_refine_step_kernel (mdx_poses.hip) calls these
// functions on the device, and a stand-alone host program can include this file and call the same ones (tests/cpp/pose_refine_driver.cpp).
//
// Every function keeps its sums in a fixed order and switches floating-point contraction off, so the device, a host compiler and the
// numpy restatement in tests/pose_refine_ref.py round alike; what is left to differ is the last bit of sqrt / sin / cos.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MDX_HD __host__ __device__
#else
#define MDX_HD
#endif
#if defined(__clang__)
#define MDX_RF_EXACT _Pragma("clang fp contract(off)")
#else
#define MDX_RF_EXACT
#endif

#define MDX_RF_CONVERGED 0u      // the MDX_REFINE_* values of include/mdx.h
#define MDX_RF_MAX_EVALS 1u
#define MDX_RF_STALLED 2u
#define MDX_RF_NONFINITE 3u
#define MDX_RF_H_MIN 1.0e-5      // A: about one fp32 ulp of a coordinate at 100 A; below it the trial is the accepted pose
#define MDX_RF_LAMBDA_REL 1.0e-6 // lambda = MDX_RF_LAMBDA_REL trace(I) + MDX_RF_LAMBDA_ABS regularises the inertia tensor:
#define MDX_RF_LAMBDA_ABS 1.0e-12 // (A^2) one atom, two atoms and collinear atoms have a null axis, about which a rotation moves nothing

#define MDX_RF_STORE 1u          // rf_decide: the trial is the accepted state now - the caller keeps its coordinates, row and rigid
#define MDX_RF_FROZEN 2u         // rf_decide / rf_direction: the pose is finished

struct mdx_rf_opts { double f_tol, tau_tol, h_start, h_max; };

struct mdx_rf_state {
    double q[4], t[3];           // accepted rotation (w, x, y, z) and translation
    double qt[4], tt[3];         // those of the trial being evaluated
    double c0[3];                // centroid of the input pose
    double v[3], w[3], m;        // descent direction of the accepted state: translation, angular velocity, largest atom speed
    double h, S;                 // step length (A), sum of the accepted row
    uint32_t status, evals, frozen, pad;
};

MDX_HD inline void rf_start(mdx_rf_state& s, const double c0[3], double h_start) {
    s.q[0] = s.qt[0] = 1.0;
    for (int d = 1; d < 4; ++d) s.q[d] = s.qt[d] = 0.0;
    for (int d = 0; d < 3; ++d) { s.t[d] = s.tt[d] = 0.0; s.c0[d] = c0[d]; s.v[d] = s.w[d] = 0.0; }
    s.m = 0.0; s.h = h_start; s.S = 0.0;
    s.status = MDX_RF_MAX_EVALS; s.evals = 0; s.frozen = 0; s.pad = 0;
}

// component d of the unweighted mean of x[n][3], atoms in order
MDX_HD inline double rf_mean(const double* x, uint32_t n, uint32_t d) {
    MDX_RF_EXACT
    double c = 0.0;
    for (uint32_t i = 0; i < n; ++i) c += x[i * 3u + d];
    return c / (double)n;
}

// element k of I = sum_i (|r_i|^2 E - r_i r_i^T), r_i = x_i - c, atoms in order: k = 0 xx, 1 yy, 2 zz, 3 xy, 4 xz, 5 yz
MDX_HD inline double rf_inertia(const double* x, uint32_t n, const double c[3], uint32_t k) {
    MDX_RF_EXACT
    const uint32_t d1 = k < 3u ? (k + 1u) % 3u : (k == 5u ? 1u : 0u), d2 = k < 3u ? (k + 2u) % 3u : (k == 3u ? 1u : 2u);
    double v = 0.0;
    for (uint32_t i = 0; i < n; ++i) {
        const double a = x[i * 3u + d1] - c[d1], b = x[i * 3u + d2] - c[d2];
        if (k < 3u) { const double aa = a * a, bb = b * b; v += aa + bb; }
        else { const double ab = a * b; v += ab; }
    }
    return k < 3u ? v : -v;
}

// w = (I + lambda E)^-1 tau through the adjugate of the symmetric matrix
MDX_HD inline void rf_solve(const double I[6], const double tau[3], double w[3]) {
    MDX_RF_EXACT
    const double lam = MDX_RF_LAMBDA_REL * ((I[0] + I[1]) + I[2]) + MDX_RF_LAMBDA_ABS;
    const double a = I[0] + lam, d = I[1] + lam, f = I[2] + lam, b = I[3], c = I[4], e = I[5];
    const double df = d * f, ee = e * e, ce = c * e, bf = b * f, be = b * e, cd = c * d, af = a * f, cc = c * c, bc = b * c, ae = a * e,
                 ad = a * d, bb = b * b;
    const double c00 = df - ee, c01 = ce - bf, c02 = be - cd, c11 = af - cc, c12 = bc - ae, c22 = ad - bb;
    const double p0 = a * c00, p1 = b * c01, p2 = c * c02;
    const double det = (p0 + p1) + p2;
    const double x0 = c00 * tau[0], x1 = c01 * tau[1], x2 = c02 * tau[2];
    const double y0 = c01 * tau[0], y1 = c11 * tau[1], y2 = c12 * tau[2];
    const double z0 = c02 * tau[0], z1 = c12 * tau[1], z2 = c22 * tau[2];
    w[0] = ((x0 + x1) + x2) / det;
    w[1] = ((y0 + y1) + y2) / det;
    w[2] = ((z0 + z1) + z2) / det;
}

MDX_HD inline double rf_norm(double x, double y, double z) {
    MDX_RF_EXACT
    const double xx = x * x, yy = y * y, zz = z * z;
    return sqrt((xx + yy) + zz);
}

// |v + w x r|: how fast the atom at r (from the centroid) moves under the rigid motion (v, w)
MDX_HD inline double rf_speed(const double v[3], const double w[3], const double r[3]) {
    MDX_RF_EXACT
    const double a0 = w[1] * r[2], b0 = w[2] * r[1], a1 = w[2] * r[0], b1 = w[0] * r[2], a2 = w[0] * r[1], b2 = w[1] * r[0];
    return rf_norm(v[0] + (a0 - b0), v[1] + (a1 - b1), v[2] + (a2 - b2));
}

// Evaluation number s.evals of the pose: S = the sum of the trial's row, rigid = its net force and torque, finite = nothing in
// the row, the forces or rigid is inf or NaN.  -> MDX_RF_STORE and / or MDX_RF_FROZEN
MDX_HD inline uint32_t rf_decide(mdx_rf_state& s, const mdx_rf_opts& o, double S, bool finite, const float* rigid) {
    MDX_RF_EXACT
    const uint32_t k = s.evals++;
    if (!finite && k == 0u) { s.S = S; s.status = MDX_RF_NONFINITE; s.frozen = 1u; return MDX_RF_STORE | MDX_RF_FROZEN; }
    if (finite && (k == 0u || S < s.S)) {
        for (int d = 0; d < 4; ++d) s.q[d] = s.qt[d];
        for (int d = 0; d < 3; ++d) s.t[d] = s.tt[d];
        s.S = S;
        if (k > 0u) { const double g = 1.2 * s.h; s.h = g < o.h_max ? g : o.h_max; }
        if (rf_norm((double)rigid[0], (double)rigid[1], (double)rigid[2]) <= o.f_tol &&
            rf_norm((double)rigid[3], (double)rigid[4], (double)rigid[5]) <= o.tau_tol) {
            s.status = MDX_RF_CONVERGED; s.frozen = 1u;
            return MDX_RF_STORE | MDX_RF_FROZEN;
        }
        return MDX_RF_STORE;
    }
    s.h = 0.5 * s.h;
    if (s.h < MDX_RF_H_MIN) { s.status = MDX_RF_STALLED; s.frozen = 1u; return MDX_RF_FROZEN; }
    return 0u;
}

// after MDX_RF_STORE alone: the direction of the newly accepted state, from its rigid and the inertia tensor of its coordinates
MDX_HD inline void rf_direction(mdx_rf_state& s, uint32_t n, const float* rigid, const double I[6]) {
    MDX_RF_EXACT
    const double tau[3] = {(double)rigid[3], (double)rigid[4], (double)rigid[5]};
    for (int d = 0; d < 3; ++d) s.v[d] = (double)rigid[d] / (double)n;
    rf_solve(I, tau, s.w);
}

// ... and its largest atom speed m = max_i rf_speed(s.v, s.w, x_i - c); m == 0: nothing pulls, the pose has converged
MDX_HD inline uint32_t rf_set_speed(mdx_rf_state& s, double m) {
    s.m = m;
    if (m == 0.0) { s.status = MDX_RF_CONVERGED; s.frozen = 1u; return MDX_RF_FROZEN; }
    return 0u;
}

// the next trial, always from the accepted state: no atom moves further than h
MDX_HD inline void rf_trial(mdx_rf_state& s) {
    MDX_RF_EXACT
    const double sc = s.h / s.m;
    for (int d = 0; d < 3; ++d) { const double p = sc * s.v[d]; s.tt[d] = s.t[d] + p; }
    const double wn = rf_norm(s.w[0], s.w[1], s.w[2]);
    if (wn == 0.0) { for (int d = 0; d < 4; ++d) s.qt[d] = s.q[d]; return; }
    const double half = 0.5 * (sc * wn), sn = sin(half), a = cos(half);
    const double b = sn * (s.w[0] / wn), c = sn * (s.w[1] / wn), e = sn * (s.w[2] / wn);
    const double* q = s.q;
    // dq (x) q: the step's rotation after the accepted one
    const double aw = a * q[0], bx = b * q[1], cy = c * q[2], ez = e * q[3];
    const double ax = a * q[1], bw = b * q[0], cz = c * q[3], ey = e * q[2];
    const double ay = a * q[2], bz = b * q[3], cw = c * q[0], ex = e * q[1];
    const double az = a * q[3], by = b * q[2], cx = c * q[1], ew = e * q[0];
    const double r0 = ((aw - bx) - cy) - ez, r1 = ((ax + bw) + cz) - ey, r2 = ((ay - bz) + cw) + ex, r3 = ((az + by) - cx) + ew;
    const double r00 = r0 * r0, r11 = r1 * r1, r22 = r2 * r2, r33 = r3 * r3;
    const double nn = sqrt(((r00 + r11) + r22) + r33);
    s.qt[0] = r0 / nn; s.qt[1] = r1 / nn; s.qt[2] = r2 / nn; s.qt[3] = r3 / nn;
}

// R(q), row-major; the identity quaternion gives the identity matrix exactly
MDX_HD inline void rf_rotation(const double q[4], double R[9]) {
    MDX_RF_EXACT
    const double xx = q[1] * q[1], yy = q[2] * q[2], zz = q[3] * q[3], xy = q[1] * q[2], xz = q[1] * q[3], yz = q[2] * q[3],
                 wx = q[0] * q[1], wy = q[0] * q[2], wz = q[0] * q[3];
    R[0] = 1.0 - 2.0 * (yy + zz); R[1] = 2.0 * (xy - wz); R[2] = 2.0 * (xz + wy);
    R[3] = 2.0 * (xy + wz); R[4] = 1.0 - 2.0 * (xx + zz); R[5] = 2.0 * (yz - wx);
    R[6] = 2.0 * (xz - wy); R[7] = 2.0 * (yz + wx); R[8] = 1.0 - 2.0 * (xx + yy);
}

// coords(q, t)_i = fp32(c0 + t + R(q) b_i), b_i = x0_i - c0.  With R the identity and t = 0 this is x0_i bit for bit: 1 b + 0 + 0 = b, and
// c0 + (x0 - c0) lies within 2^-52 relative of the fp32 value x0, so it rounds back to it.
MDX_HD inline void rf_coords(const double c0[3], const double t[3], const double R[9], const float x0[3], float y[3]) {
    MDX_RF_EXACT
    const double b0 = (double)x0[0] - c0[0], b1 = (double)x0[1] - c0[1], b2 = (double)x0[2] - c0[2];
    for (int d = 0; d < 3; ++d) {
        const double p0 = R[3 * d] * b0, p1 = R[3 * d + 1] * b1, p2 = R[3 * d + 2] * b2;
        y[d] = (float)((c0[d] + t[d]) + ((p0 + p1) + p2));
    }
}
