// mdx_search_step.h - the rule of mdx_search_poses (include/mdx.h states it): an iterated local search per walker - perturb the
// accepted pose, refine it with the flexible stepper of mdx_flex_step.h, accept or reject by Metropolis, keep the best.  Plain C++ in
// fp64, no HIP types: the search kernels (pose_search of mdx_pose_search_dev.h) call these functions on the device, and a stand-alone host program can include
// this file and call the same ones (tests/cpp/pose_search_driver.cpp).  Where the rule is a stepper's, the function is that stepper's:
// the move's rotation and translation are one rf_trial of unit step, the new start is fx_build / fx_coords of the accepted pose.
//
// As there: fixed order of every sum, contraction off, so that the device, a host compiler and the numpy restatement in
// tests/pose_search_ref.py round alike up to the last bit of sqrt / sin / cos / exp.
#pragma once
#include "mdx_flex_step.h"
#include "mdx_splitmix64.h"

#define MDX_SR_BALL_TRIES 16u                          // rejection tries of the ball draw; after them the zero vector (7e-6 of the draws)
#define MDX_SR_DRAW_CHOICE 0u                          // the draws of a round, by their place in its stream: the coordinate,
#define MDX_SR_DRAW_BALL 1u                            // 16 x 3 cube coordinates,
#define MDX_SR_DRAW_TORSION (1u + 3u * MDX_SR_BALL_TRIES)      // the torsion's angle,
#define MDX_SR_DRAW_ACCEPT (2u + 3u * MDX_SR_BALL_TRIES)       // the acceptance variate - always these 51, whatever the outcome

#define MDX_SR_NONE 0u             // mdx_sr_move.kind
#define MDX_SR_TRANSLATION 1u
#define MDX_SR_ROTATION 2u
#define MDX_SR_TORSION 3u

#define MDX_SR_ACCEPT 1u           // sr_decide: current <- the round's (Y, S)
#define MDX_SR_UPHILL 2u           // ... by the Metropolis condition, not by S_new < S_cur
#define MDX_SR_BEST 4u             // best <- the round's (Y, row, rigid, E_dih, S, r)

struct mdx_sr_opts { double trans_amp, rot_amp, tors_amp, kT; uint64_t seed; uint32_t n_rounds, pad; };

// one walker's search record; its coordinates, best row and best rigid lie beside it (SearchLayout of mdx_pose_plan.h)
struct mdx_sr_record {
    double S_cur, S_best;
    float edih_best; uint32_t best_round;
    uint32_t accepted, uphill, nonfinite, evals;       // rounds >= 1 accepted, of those by the Metropolis condition, non-finite rounds, evaluations
};

struct mdx_sr_move {
    uint32_t kind, torsion, choice, tries;             // choice: j of n_choices; tries: rejected ball tries before the one taken (16: none was)
    double v[3], w[3], dtheta;                         // translation (A), rotation vector (rad), the torsion's angle (rad); what is not moved is 0
};

// ---- the stream of (seed, stream id, round) ------------------------------------------------------------------------------------------
// M(x) = the splitmix64 output of state x (one step from x).  Start state s0 = M(M(M(seed) ^ id) ^ r); draw k of the round is the
// output of the k + 1st step from s0.  splitmix64's state is a counter, so a draw is addressed by its place.
MDX_HD inline uint64_t sr_mix(uint64_t x) { return mdx_splitmix64(&x); }
MDX_HD inline uint64_t sr_stream(uint64_t seed, uint64_t id, uint32_t r) { return sr_mix(sr_mix(sr_mix(seed) ^ id) ^ (uint64_t)r); }
MDX_HD inline uint64_t sr_bits(uint64_t s0, uint32_t k) {
    uint64_t s = s0 + 0x9E3779B97F4A7C15ull * (uint64_t)k;
    return mdx_splitmix64(&s);
}
// u01 = ((x >> 11) + 0.5) 2^-53
MDX_HD inline double sr_u01(uint64_t x) { return ((double)(x >> 11) + 0.5) * (1.0 / 9007199254740992.0); }
MDX_HD inline double sr_draw(uint64_t s0, uint32_t k) { return sr_u01(sr_bits(s0, k)); }

// how many coordinates the move chooses from: translation, rotation, then the T torsions - each where its amplitude is > 0
MDX_HD inline uint32_t sr_choices(const mdx_sr_opts& o, uint32_t n_torsions) {
    return (o.trans_amp > 0.0 ? 1u : 0u) + (o.rot_amp > 0.0 ? 1u : 0u) + (o.tors_amp > 0.0 ? n_torsions : 0u);
}

// ---- the move of a round r >= 1 ---------------------------------------------------------------------------------------------------------
// j = floor(u n_choices) (u = 1, one draw in 2^53, takes the last); the ball: the first of 16 points (2u - 1)^3 of the cube with
// |p|^2 <= 1, else 0; torsion: dtheta = (2u - 1) tors_amp.
MDX_HD inline void sr_move(const mdx_sr_opts& o, uint32_t n_torsions, uint64_t s0, mdx_sr_move& mv) {
    MDX_RF_EXACT
    const uint32_t nt = o.trans_amp > 0.0 ? 1u : 0u, nr = o.rot_amp > 0.0 ? 1u : 0u, n = sr_choices(o, n_torsions);
    mv.kind = MDX_SR_NONE; mv.torsion = 0u; mv.choice = 0u; mv.tries = MDX_SR_BALL_TRIES;
    mv.dtheta = 0.0;
    for (int d = 0; d < 3; ++d) mv.v[d] = mv.w[d] = 0.0;
    if (n == 0u) return;
    uint32_t j = (uint32_t)(sr_draw(s0, MDX_SR_DRAW_CHOICE) * (double)n);
    if (j >= n) j = n - 1u;
    mv.choice = j;
    double p[3] = {0.0, 0.0, 0.0};
    for (uint32_t i = 0; i < MDX_SR_BALL_TRIES; ++i) {
        const double a = 2.0 * sr_draw(s0, MDX_SR_DRAW_BALL + 3u * i) - 1.0, b = 2.0 * sr_draw(s0, MDX_SR_DRAW_BALL + 3u * i + 1u) - 1.0,
                     c = 2.0 * sr_draw(s0, MDX_SR_DRAW_BALL + 3u * i + 2u) - 1.0;
        const double aa = a * a, bb = b * b, cc = c * c;
        if ((aa + bb) + cc <= 1.0) { p[0] = a; p[1] = b; p[2] = c; mv.tries = i; break; }
    }
    if (j < nt) {
        mv.kind = MDX_SR_TRANSLATION;
        for (int d = 0; d < 3; ++d) mv.v[d] = o.trans_amp * p[d];
    } else if (j < nt + nr) {
        mv.kind = MDX_SR_ROTATION;
        for (int d = 0; d < 3; ++d) mv.w[d] = o.rot_amp * p[d];
    } else {
        mv.kind = MDX_SR_TORSION; mv.torsion = j - nt - nr;
        mv.dtheta = (2.0 * sr_draw(s0, MDX_SR_DRAW_TORSION) - 1.0) * o.tors_amp;
    }
}

// (dq, dt) of the move: rf_trial of step h = m = 1 from the identity along (v, w) = (translation, rotation vector) - dt = v, dq the
// rotation by |w| about w / |w|, normalised as every trial's quaternion is
MDX_HD inline void sr_xform(const mdx_sr_move& mv, double q[4], double t[3]) {
    mdx_rf_state s;
    const double zero[3] = {0.0, 0.0, 0.0};
    rf_start(s, zero, 1.0);
    for (int d = 0; d < 3; ++d) { s.v[d] = mv.v[d]; s.w[d] = mv.w[d]; }
    s.m = 1.0;
    rf_trial(s);
    for (int d = 0; d < 4; ++d) q[d] = s.qt[d];
    for (int d = 0; d < 3; ++d) t[d] = s.tt[d];
}

// X0' = fp32(coords(dq, dt, dtheta)) of the flexible stepper with the accepted pose ycur (fp32 [n][3]) as its input; x: [n][3] work space.
// (The kernel runs the same statements, one atom per thread.)
inline void sr_perturb(const float* ycur, uint32_t n, uint32_t n_torsions, const mdx_fx_torsion* tor, const mdx_sr_move& mv, double* x,
                       float* out) {
    double theta[MDX_FX_MAX_TORSIONS] = {}, q[4], t[3], R[9], c0[3], mean[3];
    if (mv.kind == MDX_SR_TORSION) theta[mv.torsion] = mv.dtheta;
    for (uint32_t i = 0; i < 3u * n; ++i) x[i] = (double)ycur[i];
    for (uint32_t d = 0; d < 3u; ++d) c0[d] = rf_mean(x, n, d);
    sr_xform(mv, q, t);
    rf_rotation(q, R);
    fx_build(x, n, n_torsions, tor, theta);
    for (uint32_t d = 0; d < 3u; ++d) mean[d] = rf_mean(x, n, d);
    for (uint32_t i = 0; i < n; ++i) fx_coords(c0, t, R, x + 3u * i, mean, out + 3u * i);
}

// ---- the decision on round r, once its refinement has ended -----------------------------------------------------------------------------
// S, edih, evals: the accepted state of the refinement (S = sum_b (double) row[b] + (double) E_dih); finite: it did not end
// MDX_REFINE_NONFINITE; s0: the round's stream.  Round 0 becomes current and best (S = +inf if it is not finite).  -> MDX_SR_* flags
MDX_HD inline uint32_t sr_decide(mdx_sr_record& rec, const mdx_sr_opts& o, uint32_t r, double S, bool finite, float edih, uint32_t evals,
                                 uint64_t s0) {
    MDX_RF_EXACT
    if (r == 0u) {
        rec.S_cur = rec.S_best = finite ? S : (double)INFINITY;
        rec.edih_best = edih; rec.best_round = 0u;
        rec.accepted = rec.uphill = 0u; rec.nonfinite = finite ? 0u : 1u; rec.evals = evals;
        return MDX_SR_ACCEPT | MDX_SR_BEST;
    }
    rec.evals += evals;
    if (!finite) { rec.nonfinite++; return 0u; }
    uint32_t fl = 0u;
    if (S < rec.S_cur) fl = MDX_SR_ACCEPT;
    else if (o.kT > 0.0) {
        const double d = S - rec.S_cur;
        if (sr_draw(s0, MDX_SR_DRAW_ACCEPT) < exp(-d / o.kT)) fl = MDX_SR_ACCEPT | MDX_SR_UPHILL;
    }
    if (!(fl & MDX_SR_ACCEPT)) return 0u;
    rec.accepted++;
    if (fl & MDX_SR_UPHILL) rec.uphill++;
    rec.S_cur = S;
    if (S < rec.S_best) { rec.S_best = S; rec.edih_best = edih; rec.best_round = r; fl |= MDX_SR_BEST; }
    return fl;
}
