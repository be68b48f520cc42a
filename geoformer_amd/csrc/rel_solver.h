// Calibrated two-view verification: essential-matrix RANSAC with pose recovery and a refit on the inliers for every pair of a match
// list, stated once for the device (k_relpose.hip) and the host (host/relpose_host.cpp).  Plain C++ in fp64 with contraction off, only
// + - * / sqrt, fabs and comparisons, so a host build and gfx950 agree bit for bit.  The minimal solver, the inlier test and the pose
// recovery are pose_solver.h's, included and not edited; OpenCV parity is UNPINNED.
//
//   1. rows         Row i = (x0, y0, x1, y1, score) of a pair takes part iff fs_row_valid: four finite coordinates and, where scores are
//                   given, a score that is not NaN and >= sc_thres.  Surviving rows are compacted stably, in row order; draws and counts
//                   run over the compacted list.
//   2. calibration  Pair n has fp32 K0[n], K1[n].  Coordinates are normalised by ps_normalise, thr = ps_threshold(K0, K1, pixel_thr).  A
//                   pair can be estimated iff it has at least RS_MIN_ROWS (5) surviving rows and the four focal entries are finite and
//                   positive (rs_k_valid).  Nothing else: no bounding-box conditioning, normalised coordinates are the conditioning.
//   3. hypotheses   Hypothesis t of pair n draws five distinct surviving rows with gs_draw_distinct<5>(seed, n, t, cnt); ps_five_point
//                   gives up to 10 E.
//   4. inliers      ps_inlier(E, .., thr^2): the squared Sampson distance on normalised coordinates.
//   5. selection    Most inliers, then the smallest hypothesis, then the smallest root.
//   6. pose         As pose_final of k_pose.hip: ps_decompose gives the four candidates in their fixed order, every inlier of the winner
//                   votes through ps_cheiral (integer counts: order-free), the most votes win, the first on a tie.  The pair is valid iff
//                   the winner has at least 5 inliers, the decomposition succeeded and the best candidate has a vote (n_cheiral);
//                   otherwise outputs and mask are zero, valid 0, best -1.
//   7. refit        (refit_rounds R in 1 .. RS_REFIT_MAX_ROUNDS only; R = 0 is everything above and nothing else.)  cur = (R, t, inlier
//                   set over the surviving rows, count) starts as step 6's, E = [t]x R.  One round:
//                   a. cur has fewer than RS_REFIT_MIN_INLIERS (6) inliers: stop.
//                   b. RS_GN_STEPS (3) Gauss-Newton steps on the signed Sampson residual r = e / sqrt(s) of cur's inliers, e = x1^T E x0,
//                      s = (E x0)_0^2 + (E x0)_1^2 + (E^T x1)_0^2 + (E^T x1)_1^2.  Five parameters (w1, w2, w3, a, b): R <- C(w) R with
//                      the Cayley map (dR / dw_k = 2 [e_k]x R at 0), t <- unit(t + a b1 + b b2) with b1 = unit(t x e_k) for the axis k
//                      of smallest |t_k| (the lowest on a tie) and b2 = t x b1 (rs_tangent).  The Jacobian is analytic and includes the
//                      derivative of s (rs_gn_basis: dE per parameter, rs_gn_row).  The 15 + 5 sums of J^T J and J^T r in the
//                      siblings' order: partial j (0 .. 255) adds the inlier rows with compacted index i = j (mod 256), ascending,
//                      then fs_refit_tree.  gs_solve<5>; a failed pivot test or a non-finite update is a failed fit: cur stays, stop.
//                   c. the candidate is scored over ALL surviving rows with ps_inlier on E = [t]x R (as rs_E builds it, not scaled) and
//                      the same thr^2, no cheirality test; it is accepted iff its count is >= cur's.  Accepted: cur <- candidate,
//                      rounds += 1.  Stop when it was rejected, or when the accepted set equals the one before.
//                   So n_inliers never decreases; rounds = 0 means every output is the five-point winner's, bit for bit; `best` keeps
//                   naming the seeding hypothesis, n_cheiral its votes, and the pose stays on the branch step 6 chose.
//   8. outputs      E fp64 of Frobenius norm 1 (after an accepted refit [t]x R scaled to norm 1: rs_E_unit), R and unit t with
//                   x1 ~ R x0 + t, valid, n_inliers, n_cheiral, best[2], rounds; per row an inlier byte, 0 for filtered rows.
//   9. limits       iters a positive multiple of 64 (the public rule of the siblings; a workgroup solves RS_HYP_PER_WG = 32 of them),
//                   N > 0 and N * iters / 32 <= 2^24, pixel_thr positive and finite, refit_rounds 0 .. 8.
// On a purely planar scene E has its twin solution: either may be returned.  Not built: a homography model test, an adaptive stop,
// robust re-weighting.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fund_solver.h"
#include "pose_solver.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define RS_HYP_PER_WG 32          /* = PS_HYP_PER_WG: 32 x PS_WS_DOUBLES x 8 B = 60,416 B of LDS */
#define RS_MIN_ROWS 5
#define RS_REFIT_MAX_ROUNDS 8
#define RS_REFIT_MIN_INLIERS 6
#define RS_GN_STEPS 3
#define RS_GN_SUMS 20             /* 15 distinct entries of J^T J, then the 5 of J^T r */

// workspace of rs_gn_solve (doubles)
#define RS_GN_OFF_ACC 0           /* [20] */
#define RS_GN_OFF_A 20            /* [5][6] the augmented normal equations */
#define RS_GN_OFF_X 50            /* [5] w1, w2, w3, a, b */
#define RS_GN_WS_DOUBLES 55

GS_HD constexpr int rs_sym5(int i, int j) { return 5 * i - (i * (i - 1)) / 2 + (j - i); }      // i <= j

GS_HD int rs_k_valid(const float* K0, const float* K1) {
    const float f[4] = {K0[0], K0[4], K1[0], K1[4]};
    int ok = 1;
    GS_UNROLL
    for (int k = 0; k < 4; ++k) ok &= (f[k] > 0.f && f[k] < INFINITY);             // a NaN fails the first comparison
    return ok;
}

// a row in normalised coordinates, fp64
struct RsRow { double x0, y0, x1, y1; };
GS_HD RsRow rs_row(const float* m4, const float* K0, const float* K1) {
    RsRow r;
    ps_normalise(K0, m4[0], m4[1], r.x0, r.y0);
    ps_normalise(K1, m4[2], m4[3], r.x1, r.y1);
    return r;
}
GS_HD int rs_inlier(const double (&E)[9], const RsRow& r, double thr2) { return ps_inlier(E, r.x0, r.y0, r.x1, r.y1, thr2); }

GS_HD void rs_cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// D = [u]x M, column by column (the expressions of ps_decompose's [b]x E)
GS_HD void rs_cross_mat(const double (&u)[3], const double (&M)[9], double (&D)[9]) {
    GS_UNROLL
    for (int j = 0; j < 3; ++j) {
        D[0 + j] = u[1] * M[6 + j] - u[2] * M[3 + j];
        D[3 + j] = u[2] * M[0 + j] - u[0] * M[6 + j];
        D[6 + j] = u[0] * M[3 + j] - u[1] * M[0 + j];
    }
}
GS_HD void rs_E(const double (&R)[9], const double (&t)[3], double (&E)[9]) { rs_cross_mat(t, R, E); }

// [t]x R scaled to Frobenius norm 1; 0 for a zero or non-finite norm
GS_HD int rs_E_unit(const double (&R)[9], const double (&t)[3], double (&E)[9]) {
    rs_E(R, t, E);
    double n2 = 0.0;
    GS_UNROLL
    for (int q = 0; q < 9; ++q) n2 = n2 + E[q] * E[q];
    const double n = sqrt(n2);
    if (!(n > 0.0) || !(n < (double)INFINITY)) return 0;
    GS_UNROLL
    for (int q = 0; q < 9; ++q) E[q] = E[q] / n;
    return 1;
}

// the tangent basis of the unit sphere at t: b1 = unit(t x e_k) for the axis k of smallest |t_k| (the lowest on a tie), b2 = t x b1
GS_HD int rs_tangent(const double (&t)[3], double (&b1)[3], double (&b2)[3]) {
    int k = 0;
    if (fabs(t[1]) < fabs(t[0])) k = 1;
    if (fabs(t[2]) < fabs(k == 1 ? t[1] : t[0])) k = 2;
    const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    double c[3];
    rs_cross(t, e, c);
    const double n = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    if (!(n > 0.0) || !(n < (double)INFINITY)) return 0;
    GS_UNROLL
    for (int i = 0; i < 3; ++i) b1[i] = c[i] / n;
    rs_cross(t, b1, b2);
    return 1;
}

// dE per parameter at 0: D[k] = [t]x (2 [e_k]x R) for w_k, D[3] = [b1]x R, D[4] = [b2]x R; 0 when t has no tangent basis
GS_HD int rs_gn_basis(const double (&R)[9], const double (&t)[3], double (&D)[5][9]) {
    double b1[3], b2[3];
    if (!rs_tangent(t, b1, b2)) return 0;
    GS_UNROLL
    for (int k = 0; k < 3; ++k) {
        const double e2[3] = {k == 0 ? 2.0 : 0.0, k == 1 ? 2.0 : 0.0, k == 2 ? 2.0 : 0.0};
        double dR[9];
        rs_cross_mat(e2, R, dR);
        rs_cross_mat(t, dR, D[k]);
    }
    rs_cross_mat(b1, R, D[3]);
    rs_cross_mat(b2, R, D[4]);
    return 1;
}

// the signed Sampson residual r = e / sqrt(s) of a row under E and its derivatives by the five parameters; 0 for a row without a
// positive finite s (it adds nothing)
GS_HD int rs_gn_row(const double (&E)[9], const double (&D)[5][9], const RsRow& q, double (&J)[5], double& res) {
    const double x0 = q.x0, y0 = q.y0, x1 = q.x1, y1 = q.y1;
    const double a0 = (E[0] * x0 + E[1] * y0) + E[2], a1 = (E[3] * x0 + E[4] * y0) + E[5], a2 = (E[6] * x0 + E[7] * y0) + E[8];
    const double b0 = (E[0] * x1 + E[3] * y1) + E[6], b1 = (E[1] * x1 + E[4] * y1) + E[7];
    const double e = (x1 * a0 + y1 * a1) + a2;
    const double s = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1;
    if (!(s > 0.0) || !(s < (double)INFINITY)) return 0;
    const double rs = sqrt(s);
    res = e / rs;
    const double g = e / (s * rs);                                    // dr = de / sqrt(s) - (e / (s sqrt(s))) (ds / 2)
    GS_UNROLL
    for (int p = 0; p < 5; ++p) {
        const double (&P)[9] = D[p];
        const double da0 = (P[0] * x0 + P[1] * y0) + P[2], da1 = (P[3] * x0 + P[4] * y0) + P[5], da2 = (P[6] * x0 + P[7] * y0) + P[8];
        const double db0 = (P[0] * x1 + P[3] * y1) + P[6], db1 = (P[1] * x1 + P[4] * y1) + P[7];
        const double de = (x1 * da0 + y1 * da1) + da2;
        const double hs = ((a0 * da0 + a1 * da1) + b0 * db0) + b1 * db1;
        J[p] = de / rs - g * hs;
    }
    return 1;
}

GS_HD void rs_gn_accum(double (&acc)[RS_GN_SUMS], const double (&J)[5], double res) {
    GS_UNROLL
    for (int i = 0; i < 5; ++i) {
        GS_UNROLL
        for (int j = i; j < 5; ++j) acc[rs_sym5(i, j)] = acc[rs_sym5(i, j)] + J[i] * J[j];
        acc[15 + i] = acc[15 + i] + J[i] * res;
    }
}

// the sums at RS_GN_OFF_ACC -> the step at RS_GN_OFF_X; 0 when the system cannot be solved
GS_HD int rs_gn_solve(const GsWs& w) {
    for (int i = 0; i < 5; ++i) {
        for (int j = 0; j < 5; ++j) w(RS_GN_OFF_A + 6 * i + j) = w(RS_GN_OFF_ACC + (i <= j ? rs_sym5(i, j) : rs_sym5(j, i)));
        w(RS_GN_OFF_A + 6 * i + 5) = -w(RS_GN_OFF_ACC + 15 + i);
    }
    return gs_solve<5>(w, RS_GN_OFF_A, RS_GN_OFF_X);
}

// R <- C(w) R (the Cayley map as as_gn_update of abs_solver.h writes it), t <- unit(t + a b1 + b b2); 0 when the result is not finite
GS_HD int rs_gn_update(const double (&d)[5], double (&R)[9], double (&t)[3]) {
    const double wx = d[0], wy = d[1], wz = d[2];
    const double ww = (wx * wx + wy * wy) + wz * wz, den = 1.0 + ww, one = 1.0 - ww;
    double C[9];
    C[0] = (one + 2.0 * (wx * wx)) / den; C[1] = (2.0 * (wx * wy) - 2.0 * wz) / den; C[2] = (2.0 * (wx * wz) + 2.0 * wy) / den;
    C[3] = (2.0 * (wy * wx) + 2.0 * wz) / den; C[4] = (one + 2.0 * (wy * wy)) / den; C[5] = (2.0 * (wy * wz) - 2.0 * wx) / den;
    C[6] = (2.0 * (wz * wx) - 2.0 * wy) / den; C[7] = (2.0 * (wz * wy) + 2.0 * wx) / den; C[8] = (one + 2.0 * (wz * wz)) / den;
    double b1[3], b2[3], Rn[9], tn[3];
    if (!rs_tangent(t, b1, b2)) return 0;
    GS_UNROLL
    for (int i = 0; i < 3; ++i) {
        GS_UNROLL
        for (int k = 0; k < 3; ++k) Rn[3 * i + k] = (C[3 * i] * R[k] + C[3 * i + 1] * R[3 + k]) + C[3 * i + 2] * R[6 + k];
        tn[i] = (t[i] + d[3] * b1[i]) + d[4] * b2[i];
    }
    const double n = sqrt((tn[0] * tn[0] + tn[1] * tn[1]) + tn[2] * tn[2]);
    if (!(n > 0.0) || !(n < (double)INFINITY)) return 0;
    int finite = 1;
    GS_UNROLL
    for (int k = 0; k < 9; ++k) finite &= (Rn[k] - Rn[k] == 0.0);
    if (!finite) return 0;
    GS_UNROLL
    for (int k = 0; k < 9; ++k) R[k] = Rn[k];
    GS_UNROLL
    for (int k = 0; k < 3; ++k) t[k] = tn[k] / n;
    return 1;
}
