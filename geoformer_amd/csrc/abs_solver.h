// Absolute-pose RANSAC for localising a query image from 2-D - 3-D correspondences: the algorithm, stated once for the device
// (k_abspose.hip) and the host (host/abspose_host.cpp).  Plain C++ in fp64 with contraction off, only + - * / sqrt, fabs and comparisons
// (solver_common.h) - no acos, cos or atan anywhere - so a host build and gfx950 agree bit for bit.
//
//   rows            A row is (u, v) in query pixels and (X, Y, Z) in world units, fp32, with a score.  It takes part iff as_row_valid: its
//                   five numbers are finite and, where scores are given, its score is not NaN and >= sc_thres.  Surviving rows are
//                   compacted stably, in row order; draws and counts run over the compacted list.  A problem is a QUERY: its rows may
//                   come from several database images.
//   as_box_norm     Conditioning of the 3-D side.  nm = (cx, cy, cz, s): the centre of the bounding box of the surviving 3-D points and
//                   half its longest side (fs_box_norm on three axes: min / max, order-free).  X' = (X - c) / s.  s = 0 or not finite:
//                   no model.  The 2-D side: as_bearing, the unit vector of ((u - K[2]) / K[0], (v - K[5]) / K[4], 1) - ps_normalise's
//                   arithmetic; K is the query's fp32 [9].
//   as_draw3        three distinct surviving rows of hypothesis t of problem n from draw(seed, n, t, k, attempt), as gs_draw_distinct; a
//                   candidate that repeats an already drawn row's 2-D point OR its 3-D point is drawn again (the rule of fs_draw7).
//   as_p3p          The minimal solver: GRUNERT's formulation of the three-point problem with the quartic of Haralick, Lee, Ottenberg
//                   and Noelle (IJCV 13, 1994, eqs. 9 - 10).  a = |P2 P3|, b = |P1 P3|, c = |P1 P2| in conditioned coordinates, alpha,
//                   beta, gamma the angles between the bearings (j2, j3), (j1, j3), (j1, j2) - only their cosines, as dot products.
//                   With s2 = u s1, s3 = v s1: the quartic A4 v^4 + .. + A0 = 0, real roots by gs_real_roots<4>, ascending;
//                   u = ((q - 1) v^2 - 2 q cos(beta) v + 1 + q) / (2 (cos(gamma) - v cos(alpha))), q = (a^2 - c^2) / b^2;
//                   s1 = sqrt(b^2 / (1 + v^2 - 2 v cos(beta))).  A root is kept iff |2 (cos(gamma) - v cos(alpha))| > AS_DEN_TINY and
//                   s1, s2, s3 are finite and positive.  The pose in closed form from the two triangles T = (P1, P2, P3) and
//                   (s1 j1, s2 j2, s3 j3), no SVD: the orthonormal frame e1 = (T1 - T0) / |.|, e3 = e1 x (T2 - T0) / |.|, e2 = e3 x e1 of
//                   each, R = F_cam F_world^T, t' = Q0 - R P0.  At most 4 solutions.  No solution for non-finite input, a triangle whose
//                   sin^2 at P1 is <= AS_SIN2_TINY (collinear or coincident points) or two bearings with 1 - cos^2 <= AS_BEAR_TINY.
//   solution        9 doubles: rows 0 and 1 of R, then t'.  Row 2 is rebuilt as row 0 x row 1 by as_unpack, the ONE place where that is
//                   written; nothing else ever reads a pose out of a solution.
//   as_inlier       Y = R X' + t' (the camera frame, in units of s).  Inlier iff Y.z > 0 and the squared reprojection error in pixels,
//                   (K[0] Y.x / Y.z + K[2] - u)^2 + (K[4] Y.y / Y.z + K[5] - v)^2, is < thr^2 (a NaN is never an inlier).
//   selection       most inliers, then the smallest hypothesis, then the smallest root (rt_key).  valid = 1 iff at least AS_MIN_ROWS (4)
//                   rows survive, the box has an extent and some hypothesis produced a solution.  The mask is the winner's inlier set
//                   over the problem's ORIGINAL rows; filtered rows are 0.
//   output          as_to_world: R as it is, t = s t' - R c, so that x_cam = R X + t in world units.
//
//   refit           (refit_rounds R in 1 .. AS_REFIT_MAX_ROUNDS only; R = 0 is everything above and nothing else.)
//                   cur = (R, t', inlier set over the surviving rows, count) starts as the winner's.  One round:
//                   1. cur has fewer than AS_REFIT_MIN_INLIERS (6) inliers: stop.
//                   2. AS_GN_STEPS (3) Gauss-Newton steps on cur's inlier set, from cur's pose, minimising the reprojection error in
//                      pixels.  A step: as_gn_row gives the two residuals of a row and their derivatives by (omega, tau) at 0 for the
//                      update R <- C(omega) R, t' <- C(omega) t' + tau, C the Cayley map ((1 - w.w) I + 2 w w^T + 2 [w]x) / (1 + w.w): an
//                      exact rotation from rational arithmetic, C = I + 2 [w]x to first order.  A row of the set whose Y.z is not > 0
//                      under the step's pose adds nothing.  as_gn_accum adds the 21 distinct entries of J^T J (as_sym6) and the 6 of
//                      J^T r: 27 numbers, summed in the order of the fundamental refit - partial j (0 .. 255) starts from +0.0 and adds
//                      the set's rows with compacted index i = j (mod 256), ascending, then fs_refit_tree.  as_gn_solve: J^T J d = -J^T r
//                      by gs_solve<6>, then as_gn_update.
//                   3. a failed solve or a non-finite pose: the round fails; cur stays, stop.
//                   4. the candidate is scored over ALL surviving rows with as_inlier's rule and the same thr^2; it is accepted iff its
//                      count is >= cur's.  Accepted: cur <- candidate, rounds += 1.  Stop when it was rejected, or when the accepted set
//                      equals the one before.
//                   So n_inliers never decreases; rounds = 0 means every output is the P3P winner's, bit for bit; `hypothesis` keeps
//                   naming the (hypothesis, root) that seeded the result.
//
// NOT part of this: no covisibility clustering of the database images, no adaptive stop, no robust re-weighting, no distortion parameters.
// pycolmap parity is UNPINNED; what is pinned is the algorithm written here.
//
// Workspace: AS_WS_DOUBLES doubles through GsWs for as_p3p, AS_GN_WS_DOUBLES for as_gn_solve.
#pragma once
#include "fund_solver.h"
#include "solver_common.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define AS_MAX_ROOTS 4
#define AS_HYP_PER_WG 64          /* hypotheses one workgroup of rt_score<AbsModel> solves: iters must be a positive multiple */
#define AS_MIN_ROWS 4
#define AS_BISECT_LOW 40
#define AS_BISECT_TOP 56
#define AS_NEWTON 4
#define AS_DEN_TINY 1e-12
#define AS_SIN2_TINY 1e-16
#define AS_BEAR_TINY 1e-12

// workspace layout (doubles)
#define AS_OFF_P 0                /* [5] the quartic, ascending */
#define AS_OFF_R0 5               /* [6] roots of the previous derivative */
#define AS_OFF_R1 11              /* [6] roots being found */
#define AS_OFF_SOL 17             /* [4][9] the solutions */
#define AS_WS_DOUBLES 53

GS_HD bool as_row_valid(const float* uv, const float* xyz, const float* scores, long i, float sc_thres) {
    const bool fin = kp_finite(uv[0]) && kp_finite(uv[1]) && kp_finite(xyz[0]) && kp_finite(xyz[1]) && kp_finite(xyz[2]);
    return fin && (scores ? scores[i] >= sc_thres : true);
}

// mn, mx [3]: the bounding box of the 3-D points -> nm (centre, half the longest side); 0 for a box without extent
GS_HD int as_box_norm(const float* mn, const float* mx, double* nm4) {
    double s = 0.0;
    GS_UNROLL
    for (int k = 0; k < 3; ++k) {
        nm4[k] = 0.5 * ((double)mn[k] + (double)mx[k]);
        const double h = 0.5 * ((double)mx[k] - (double)mn[k]);
        s = h > s ? h : s;
    }
    nm4[3] = s;
    return s > 0.0 && s < (double)INFINITY;
}

// three distinct positions of the compacted list `rows` (cnt entries, row indices into uv [..][2] and xyz [..][3]) of hypothesis t
GS_HD int as_draw3(uint32_t seed, uint32_t sample, uint32_t t, int cnt, const float* uv, const float* xyz, const int32_t* rows, int (&idx)[3]) {
    int ok = 1;
    float p[3][5];
    GS_UNROLL
    for (int k = 0; k < 3; ++k) {
        idx[k] = 0;
        p[k][0] = p[k][1] = p[k][2] = p[k][3] = p[k][4] = 0.f;
    }
    GS_UNROLL
    for (int k = 0; k < 3; ++k) {
        int found = 0;
        for (uint32_t attempt = 0; attempt < GS_DRAW_ATTEMPTS && !found && ok; ++attempt) {
            const int c = (int)(draw(seed, sample, t, (uint32_t)k, attempt) % (uint32_t)cnt);
            const float* q = uv + 2 * (long)rows[c];
            const float* x = xyz + 3 * (long)rows[c];
            const float q0 = q[0], q1 = q[1], x0 = x[0], x1 = x[1], x2 = x[2];
            int dup = 0;
            GS_UNROLL
            for (int j = 0; j < 3; ++j)
                dup |= (j < k && (idx[j] == c || (p[j][0] == q0 && p[j][1] == q1) || (p[j][2] == x0 && p[j][3] == x1 && p[j][4] == x2)));
            if (!dup) { idx[k] = c; p[k][0] = q0; p[k][1] = q1; p[k][2] = x0; p[k][3] = x1; p[k][4] = x2; found = 1; }
        }
        if (!found) ok = 0;
    }
    return ok;
}

GS_HD void as_cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
GS_HD double as_dot(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the unit bearing of pixel (u, v) through K
GS_HD void as_bearing(const float* K, double u, double v, double (&j)[3]) {
    const double x = (u - (double)K[2]) / (double)K[0], y = (v - (double)K[5]) / (double)K[4];
    const double n = sqrt((x * x + y * y) + 1.0);
    j[0] = x / n; j[1] = y / n; j[2] = 1.0 / n;
}

// the orthonormal frame of a triangle: e[0] = (T1 - T0) / |.|, e[2] = e[0] x (T2 - T0) / |.|, e[1] = e[2] x e[0]; 0 when a norm is not
// positive and finite
GS_HD int as_frame(const double (&T0)[3], const double (&T1)[3], const double (&T2)[3], double (&e)[3][3]) {
    double d1[3], d2[3], c[3];
    GS_UNROLL
    for (int k = 0; k < 3; ++k) { d1[k] = T1[k] - T0[k]; d2[k] = T2[k] - T0[k]; }
    const double n1 = sqrt(as_dot(d1, d1));
    if (!(n1 > 0.0) || !(n1 < (double)INFINITY)) return 0;
    GS_UNROLL
    for (int k = 0; k < 3; ++k) e[0][k] = d1[k] / n1;
    as_cross(e[0], d2, c);
    const double n3 = sqrt(as_dot(c, c));
    if (!(n3 > 0.0) || !(n3 < (double)INFINITY)) return 0;
    GS_UNROLL
    for (int k = 0; k < 3; ++k) e[2][k] = c[k] / n3;
    as_cross(e[2], e[0], e[1]);
    return 1;
}

// a solution (rows 0 and 1 of R, t') -> R [9] row-major and t' [3]
GS_HD void as_unpack(const double (&S)[9], double (&R)[9], double (&t)[3]) {
    GS_UNROLL
    for (int k = 0; k < 6; ++k) R[k] = S[k];
    R[6] = S[1] * S[5] - S[2] * S[4];
    R[7] = S[2] * S[3] - S[0] * S[5];
    R[8] = S[0] * S[4] - S[1] * S[3];
    t[0] = S[6]; t[1] = S[7]; t[2] = S[8];
}

// uv: three pixels; Xw: their 3-D points in world units; nm = (c, s).  Returns the number of solutions (0 .. 4) left at AS_OFF_SOL in
// CONDITIONED coordinates, in ascending order of the quartic's root.
GS_HD int as_p3p(const double (&uv)[3][2], const double (&Xw)[3][3], const float* K, const double (&nm)[4], const GsWs& w) {
    double P[3][3], j[3][3];
    GS_UNROLL
    for (int i = 0; i < 3; ++i) {
        GS_UNROLL
        for (int k = 0; k < 3; ++k) P[i][k] = (Xw[i][k] - nm[k]) / nm[3];
        as_bearing(K, uv[i][0], uv[i][1], j[i]);
    }
    double d12[3], d13[3], d23[3], cr[3];
    GS_UNROLL
    for (int k = 0; k < 3; ++k) { d12[k] = P[1][k] - P[0][k]; d13[k] = P[2][k] - P[0][k]; d23[k] = P[2][k] - P[1][k]; }
    const double a2 = as_dot(d23, d23), b2 = as_dot(d13, d13), c2 = as_dot(d12, d12);
    as_cross(d12, d13, cr);
    const double area2 = as_dot(cr, cr), lim = c2 * b2;
    if (!(lim < (double)INFINITY) || !(area2 > AS_SIN2_TINY * lim)) return 0;          // (a NaN fails the second test)
    const double ca = as_dot(j[1], j[2]), cb = as_dot(j[0], j[2]), cg = as_dot(j[0], j[1]);
    if (!(1.0 - ca * ca > AS_BEAR_TINY) || !(1.0 - cb * cb > AS_BEAR_TINY) || !(1.0 - cg * cg > AS_BEAR_TINY)) return 0;
    double ew[3][3];
    if (!as_frame(P[0], P[1], P[2], ew)) return 0;
    const double q1 = (a2 - c2) / b2, q2 = (a2 + c2) / b2, q3 = (b2 - c2) / b2, q4 = (b2 - a2) / b2, ra = a2 / b2, rc = c2 / b2;
    w(AS_OFF_P + 4) = (q1 - 1.0) * (q1 - 1.0) - (4.0 * rc) * (ca * ca);
    w(AS_OFF_P + 3) = 4.0 * (((q1 * (1.0 - q1)) * cb - ((1.0 - q2) * ca) * cg) + ((2.0 * rc) * (ca * ca)) * cb);
    w(AS_OFF_P + 2) = 2.0 * (((((q1 * q1 - 1.0) + ((2.0 * (q1 * q1)) * (cb * cb))) + ((2.0 * q3) * (ca * ca))) - (((4.0 * q2) * ca) * cb) * cg) +
                             ((2.0 * q4) * (cg * cg)));
    w(AS_OFF_P + 1) = 4.0 * (((-(q1 * (1.0 + q1)) * cb) + (((2.0 * ra) * (cg * cg)) * cb)) - ((1.0 - q2) * ca) * cg);
    w(AS_OFF_P + 0) = (1.0 + q1) * (1.0 + q1) - (4.0 * ra) * (cg * cg);
    const int nz = gs_real_roots<4>(w, AS_OFF_P, AS_OFF_R0, AS_OFF_R1, AS_BISECT_LOW, AS_BISECT_TOP, AS_NEWTON);
    double z[4] = {0.0, 0.0, 0.0, 0.0};
    GS_UNROLL
    for (int r = 0; r < 4; ++r)
        if (r < nz) z[r] = w(AS_OFF_R0 + r);
    int n = 0;
    GS_UNROLL
    for (int r = 0; r < 4; ++r) {
        if (r >= nz) continue;
        const double v = z[r];
        const double den = 2.0 * (cg - v * ca);
        if (!(fabs(den) > AS_DEN_TINY)) continue;
        const double u = ((((q1 - 1.0) * (v * v)) - ((2.0 * q1) * cb) * v) + (1.0 + q1)) / den;
        const double s1 = sqrt(b2 / ((1.0 + v * v) - (2.0 * v) * cb));
        const double s2 = u * s1, s3 = v * s1;
        if (!(s1 > 0.0 && s1 < (double)INFINITY && s2 > 0.0 && s2 < (double)INFINITY && s3 > 0.0 && s3 < (double)INFINITY)) continue;
        double Q[3][3], ec[3][3];
        GS_UNROLL
        for (int k = 0; k < 3; ++k) { Q[0][k] = s1 * j[0][k]; Q[1][k] = s2 * j[1][k]; Q[2][k] = s3 * j[2][k]; }
        if (!as_frame(Q[0], Q[1], Q[2], ec)) continue;
        double S[9];
        int finite = 1;
        GS_UNROLL
        for (int i = 0; i < 2; ++i) {
            GS_UNROLL
            for (int k = 0; k < 3; ++k) S[3 * i + k] = (ec[0][i] * ew[0][k] + ec[1][i] * ew[1][k]) + ec[2][i] * ew[2][k];
        }
        GS_UNROLL
        for (int i = 0; i < 3; ++i) {
            const double ri0 = (ec[0][i] * ew[0][0] + ec[1][i] * ew[1][0]) + ec[2][i] * ew[2][0];
            const double ri1 = (ec[0][i] * ew[0][1] + ec[1][i] * ew[1][1]) + ec[2][i] * ew[2][1];
            const double ri2 = (ec[0][i] * ew[0][2] + ec[1][i] * ew[1][2]) + ec[2][i] * ew[2][2];
            S[6 + i] = Q[0][i] - ((ri0 * P[0][0] + ri1 * P[0][1]) + ri2 * P[0][2]);
        }
        GS_UNROLL
        for (int k = 0; k < 9; ++k) finite &= (S[k] - S[k] == 0.0);
        if (!finite) continue;
        GS_UNROLL
        for (int k = 0; k < 9; ++k) w(AS_OFF_SOL + 9 * n + k) = S[k];
        ++n;
    }
    return n;
}

// a row as the inlier test and the refit want it: the conditioned 3-D point and the pixel, fp64
struct AsRow { double x, y, z, u, v; };
GS_HD AsRow as_row(const float* uv, const float* xyz, const double (&nm)[4]) {
    AsRow r;
    r.x = ((double)xyz[0] - nm[0]) / nm[3]; r.y = ((double)xyz[1] - nm[1]) / nm[3]; r.z = ((double)xyz[2] - nm[2]) / nm[3];
    r.u = (double)uv[0]; r.v = (double)uv[1];
    return r;
}

// Y = R X' + t'
GS_HD void as_transform(const double (&R)[9], const double (&t)[3], const AsRow& r, double (&Y)[3]) {
    GS_UNROLL
    for (int i = 0; i < 3; ++i) Y[i] = ((R[3 * i] * r.x + R[3 * i + 1] * r.y) + R[3 * i + 2] * r.z) + t[i];
}

GS_HD int as_inlier_rt(const double (&R)[9], const double (&t)[3], const float* K, const AsRow& r, double thr2) {
    double Y[3];
    as_transform(R, t, r, Y);
    const double du = ((double)K[0] * (Y[0] / Y[2]) + (double)K[2]) - r.u, dv = ((double)K[4] * (Y[1] / Y[2]) + (double)K[5]) - r.v;
    return Y[2] > 0.0 && (du * du + dv * dv) < thr2;                 // a NaN is never an inlier
}
GS_HD int as_inlier(const double (&S)[9], const float* K, const AsRow& r, double thr2) {
    double R[9], t[3];
    as_unpack(S, R, t);
    return as_inlier_rt(R, t, K, r, thr2);
}

// conditioned pose -> world units: t = s t' - R c
GS_HD void as_to_world(const double (&R)[9], const double (&t)[3], const double (&nm)[4], double (&tw)[3]) {
    GS_UNROLL
    for (int i = 0; i < 3; ++i) tw[i] = nm[3] * t[i] - ((R[3 * i] * nm[0] + R[3 * i + 1] * nm[1]) + R[3 * i + 2] * nm[2]);
}

// ------------------------------------------------------------------------------------------------------------ refit on the inliers
#define AS_REFIT_MAX_ROUNDS 8
#define AS_REFIT_MIN_INLIERS 6
#define AS_GN_STEPS 3
#define AS_GN_SUMS 27             /* 21 distinct entries of J^T J, then the 6 of J^T r */

// workspace of as_gn_solve (doubles)
#define AS_GN_OFF_ACC 0           /* [27] */
#define AS_GN_OFF_A 27            /* [6][7] the augmented normal equations */
#define AS_GN_OFF_X 69            /* [6] omega, tau */
#define AS_GN_WS_DOUBLES 75

GS_HD constexpr int as_sym6(int i, int j) { return 6 * i - (i * (i - 1)) / 2 + (j - i); }      // i <= j

// the residuals (pixels) of a row under (R, t') and their derivatives by (omega, tau) at 0; 0 when the point is not in front
GS_HD int as_gn_row(const double (&R)[9], const double (&t)[3], const float* K, const AsRow& r, double (&Ju)[6], double (&Jv)[6], double (&res)[2]) {
    double Y[3];
    as_transform(R, t, r, Y);
    if (!(Y[2] > 0.0)) return 0;
    const double fx = (double)K[0], fy = (double)K[4];
    const double xz = Y[0] / Y[2], yz = Y[1] / Y[2];
    res[0] = (fx * xz + (double)K[2]) - r.u;
    res[1] = (fy * yz + (double)K[5]) - r.v;
    // d(pixel) / dY, then dY / d(omega) = -2 [Y]x: the row a of the first gives 2 (Y x a)
    const double au[3] = {fx / Y[2], 0.0, -(fx * xz) / Y[2]}, av[3] = {0.0, fy / Y[2], -(fy * yz) / Y[2]};
    double cu[3], cv[3];
    as_cross(Y, au, cu);
    as_cross(Y, av, cv);
    GS_UNROLL
    for (int k = 0; k < 3; ++k) { Ju[k] = 2.0 * cu[k]; Jv[k] = 2.0 * cv[k]; Ju[3 + k] = au[k]; Jv[3 + k] = av[k]; }
    return 1;
}

GS_HD void as_gn_accum(double (&acc)[AS_GN_SUMS], const double (&Ju)[6], const double (&Jv)[6], const double (&res)[2]) {
    GS_UNROLL
    for (int i = 0; i < 6; ++i) {
        GS_UNROLL
        for (int j = i; j < 6; ++j) acc[as_sym6(i, j)] = acc[as_sym6(i, j)] + (Ju[i] * Ju[j] + Jv[i] * Jv[j]);
        acc[21 + i] = acc[21 + i] + (Ju[i] * res[0] + Jv[i] * res[1]);
    }
}

// the sums at AS_GN_OFF_ACC -> (omega, tau) at AS_GN_OFF_X; 0 when the system cannot be solved
GS_HD int as_gn_solve(const GsWs& w) {
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < 6; ++j) w(AS_GN_OFF_A + 7 * i + j) = w(AS_GN_OFF_ACC + (i <= j ? as_sym6(i, j) : as_sym6(j, i)));
        w(AS_GN_OFF_A + 7 * i + 6) = -w(AS_GN_OFF_ACC + 21 + i);
    }
    return gs_solve<6>(w, AS_GN_OFF_A, AS_GN_OFF_X);
}

// R <- C(omega) R, t' <- C(omega) t' + tau with d = (omega, tau); 0 when the result is not finite
GS_HD int as_gn_update(const double (&d)[6], double (&R)[9], double (&t)[3]) {
    const double wx = d[0], wy = d[1], wz = d[2];
    const double ww = (wx * wx + wy * wy) + wz * wz, den = 1.0 + ww, one = 1.0 - ww;
    double C[9];
    C[0] = (one + 2.0 * (wx * wx)) / den; C[1] = (2.0 * (wx * wy) - 2.0 * wz) / den; C[2] = (2.0 * (wx * wz) + 2.0 * wy) / den;
    C[3] = (2.0 * (wy * wx) + 2.0 * wz) / den; C[4] = (one + 2.0 * (wy * wy)) / den; C[5] = (2.0 * (wy * wz) - 2.0 * wx) / den;
    C[6] = (2.0 * (wz * wx) - 2.0 * wy) / den; C[7] = (2.0 * (wz * wy) + 2.0 * wx) / den; C[8] = (one + 2.0 * (wz * wz)) / den;
    double Rn[9], tn[3];
    int finite = 1;
    GS_UNROLL
    for (int i = 0; i < 3; ++i) {
        GS_UNROLL
        for (int k = 0; k < 3; ++k) Rn[3 * i + k] = (C[3 * i] * R[k] + C[3 * i + 1] * R[3 + k]) + C[3 * i + 2] * R[6 + k];
        tn[i] = ((C[3 * i] * t[0] + C[3 * i + 1] * t[1]) + C[3 * i + 2] * t[2]) + d[3 + i];
    }
    GS_UNROLL
    for (int k = 0; k < 9; ++k) finite &= (Rn[k] - Rn[k] == 0.0);
    GS_UNROLL
    for (int k = 0; k < 3; ++k) finite &= (tn[k] - tn[k] == 0.0);
    if (!finite) return 0;
    GS_UNROLL
    for (int k = 0; k < 9; ++k) R[k] = Rn[k];
    GS_UNROLL
    for (int k = 0; k < 3; ++k) t[k] = tn[k];
    return 1;
}

// ------------------------------------------------------------------------------------------------------------ 3-D map lookup
// Bilinear sample of a map [H][W][3] fp32 (a pixel without a 3-D point is NaN) at (x, y), integer coordinates at pixel centres: fp64 in
// this order, rounded once to fp32.  NaN when the point is outside [0, W - 1] x [0, H - 1] or not finite, or a neighbour is not finite.
GS_HD void as_xyz_sample(const float* map, int H, int W, float xf, float yf, float* out3) {
    const double x = (double)xf, y = (double)yf;
    const float nanf_ = __builtin_nanf("");
    out3[0] = out3[1] = out3[2] = nanf_;
    if (!(x >= 0.0 && x <= (double)(W - 1) && y >= 0.0 && y <= (double)(H - 1))) return;
    const int x0 = (int)x, y0 = (int)y;
    const int x1 = x0 + 1 < W ? x0 + 1 : W - 1, y1 = y0 + 1 < H ? y0 + 1 : H - 1;
    const double fx = x - (double)x0, fy = y - (double)y0;
    const float* p00 = map + 3 * ((long)y0 * W + x0);
    const float* p01 = map + 3 * ((long)y0 * W + x1);
    const float* p10 = map + 3 * ((long)y1 * W + x0);
    const float* p11 = map + 3 * ((long)y1 * W + x1);
    float v[3];
    int fin = 1;
    GS_UNROLL
    for (int k = 0; k < 3; ++k) {
        fin &= kp_finite(p00[k]) && kp_finite(p01[k]) && kp_finite(p10[k]) && kp_finite(p11[k]);
        const double top = (double)p00[k] * (1.0 - fx) + (double)p01[k] * fx, bot = (double)p10[k] * (1.0 - fx) + (double)p11[k] * fx;
        v[k] = (float)(top * (1.0 - fy) + bot * fy);
    }
    if (!fin) return;
    out3[0] = v[0]; out3[1] = v[1]; out3[2] = v[2];
}
