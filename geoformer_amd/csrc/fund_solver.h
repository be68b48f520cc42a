// Fundamental-matrix RANSAC for two-view verification without intrinsics: the algorithm, stated once for the device (k_fundamental.hip)
// and the host (host/fund_host.cpp).  Plain C++ in fp64 with contraction off, only + - * / sqrt, fabs and comparisons (solver_common.h):
// a host build and gfx950 agree bit for bit.
//
//   rows            Row i of a pair takes part iff fs_row_valid: its four coordinates are finite and, where scores are given, its score is
//                   not NaN and >= sc_thres (kp_row_valid of keypoint_spec.h, the filter of the keypoint consolidation).  Surviving rows are
//                   compacted stably, in row order; draws and counts run over the compacted list.
//   fs_box_norm     Conditioning.  Per pair and image the bounding box of the surviving points: centre -> 0, half the longer side -> 1.
//                   Min and max do not depend on the order of reduction, so the parallel form gives the serial form's bits (a mean / RMS
//                   normalisation would not).  A zero extent makes the pair invalid.
//   fs_draw7        seven distinct surviving rows of hypothesis t of pair n from (seed, n, t) and an attempt counter, as gs_draw_distinct; a candidate
//                   equal to an earlier one in EITHER image's point is drawn again.
//   fs_seven_point  7x9 system x1^T F x0 = 0 in normalised coordinates -> its 2-dimensional null space (F1, F2) by Gauss-Jordan with full
//                   pivoting -> the cubic det(x F1 + F2) in closed form (determinants and mixed cofactor sums).  The pencil is read from the
//                   end with the LARGER |det|: x F1 + F2 when |det F1| >= |det F2|, else F1 + x F2 (the same pencil, x -> 1 / x, coefficients
//                   reversed), so a vanishing leading coefficient of one form is the root 0 of the other - the end of the pencil itself - and
//                   never a division by zero; with both ends singular to the last bit there is no solution.  Real roots by gs_real_roots<3>
//                   (fixed bisection counts + guarded Newton): one or three.  Each solution is scaled to Frobenius norm 1, taken back to
//                   pixels as T1^T F T0 and scaled to norm 1 again.  Non-finite input, a rank-deficient system or seven coincident points
//                   give 0 solutions.
//   fs_inlier       the squared Sampson distance in pixels (gs_sampson); inlier iff < thr^2 (a NaN is never an inlier).
//   selection       most inliers, then the smallest hypothesis, then the smallest root.  valid = 1 iff at least FS_MIN_MATCHES rows survive,
//                   both boxes have an extent and some hypothesis produced a solution.  The mask is the winner's inlier set over the pair's
//                   ORIGINAL rows; filtered rows are 0.
//
// NOT part of this: no refit on the inliers, no local optimisation, no planar-degeneracy test (matches on one plane give a valid but
// arbitrary F), no adaptive stop.  OpenCV parity (cv2.findFundamentalMat) is UNPINNED; what is pinned is the algorithm written here.
//
// Workspace: FS_WS_DOUBLES doubles through GsWs.
#pragma once
#include "keypoint_spec.h"
#include "solver_common.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define FS_MAX_ROOTS 3
#define FS_HYP_PER_WG 64          /* hypotheses one workgroup of rt_score<FundModel> solves: iters must be a positive multiple */
#define FS_MIN_MATCHES 7
#define FS_BISECT_LOW 40
#define FS_BISECT_TOP 56
#define FS_NEWTON 4

// workspace layout (doubles)
#define FS_OFF_M 0                /* [7][9] epipolar system (gs_eliminate9 expects it at 0) */
#define FS_OFF_BASIS 63           /* [2][9] F1, F2 */
#define FS_WS_DOUBLES 81
// after the elimination the system is dead:
#define FS_OFF_P 0                /* [4] the cubic, ascending */
#define FS_OFF_R0 4               /* [5] roots of the previous derivative */
#define FS_OFF_R1 9               /* [5] roots being found */
#define FS_OFF_F 14               /* [3][9] the solutions, Frobenius norm 1 */

GS_HD bool fs_row_valid(const float* m4, const float* scores, long i, float sc_thres) {
    return scores ? kp_row_valid(m4, scores[i], sc_thres) : kp_row_valid(m4, 1.f, 0.f);
}

// (centre x, centre y, half the longer side) of a bounding box; 0 for a box without extent
GS_HD int fs_box_norm(float minx, float maxx, float miny, float maxy, double* out3) {
    const double cx = 0.5 * ((double)minx + (double)maxx), cy = 0.5 * ((double)miny + (double)maxy);
    const double hx = 0.5 * ((double)maxx - (double)minx), hy = 0.5 * ((double)maxy - (double)miny);
    const double s = hx > hy ? hx : hy;
    out3[0] = cx; out3[1] = cy; out3[2] = s;
    return s > 0.0 && s < (double)INFINITY;
}

// seven distinct positions of the compacted list `rows` (cnt entries, row indices into m [..][4]) of hypothesis t
GS_HD int fs_draw7(uint32_t seed, uint32_t sample, uint32_t t, int cnt, const float* m, const int32_t* rows, int (&idx)[7]) {
    int ok = 1;
    float p[7][4];
    GS_UNROLL
    for (int k = 0; k < 7; ++k) {
        idx[k] = 0;
        p[k][0] = p[k][1] = p[k][2] = p[k][3] = 0.f;
    }
    GS_UNROLL
    for (int k = 0; k < 7; ++k) {
        int found = 0;
        for (uint32_t attempt = 0; attempt < GS_DRAW_ATTEMPTS && !found && ok; ++attempt) {
            const int c = (int)(draw(seed, sample, t, (uint32_t)k, attempt) % (uint32_t)cnt);
            const float* q = m + 4 * (long)rows[c];
            const float q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
            int dup = 0;
            GS_UNROLL
            for (int j = 0; j < 7; ++j)
                dup |= (j < k && (idx[j] == c || (p[j][0] == q0 && p[j][1] == q1) || (p[j][2] == q2 && p[j][3] == q3)));
            if (!dup) { idx[k] = c; p[k][0] = q0; p[k][1] = q1; p[k][2] = q2; p[k][3] = q3; found = 1; }
        }
        if (!found) ok = 0;
    }
    return ok;
}

GS_HD double fs_det3(const double (&A)[9]) {
    return (A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6])) + A[2] * (A[3] * A[7] - A[4] * A[6]);
}
// sum of cofactor(A)[i][j] B[i][j]: the coefficient of x in det(A + x B)
GS_HD double fs_cof_dot(const double (&A)[9], const double (&B)[9]) {
    double s = 0.0;
    GS_UNROLL
    for (int i = 0; i < 3; ++i) {
        const int a = (i + 1) % 3, q = (i + 2) % 3;
        s = s + (A[3 * a + 1] * A[3 * q + 2] - A[3 * a + 2] * A[3 * q + 1]) * B[3 * i + 0];
        s = s + (A[3 * a + 2] * A[3 * q + 0] - A[3 * a + 0] * A[3 * q + 2]) * B[3 * i + 1];
        s = s + (A[3 * a + 0] * A[3 * q + 1] - A[3 * a + 1] * A[3 * q + 0]) * B[3 * i + 2];
    }
    return s;
}

// the singular members of the pencil spanned by F1, F2 (at FS_OFF_BASIS), Frobenius norm 1, at FS_OFF_F; returns their number
GS_HD int fs_pencil(const GsWs& w) {
    double F1[9], F2[9];
    GS_UNROLL
    for (int k = 0; k < 9; ++k) { F1[k] = w(FS_OFF_BASIS + k); F2[k] = w(FS_OFF_BASIS + 9 + k); }
    // det(x F1 + F2) = d1 x^3 + c2 x^2 + c1 x + d2
    const double d1 = fs_det3(F1), d2 = fs_det3(F2), c1 = fs_cof_dot(F2, F1), c2 = fs_cof_dot(F1, F2);
    const bool fwd = gs_abs_or_inf(d1) >= gs_abs_or_inf(d2);       // else F1 + x F2: the coefficients reversed
    w(FS_OFF_P + 0) = fwd ? d2 : d1;
    w(FS_OFF_P + 1) = fwd ? c1 : c2;
    w(FS_OFF_P + 2) = fwd ? c2 : c1;
    w(FS_OFF_P + 3) = fwd ? d1 : d2;
    const int nz = gs_real_roots<3>(w, FS_OFF_P, FS_OFF_R0, FS_OFF_R1, FS_BISECT_LOW, FS_BISECT_TOP, FS_NEWTON);
    double z[3] = {0.0, 0.0, 0.0};
    GS_UNROLL
    for (int j = 0; j < 3; ++j)
        if (j < nz) z[j] = w(FS_OFF_R0 + j);                        // (the roots leave the workspace before the solutions overwrite it)
    int n = 0;
    GS_UNROLL
    for (int j = 0; j < 3; ++j) {
        if (j >= nz) continue;
        double F[9], n2 = 0.0;
        GS_UNROLL
        for (int k = 0; k < 9; ++k) {
            F[k] = fwd ? z[j] * F1[k] + F2[k] : F1[k] + z[j] * F2[k];
            n2 = n2 + F[k] * F[k];
        }
        const double nn = sqrt(n2);
        if (!(nn > 0.0) || !(nn < (double)INFINITY)) continue;
        GS_UNROLL
        for (int k = 0; k < 9; ++k) w(FS_OFF_F + 9 * n + k) = F[k] / nn;
        ++n;
    }
    return n;
}

// x0, x1: seven matches in pixels; nm = (cx, cy, s) of image 0, then of image 1.  Returns the number of solutions (0 .. 3) left at
// FS_OFF_F in PIXEL coordinates: x1^T F x0 = 0, Frobenius norm 1.
GS_HD int fs_seven_point(const double (&x0)[7][2], const double (&x1)[7][2], const double (&nm)[6], const GsWs& w) {
    for (int r = 0; r < 7; ++r) {
        const double a = (x0[r][0] - nm[0]) / nm[2], b = (x0[r][1] - nm[1]) / nm[2];
        const double u = (x1[r][0] - nm[3]) / nm[5], v = (x1[r][1] - nm[4]) / nm[5];
        w(9 * r + 0) = u * a; w(9 * r + 1) = u * b; w(9 * r + 2) = u;
        w(9 * r + 3) = v * a; w(9 * r + 4) = v * b; w(9 * r + 5) = v;
        w(9 * r + 6) = a; w(9 * r + 7) = b; w(9 * r + 8) = 1.0;
    }
    unsigned long long perm;
    if (!gs_eliminate9<7>(w, perm)) return 0;
    gs_null_basis<7>(w, perm, FS_OFF_BASIS);
    const int nsol = fs_pencil(w);
    // back to pixels: T = [[1/s, 0, -cx/s], [0, 1/s, -cy/s], [0, 0, 1]] per image, G = T1^T F T0
    const double i0 = 1.0 / nm[2], i1 = 1.0 / nm[5];
    const double t0x = -(nm[0] * i0), t0y = -(nm[1] * i0), t1x = -(nm[3] * i1), t1y = -(nm[4] * i1);
    int n = 0;
    for (int r = 0; r < nsol; ++r) {
        double F[9], H[9], G[9], n2 = 0.0;
        GS_UNROLL
        for (int k = 0; k < 9; ++k) F[k] = w(FS_OFF_F + 9 * r + k);
        GS_UNROLL
        for (int i = 0; i < 3; ++i) {
            H[3 * i + 0] = F[3 * i + 0] * i0;
            H[3 * i + 1] = F[3 * i + 1] * i0;
            H[3 * i + 2] = (F[3 * i + 0] * t0x + F[3 * i + 1] * t0y) + F[3 * i + 2];
        }
        GS_UNROLL
        for (int c = 0; c < 3; ++c) {
            G[c] = H[c] * i1;
            G[3 + c] = H[3 + c] * i1;
            G[6 + c] = (H[c] * t1x + H[3 + c] * t1y) + H[6 + c];
        }
        GS_UNROLL
        for (int k = 0; k < 9; ++k) n2 = n2 + G[k] * G[k];
        const double nn = sqrt(n2);
        if (!(nn > 0.0) || !(nn < (double)INFINITY)) continue;
        GS_UNROLL
        for (int k = 0; k < 9; ++k) w(FS_OFF_F + 9 * n + k) = G[k] / nn;          // n <= r: never ahead of what is still to be read
        ++n;
    }
    return n;
}

// inlier iff the squared Sampson distance of the pixel match under F is below thr^2
GS_HD int fs_inlier(const double (&F)[9], const float* m4, double thr2) {
    return gs_sampson(F, (double)m4[0], (double)m4[1], (double)m4[2], (double)m4[3]) < thr2;      // a NaN is never an inlier
}
