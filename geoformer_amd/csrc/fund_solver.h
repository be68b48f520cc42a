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
//   refit           (gf_fundamental_ransac_lo with refit_rounds R in 1 .. FS_REFIT_MAX_ROUNDS only; R = 0 is everything above and nothing
//                   else.)  The winner is ONE seven-point model; a least-squares fit on its consensus set follows, up to R times.
//                   cur = (F, inlier set over the surviving rows, count) starts as the winner's.  One round:
//                   1. cur has fewer than FS_REFIT_MIN_INLIERS (8) inliers: stop.
//                   2. fs_refit_row: a = x1 (x) x0 of a surviving row in box-normalised coordinates, the row fs_seven_point builds.
//                      fs_refit_accum adds the 45 distinct entries of a a^T (entry (i, j), i <= j, at fs_sym_index) to an accumulator.
//                      M = sum over the inliers, in THIS order: partial j (0 .. FS_REFIT_PARTIALS - 1 = 255) starts from +0.0 and adds
//                      the inlier rows with compacted index i = j (mod 256), ascending i; the partials are combined inside each block of
//                      64 with strides 32, 16, 8, 4, 2, 1 (s[j] = s[j] + s[j + stride], j < stride within the block) and the four block
//                      sums as (b0 + b1) + (b2 + b3): fs_refit_tree.  (A wave's xor butterfly gives lane 0 these bits: the addition of
//                      two fp64 numbers is commutative.)
//                   3. fs_refit_solve: the eigenvector of M's smallest eigenvalue by gs_jacobi_sym<9>, FS_JACOBI9_SWEEPS sweeps.
//                   4. rank 2 without an SVD: v = the eigenvector of F^T F's smallest eigenvalue (gs_jacobi_sym<3>, FS_JACOBI3_SWEEPS),
//                      F <- F - (F v) v^T, the Frobenius-closest rank-2 matrix.  Then Frobenius norm 1, T1^T F T0, norm 1 again, as
//                      the seven-point solutions.
//                   5. a non-finite entry or a zero norm: the round fails; cur stays, stop.
//                   6. the candidate is scored over ALL surviving rows with fs_inlier and the same thr^2; it is accepted iff its count
//                      is >= cur's.  Accepted: cur <- candidate, rounds += 1.  Stop when it was rejected, or when the accepted set equals
//                      the one before (a fixed point).
//                   So n_inliers never decreases; rounds = 0 means every output is the seven-point winner's, bit for bit; `best` keeps
//                   naming the (hypothesis, root) that seeded the result.  A planar or otherwise degenerate consensus set gives SOME
//                   eigenvector of a rank-deficient M and the accept test alone decides.
//
// NOT part of this: no Sampson re-weighting (IRLS) or other local optimisation, no planar-degeneracy test (matches on one plane give a
// valid but arbitrary F), no adaptive stop.  OpenCV parity (cv2.findFundamentalMat) is UNPINNED; what is pinned is the algorithm written here.
//
// Workspace: FS_WS_DOUBLES doubles through GsWs for the seven-point solver, FS_REFIT_WS_DOUBLES for fs_refit_solve.
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

// ------------------------------------------------------------------------------------------------------------ refit on the inliers
#define FS_REFIT_MAX_ROUNDS 8
#define FS_REFIT_MIN_INLIERS 8
#define FS_REFIT_PARTIALS 256     /* partial sums of the normal matrix: the threads of one workgroup */
#define FS_JACOBI9_SWEEPS 10
#define FS_JACOBI3_SWEEPS 8
#define FS_SYM9 45                /* distinct entries of a symmetric 9 x 9 matrix */

// workspace of fs_refit_solve (doubles, stride as the caller likes)
#define FS_REFIT_OFF_ACC 0        /* [45] the normal matrix, entry (i, j), i <= j, at fs_sym_index(i, j) */
#define FS_REFIT_OFF_A 45         /* [9][9] the same, both triangles; its eigenvalues on the diagonal afterwards */
#define FS_REFIT_OFF_V 126        /* [9][9] eigenvectors in the columns */
#define FS_REFIT_OFF_G 207        /* [3][3] F^T F */
#define FS_REFIT_OFF_W 216        /* [3][3] its eigenvectors */
#define FS_REFIT_WS_DOUBLES 225

GS_HD constexpr int fs_sym_index(int i, int j) { return 9 * i - (i * (i - 1)) / 2 + (j - i); }      // i <= j

// a = x1 (x) x0 in box-normalised coordinates: the row of the epipolar system, with the expressions of fs_seven_point
GS_HD void fs_refit_row(const float* m4, const double (&nm)[6], double (&r)[9]) {
    const double a = ((double)m4[0] - nm[0]) / nm[2], b = ((double)m4[1] - nm[1]) / nm[2];
    const double u = ((double)m4[2] - nm[3]) / nm[5], v = ((double)m4[3] - nm[4]) / nm[5];
    r[0] = u * a; r[1] = u * b; r[2] = u;
    r[3] = v * a; r[4] = v * b; r[5] = v;
    r[6] = a; r[7] = b; r[8] = 1.0;
}

GS_HD void fs_refit_accum(double (&acc)[FS_SYM9], const double (&r)[9]) {
    GS_UNROLL
    for (int i = 0; i < 9; ++i) {
        GS_UNROLL
        for (int j = i; j < 9; ++j) acc[fs_sym_index(i, j)] = acc[fs_sym_index(i, j)] + r[i] * r[j];
    }
}

// the order in which the FS_REFIT_PARTIALS partial sums of one entry become the entry: s [256] is overwritten, the sum is returned
GS_HD double fs_refit_tree(double* s) {
    for (int b = 0; b < FS_REFIT_PARTIALS; b += 64)
        for (int stride = 32; stride >= 1; stride >>= 1)
            for (int j = 0; j < stride; ++j) s[b + j] = s[b + j] + s[b + j + stride];
    return (s[0] + s[64]) + (s[128] + s[192]);
}

// G = T1^T F T0 scaled to Frobenius norm 1: a matrix of normalised coordinates taken back to pixels, with the expressions of
// fs_seven_point (which keeps its own copy: its kernel is left as it compiled before the refit existed).  Returns 0 for a zero or
// non-finite norm.
GS_HD int fs_to_pixels(const double (&F)[9], const double (&nm)[6], double (&out)[9]) {
    const double i0 = 1.0 / nm[2], i1 = 1.0 / nm[5];
    const double t0x = -(nm[0] * i0), t0y = -(nm[1] * i0), t1x = -(nm[3] * i1), t1y = -(nm[4] * i1);
    double H[9], G[9], n2 = 0.0;
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
    if (!(nn > 0.0) || !(nn < (double)INFINITY)) return 0;
    GS_UNROLL
    for (int k = 0; k < 9; ++k) out[k] = G[k] / nn;
    return 1;
}

// Steps 3 - 5 of a round are fs_refit_solve (below): the normal matrix at FS_REFIT_OFF_ACC -> the candidate in PIXEL coordinates,
// Frobenius norm 1, rank 2; 0 when the round fails (out is then unspecified).  It is written in three parts so that k_fundamental.hip can
// run the middle one - gs_jacobi_sym<9> - with the elements of a rotation on several lanes, which gives the same bits.
GS_HD void fs_refit_fill(const GsWs& w) {
    for (int i = 0; i < 9; ++i)
        for (int j = i; j < 9; ++j) {
            const double v = w(FS_REFIT_OFF_ACC + fs_sym_index(i, j));
            w(FS_REFIT_OFF_A + 9 * i + j) = v;
            w(FS_REFIT_OFF_A + 9 * j + i) = v;
        }
}

GS_HD int fs_refit_finish(const GsWs& w, const double (&nm)[6], double (&out)[9]) {
    const int col = gs_min_diag<9>(w, FS_REFIT_OFF_A);
    double F[9];
    GS_UNROLL
    for (int k = 0; k < 9; ++k) F[k] = w(FS_REFIT_OFF_V + 9 * k + col);
    // rank 2: the right singular vector of the smallest singular value is the eigenvector of F^T F's smallest eigenvalue
    GS_UNROLL
    for (int i = 0; i < 3; ++i) {
        GS_UNROLL
        for (int j = 0; j < 3; ++j) w(FS_REFIT_OFF_G + 3 * i + j) = (F[i] * F[j] + F[3 + i] * F[3 + j]) + F[6 + i] * F[6 + j];
    }
    gs_jacobi_sym<3>(w, FS_REFIT_OFF_G, FS_REFIT_OFF_W, FS_JACOBI3_SWEEPS);
    const int c3 = gs_min_diag<3>(w, FS_REFIT_OFF_G);
    const double v0 = w(FS_REFIT_OFF_W + c3), v1 = w(FS_REFIT_OFF_W + 3 + c3), v2 = w(FS_REFIT_OFF_W + 6 + c3);
    double n2 = 0.0;
    GS_UNROLL
    for (int i = 0; i < 3; ++i) {
        const double fv = (F[3 * i] * v0 + F[3 * i + 1] * v1) + F[3 * i + 2] * v2;
        F[3 * i] = F[3 * i] - fv * v0;
        F[3 * i + 1] = F[3 * i + 1] - fv * v1;
        F[3 * i + 2] = F[3 * i + 2] - fv * v2;
    }
    GS_UNROLL
    for (int k = 0; k < 9; ++k) n2 = n2 + F[k] * F[k];
    const double nn = sqrt(n2);
    if (!(nn > 0.0) || !(nn < (double)INFINITY)) return 0;
    GS_UNROLL
    for (int k = 0; k < 9; ++k) F[k] = F[k] / nn;
    if (!fs_to_pixels(F, nm, out)) return 0;
    int finite = 1;
    GS_UNROLL
    for (int k = 0; k < 9; ++k) finite &= (out[k] - out[k] == 0.0);
    return finite;
}

GS_HD int fs_refit_solve(const GsWs& w, const double (&nm)[6], double (&out)[9]) {
    fs_refit_fill(w);
    gs_jacobi_sym<9>(w, FS_REFIT_OFF_A, FS_REFIT_OFF_V, FS_JACOBI9_SWEEPS);
    return fs_refit_finish(w, nm, out);
}
