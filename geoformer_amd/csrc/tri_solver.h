// Triangulation of database tracks from known camera poses: the algorithm, stated once for the device (k_triangulate.hip) and the host
// (host/tri_host.cpp).  Plain C++ in fp64 with contraction off, only + - * / sqrt, fabs and comparisons (solver_common.h) - no acos or cos
// anywhere: the angle threshold arrives as a cosine - so a host build and gfx950 agree bit for bit.
//
//   1  nodes        Keypoint k of image i is node kp_off[i] + k, kp_off the prefix sum of the per-image keypoint counts.  Every match row
//                   of every pair is an edge between two nodes.  A row whose two nodes are equal adds nothing; duplicate edges are
//                   harmless.  A row that names an image outside [0, n_images) or a keypoint its image does not have is skipped and
//                   reported (TR_FLAG_EDGE_RANGE).
//   2  tracks       A track is a connected component with at least two nodes.  Tracks are numbered by their smallest node, ascending; a
//                   track's observations are its nodes in ascending order - image-major, so two observations of one image are
//                   neighbours.  A track in which two neighbouring observations have the same image is a CONFLICT: reported, not
//                   triangulated.
//   3  cameras      Image i has fp32 K[9] and fp64 R[9], t[3] with x_cam = R X + t.  tr_cam_ok: K[0], K[2], K[4], K[5], R and t are all
//                   finite.  An observation whose image fails that (an image without a pose carries NaN) or lies outside [0, n_images)
//                   takes no part, exactly as if it were absent: the track's EFFECTIVE length L excludes it, and positions below count
//                   effective observations only.  The ray of an observation: o = -R^T t (tr_centre), d = R^T unit((u - K[2]) / K[0],
//                   (v - K[5]) / K[4], 1) (tr_dir: as_bearing's arithmetic).
//   4  hypotheses   H = tr_hyp_count(L) = min(L (L - 1) / 2, TR_MAX_HYP).  L <= TR_LEX_MAX (11): hypothesis t is the t-th pair (a, b),
//                   a < b, in lexicographic order.  Otherwise hypothesis t draws two distinct positions with
//                   gs_draw_distinct<2>(seed, track, t, L, .).  (tr_hyp_pair.)
//   5  two views    tr_midpoint: c = d_a . d_b, w = o_b - o_a, p = w . d_a, q = w . d_b; lambda = (p - c q) / (1 - c^2),
//                   mu = (c p - q) / (1 - c^2); X = ((o_a + lambda d_a) + (o_b + mu d_b)) / 2.  No solution when 1 - c^2 <= TR_PAR_TINY,
//                   when lambda or mu is not > 0, when c is not < cos_min_angle (the triangulation-angle test, made at the hypothesis
//                   pair), or when an input or X is not finite.
//   6  inliers      tr_residual: Y = R X + t, e2 = (K[0] Y.x / Y.z + K[2] - u)^2 + (K[4] Y.y / Y.z + K[5] - v)^2.  Inlier iff Y.z > 0 and
//                   e2 < thr^2; a NaN is never an inlier.  as_inlier's arithmetic without the conditioning.
//   7  selection    most inliers (over the effective observations), then the smallest hypothesis.  valid iff the track has no conflict,
//                   some hypothesis had a solution and n_inliers >= min_obs (min_obs >= 2).
//   8  refit        (refit = R in 1 .. TR_REFIT_MAX_ROUNDS only; R = 0: the midpoint winner's bits.)  Up to R times: TR_GN_STEPS (3)
//                   Gauss-Newton steps on X over the current inlier set - the six distinct entries of J^T J and the three of J^T r summed
//                   serially in observation order from +0.0 (tracks are short: no partial sums), J^T J d = -J^T r by gs_solve<3>, a row
//                   whose Y.z is not > 0 under the step's point adds nothing.  The candidate is scored over all effective observations
//                   and taken iff it has at least as many inliers.  A rejected candidate, a failed solve, a non-finite point or an
//                   unchanged set ends the rounds.  So n_inliers never decreases, rounds = 0 means the midpoint's bits, and `hypothesis`
//                   keeps naming the seeding pair.
//   9  output       per track: X [3] (zeros when not valid), valid, conflict, n_inliers (the winner's count, also where it stays below
//                   min_obs; 0 without a winner), hypothesis (-1 without a winner), rounds, err2 = the sum of e2 over the inliers in
//                   observation order / n_inliers (0 when not valid).  Per observation: an inlier byte, 0 for every observation of a track
//                   that is not valid.
//  10  limits       nodes, edges and tracks x 64 each below 2^31, thr > 0, min_obs >= 2, refit 0 .. 8: anything else is an error of the
//                   entry point, never a wrapped index.
//
// tr_track_finish is the whole of steps 7 - 9 for one track and tr_hypothesis the whole of steps 4 - 6 for one (track, hypothesis): the
// device runs each on one thread, the host in a loop - one text.
//
// NOT part of this: no bundle adjustment, no re-triangulation or track merging after the fact, no splitting of conflict tracks, no
// distortion parameters.  COLMAP parity is UNPINNED; what is pinned is the algorithm written here.
#pragma once
#include "abs_solver.h"
#include "solver_common.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define TR_MAX_HYP 64
#define TR_LEX_MAX 11             /* the longest track whose pairs are all tried: 11 * 10 / 2 = 55 <= TR_MAX_HYP */
#define TR_PAR_TINY 1e-12
#define TR_GN_STEPS 3
#define TR_REFIT_MAX_ROUNDS 8
#define TR_FLAG_EDGE_RANGE 1

// workspace of tr_gn_solve (doubles, through GsWs)
#define TR_GN_OFF_A 0             /* [3][4] the augmented normal equations */
#define TR_GN_OFF_X 12            /* [3] */
#define TR_GN_WS_DOUBLES 15

GS_HD bool tr_finite(double v) { return v - v == 0.0; }

GS_HD int tr_cam_ok(const float* K, const double* R, const double* t) {
    int ok = kp_finite(K[0]) && kp_finite(K[2]) && kp_finite(K[4]) && kp_finite(K[5]);
    GS_UNROLL
    for (int k = 0; k < 9; ++k) ok &= tr_finite(R[k]);
    GS_UNROLL
    for (int k = 0; k < 3; ++k) ok &= tr_finite(t[k]);
    return ok;
}

// o = -R^T t
GS_HD void tr_centre(const double* R, const double* t, double (&o)[3]) {
    GS_UNROLL
    for (int k = 0; k < 3; ++k) o[k] = -((R[k] * t[0] + R[3 + k] * t[1]) + R[6 + k] * t[2]);
}

// d = R^T bearing(u, v)
GS_HD void tr_dir(const float* K, const double* R, double u, double v, double (&d)[3]) {
    double j[3];
    as_bearing(K, u, v, j);
    GS_UNROLL
    for (int k = 0; k < 3; ++k) d[k] = (R[k] * j[0] + R[3 + k] * j[1]) + R[6 + k] * j[2];
}

GS_HD int tr_hyp_count(int L) { return L < 2 ? 0 : (L > TR_LEX_MAX ? TR_MAX_HYP : L * (L - 1) / 2); }

// the two positions (among the L effective observations) of hypothesis t of `track`; 0 when the draw failed
GS_HD int tr_hyp_pair(uint32_t seed, uint32_t track, int t, int L, int& a, int& b) {
    a = 0; b = 1;
    if (L < 2 || t < 0 || t >= tr_hyp_count(L)) return 0;
    if (L <= TR_LEX_MAX) {
        int rem = t, first = 0;
        while (rem >= L - 1 - first) { rem -= L - 1 - first; ++first; }
        a = first; b = first + 1 + rem;
        return 1;
    }
    int idx[2] = {0, 0};
    const int ok = gs_draw_distinct<2>(seed, track, (uint32_t)t, L, idx);
    a = idx[0]; b = idx[1];
    return ok;
}

GS_HD int tr_midpoint(const double (&oa)[3], const double (&da)[3], const double (&ob)[3], const double (&db)[3], double cos_min,
                      double (&X)[3]) {
    const double c = as_dot(da, db);
    const double den = 1.0 - c * c;
    if (!(den > TR_PAR_TINY) || !(c < cos_min)) return 0;                // (a NaN fails the first test)
    double w[3];
    GS_UNROLL
    for (int k = 0; k < 3; ++k) w[k] = ob[k] - oa[k];
    const double p = as_dot(w, da), q = as_dot(w, db);
    const double lam = (p - c * q) / den, mu = (c * p - q) / den;
    if (!(lam > 0.0) || !(mu > 0.0)) return 0;
    int fin = 1;
    GS_UNROLL
    for (int k = 0; k < 3; ++k) {
        X[k] = 0.5 * ((oa[k] + lam * da[k]) + (ob[k] + mu * db[k]));
        fin &= tr_finite(X[k]);
    }
    return fin;
}

GS_HD void tr_transform(const double* R, const double* t, const double (&X)[3], double (&Y)[3]) {
    GS_UNROLL
    for (int i = 0; i < 3; ++i) Y[i] = ((R[3 * i] * X[0] + R[3 * i + 1] * X[1]) + R[3 * i + 2] * X[2]) + t[i];
}

// the squared reprojection error in pixels; returns Y.z > 0
GS_HD int tr_residual(const float* K, const double* R, const double* t, const double (&X)[3], double u, double v, double& e2) {
    double Y[3];
    tr_transform(R, t, X, Y);
    const double du = ((double)K[0] * (Y[0] / Y[2]) + (double)K[2]) - u, dv = ((double)K[4] * (Y[1] / Y[2]) + (double)K[5]) - v;
    e2 = du * du + dv * dv;
    return Y[2] > 0.0;
}
GS_HD int tr_inlier(const float* K, const double* R, const double* t, const double (&X)[3], double u, double v, double thr2) {
    double e2;
    const int front = tr_residual(K, R, t, X, u, v, e2);
    return front && e2 < thr2;                                           // a NaN is never an inlier
}

// the two residuals of an observation under X and their derivatives by X; 0 when the point is not in front
GS_HD int tr_gn_row(const float* K, const double* R, const double* t, const double (&X)[3], double u, double v, double (&Ju)[3],
                    double (&Jv)[3], double (&res)[2]) {
    double Y[3];
    tr_transform(R, t, X, Y);
    if (!(Y[2] > 0.0)) return 0;
    const double fx = (double)K[0], fy = (double)K[4];
    const double xz = Y[0] / Y[2], yz = Y[1] / Y[2];
    res[0] = (fx * xz + (double)K[2]) - u;
    res[1] = (fy * yz + (double)K[5]) - v;
    const double au0 = fx / Y[2], au2 = -(fx * xz) / Y[2], av1 = fy / Y[2], av2 = -(fy * yz) / Y[2];      // d(pixel) / dY; dY / dX = R
    GS_UNROLL
    for (int k = 0; k < 3; ++k) {
        Ju[k] = au0 * R[k] + au2 * R[6 + k];
        Jv[k] = av1 * R[3 + k] + av2 * R[6 + k];
    }
    return 1;
}

GS_HD constexpr int tr_sym3(int i, int j) { return 3 * i - (i * (i - 1)) / 2 + (j - i); }      // i <= j

// acc [9]: the 6 distinct entries of J^T J, then the 3 of J^T r
GS_HD void tr_gn_accum(double (&acc)[9], const double (&Ju)[3], const double (&Jv)[3], const double (&res)[2]) {
    GS_UNROLL
    for (int i = 0; i < 3; ++i) {
        GS_UNROLL
        for (int j = i; j < 3; ++j) acc[tr_sym3(i, j)] = acc[tr_sym3(i, j)] + (Ju[i] * Ju[j] + Jv[i] * Jv[j]);
        acc[6 + i] = acc[6 + i] + (Ju[i] * res[0] + Jv[i] * res[1]);
    }
}

// J^T J d = -J^T r; 0 when the system cannot be solved
GS_HD int tr_gn_solve(const double (&acc)[9], const GsWs& w, double (&d)[3]) {
    GS_UNROLL
    for (int i = 0; i < 3; ++i) {
        GS_UNROLL
        for (int j = 0; j < 3; ++j) w(TR_GN_OFF_A + 4 * i + j) = acc[i <= j ? tr_sym3(i, j) : tr_sym3(j, i)];
        w(TR_GN_OFF_A + 4 * i + 3) = -acc[6 + i];
    }
    if (!gs_solve<3>(w, TR_GN_OFF_A, TR_GN_OFF_X)) return 0;
    GS_UNROLL
    for (int k = 0; k < 3; ++k) d[k] = w(TR_GN_OFF_X + k);
    return 1;
}

// ------------------------------------------------------------------------------------------------------------ one launch's data
struct TrView {
    const int32_t* obs_image;    // [n_obs]
    const float* obs_uv;         // [n_obs][2]
    const float* K;              // [n_images][9]
    const double* R;             // [n_images][9]
    const double* t;             // [n_images][3]
    const int32_t* cam_ok;       // [n_images] tr_cam_ok
    const double* cam_o;         // [n_images][3] tr_centre (unspecified where cam_ok is 0)
    int n_images;
    double thr2, cos_min;
    int min_obs, refit;
    uint32_t seed;
};

// does observation i take part?
GS_HD int tr_obs_eff(const TrView& v, long i) {
    const int img = v.obs_image[i];
    return img >= 0 && img < v.n_images && v.cam_ok[img] != 0;
}

// observations [b, e) of a track -> its effective length and whether it is a conflict
GS_HD void tr_track_scan(const TrView& v, long b, long e, int& L, int& conflict) {
    L = 0; conflict = 0;
    for (long i = b; i < e; ++i) {
        L += tr_obs_eff(v, i);
        conflict |= (i > b && v.obs_image[i] == v.obs_image[i - 1]);
    }
}

GS_HD int tr_obs_inlier(const TrView& v, long i, const double (&X)[3]) {
    const size_t img = (size_t)v.obs_image[i];
    return tr_inlier(v.K + 9 * img, v.R + 9 * img, v.t + 3 * img, X, (double)v.obs_uv[2 * i], (double)v.obs_uv[2 * i + 1], v.thr2);
}

// steps 4 and 5 for hypothesis t of a track of effective length L; 0: no solution
GS_HD int tr_hyp_solve(const TrView& v, uint32_t track, long b, long e, int L, int t, double (&X)[3]) {
    int pa, pb;
    if (!tr_hyp_pair(v.seed, track, t, L, pa, pb)) return 0;
    long ia = -1, ib = -1;
    int pos = 0;
    for (long i = b; i < e; ++i) {
        if (!tr_obs_eff(v, i)) continue;
        if (pos == pa) ia = i;
        if (pos == pb) ib = i;
        ++pos;
    }
    if (ia < 0 || ib < 0) return 0;
    const size_t ma = (size_t)v.obs_image[ia], mb = (size_t)v.obs_image[ib];
    double oa[3], ob[3], da[3], db[3];
    GS_UNROLL
    for (int k = 0; k < 3; ++k) { oa[k] = v.cam_o[3 * ma + k]; ob[k] = v.cam_o[3 * mb + k]; }
    tr_dir(v.K + 9 * ma, v.R + 9 * ma, (double)v.obs_uv[2 * ia], (double)v.obs_uv[2 * ia + 1], da);
    tr_dir(v.K + 9 * mb, v.R + 9 * mb, (double)v.obs_uv[2 * ib], (double)v.obs_uv[2 * ib + 1], db);
    return tr_midpoint(oa, da, ob, db, v.cos_min, X);
}

// steps 4 - 6: the inlier count of hypothesis t, -1 when it has no solution
GS_HD int tr_hypothesis(const TrView& v, uint32_t track, long b, long e, int L, int t) {
    double X[3];
    if (!tr_hyp_solve(v, track, b, e, L, t, X)) return -1;
    int c = 0;
    for (long i = b; i < e; ++i)
        if (tr_obs_eff(v, i)) c += tr_obs_inlier(v, i, X);
    return c;
}

// steps 7 - 9 for one track: best_t is the winning hypothesis (-1: none had a solution).  mask is the launch's [n_obs] inlier bytes; the
// track's slice [b, e) holds the current inlier set between the rounds.
GS_HD void tr_track_finish(const TrView& v, uint32_t track, long b, long e, int L, int conflict, int best_t, const GsWs& w, double* X_out,
                           int32_t* valid, int32_t* n_inliers, int32_t* hypothesis, int32_t* rounds, double* err2, uint8_t* mask) {
    double X[3] = {0.0, 0.0, 0.0};
    int nin = 0, nr = 0, have = 0;
    for (long i = b; i < e; ++i) mask[i] = 0;
    if (!conflict && best_t >= 0) have = tr_hyp_solve(v, track, b, e, L, best_t, X);
    if (have) {
        for (long i = b; i < e; ++i)
            if (tr_obs_eff(v, i)) {
                const int in = tr_obs_inlier(v, i, X);
                mask[i] = (uint8_t)in;
                nin += in;
            }
        for (int r = 0; r < v.refit; ++r) {
            double Xc[3] = {X[0], X[1], X[2]};
            int ok = 1;
            for (int step = 0; step < TR_GN_STEPS && ok; ++step) {
                double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                for (long i = b; i < e; ++i) {
                    if (!mask[i]) continue;
                    const size_t img = (size_t)v.obs_image[i];
                    double Ju[3], Jv[3], res[2];
                    if (tr_gn_row(v.K + 9 * img, v.R + 9 * img, v.t + 3 * img, Xc, (double)v.obs_uv[2 * i], (double)v.obs_uv[2 * i + 1], Ju, Jv, res))
                        tr_gn_accum(acc, Ju, Jv, res);
                }
                double d[3];
                ok = tr_gn_solve(acc, w, d);
                if (ok) {
                    GS_UNROLL
                    for (int k = 0; k < 3; ++k) {
                        Xc[k] = Xc[k] + d[k];
                        ok &= tr_finite(Xc[k]);
                    }
                }
            }
            if (!ok) break;
            int c = 0, differ = 0;
            for (long i = b; i < e; ++i)
                if (tr_obs_eff(v, i)) {
                    const int in = tr_obs_inlier(v, i, Xc);
                    c += in;
                    differ |= in != (int)mask[i];
                }
            if (c < nin) break;
            GS_UNROLL
            for (int k = 0; k < 3; ++k) X[k] = Xc[k];
            nin = c;
            ++nr;
            if (!differ) break;
            for (long i = b; i < e; ++i)
                if (tr_obs_eff(v, i)) mask[i] = (uint8_t)tr_obs_inlier(v, i, X);
        }
    }
    const int ok = have && nin >= v.min_obs;
    double sum = 0.0;
    if (ok) {
        for (long i = b; i < e; ++i) {
            if (!mask[i]) continue;
            const size_t img = (size_t)v.obs_image[i];
            double e2;
            tr_residual(v.K + 9 * img, v.R + 9 * img, v.t + 3 * img, X, (double)v.obs_uv[2 * i], (double)v.obs_uv[2 * i + 1], e2);
            sum = sum + e2;
        }
    } else {
        for (long i = b; i < e; ++i) mask[i] = 0;
    }
    GS_UNROLL
    for (int k = 0; k < 3; ++k) X_out[k] = ok ? X[k] : 0.0;
    *valid = ok;
    *n_inliers = have ? nin : 0;
    *hypothesis = have ? best_t : -1;
    *rounds = have ? nr : 0;
    *err2 = ok ? sum / (double)nin : 0.0;
}

// ------------------------------------------------------------------------------------------------------------ tracks (steps 1 and 2)
// the pair of edge e: the last p with id_off[p] <= e (id_off [P + 1] ascending; -1 when e is in no pair)
GS_HD int tr_find_pair(const int32_t* id_off, int P, int e) {
    int lo = 0, hi = P;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (id_off[mid] <= e) lo = mid; else hi = mid;
    }
    return (P > 0 && id_off[lo] <= e && e < id_off[lo + 1]) ? lo : -1;
}

// the two nodes of edge e; 0 when the row is out of range (step 1)
GS_HD int tr_edge_nodes(const int32_t* ids, const int32_t* id_off, const int32_t* pair_images, int P, const int32_t* kp_off, int n_images,
                        int n_nodes, int e, int& u, int& v) {
    u = v = 0;
    const int p = tr_find_pair(id_off, P, e);
    if (p < 0) return 0;
    int node[2];
    GS_UNROLL
    for (int s = 0; s < 2; ++s) {
        const int img = pair_images[2 * (long)p + s], k = ids[2 * (long)e + s];
        if (img < 0 || img >= n_images) return 0;
        const int lo = kp_off[img], hi = kp_off[img + 1];
        if (k < 0 || lo < 0 || hi > n_nodes || k >= hi - lo) return 0;
        node[s] = lo + k;
    }
    u = node[0]; v = node[1];
    return 1;
}
