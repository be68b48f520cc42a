// Bundle adjustment - the joint refinement of camera poses and 3-D points: the algorithm, stated once for the device (k_bundle.hip) and the
// host (host/ba_host.cpp).  Plain C++ in fp64 with contraction off, only + - * / sqrt, fabs and comparisons (solver_common.h), every sum in
// a stated order and no floating-point atomics, so a host build and gfx950 agree bit for bit.  Levenberg-Marquardt with the points
// eliminated (Schur complement) and a dense Cholesky of the reduced camera system.
//
//   1  inputs       Image i has fp32 K[9] and fp64 R[9], t[3] with x_cam = R X + t, and cam_free[i]: its FREE INDEX in 0 .. F - 1 (ascending
//                   with i), or -1 for a fixed image.  tr_cam_ok decides whether the image has a pose; one without takes no part, exactly as
//                   if its observations were absent; a free image without a pose keeps its bits, moves nowhere and raises BA_FLAG_FREE_NO_POSE.
//                   T points X in fp64.  Observations point-major: obs_off [T + 1], obs_image, fp32 pixels obs_uv; the same observations
//                   image-major: img_off [n_images + 1], img_obs (the observations of an image ascending).
//   2  taking part  At a state, observation o of point p TAKES PART iff its image has a pose, Y = R X_p + t has Y.z > 0 and
//                   e2 = (K[0] Y.x / Y.z + K[2] - u)^2 + (K[4] Y.y / Y.z + K[5] - v)^2 < thr^2 (tr_residual's arithmetic; NaN: no part).
//   3  cost         Every observation of an image with a pose adds e2 when it takes part and thr^2 otherwise: the truncated cost.  Summed per
//                   point serially in observation order from +0.0 (ba_point_cost); the points of a block of BA_BLOCK (256) by the pairwise
//                   tree s[t] += s[t + h], h = 128, 64 .. 1, on the zero-padded block (ba_block_tree); the blocks serially, ascending.
//   4  jacobians    ba_jacobian, for an observation that takes part: the residual (pixels), a = d(pixel) / dY, the point's 2 x 3 block a R
//                   (tr_gn_row's arithmetic) and the camera's 2 x 6 block by (omega, tau) at 0 of the left update R <- C(omega) R,
//                   t <- C(omega) t + tau, C the Cayley map: (2 (Y x a), a) (as_gn_row's arithmetic).
//   5  points       Per point (ba_point_build), over its observations that take part, in order: V = sum Jp^T Jp (6 distinct entries),
//                   g = sum Jp^T (-r), and per observation of a FREE camera W = Jc^T Jp (6 x 3).  A = V + lambda diag(V); its inverse column
//                   by column: gs_solve<3> on (A | e_k), k = 0, 1, 2.  A failed pivot test HOLDS the point for this iteration: delta = 0, no
//                   Schur terms, its observations still feed U and b (BA_FLAG_POINT_HELD).  Otherwise T = W A^-1 per observation.
//   6  camera rows  Per free camera with free index f (ba_camera_row), the six rows 6 f .. 6 f + 5 of the reduced system, blocks j <= f only
//                   (the factorisation reads the lower triangle).  First walk, the image's observations ascending, those that take part:
//                   U += Jc^T Jc into block f, b += Jc^T (-r).  Then the diagonal of block f gets + lambda * itself; a camera with no
//                   observation taking part gets diagonal 1 instead and moves nowhere.  Second walk, the image's observations k ascending,
//                   taking part, point not held: for the point's observations l ascending, taking part, camera free with index j <= f:
//                   S[f][j][r][c] -= (T_k[r][0] W_l[c][0] + T_k[r][1] W_l[c][1]) + T_k[r][2] W_l[c][2]; after them
//                   rhs[r] -= (T_k[r][0] g[0] + T_k[r][1] g[1]) + T_k[r][2] g[2].  Every entry has ONE chain of additions, in this order.
//   7  solve        S delta_c = rhs by Cholesky on the lower triangle, n = 6 F: column c, entry a >= c: s = S[a][c]; s = s - L[a][k] L[c][k]
//                   for k = 0 .. c - 1 ascending (ba_chol_chain); L[c][c] = sqrt(s), needs s > 0, else the step FAILED
//                   (BA_FLAG_STEP_FAILED); L[a][c] = s / L[c][c].  L y = rhs: y[a] = (rhs[a] - sum_k L[a][k] y[k]) / L[a][a], k ascending;
//                   L^T x = y: x[a] = (y[a] - sum_k L[k][a] x[k]) / L[a][a], k DESCENDING from n - 1.
//   8  back         Per point not held (ba_point_delta): s = g; for its observations taking part with a free camera, in order, and r = 0 .. 5:
//                   s[m] = s[m] - W[r][m] delta_c[r]; delta = A^-1 s; candidate X = X + delta.  Cameras: as_gn_update(delta_c) on a free
//                   one (a result that is not finite fails the step: BA_FLAG_STEP_FAILED), the input bits for every other.
//   9  decision     The candidate's cost by rule 3.  Accepted iff the step did not fail and cost_candidate < cost_current.  Accepted: the
//                   state becomes the candidate, lambda = max(lambda / 10, BA_LAMBDA_MIN).  Else the state stays and
//                   lambda = min(lambda * 10, BA_LAMBDA_MAX).  lambda starts at BA_LAMBDA_INIT (1e-4).  Participation (rule 2) is
//                   evaluated anew at the state of every iteration.
//  10  outputs      R, t of all images (fixed and pose-less ones: their input bits), X; per observation the byte "takes part at the final
//                   state"; per point the count of those; cost [iters + 1], accepted [iters], lambda [iters + 1]; status = the OR of the flags.
//  11  limits       1 <= iters <= BA_MAX_ITERS (64), thr > 0 and finite, F <= BA_MAX_FREE (128), T and n_obs below 2^31, consistent tables:
//                   anything else is an error of the entry point, never a wrapped index.  F = 0 is legal: every point on its own.
//
// Rules 6 and 7 have a second form, 6' and 7' - 7''' in ba_pcg_spec.h: the same reduced system solved by matrix-free preconditioned
// conjugate gradients (per-camera blocks U + lambda diag(U) - sum Tm W^T as the preconditioner, q = S p in two sweeps over the
// observations, every sum of many terms by 256 partials and ba_block_tree), for up to BA_PCG_MAX_FREE (65536) free cameras.  Rules 1 - 5
// and 8 - 11 are shared as they stand; the dense form keeps its limit of BA_MAX_FREE.
//
// NOT part of this: intrinsics or distortion, more than 128 free cameras with the dense solve (ba_pcg_spec.h takes 65536), a
// preconditioner other than block Jacobi or an adaptive tolerance for the iterative one, robust losses other than the truncation,
// re-triangulation inside the loop.
#pragma once
#include "tri_solver.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define BA_MAX_ITERS 64
#define BA_MAX_FREE 128
#define BA_BLOCK 256
#define BA_LAMBDA_INIT 1e-4
#define BA_LAMBDA_DOWN 10.0
#define BA_LAMBDA_UP 10.0
#define BA_LAMBDA_MIN 1e-12
#define BA_LAMBDA_MAX 1e12
#define BA_FLAG_STEP_FAILED 1
#define BA_FLAG_POINT_HELD 2
#define BA_FLAG_FREE_NO_POSE 4

// workspace of ba_point_build's solves (doubles, through GsWs)
#define BA_PT_OFF_A 0             /* [3][4] */
#define BA_PT_OFF_X 12            /* [3] */
#define BA_PT_WS_DOUBLES 15

// the Jacobians' arrays must not be handed to an out-of-line function on the device: they would live in scratch memory
#if defined(__HIPCC__)
#define BA_HD_FLAT __host__ __device__ __forceinline__
#else
#define BA_HD_FLAT static inline
#endif

struct BaView {
    const int32_t* obs_off;      // [T + 1]
    const int32_t* obs_image;    // [n_obs]
    const float* obs_uv;         // [n_obs][2]
    const int32_t* obs_point;    // [n_obs]
    const int32_t* img_off;      // [n_images + 1]
    const int32_t* img_obs;      // [n_obs]
    const int32_t* cam_free;     // [n_images] the free index, -1: not free
    const int32_t* cam_ok;       // [n_images] tr_cam_ok
    const float* K;              // [n_images][9]
    int T, n_obs, n_images, F;
    double thr2;
};

struct BaState {
    const double* R;             // [n_images][9]
    const double* t;             // [n_images][3]
    const double* X;             // [T][3]
};

// what one iteration keeps between its stages
struct BaIter {
    uint8_t* part;               // [n_obs] takes part at the current state
    double* W;                   // [n_obs][18] Jc^T Jp, row r of 3 at 3 r (free cameras, taking part)
    double* Tm;                  // [n_obs][18] W A^-1
    double* g;                   // [T][3]
    double* Ainv;                // [T][9] row-major
    int32_t* hold;               // [T]
};

GS_HD void ba_point_range(const BaView& v, int p, int& b, int& e) {
    int len;
    gs_offsets_range(v.obs_off, p, v.n_obs, b, len);
    e = b + len;
}

// rule 2 and, when it takes part, rule 4: res = the residual, Pu / Pv the point's block, Cu / Cv the camera's.  One convention for both.
BA_HD_FLAT int ba_jacobian(const float* K, const double* R, const double* t, const double (&X)[3], double u, double v, double thr2, double (&res)[2],
                      double (&Pu)[3], double (&Pv)[3], double (&Cu)[6], double (&Cv)[6]) {
    double Y[3];
    tr_transform(R, t, X, Y);
    if (!(Y[2] > 0.0)) return 0;
    const double fx = (double)K[0], fy = (double)K[4];
    const double xz = Y[0] / Y[2], yz = Y[1] / Y[2];
    res[0] = (fx * xz + (double)K[2]) - u;
    res[1] = (fy * yz + (double)K[5]) - v;
    if (!(res[0] * res[0] + res[1] * res[1] < thr2)) return 0;
    const double au[3] = {fx / Y[2], 0.0, -(fx * xz) / Y[2]}, av[3] = {0.0, fy / Y[2], -(fy * yz) / Y[2]};
    double cu[3], cv[3];
    as_cross(Y, au, cu);
    as_cross(Y, av, cv);
    GS_UNROLL
    for (int k = 0; k < 3; ++k) {
        Pu[k] = au[0] * R[k] + au[2] * R[6 + k];
        Pv[k] = av[1] * R[3 + k] + av[2] * R[6 + k];
        Cu[k] = 2.0 * cu[k]; Cv[k] = 2.0 * cv[k];
        Cu[3 + k] = au[k]; Cv[3 + k] = av[k];
    }
    return 1;
}

// observation o of point p at state s; 0 when it takes no part
BA_HD_FLAT int ba_obs_jacobian(const BaView& v, const BaState& s, int o, int p, double (&res)[2], double (&Pu)[3], double (&Pv)[3], double (&Cu)[6],
                          double (&Cv)[6]) {
    const int img = v.obs_image[o];
    if (img < 0 || img >= v.n_images || !v.cam_ok[img]) return 0;
    const double X[3] = {s.X[3 * (size_t)p], s.X[3 * (size_t)p + 1], s.X[3 * (size_t)p + 2]};
    return ba_jacobian(v.K + 9 * (size_t)img, s.R + 9 * (size_t)img, s.t + 3 * (size_t)img, X, (double)v.obs_uv[2 * (size_t)o],
                       (double)v.obs_uv[2 * (size_t)o + 1], v.thr2, res, Pu, Pv, Cu, Cv);
}

// rule 3 for one point; takes_part (may be null) gets the per-observation bytes, *count their number
GS_HD double ba_point_cost(const BaView& v, const BaState& s, int p, uint8_t* takes_part, int32_t* count) {
    int b, e, c = 0;
    ba_point_range(v, p, b, e);
    const double X[3] = {s.X[3 * (size_t)p], s.X[3 * (size_t)p + 1], s.X[3 * (size_t)p + 2]};
    double sum = 0.0;
    for (int o = b; o < e; ++o) {
        const int img = v.obs_image[o];
        int in = 0;
        if (img >= 0 && img < v.n_images && v.cam_ok[img]) {
            double e2;
            const int front = tr_residual(v.K + 9 * (size_t)img, s.R + 9 * (size_t)img, s.t + 3 * (size_t)img, X, (double)v.obs_uv[2 * (size_t)o],
                                          (double)v.obs_uv[2 * (size_t)o + 1], e2);
            in = front && e2 < v.thr2;
            sum = sum + (in ? e2 : v.thr2);
        }
        if (takes_part) takes_part[o] = (uint8_t)in;
        c += in;
    }
    if (count) *count = c;
    return sum;
}

// the sum of a zero-padded block of BA_BLOCK partials, in place: the host's form; the device runs the same pairs on 256 threads
GS_HD double ba_block_tree(double* s) {
    for (int h = BA_BLOCK / 2; h >= 1; h >>= 1)
        for (int t = 0; t < h; ++t) s[t] = s[t] + s[t + h];
    return s[0];
}

// rule 5 for point p under damping lambda; returns the hold flag
GS_HD int ba_point_build(const BaView& v, const BaState& s, const BaIter& it, int p, double lambda, const GsWs& w) {
    int b, e;
    ba_point_range(v, p, b, e);
    double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int o = b; o < e; ++o) {
        double res[2], Pu[3], Pv[3], Cu[6], Cv[6];
        const int in = ba_obs_jacobian(v, s, o, p, res, Pu, Pv, Cu, Cv);
        it.part[o] = (uint8_t)in;
        if (!in) continue;
        const double nres[2] = {-res[0], -res[1]};
        tr_gn_accum(acc, Pu, Pv, nres);
        if (v.cam_free[v.obs_image[o]] >= 0) {
            double* W = it.W + 18 * (size_t)o;
            GS_UNROLL
            for (int r = 0; r < 6; ++r) {
                GS_UNROLL
                for (int m = 0; m < 3; ++m) W[3 * r + m] = Cu[r] * Pu[m] + Cv[r] * Pv[m];
            }
        }
    }
    double Ai[9];
    int ok = 1;
    GS_UNROLL
    for (int k = 0; k < 3; ++k) {
        GS_UNROLL
        for (int i = 0; i < 3; ++i) {
            GS_UNROLL
            for (int j = 0; j < 3; ++j) {
                const double a = acc[i <= j ? tr_sym3(i, j) : tr_sym3(j, i)];
                w(BA_PT_OFF_A + 4 * i + j) = i == j ? a + lambda * a : a;
            }
            w(BA_PT_OFF_A + 4 * i + 3) = i == k ? 1.0 : 0.0;
        }
        ok &= gs_solve<3>(w, BA_PT_OFF_A, BA_PT_OFF_X);
        GS_UNROLL
        for (int i = 0; i < 3; ++i) Ai[3 * i + k] = w(BA_PT_OFF_X + i);
    }
    GS_UNROLL
    for (int i = 0; i < 9; ++i) ok &= tr_finite(Ai[i]);
    GS_UNROLL
    for (int i = 0; i < 9; ++i) it.Ainv[9 * (size_t)p + i] = ok ? Ai[i] : 0.0;
    GS_UNROLL
    for (int i = 0; i < 3; ++i) it.g[3 * (size_t)p + i] = acc[6 + i];
    it.hold[p] = !ok;
    if (!ok) return 1;
    for (int o = b; o < e; ++o) {
        if (!it.part[o] || v.cam_free[v.obs_image[o]] < 0) continue;
        const double* W = it.W + 18 * (size_t)o;
        double* Tm = it.Tm + 18 * (size_t)o;
        GS_UNROLL
        for (int r = 0; r < 6; ++r) {
            GS_UNROLL
            for (int m = 0; m < 3; ++m) Tm[3 * r + m] = (W[3 * r] * Ai[m] + W[3 * r + 1] * Ai[3 + m]) + W[3 * r + 2] * Ai[6 + m];
        }
    }
    return 0;
}

// a[i] by compares: an index known only at run time would put the array into scratch memory on the device.  (BA_KEEP: an empty statement
// the optimiser cannot see through - it would turn the compares back into that index.  It changes no value.)
#if defined(__HIP_DEVICE_COMPILE__)
#define BA_KEEP(x) asm volatile("" : "+v"(x))
#else
#define BA_KEEP(x) (void)0
#endif
BA_HD_FLAT double ba_pick6(const double (&a)[6], int i) {
    double x = a[0];
    GS_UNROLL
    for (int k = 1; k < 6; ++k) {
        x = i == k ? a[k] : x;
        BA_KEEP(x);
    }
    return x;
}

// Which entries of a camera row a caller adds to: the host all of them, a device thread those whose index is its own modulo the block size.
struct BaOwnAll {
    GS_HD_MEMBER int first(int lo) const { return lo; }
    GS_HD_MEMBER int step() const { return 1; }
};
struct BaOwnLane {
    int lane, width;
    GS_HD_MEMBER int first(int lo) const { return lo + (((lane - lo) % width) + width) % width; }
    GS_HD_MEMBER int step() const { return width; }
};

// rule 6 for image img with free index f.  row: 36 (f + 1) doubles, block j at 36 j, entry (r, c) at 6 r + c; rhs: 6 doubles.  The caller
// has zeroed the entries it owns.  Own says which entries this caller adds to: an entry is only ever touched by its owner, so the stages need
// no barrier between them.
template <class Own>
BA_HD_FLAT void ba_camera_row(const BaView& v, const BaState& s, const BaIter& it, int img, int f, double lambda, double* row, double* rhs,
                         const Own& own) {
    int qb, qlen;
    gs_offsets_range(v.img_off, img, v.n_obs, qb, qlen);
    const int d0 = 36 * f;
    int n_part = 0;
    for (int q = qb; q < qb + qlen; ++q) {
        const int k = v.img_obs[q];
        if (k < 0 || k >= v.n_obs || !it.part[k]) continue;
        const int p = v.obs_point[k];
        double res[2], Pu[3], Pv[3], Cu[6], Cv[6];
        if (!ba_obs_jacobian(v, s, k, p, res, Pu, Pv, Cu, Cv)) continue;
        ++n_part;
        for (int e = own.first(d0); e < d0 + 36; e += own.step()) {
            const int r = (e - d0) / 6, c = (e - d0) % 6;
            row[e] = row[e] + (ba_pick6(Cu, r) * ba_pick6(Cu, c) + ba_pick6(Cv, r) * ba_pick6(Cv, c));
        }
        for (int r = own.first(0); r < 6; r += own.step()) rhs[r] = rhs[r] + (ba_pick6(Cu, r) * (-res[0]) + ba_pick6(Cv, r) * (-res[1]));
    }
    for (int e = own.first(d0); e < d0 + 36; e += own.step()) {
        const int r = (e - d0) / 6, c = (e - d0) % 6;
        if (r == c) row[e] = n_part ? row[e] + lambda * row[e] : 1.0;
    }
    for (int q = qb; q < qb + qlen; ++q) {
        const int k = v.img_obs[q];
        if (k < 0 || k >= v.n_obs || !it.part[k]) continue;
        const int p = v.obs_point[k];
        if (p < 0 || p >= v.T || it.hold[p]) continue;
        const double* Tk = it.Tm + 18 * (size_t)k;
        int lb, le;
        ba_point_range(v, p, lb, le);
        for (int l = lb; l < le; ++l) {
            if (!it.part[l]) continue;
            const int j = v.cam_free[v.obs_image[l]];
            if (j < 0 || j > f) continue;
            const double* Wl = it.W + 18 * (size_t)l;
            const int j0 = 36 * j;
            for (int e = own.first(j0); e < j0 + 36; e += own.step()) {
                const int r = (e - j0) / 6, c = (e - j0) % 6;
                row[e] = row[e] - ((Tk[3 * r] * Wl[3 * c] + Tk[3 * r + 1] * Wl[3 * c + 1]) + Tk[3 * r + 2] * Wl[3 * c + 2]);
            }
        }
        const double* g = it.g + 3 * (size_t)p;
        for (int r = own.first(0); r < 6; r += own.step()) rhs[r] = rhs[r] - ((Tk[3 * r] * g[0] + Tk[3 * r + 1] * g[1]) + Tk[3 * r + 2] * g[2]);
    }
}

// rule 11 for the small tables, on host copies: the message of the first violation, or null
static inline const char* ba_check_tables(const int32_t* obs_off, int T, int n_obs, const int32_t* obs_image, const int32_t* img_off,
                                          const int32_t* img_obs, const int32_t* cam_free, int n_images, int F) {
    if (obs_off[0] != 0 || obs_off[T] != n_obs) return "obs_offsets must start at 0 and end at n_obs";
    for (int p = 0; p < T; ++p)
        if (obs_off[p + 1] < obs_off[p]) return "obs_offsets must ascend";
    for (int o = 0; o < n_obs; ++o)
        if (obs_image[o] < 0 || obs_image[o] >= n_images) return "an observation names an image outside [0, n_images)";
    if (img_off[0] != 0 || img_off[n_images] != n_obs) return "img_offsets must start at 0 and end at n_obs";
    for (int i = 0; i < n_images; ++i) {
        if (img_off[i + 1] < img_off[i]) return "img_offsets must ascend";
        for (int q = img_off[i]; q < img_off[i + 1]; ++q) {
            const int k = img_obs[q];
            if (k < 0 || k >= n_obs || obs_image[k] != i) return "img_obs lists an observation that is not its image's";
            if (q > img_off[i] && img_obs[q - 1] >= k) return "img_obs must ascend inside an image";
        }
    }
    int next = 0;
    for (int i = 0; i < n_images; ++i) {
        if (cam_free[i] == -1) continue;
        if (cam_free[i] != next) return "cam_free must hold -1 or the free indices 0 .. F - 1 in ascending order";
        ++next;
    }
    if (next != F) return "F is not the number of free cameras";
    return nullptr;
}

// rule 7: the chain of entry (a, c), c <= a: s = S[a][c], ra[k * stride] = L[a][k] and rc[k] = L[c][k] for k < c.  (The stride: the device
// keeps a transposed copy of L, so that neighbouring threads - neighbouring rows a - read neighbouring addresses.)
GS_HD double ba_chol_chain(double s, const double* ra, long stride, const double* rc, int c) {
    for (int k = 0; k < c; ++k) s = s - ra[(long)k * stride] * rc[k];
    return s;
}

// rule 8 for point p: the candidate's X (the current one for a held point)
GS_HD void ba_point_delta(const BaView& v, const BaState& s, const BaIter& it, int p, const double* dc, double* X_out) {
    double d[3] = {0.0, 0.0, 0.0};
    if (!it.hold[p]) {
        int b, e;
        ba_point_range(v, p, b, e);
        double sg[3] = {it.g[3 * (size_t)p], it.g[3 * (size_t)p + 1], it.g[3 * (size_t)p + 2]};
        for (int o = b; o < e; ++o) {
            if (!it.part[o]) continue;
            const int j = v.cam_free[v.obs_image[o]];
            if (j < 0) continue;
            const double* W = it.W + 18 * (size_t)o;
            for (int r = 0; r < 6; ++r) {
                GS_UNROLL
                for (int m = 0; m < 3; ++m) sg[m] = sg[m] - W[3 * r + m] * dc[6 * j + r];
            }
        }
        const double* Ai = it.Ainv + 9 * (size_t)p;
        GS_UNROLL
        for (int i = 0; i < 3; ++i) d[i] = (Ai[3 * i] * sg[0] + Ai[3 * i + 1] * sg[1]) + Ai[3 * i + 2] * sg[2];
    }
    GS_UNROLL
    for (int i = 0; i < 3; ++i) X_out[3 * (size_t)p + i] = s.X[3 * (size_t)p + i] + d[i];
}

// rule 8 for image img: the candidate's pose; 0 when a free camera's update is not finite (the pose is then the current one)
GS_HD int ba_camera_delta(const BaView& v, const BaState& s, int img, const double* dc, double* R_out, double* t_out) {
    double R[9], t[3];
    GS_UNROLL
    for (int k = 0; k < 9; ++k) R[k] = s.R[9 * (size_t)img + k];
    GS_UNROLL
    for (int k = 0; k < 3; ++k) t[k] = s.t[3 * (size_t)img + k];
    int ok = 1;
    const int f = v.cam_free[img];
    if (f >= 0 && v.cam_ok[img]) {
        const double d[6] = {dc[6 * f], dc[6 * f + 1], dc[6 * f + 2], dc[6 * f + 3], dc[6 * f + 4], dc[6 * f + 5]};
        ok = as_gn_update(d, R, t);
    }
    GS_UNROLL
    for (int k = 0; k < 9; ++k) R_out[9 * (size_t)img + k] = R[k];
    GS_UNROLL
    for (int k = 0; k < 3; ++k) t_out[3 * (size_t)img + k] = t[k];
    return ok;
}

// rule 9: the decision of one iteration.  Returns accepted.
GS_HD int ba_decide_step(int step_ok, double cost_cur, double cost_cand, double& lambda) {
    const int acc = step_ok && cost_cand < cost_cur;
    if (acc) {
        const double l = lambda / BA_LAMBDA_DOWN;
        lambda = l < BA_LAMBDA_MIN ? BA_LAMBDA_MIN : l;
    } else {
        const double l = lambda * BA_LAMBDA_UP;
        lambda = l > BA_LAMBDA_MAX ? BA_LAMBDA_MAX : l;
    }
    return acc;
}
