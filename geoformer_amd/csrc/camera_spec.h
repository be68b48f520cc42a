// Lens distortion of match coordinates: THE RULE, compiled by k_camera.hip for the device and by host/camera_host.cpp for the CPU.  Plain
// C++ in fp64 with contraction off, only + - * /, comparisons and fabs (no atan, tan or pow: the fisheye models are out of scope), so the
// two builds agree bit for bit.  The models and their parameter order are COLMAP's; pycolmap parity is UNPINNED.
//
// A camera is one canonical record of CM_REC doubles (fx, fy, cx, cy, k1, k2, p1, p2).  matcher.canonical_camera brings every model to it:
//   SIMPLE_PINHOLE f, cx, cy             -> (f, f, cx, cy, 0, 0, 0, 0)        PINHOLE fx, fy, cx, cy -> (fx, fy, cx, cy, 0, 0, 0, 0)
//   SIMPLE_RADIAL  f, cx, cy, k          -> (f, f, cx, cy, k, 0, 0, 0)        RADIAL  f, cx, cy, k1, k2 -> (f, f, cx, cy, k1, k2, 0, 0)
//   OPENCV         fx, fy, cx, cy, k1, k2, p1, p2 as they are
// Points come as a list of P rows (row i starts pts_stride floats after row i - 1: the two sides of an [M, 4] match block are read in
// place), cut into S segments by seg_off [S + 1]; segment s belongs to camera seg_camera[s] of a table of C records.
//
//  1. The segment of point i is the last s with seg_off[s] <= i (bisection; empty segments are skipped by it).  A point outside
//     [seg_off[s], seg_off[s + 1]) or with a camera index outside [0, C) gets NaN and status CM_ST_ARGS, and the call's flag words say
//     which (CM_FLAG_OFFSETS also for seg_off[0] != 0, seg_off[S] != P and a descending step): reported, never a wrapped index.
//  2. A point with a non-finite coordinate gets NaN and status CM_ST_NONFINITE, whatever the camera.
//  3. A camera whose k1, k2, p1, p2 are all zero (cm_no_distortion; both pinhole models) passes the coordinates through with their input
//     bits, in both directions.
//  4. DISTORT (cm_distort, closed form), with r2 = x x + y y and rad = 1 + k1 r2 + k2 r2 r2:
//        x' = x rad + 2 p1 x y + p2 (r2 + 2 x x)        y' = y rad + p1 (r2 + 2 y y) + 2 p2 x y
//     gf_distort_points: (x, y) = ((u - cx) / fx, (v - cy) / fy) of an ideal pixel, (u', v') = (fx x' + cx, fy y' + cy).
//  5. UNDISTORT (cm_undistort): Newton on f(x) = distort(x) - target with the analytic 2 x 2 Jacobian (cm_jacobian), target =
//     ((u - cx) / fx, (v - cy) / fy), start at the target, at most CM_MAX_STEPS steps.  A step is taken only if it strictly lowers
//     |f|^2 (a NaN is never lower); the iteration ends at |f|^2 == 0, at a rejected step or at the cap.  A Jacobian determinant that is
//     not > 0 ends it as a failure.  The result is accepted iff max(|f_x|, |f_y|) <= CM_ACCEPT (normalised units; 1e-6 px at f = 1000)
//     and the determinant at the result is > 0: status CM_ST_OK, else NaN and CM_ST_NO_PREIMAGE.
//     CONVENTION: Newton from the target stays inside the first fold of the model (determinant > 0 along the way), so a pixel whose true
//     pre-image lies beyond the fold gets the pre-image inside it, and a target beyond the model's range is a failure.
//  6. Output: u' = fx x + cx, v' = fy y + cy in fp64, each rounded once to fp32 (cm_pixel).  On status != 0 both are NaN.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CM_HD __host__ __device__ inline
#else
#define CM_HD static inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define CM_REC 8                 /* doubles of a canonical record: fx, fy, cx, cy, k1, k2, p1, p2 */
#define CM_MAX_STEPS 32
#define CM_ACCEPT 1e-9
#define CM_ST_OK 0
#define CM_ST_NONFINITE 1        /* non-finite input */
#define CM_ST_NO_PREIMAGE 2      /* no pre-image found */
#define CM_ST_ARGS 3             /* the point lies in no segment, or its segment names a camera outside the table */
#define CM_FLAG_WORDS 2          /* int32 flag words of a call, each 0 or 1: [CM_FLAG_OFFSETS], [CM_FLAG_CAMERA] */
#define CM_FLAG_OFFSETS 0
#define CM_FLAG_CAMERA 1

CM_HD int cm_finite(double v) { return v - v == 0.0; }

CM_HD int cm_no_distortion(const double* c) { return c[4] == 0.0 && c[5] == 0.0 && c[6] == 0.0 && c[7] == 0.0; }

CM_HD void cm_distort(const double* c, double x, double y, double& xd, double& yd) {
    const double k1 = c[4], k2 = c[5], p1 = c[6], p2 = c[7];
    const double xx = x * x, yy = y * y, xy = x * y;
    const double r2 = xx + yy;
    const double rad = (1.0 + k1 * r2) + k2 * (r2 * r2);
    xd = (x * rad + (2.0 * p1) * xy) + p2 * (r2 + 2.0 * xx);
    yd = (y * rad + p1 * (r2 + 2.0 * yy)) + (2.0 * p2) * xy;
}

// the Jacobian of cm_distort at (x, y): j = (dx'/dx, dx'/dy, dy'/dx, dy'/dy); returns its determinant
CM_HD double cm_jacobian(const double* c, double x, double y, double* j) {
    const double k1 = c[4], k2 = c[5], p1 = c[6], p2 = c[7];
    const double xx = x * x, yy = y * y, xy = x * y;
    const double r2 = xx + yy;
    const double rad = (1.0 + k1 * r2) + k2 * (r2 * r2);
    const double g = 2.0 * (k1 + (2.0 * k2) * r2);                      // d rad / d r2, doubled
    const double off = (g * xy + (2.0 * p1) * x) + (2.0 * p2) * y;
    j[0] = ((rad + g * xx) + (2.0 * p1) * y) + (6.0 * p2) * x;
    j[1] = off;
    j[2] = off;
    j[3] = ((rad + g * yy) + (6.0 * p1) * y) + (2.0 * p2) * x;
    return j[0] * j[3] - j[1] * j[2];
}

// step 5: the pre-image (x, y) of the normalised target (tx, ty); returns 1 when it is accepted.  steps (may be null): Newton steps taken
CM_HD int cm_undistort(const double* c, double tx, double ty, double& x, double& y, int* steps) {
    double j[4], dx, dy;
    x = tx; y = ty;
    cm_distort(c, x, y, dx, dy);
    double f0 = dx - tx, f1 = dy - ty;
    double n2 = f0 * f0 + f1 * f1;
    int taken = 0, ok = 1;
    for (int it = 0; it < CM_MAX_STEPS; ++it) {
        if (n2 == 0.0) break;
        const double det = cm_jacobian(c, x, y, j);
        if (!(det > 0.0)) { ok = 0; break; }
        const double xn = x - (j[3] * f0 - j[1] * f1) / det;
        const double yn = y - (j[0] * f1 - j[2] * f0) / det;
        cm_distort(c, xn, yn, dx, dy);
        const double g0 = dx - tx, g1 = dy - ty;
        const double m2 = g0 * g0 + g1 * g1;
        if (!(m2 < n2)) break;                                          // a NaN or a step that does not lower |f|^2 is not taken
        x = xn; y = yn; f0 = g0; f1 = g1; n2 = m2;
        ++taken;
    }
    if (steps) *steps = taken;
    if (!ok) return 0;
    const double a0 = fabs(f0), a1 = fabs(f1);
    if (!((a0 > a1 ? a0 : a1) <= CM_ACCEPT)) return 0;
    return cm_jacobian(c, x, y, j) > 0.0;
}

CM_HD float cm_pixel(double f, double x, double c) { return (float)(f * x + c); }

// steps 2 - 6 for one point of camera c: (u, v) -> out [2]; returns the status.  inverse = 1 undistorts, 0 distorts.
CM_HD int cm_point(const double* c, float u, float v, int inverse, float* out) {
    const float nanf_ = __builtin_nanf("");
    out[0] = nanf_; out[1] = nanf_;
    if (!cm_finite((double)u) || !cm_finite((double)v)) return CM_ST_NONFINITE;
    if (cm_no_distortion(c)) { out[0] = u; out[1] = v; return CM_ST_OK; }
    const double tx = ((double)u - c[2]) / c[0], ty = ((double)v - c[3]) / c[1];
    double x, y;
    if (inverse) {
        if (!cm_undistort(c, tx, ty, x, y, 0)) return CM_ST_NO_PREIMAGE;
    } else {
        cm_distort(c, tx, ty, x, y);
    }
    out[0] = cm_pixel(c[0], x, c[2]); out[1] = cm_pixel(c[1], y, c[3]);
    return CM_ST_OK;
}

// step 1 for point i: its camera record, or null (flags written).  P > 0, S > 0.
CM_HD const double* cm_camera_of(const int32_t* seg_off, const int32_t* seg_camera, int S, const double* cameras, int C, int i, int32_t* flags) {
    int lo = 0, hi = S;                                                 // the last segment whose first point is <= i
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (seg_off[mid] <= i) lo = mid; else hi = mid;
    }
    if (!(seg_off[lo] <= i && i < seg_off[lo + 1])) { flags[CM_FLAG_OFFSETS] = 1; return 0; }
    const int cam = seg_camera[lo];
    if (cam < 0 || cam >= C) { flags[CM_FLAG_CAMERA] = 1; return 0; }
    return cameras + (size_t)CM_REC * (size_t)cam;
}

// step 1 for boundary j in 0 .. S of the offsets and for segment j (an empty one included): every thread / iteration checks one
CM_HD void cm_check_segment(const int32_t* seg_off, const int32_t* seg_camera, int S, int C, int P, int j, int32_t* flags) {
    if (j == 0 && seg_off[0] != 0) flags[CM_FLAG_OFFSETS] = 1;
    if (j == S && seg_off[S] != P) flags[CM_FLAG_OFFSETS] = 1;
    if (j < S && seg_off[j] > seg_off[j + 1]) flags[CM_FLAG_OFFSETS] = 1;
    if (j < S && (seg_camera[j] < 0 || seg_camera[j] >= C)) flags[CM_FLAG_CAMERA] = 1;
}
