// Essential-matrix RANSAC: the algorithm, stated once for the device (k_pose.hip) and the host (host/pose_host.cpp).
//
// Plain C++ in fp64 with contraction off, only + - * / sqrt, fabs and comparisons: no libm transcendental, no library call whose
// rounding could differ between the two builds, so a host build and gfx950 agree bit for bit (as k_ransac.hip does with
// oracle/ransac_oracle.c).  OpenCV parity (cv2.findEssentialMat / cv2.recoverPose, model/loftr_src/utils/metrics.py:72-98) is
// UNPINNED; what is pinned is the algorithm written here.
//
//   ps_five_point   Nister's five-point solver.  5x9 epipolar system x1^T E x0 = 0 -> its 4-dimensional null space by Gauss-Jordan
//                   with full pivoting (E = xX + yY + zZ + W) -> the ten cubic constraints det E = 0, 2 E E^T E - tr(E E^T) E = 0 over
//                   the 20 monomials of degree <= 3 -> Gauss-Jordan on the ten columns of highest order in (x, y) -> three rows
//                   [x y 1] B(z) = 0 with B's entries of degree 3, 3, 4 in z -> det B(z), degree 10 -> its real roots -> each polished on the cubic constraints themselves (ps_root_to_E).
//                   Roots without an eigen-solver: the roots of the k-th derivative separate those of the (k-1)-th, so the chain
//                   p^(9) (linear) .. p^(0) is walked upwards, every sign change between neighbouring critical points bisected a
//                   FIXED number of times (PS_BISECT_LOW on the derivatives, PS_BISECT_TOP + PS_NEWTON guarded Newton steps on p).
//                   Between -bound and +bound an even-degree polynomial changes sign an even number of times: 0, 2, .. 10 roots.
//   ps_inlier       OpenCV's essential-matrix residual (gs_sampson of solver_common.h) on normalised coordinates; inlier iff < thr^2.
//                   The five matches of a hypothesis: gs_draw_distinct<5>.
//   ps_decompose    E -> (R1, R2, t) without an SVD: t from the largest column of 1/2 tr(EE^T) I - EE^T, R = (cof(E) -+ [t]x E) / |t|^2
//                   (Horn 1990).  Candidates in the fixed order (R1, t), (R2, t), (R1, -t), (R2, -t).
//   ps_cheiral      a match votes for a candidate when it triangulates to a depth in (0, 1e9) in both cameras (recoverPose's
//                   distanceThresh as metrics.py:93 passes it).
//
// Workspace: everything indexed at run time lives in PS_WS_DOUBLES doubles reached through PsWs (element i at p[i * stride]), so the
// caller decides where: a local array on the host, an LDS tile interleaved across the lanes of a workgroup on the device.
#pragma once
#include <math.h>
#include <stdint.h>

#include "solver_common.h"

#define PS_HD GS_HD
#define PS_HD_MEMBER GS_HD_MEMBER
#define PS_UNROLL GS_UNROLL
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define PS_MAX_ROOTS 10
#define PS_HYP_PER_WG 32          /* hypotheses one workgroup of pose_score solves: iters must be a positive multiple */
#define PS_MIN_MATCHES 5
#define PS_BISECT_LOW 40
#define PS_BISECT_TOP 56
#define PS_NEWTON 2
#define PS_POLISH 16
#define PS_DEPTH_MAX 1e9

// workspace layout (doubles)
#define PS_OFF_M 0                /* [10][20] constraint matrix; the 5x9 epipolar system before it */
#define PS_OFF_BASIS 200          /* [4][9]  X, Y, Z, W */
#define PS_WS_DOUBLES 236
// after the elimination rows 0-3 of M are dead, and rows 4-9 once B(z) is out:
#define PS_OFF_B 0                /* [3][13]  per row: x coefficient (4, ascending in z), y coefficient (4), constant (5) */
#define PS_OFF_P 40               /* [11] det B(z), ascending */
#define PS_OFF_T 52               /* [8 + 8 + 7] the three 2x2 minors of rows 1, 2 */
#define PS_OFF_R0 76              /* [12] roots of the previous derivative */
#define PS_OFF_R1 88              /* [12] roots being found */
#define PS_OFF_E 100              /* [10][9] the solutions, Frobenius norm 1 */

typedef GsWs PsWs;

PS_HD double ps_abs_or_inf(double v) { return gs_abs_or_inf(v); }

// ---- monomials: exponents (a, b, c) of x, y, z packed as 16 a + 4 b + c (no carries up to degree 3)
PS_HD int ps_key1(int i) { return i == 0 ? 16 : i == 1 ? 4 : i == 2 ? 1 : 0; }                      // x y z 1
PS_HD int ps_key2(int i) {                                                                             // x2 y2 z2 xy xz yz x y z 1
    switch (i) { case 0: return 32; case 1: return 8; case 2: return 2; case 3: return 20; case 4: return 17;
                 case 5: return 5; case 6: return 16; case 7: return 4; case 8: return 1; default: return 0; }
}
PS_HD int ps_idx2(int key) {
    switch (key) { case 32: return 0; case 8: return 1; case 2: return 2; case 20: return 3; case 17: return 4;
                   case 5: return 5; case 16: return 6; case 4: return 7; case 1: return 8; default: return 9; }
}
// columns of the constraint matrix (Nister's order): x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1
PS_HD int ps_idx3(int key) {
    switch (key) { case 48: return 0; case 12: return 1; case 36: return 2; case 24: return 3; case 33: return 4; case 32: return 5;
                   case 9: return 6; case 8: return 7; case 21: return 8; case 20: return 9; case 18: return 10; case 17: return 11;
                   case 16: return 12; case 6: return 13; case 5: return 14; case 4: return 15; case 3: return 16; case 2: return 17;
                   case 1: return 18; default: return 19; }
}
// d (degree 2) += / -= a (degree 1) * b (degree 1)
PS_HD void ps_mul11(double (&d)[10], const double (&a)[4], const double (&b)[4], bool neg) {
    PS_UNROLL
    for (int i = 0; i < 4; ++i) {
        PS_UNROLL
        for (int j = 0; j < 4; ++j) {
            const double p = a[i] * b[j];
            const int k = ps_idx2(ps_key1(i) + ps_key1(j));
            d[k] = neg ? d[k] - p : d[k] + p;
        }
    }
}
// d (degree 3) += / -= a (degree 2) * b (degree 1)
PS_HD void ps_mul21(double (&d)[20], const double (&a)[10], const double (&b)[4], bool neg) {
    PS_UNROLL
    for (int i = 0; i < 10; ++i) {
        PS_UNROLL
        for (int j = 0; j < 4; ++j) {
            const double p = a[i] * b[j];
            const int k = ps_idx3(ps_key2(i) + ps_key1(j));
            d[k] = neg ? d[k] - p : d[k] + p;
        }
    }
}

// ---- null space of the 5x9 epipolar system: Gauss-Jordan with full pivoting (solver_common.h: gs_eliminate9, gs_null_basis)
PS_HD int ps_nullspace(const double (&x0)[5][2], const double (&x1)[5][2], const PsWs& w) {
    for (int r = 0; r < 5; ++r) {
        const double a = x0[r][0], b = x0[r][1], u = x1[r][0], v = x1[r][1];
        w(9 * r + 0) = u * a; w(9 * r + 1) = u * b; w(9 * r + 2) = u;
        w(9 * r + 3) = v * a; w(9 * r + 4) = v * b; w(9 * r + 5) = v;
        w(9 * r + 6) = a; w(9 * r + 7) = b; w(9 * r + 8) = 1.0;
    }
    unsigned long long perm;
    if (!gs_eliminate9<5>(w, perm)) return 0;
    gs_null_basis<5>(w, perm, PS_OFF_BASIS);
    // Mix the four vectors by the orthogonal 4x4 Hadamard matrix / 2.  Small rotations make E nearly skew-symmetric, and when the free
    // columns hold a pair E[i][j], E[j][i] EVERY solution has z = E[i][j] / E[j][i] near -1: ten roots in a cluster of radius rho, whose
    // expanded polynomial cancels by rho^-10.  In the mixed basis no coordinate ratio is tied to a pair of entries of E.
    for (int j = 0; j < 9; ++j) {
        const double a = w(PS_OFF_BASIS + j), b = w(PS_OFF_BASIS + 9 + j), c = w(PS_OFF_BASIS + 18 + j), d = w(PS_OFF_BASIS + 27 + j);
        w(PS_OFF_BASIS + j) = 0.5 * ((a + b) + (c + d));
        w(PS_OFF_BASIS + 9 + j) = 0.5 * ((a - b) + (c - d));
        w(PS_OFF_BASIS + 18 + j) = 0.5 * ((a + b) - (c + d));
        w(PS_OFF_BASIS + 27 + j) = 0.5 * ((a - b) - (c - d));
    }
    return 1;
}

// ---- the ten cubic constraints, rows 0-8: (E E^T - 1/2 tr(E E^T) I) E = 0, row 9: det E = 0
PS_HD void ps_constraints(const PsWs& w) {
    double e[9][4];                                   // E[i][j] as a polynomial of degree 1: coefficients of x, y, z, 1
    PS_UNROLL
    for (int ij = 0; ij < 9; ++ij) {
        PS_UNROLL
        for (int k = 0; k < 4; ++k) e[ij][k] = w(PS_OFF_BASIS + 9 * k + ij);
    }
    double half_tr[10];
    PS_UNROLL
    for (int k = 0; k < 10; ++k) half_tr[k] = 0.0;
    PS_UNROLL
    for (int ij = 0; ij < 9; ++ij) ps_mul11(half_tr, e[ij], e[ij], false);
    PS_UNROLL
    for (int k = 0; k < 10; ++k) half_tr[k] = 0.5 * half_tr[k];
    PS_UNROLL
    for (int i = 0; i < 3; ++i) {
        double lam[3][10];                            // row i of E E^T - 1/2 tr I
        PS_UNROLL
        for (int k = 0; k < 3; ++k) {
            PS_UNROLL
            for (int q = 0; q < 10; ++q) lam[k][q] = 0.0;
            PS_UNROLL
            for (int m = 0; m < 3; ++m) ps_mul11(lam[k], e[3 * i + m], e[3 * k + m], false);
            if (k == i) {
                PS_UNROLL
                for (int q = 0; q < 10; ++q) lam[k][q] = lam[k][q] - half_tr[q];
            }
        }
        PS_UNROLL
        for (int j = 0; j < 3; ++j) {
            double row[20];
            PS_UNROLL
            for (int q = 0; q < 20; ++q) row[q] = 0.0;
            PS_UNROLL
            for (int k = 0; k < 3; ++k) ps_mul21(row, lam[k], e[3 * k + j], false);
            PS_UNROLL
            for (int q = 0; q < 20; ++q) w(PS_OFF_M + 20 * (3 * i + j) + q) = row[q];
        }
    }
    double row[20];
    PS_UNROLL
    for (int q = 0; q < 20; ++q) row[q] = 0.0;
    PS_UNROLL
    for (int j = 0; j < 3; ++j) {                     // cofactor expansion along row 0
        const int j1 = j == 0 ? 1 : 0, j2 = j == 2 ? 1 : 2;
        double minor[10];
        PS_UNROLL
        for (int q = 0; q < 10; ++q) minor[q] = 0.0;
        ps_mul11(minor, e[3 + j1], e[6 + j2], false);
        ps_mul11(minor, e[3 + j2], e[6 + j1], true);
        ps_mul21(row, minor, e[j], j == 1);
    }
    PS_UNROLL
    for (int q = 0; q < 20; ++q) w(PS_OFF_M + 180 + q) = row[q];
}

// ---- Gauss-Jordan with partial pivoting on the first ten columns; rows 4-9 end with the identity there (rows 0-3 are only
// eliminated downwards: nothing reads them again)
PS_HD int ps_eliminate(const PsWs& w) {
    for (int c = 0; c < 10; ++c) {
        int p = c;
        double best = ps_abs_or_inf(w(20 * c + c));
        for (int r = c + 1; r < 10; ++r) {
            const double v = ps_abs_or_inf(w(20 * r + c));
            if (v > best) { best = v; p = r; }
        }
        if (!(best > 1e-12) || best == (double)INFINITY) return 0;
        if (p != c)
            for (int k = c; k < 20; ++k) { const double tmp = w(20 * c + k); w(20 * c + k) = w(20 * p + k); w(20 * p + k) = tmp; }
        const double inv = 1.0 / w(20 * c + c);
        for (int k = c; k < 20; ++k) w(20 * c + k) = w(20 * c + k) * inv;
        for (int r = 4; r < 10; ++r) {
            if (r == c) continue;
            const double f = w(20 * r + c);
            if (f != 0.0)
                for (int k = c; k < 20; ++k) w(20 * r + k) = w(20 * r + k) - f * w(20 * c + k);
        }
        for (int r = c + 1; r < 4; ++r) {
            const double f = w(20 * r + c);
            if (f != 0.0)
                for (int k = c; k < 20; ++k) w(20 * r + k) = w(20 * r + k) - f * w(20 * c + k);
        }
    }
    return 1;
}

// polynomial product into the workspace: d[0 .. na + nb - 2] += / -= a[0 .. na - 1] * b[0 .. nb - 1] (ascending coefficients)
PS_HD void ps_polymul(const PsWs& w, int d, int a, int na, int b, int nb, bool neg) {
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < nb; ++j) {
            const double p = w(a + i) * w(b + j);
            w(d + i + j) = neg ? w(d + i + j) - p : w(d + i + j) + p;
        }
}

// rows (e, f) = (4, 5), (6, 7), (8, 9): e - z f has no term of degree 2 in (x, y) left
PS_HD void ps_bz(const PsWs& w) {
    for (int i = 0; i < 3; ++i) {
        const int e = 20 * (4 + 2 * i), f = e + 20, o = PS_OFF_B + 13 * i;
        for (int g = 0; g < 2; ++g) {                 // x (columns 10-12) and y (columns 13-15): z2, z, 1
            const int c = 10 + 3 * g;
            const double e2 = w(e + c), e1 = w(e + c + 1), e0 = w(e + c + 2), f2 = w(f + c), f1 = w(f + c + 1), f0 = w(f + c + 2);
            w(o + 4 * g + 0) = e0; w(o + 4 * g + 1) = e1 - f0; w(o + 4 * g + 2) = e2 - f1; w(o + 4 * g + 3) = -f2;
        }
        const double e3 = w(e + 16), e2 = w(e + 17), e1 = w(e + 18), e0 = w(e + 19);
        const double f3 = w(f + 16), f2 = w(f + 17), f1 = w(f + 18), f0 = w(f + 19);
        w(o + 8) = e0; w(o + 9) = e1 - f0; w(o + 10) = e2 - f1; w(o + 11) = e3 - f2; w(o + 12) = -f3;
    }
}

PS_HD void ps_detpoly(const PsWs& w) {
    for (int k = PS_OFF_P; k < PS_OFF_R0; ++k) w(k) = 0.0;
    const int r0 = PS_OFF_B, r1 = PS_OFF_B + 13, r2 = PS_OFF_B + 26, t1 = PS_OFF_T, t2 = PS_OFF_T + 8, t3 = PS_OFF_T + 16;
    ps_polymul(w, t1, r1 + 4, 4, r2 + 8, 5, false); ps_polymul(w, t1, r1 + 8, 5, r2 + 4, 4, true);    // b1 c2 - c1 b2
    ps_polymul(w, t2, r1 + 0, 4, r2 + 8, 5, false); ps_polymul(w, t2, r1 + 8, 5, r2 + 0, 4, true);    // a1 c2 - c1 a2
    ps_polymul(w, t3, r1 + 0, 4, r2 + 4, 4, false); ps_polymul(w, t3, r1 + 4, 4, r2 + 0, 4, true);    // a1 b2 - b1 a2
    ps_polymul(w, PS_OFF_P, r0 + 0, 4, t1, 8, false);
    ps_polymul(w, PS_OFF_P, r0 + 4, 4, t2, 8, true);
    ps_polymul(w, PS_OFF_P, r0 + 8, 5, t3, 7, false);
}

// real roots of the polynomial at PS_OFF_P, ascending, into PS_OFF_R0; returns their number (0 when the polynomial is not of
// degree 10 in finite numbers)
PS_HD int ps_real_roots(const PsWs& w) {
    return gs_real_roots<10>(w, PS_OFF_P, PS_OFF_R0, PS_OFF_R1, PS_BISECT_LOW, PS_BISECT_TOP, PS_NEWTON);
}

// residuals of the ten cubic constraints at a numeric E: c[0..8] = 2 E E^T E - tr(E E^T) E, c[9] = det E
PS_HD void ps_cubic(const double (&E)[9], double (&c)[10]) {
    double M[9];
    PS_UNROLL
    for (int i = 0; i < 3; ++i) {
        PS_UNROLL
        for (int j = 0; j < 3; ++j) M[3 * i + j] = (E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1]) + E[3 * i + 2] * E[3 * j + 2];
    }
    const double tr = (M[0] + M[4]) + M[8];
    PS_UNROLL
    for (int i = 0; i < 3; ++i) {
        PS_UNROLL
        for (int j = 0; j < 3; ++j)
            c[3 * i + j] = 2.0 * ((M[3 * i] * E[j] + M[3 * i + 1] * E[3 + j]) + M[3 * i + 2] * E[6 + j]) - tr * E[3 * i + j];
    }
    c[9] = (E[0] * (E[4] * E[8] - E[5] * E[7]) - E[1] * (E[3] * E[8] - E[5] * E[6])) + E[2] * (E[3] * E[7] - E[4] * E[6]);
}
// their derivative along the direction D
PS_HD void ps_cubic_d(const double (&E)[9], const double (&D)[9], double (&dc)[10]) {
    double M[9], dM[9];
    PS_UNROLL
    for (int i = 0; i < 3; ++i) {
        PS_UNROLL
        for (int j = 0; j < 3; ++j) {
            M[3 * i + j] = (E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1]) + E[3 * i + 2] * E[3 * j + 2];
            dM[3 * i + j] = ((D[3 * i] * E[3 * j] + D[3 * i + 1] * E[3 * j + 1]) + D[3 * i + 2] * E[3 * j + 2]) +
                            ((E[3 * i] * D[3 * j] + E[3 * i + 1] * D[3 * j + 1]) + E[3 * i + 2] * D[3 * j + 2]);
        }
    }
    const double tr = (M[0] + M[4]) + M[8], dtr = (dM[0] + dM[4]) + dM[8];
    PS_UNROLL
    for (int i = 0; i < 3; ++i) {
        PS_UNROLL
        for (int j = 0; j < 3; ++j)
            dc[3 * i + j] = (2.0 * (((dM[3 * i] * E[j] + dM[3 * i + 1] * E[3 + j]) + dM[3 * i + 2] * E[6 + j]) +
                                    ((M[3 * i] * D[j] + M[3 * i + 1] * D[3 + j]) + M[3 * i + 2] * D[6 + j])) - dtr * E[3 * i + j]) - tr * D[3 * i + j];
    }
    double s = 0.0;
    PS_UNROLL
    for (int i = 0; i < 3; ++i) {                     // sum of cofactor(E)[i][j] D[i][j]
        const int a = (i + 1) % 3, q = (i + 2) % 3;
        s = s + (E[3 * a + 1] * E[3 * q + 2] - E[3 * a + 2] * E[3 * q + 1]) * D[3 * i + 0];
        s = s + (E[3 * a + 2] * E[3 * q + 0] - E[3 * a + 0] * E[3 * q + 2]) * D[3 * i + 1];
        s = s + (E[3 * a + 0] * E[3 * q + 1] - E[3 * a + 1] * E[3 * q + 0]) * D[3 * i + 2];
    }
    dc[9] = s;
}

// (x, y) of a root z from the null vector of B(z) (the cross product of two rows with the largest third component); then
// PS_POLISH guarded Gauss-Newton / Levenberg steps on the ten cubic constraints themselves, in the coefficients of the null-space basis with the
// largest one held fixed (the expanded degree-10 polynomial loses digits when |z| is large; the constraints at a numeric E do not);
// E = aX + bY + cZ + dW scaled to Frobenius norm 1 at PS_OFF_E + 9 r.  Returns 0 for a root that gives no finite E.
PS_HD int ps_root_to_E(const PsWs& w, double z, int r) {
    double B[3][3];
    PS_UNROLL
    for (int i = 0; i < 3; ++i) {
        const int o = PS_OFF_B + 13 * i;
        B[i][0] = ((w(o + 3) * z + w(o + 2)) * z + w(o + 1)) * z + w(o + 0);
        B[i][1] = ((w(o + 7) * z + w(o + 6)) * z + w(o + 5)) * z + w(o + 4);
        B[i][2] = (((w(o + 12) * z + w(o + 11)) * z + w(o + 10)) * z + w(o + 9)) * z + w(o + 8);
    }
    double nx = 0.0, ny = 0.0, nw = 0.0;
    PS_UNROLL
    for (int i = 0; i < 3; ++i) {
        const int a = (i + 1) % 3, b = (i + 2) % 3;
        const double cx = B[a][1] * B[b][2] - B[a][2] * B[b][1];
        const double cy = B[a][2] * B[b][0] - B[a][0] * B[b][2];
        const double cw = B[a][0] * B[b][1] - B[a][1] * B[b][0];
        if (fabs(cw) > fabs(nw)) { nx = cx; ny = cy; nw = cw; }
    }
    if (!(fabs(nw) > 0.0)) return 0;
    double a[4] = {nx / nw, ny / nw, z, 1.0};
    double big = 1.0;
    int m = 3;                                        // the coefficient held fixed: the largest (first of equals)
    PS_UNROLL
    for (int k = 2; k >= 0; --k)
        if (fabs(a[k]) >= big) { big = fabs(a[k]); m = k; }
    if (!(big < (double)INFINITY)) return 0;
    PS_UNROLL
    for (int k = 0; k < 4; ++k) a[k] = a[k] / big;
    double X[4][9];
    PS_UNROLL
    for (int k = 0; k < 4; ++k) {
        PS_UNROLL
        for (int q = 0; q < 9; ++q) X[k][q] = w(PS_OFF_BASIS + 9 * k + q);
    }
    double E[9], c[10], f = 0.0;
    PS_UNROLL
    for (int q = 0; q < 9; ++q) E[q] = ((a[0] * X[0][q] + a[1] * X[1][q]) + a[2] * X[2][q]) + a[3] * X[3][q];
    ps_cubic(E, c);
    PS_UNROLL
    for (int q = 0; q < 10; ++q) f = f + c[q] * c[q];
    double lambda = 0.0;                              // Gauss-Newton; damped (Levenberg) only after a step that gained nothing
    for (int it = 0; it < PS_POLISH; ++it) {
        if (!(f > 1e-28)) break;                      // residuals at rounding level: nothing left to gain
        double N[4][4], g[4];
        PS_UNROLL
        for (int k = 0; k < 4; ++k) {
            g[k] = 0.0;
            PS_UNROLL
            for (int l = 0; l < 4; ++l) N[k][l] = 0.0;
        }
        {
            double J[4][10];
            PS_UNROLL
            for (int k = 0; k < 4; ++k) ps_cubic_d(E, X[k], J[k]);
            PS_UNROLL
            for (int k = 0; k < 4; ++k) {
                PS_UNROLL
                for (int l = k; l < 4; ++l) {
                    double s = 0.0;
                    PS_UNROLL
                    for (int q = 0; q < 10; ++q) s = s + J[k][q] * J[l][q];
                    N[k][l] = s; N[l][k] = s;
                }
                double s = 0.0;
                PS_UNROLL
                for (int q = 0; q < 10; ++q) s = s + J[k][q] * c[q];
                g[k] = -s;
            }
        }
        PS_UNROLL
        for (int k = 0; k < 4; ++k) {                 // the fixed coefficient: row and column m of the identity, no step
            PS_UNROLL
            for (int l = 0; l < 4; ++l)
                if (k == m || l == m) N[k][l] = k == l ? 1.0 : 0.0;
            if (k == m) g[k] = 0.0;
            N[k][k] = N[k][k] + lambda * N[k][k];
        }
        int ok = 1;                                   // symmetric positive definite: elimination without pivoting
        PS_UNROLL
        for (int k = 0; k < 4; ++k) {
            if (!(N[k][k] > 0.0)) ok = 0;
            const double inv = 1.0 / N[k][k];
            PS_UNROLL
            for (int l = k + 1; l < 4; ++l) {
                const double fac = N[l][k] * inv;
                PS_UNROLL
                for (int q = k; q < 4; ++q) N[l][q] = N[l][q] - fac * N[k][q];
                g[l] = g[l] - fac * g[k];
            }
        }
        double d[4];
        PS_UNROLL
        for (int k = 3; k >= 0; --k) {
            double s = g[k];
            PS_UNROLL
            for (int l = k + 1; l < 4; ++l) s = s - N[k][l] * d[l];
            d[k] = s / N[k][k];
        }
        if (!ok) break;
        double an[4], En[9], cn[10], fn = 0.0;
        PS_UNROLL
        for (int k = 0; k < 4; ++k) an[k] = a[k] + d[k];
        PS_UNROLL
        for (int q = 0; q < 9; ++q) En[q] = ((an[0] * X[0][q] + an[1] * X[1][q]) + an[2] * X[2][q]) + an[3] * X[3][q];
        ps_cubic(En, cn);
        PS_UNROLL
        for (int q = 0; q < 10; ++q) fn = fn + cn[q] * cn[q];
        if (!(fn < f)) {                              // no gain (or a NaN): keep what there is, damp the next step
            lambda = lambda > 0.0 ? lambda * 10.0 : 1e-4;
            continue;
        }
        lambda = lambda * 0.1;
        f = fn;
        PS_UNROLL
        for (int k = 0; k < 4; ++k) a[k] = an[k];
        PS_UNROLL
        for (int q = 0; q < 9; ++q) E[q] = En[q];
        PS_UNROLL
        for (int q = 0; q < 10; ++q) c[q] = cn[q];
    }
    double n2 = 0.0;
    PS_UNROLL
    for (int q = 0; q < 9; ++q) n2 = n2 + E[q] * E[q];
    const double n = sqrt(n2);
    if (!(n > 0.0) || !(n < (double)INFINITY)) return 0;
    PS_UNROLL
    for (int q = 0; q < 9; ++q) w(PS_OFF_E + 9 * r + q) = E[q] / n;
    return 1;
}

// x0, x1: five matches in normalised coordinates.  Returns the number of solutions (0 .. 10) left at PS_OFF_E.
PS_HD int ps_five_point(const double (&x0)[5][2], const double (&x1)[5][2], const PsWs& w) {
    if (!ps_nullspace(x0, x1, w)) return 0;
    ps_constraints(w);
    if (!ps_eliminate(w)) return 0;
    ps_bz(w);
    ps_detpoly(w);
    const int nz = ps_real_roots(w);
    int n = 0;
    for (int j = 0; j < nz; ++j) n += ps_root_to_E(w, w(PS_OFF_R0 + j), n);
    return n;
}

// ---- scoring
PS_HD void ps_normalise(const float* K, float px, float py, double& x, double& y) {     // metrics.py:76-77
    x = ((double)px - (double)K[2]) / (double)K[0];
    y = ((double)py - (double)K[5]) / (double)K[4];
}
PS_HD double ps_threshold(const float* K0, const float* K1, double pixel_thr) {           // metrics.py:80, as written
    const double f0 = (double)K0[0], f1 = (double)K1[4];
    return pixel_thr / ((((f0 + f1) + f0) + f1) / 4.0);
}
PS_HD int ps_inlier(const double (&E)[9], double x0, double y0, double x1, double y1, double thr2) {
    return gs_sampson(E, x0, y0, x1, y1) < thr2;                   // a NaN is never an inlier
}

// ---- pose from E
PS_HD int ps_decompose(const double (&E)[9], double (&R1)[9], double (&R2)[9], double (&t)[3]) {
    double M[9], tr = 0.0;
    PS_UNROLL
    for (int i = 0; i < 3; ++i) {
        PS_UNROLL
        for (int j = 0; j < 3; ++j) M[3 * i + j] = (E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1]) + E[3 * i + 2] * E[3 * j + 2];
    }
    tr = (M[0] + M[4]) + M[8];
    double bb[9];
    PS_UNROLL
    for (int k = 0; k < 9; ++k) bb[k] = -M[k];
    bb[0] = bb[0] + 0.5 * tr; bb[4] = bb[4] + 0.5 * tr; bb[8] = bb[8] + 0.5 * tr;
    int c = 0;
    if (bb[4] > bb[0]) c = 1;
    if (bb[8] > (c == 1 ? bb[4] : bb[0])) c = 2;
    const double d = c == 0 ? bb[0] : c == 1 ? bb[4] : bb[8];
    if (!(d > 0.0) || !(d < (double)INFINITY)) return 0;
    const double s = sqrt(d);
    double b[3];
    PS_UNROLL
    for (int i = 0; i < 3; ++i) b[i] = (c == 0 ? bb[3 * i] : c == 1 ? bb[3 * i + 1] : bb[3 * i + 2]) / s;
    const double nb2 = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    if (!(nb2 > 0.0)) return 0;
    double cof[9], be[9];
    PS_UNROLL
    for (int i = 0; i < 3; ++i) {                     // cofactor rows: e1 x e2, e2 x e0, e0 x e1
        const int a = (i + 1) % 3, q = (i + 2) % 3;
        cof[3 * i + 0] = E[3 * a + 1] * E[3 * q + 2] - E[3 * a + 2] * E[3 * q + 1];
        cof[3 * i + 1] = E[3 * a + 2] * E[3 * q + 0] - E[3 * a + 0] * E[3 * q + 2];
        cof[3 * i + 2] = E[3 * a + 0] * E[3 * q + 1] - E[3 * a + 1] * E[3 * q + 0];
    }
    PS_UNROLL
    for (int j = 0; j < 3; ++j) {                     // [b]x E, column by column
        be[0 + j] = b[1] * E[6 + j] - b[2] * E[3 + j];
        be[3 + j] = b[2] * E[0 + j] - b[0] * E[6 + j];
        be[6 + j] = b[0] * E[3 + j] - b[1] * E[0 + j];
    }
    PS_UNROLL
    for (int k = 0; k < 9; ++k) {
        R1[k] = (cof[k] - be[k]) / nb2;
        R2[k] = (cof[k] + be[k]) / nb2;
    }
    const double nb = sqrt(nb2);
    PS_UNROLL
    for (int i = 0; i < 3; ++i) t[i] = b[i] / nb;
    return 1;
}

// does the match triangulate in front of both cameras P0 = [I | 0], P1 = [R | t], closer than PS_DEPTH_MAX?
PS_HD int ps_cheiral(const double (&R)[9], const double (&t)[3], double x0, double y0, double x1, double y1) {
    const double r0 = (R[0] * x0 + R[1] * y0) + R[2], r1 = (R[3] * x0 + R[4] * y0) + R[5], r2 = (R[6] * x0 + R[7] * y0) + R[8];
    const double u0 = y1 * r2 - r1, u1 = r0 - x1 * r2, u2 = x1 * r1 - y1 * r0;             // x1 x (R x0)
    const double v0 = y1 * t[2] - t[1], v1 = t[0] - x1 * t[2], v2 = x1 * t[1] - y1 * t[0]; // x1 x t
    const double d0 = -((u0 * v0 + u1 * v1) + u2 * v2) / ((u0 * u0 + u1 * u1) + u2 * u2);  // depth along x0
    const double d1 = d0 * r2 + t[2];                                                          // depth in camera 1
    return d0 > 0.0 && d1 > 0.0 && d0 < PS_DEPTH_MAX && d1 < PS_DEPTH_MAX;
}
// candidate c of the fixed order (R1, t), (R2, t), (R1, -t), (R2, -t)
PS_HD void ps_candidate(int c, const double (&R1)[9], const double (&R2)[9], const double (&t)[3], double (&R)[9], double (&tc)[3]) {
    PS_UNROLL
    for (int k = 0; k < 9; ++k) R[k] = (c & 1) ? R2[k] : R1[k];
    PS_UNROLL
    for (int k = 0; k < 3; ++k) tc[k] = (c & 2) ? -t[k] : t[k];
}
