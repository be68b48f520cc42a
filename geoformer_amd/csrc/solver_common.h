// What the minimal solvers share (pose_solver.h: five points, essential matrix; fund_solver.h: seven points, fundamental matrix;
// abs_solver.h: three points, absolute pose), stated
// once for the device and the host.  Plain C++ in fp64 with contraction off, only + - * / sqrt, fabs and comparisons, so a host build and
// gfx950 agree bit for bit.  Everything indexed at run time is reached through GsWs (element i at p[i * stride]): the caller decides where
// it lives - a local array on the host, an LDS tile interleaved across the lanes of a workgroup on the device.
//
//   gs_eliminate9<R>   Gauss-Jordan with full pivoting on the R x 9 epipolar system at the start of the workspace, columns swapped in
//                      place (perm: nibble j = the original column now at position j).
//   gs_solve<N>        the same elimination on an N x N system with a right-hand side (abs_solver.h: the 6 x 6 normal equations of a
//                      Gauss-Newton step).
//   gs_null_basis<R>   the 9 - R null vectors of the eliminated system: vector k has 1 at free column R + k, -A[i][R + k] at pivot column i.
//   gs_real_roots<D>   real roots of a polynomial of degree D without an eigen-solver: the roots of the k-th derivative separate those of
//                      the (k-1)-th, so the chain p^(D-1) (linear) .. p^(0) is walked upwards, every sign change between neighbouring
//                      critical points bisected a FIXED number of times, then guarded Newton steps on p itself.
//   gs_draw_distinct<K> K distinct rows of hypothesis t of pair `sample` among cnt, from the counter-based hash of gf_hash.h: a duplicate is
//                      drawn again through the attempt counter, GS_DRAW_ATTEMPTS times at most.
//   gs_sampson         the squared Sampson distance of a match under a 3x3 matrix: (x1^T S x0)^2 / (Sx0[0]^2 + Sx0[1]^2 + S^Tx1[0]^2 +
//                      S^Tx1[1]^2), OpenCV's residual for E and F alike.
//   gs_jacobi_sym<N>   all eigenvectors of a symmetric N x N matrix by cyclic Jacobi: a FIXED number of sweeps, rotations in lexicographic
//                      (p, q) order, a rotation whose off-diagonal entry is exactly 0 skipped, t = sign(theta) / (|theta| + sqrt(theta^2 + 1)).
//                      No convergence test: nothing that could differ between two builds decides how much work is done.
//   gs_min_diag<N>     the index of the smallest diagonal entry (the smallest eigenvalue after gs_jacobi_sym); ties go to the lower index.
//   gs_offsets_range   problem n's slice of a list of M rows addressed by an offsets array [N + 1], clamped into the list.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gf_hash.h"

#if defined(__HIPCC__)
#define GS_HD __host__ __device__ inline
#define GS_HD_MEMBER __host__ __device__
#else
#define GS_HD static inline
#define GS_HD_MEMBER
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#define GS_UNROLL _Pragma("unroll")
#else
#define GS_UNROLL
#endif

#define GS_DRAW_ATTEMPTS 16

struct GsWs {
    double* p;
    int s;
    GS_HD_MEMBER double& operator()(int i) const { return p[(long)i * s]; }
};

// offsets come from device memory, so nothing read from them is trusted: off = clamp(offsets[n], 0, M) and the slice ends at
// clamp(max(offsets[n + 1], off), 0, M) - a descending pair is an empty slice, and nothing indexed with (off, len) leaves [0, M)
GS_HD void gs_offsets_range(const int32_t* offsets, int n, int M, int& off, int& len) {
    int o = offsets[n], e = offsets[n + 1];
    o = o < 0 ? 0 : o; o = o > M ? M : o;
    e = e < o ? o : e; e = e > M ? M : e;
    off = o;
    len = e - o;
}

GS_HD double gs_abs_or_inf(double v) {            // |v|, a NaN counted as +inf: it wins every pivot search and fails the solve
    const double a = fabs(v);
    return a == a ? a : (double)INFINITY;
}

// rows 0 .. R - 1 of 9 doubles each at w(9 r + j).  Returns 0 for a rank-deficient or non-finite system.
template <int R>
GS_HD int gs_eliminate9(const GsWs& w, unsigned long long& perm) {
    perm = 0x876543210ull;
    for (int c = 0; c < R; ++c) {
        int pr = c, pc = c;
        double best = -1.0;
        for (int r = c; r < R; ++r)
            for (int j = c; j < 9; ++j) {
                const double v = gs_abs_or_inf(w(9 * r + j));
                if (v > best) { best = v; pr = r; pc = j; }
            }
        if (!(best > 1e-12) || best == (double)INFINITY) return 0;
        if (pr != c)
            for (int j = 0; j < 9; ++j) { const double tmp = w(9 * c + j); w(9 * c + j) = w(9 * pr + j); w(9 * pr + j) = tmp; }
        if (pc != c) {
            for (int r = 0; r < R; ++r) { const double tmp = w(9 * r + c); w(9 * r + c) = w(9 * r + pc); w(9 * r + pc) = tmp; }
            const unsigned long long nc = (perm >> (4 * c)) & 15ull, np = (perm >> (4 * pc)) & 15ull;
            perm = (perm & ~(15ull << (4 * c)) & ~(15ull << (4 * pc))) | (np << (4 * c)) | (nc << (4 * pc));
        }
        const double inv = 1.0 / w(9 * c + c);
        for (int j = c; j < 9; ++j) w(9 * c + j) = w(9 * c + j) * inv;
        for (int r = 0; r < R; ++r) {
            if (r == c) continue;
            const double f = w(9 * r + c);
            if (f != 0.0)
                for (int j = c; j < 9; ++j) w(9 * r + j) = w(9 * r + j) - f * w(9 * c + j);
        }
    }
    return 1;
}

// the N x N system A x = b, augmented: row r is N + 1 doubles at w(off + (N + 1) r + j), b in column N.  Gauss-Jordan with full pivoting as
// gs_eliminate9 (the same pivot threshold, a NaN wins the pivot search and fails the solve); x goes to w(off_x + i) in the ORIGINAL order of
// the unknowns.  N <= 15.  Returns 0 for a rank-deficient or non-finite system (x is then unspecified).
template <int N>
GS_HD int gs_solve(const GsWs& w, int off, int off_x) {
    constexpr int C = N + 1;
    unsigned long long perm = 0xFEDCBA9876543210ull;
    for (int c = 0; c < N; ++c) {
        int pr = c, pc = c;
        double best = -1.0;
        for (int r = c; r < N; ++r)
            for (int j = c; j < N; ++j) {
                const double v = gs_abs_or_inf(w(off + C * r + j));
                if (v > best) { best = v; pr = r; pc = j; }
            }
        if (!(best > 1e-12) || best == (double)INFINITY) return 0;
        if (pr != c)
            for (int j = 0; j < C; ++j) { const double tmp = w(off + C * c + j); w(off + C * c + j) = w(off + C * pr + j); w(off + C * pr + j) = tmp; }
        if (pc != c) {
            for (int r = 0; r < N; ++r) { const double tmp = w(off + C * r + c); w(off + C * r + c) = w(off + C * r + pc); w(off + C * r + pc) = tmp; }
            const unsigned long long nc = (perm >> (4 * c)) & 15ull, np = (perm >> (4 * pc)) & 15ull;
            perm = (perm & ~(15ull << (4 * c)) & ~(15ull << (4 * pc))) | (np << (4 * c)) | (nc << (4 * pc));
        }
        const double inv = 1.0 / w(off + C * c + c);
        for (int j = c; j < C; ++j) w(off + C * c + j) = w(off + C * c + j) * inv;
        for (int r = 0; r < N; ++r) {
            if (r == c) continue;
            const double f = w(off + C * r + c);
            if (f != 0.0)
                for (int j = c; j < C; ++j) w(off + C * r + j) = w(off + C * r + j) - f * w(off + C * c + j);
        }
    }
    for (int i = 0; i < N; ++i) w(off_x + (int)((perm >> (4 * i)) & 15ull)) = w(off + C * i + N);
    return 1;
}

template <int R>
GS_HD void gs_null_basis(const GsWs& w, unsigned long long perm, int off_basis) {
    for (int k = 0; k < 9 - R; ++k) {
        for (int j = 0; j < 9; ++j) w(off_basis + 9 * k + j) = 0.0;
        w(off_basis + 9 * k + (int)((perm >> (4 * (R + k))) & 15ull)) = 1.0;
        for (int i = 0; i < R; ++i) w(off_basis + 9 * k + (int)((perm >> (4 * i)) & 15ull)) = -w(9 * i + R + k);
    }
}

template <int D>
GS_HD double gs_horner(const double (&q)[D + 1], double x) {
    double s = q[D];
    GS_UNROLL
    for (int k = D - 1; k >= 0; --k) s = s * x + q[k];
    return s;
}

// real roots of the polynomial at off_p (D + 1 coefficients, ascending), ascending, into off_r0 (off_r0, off_r1: D + 2 doubles each);
// returns their number (0 when the polynomial is not of degree D in finite numbers)
template <int D>
GS_HD int gs_real_roots(const GsWs& w, int off_p, int off_r0, int off_r1, int bisect_low, int bisect_top, int newton) {
    const double lead = w(off_p + D);
    double big = 0.0;
    for (int k = 0; k < D; ++k) {
        const double v = gs_abs_or_inf(w(off_p + k));
        big = v > big ? v : big;
    }
    if (!(fabs(lead) > 0.0)) return 0;
    const double bound = 1.0 + big / fabs(lead);                   // Cauchy
    if (!(bound < (double)INFINITY)) return 0;
    int nprev = 0;
    for (int m = 1; m <= D; ++m) {
        const int s = D - m;                                       // q = the s-th derivative of p, degree m
        double q[D + 1];
        GS_UNROLL
        for (int i = 0; i <= D; ++i) {
            double c = 0.0;
            if (i <= m) {
                c = w(off_p + i + s);
                for (int t = 1; t <= s; ++t) c = c * (double)(i + t);
            }
            q[i] = c;
        }
        const int iters = m == D ? bisect_top : bisect_low;
        int nnew = 0;
        double lo = -bound, flo = gs_horner<D>(q, lo);
        for (int j = 0; j <= nprev; ++j) {
            const double hi = j < nprev ? w(off_r0 + j) : bound;
            const double fhi = gs_horner<D>(q, hi);
            if ((flo > 0.0) != (fhi > 0.0)) {
                double a = lo, b = hi;
                for (int it = 0; it < iters; ++it) {
                    const double mid = 0.5 * (a + b);
                    const double fm = gs_horner<D>(q, mid);
                    if ((fm > 0.0) == (flo > 0.0)) a = mid; else b = mid;
                }
                w(off_r1 + nnew) = 0.5 * (a + b);
                ++nnew;
            }
            lo = hi; flo = fhi;
        }
        for (int j = 0; j < nnew; ++j) w(off_r0 + j) = w(off_r1 + j);
        nprev = nnew;
        if (m == D) {
            double dq[D + 1];
            GS_UNROLL
            for (int i = 0; i < D; ++i) dq[i] = q[i + 1] * (double)(i + 1);
            dq[D] = 0.0;
            for (int j = 0; j < nnew; ++j) {
                double z = w(off_r0 + j), f = gs_horner<D>(q, z);
                for (int it = 0; it < newton; ++it) {
                    const double zn = z - f / gs_horner<D>(dq, z);
                    const double fn = gs_horner<D>(q, zn);
                    if (fabs(fn) < fabs(f)) { z = zn; f = fn; }     // a NaN or a worse step is not taken
                }
                w(off_r0 + j) = z;
            }
        }
    }
    return nprev;
}

// returns 0 (and idx[k] = 0 from the first failure on) when some row stayed a duplicate after GS_DRAW_ATTEMPTS draws
template <int K>
GS_HD int gs_draw_distinct(uint32_t seed, uint32_t sample, uint32_t t, int cnt, int (&idx)[K]) {
    int ok = 1;
    GS_UNROLL
    for (int k = 0; k < K; ++k) {
        int found = 0;
        for (uint32_t attempt = 0; attempt < GS_DRAW_ATTEMPTS && !found && ok; ++attempt) {
            const int c = (int)(draw(seed, sample, t, (uint32_t)k, attempt) % (uint32_t)cnt);
            int dup = 0;
            GS_UNROLL
            for (int j = 0; j < K; ++j) dup |= (j < k && idx[j] == c);
            if (!dup) { idx[k] = c; found = 1; }
        }
        if (!found) { ok = 0; idx[k] = 0; }
    }
    return ok;
}

GS_HD double gs_sampson(const double (&S)[9], double x0, double y0, double x1, double y1) {
    const double a0 = (S[0] * x0 + S[1] * y0) + S[2], a1 = (S[3] * x0 + S[4] * y0) + S[5], a2 = (S[6] * x0 + S[7] * y0) + S[8];
    const double b0 = (S[0] * x1 + S[3] * y1) + S[6], b1 = (S[1] * x1 + S[4] * y1) + S[7];
    const double num = (x1 * a0 + y1 * a1) + a2;
    return (num * num) / (((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1);
}

// A [N][N] symmetric at w(off_a + N i + j), BOTH triangles filled and both kept up to date; V [N][N] at w(off_v + N i + j) is set to the
// identity and leaves with the eigenvectors in its COLUMNS, the eigenvalues on A's diagonal.  Every element of a rotation is independent
// arithmetic given (c, s, t), so the elements may be spread over lanes without changing a bit.
template <int N>
GS_HD void gs_jacobi_sym(const GsWs& w, int off_a, int off_v, int sweeps) {
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) w(off_v + N * i + j) = i == j ? 1.0 : 0.0;
    for (int sw = 0; sw < sweeps; ++sw)
        for (int p = 0; p < N - 1; ++p)
            for (int q = p + 1; q < N; ++q) {
                const double apq = w(off_a + N * p + q);
                if (apq == 0.0) continue;
                const double app = w(off_a + N * p + p), aqq = w(off_a + N * q + q);
                const double theta = (aqq - app) / (2.0 * apq);
                const double mag = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double t = theta < 0.0 ? -mag : mag;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                w(off_a + N * p + p) = app - t * apq;
                w(off_a + N * q + q) = aqq + t * apq;
                w(off_a + N * p + q) = 0.0;
                w(off_a + N * q + p) = 0.0;
                for (int k = 0; k < N; ++k) {
                    if (k != p && k != q) {
                        const double akp = w(off_a + N * k + p), akq = w(off_a + N * k + q);
                        const double np = c * akp - s * akq, nq = s * akp + c * akq;
                        w(off_a + N * k + p) = np; w(off_a + N * p + k) = np;
                        w(off_a + N * k + q) = nq; w(off_a + N * q + k) = nq;
                    }
                    const double vkp = w(off_v + N * k + p), vkq = w(off_v + N * k + q);
                    w(off_v + N * k + p) = c * vkp - s * vkq;
                    w(off_v + N * k + q) = s * vkp + c * vkq;
                }
            }
}

template <int N>
GS_HD int gs_min_diag(const GsWs& w, int off_a) {
    int best = 0;
    double lo = w(off_a);
    for (int i = 1; i < N; ++i) {
        const double d = w(off_a + N * i + i);
        if (d < lo) { lo = d; best = i; }
    }
    return best;
}
