// Bundle adjustment, the second solver of the reduced camera system: matrix-free preconditioned conjugate gradients (PCG) with the
// per-camera blocks as the preconditioner.  Rules 1 - 5 and 8 - 11 are ba_spec.h's, unchanged and shared; rules 6 and 7 (build S, Cholesky)
// get the form below.  Stated once for the device (k_bundle.hip) and the host (host/ba_host.cpp) in the same style: fp64 with contraction
// off, only + - * / sqrt, fabs and comparisons, every sum in a stated order, no floating-point atomics.  S is never stored: one product
// S p costs O(n_obs), and nothing grows with F^2.
//
//  R256  the fixed-order sum of many terms numbered by a POSITION 0, 1, ..: BA_BLOCK (256) partial sums, partial j takes the positions that are
//        j modulo 256, ascending, from +0.0; then ba_block_tree over the 256 partials.
//  6'    camera blocks.  Per free camera f (image i), over the image's observations in img_obs order, the position of entry q being
//        q - img_off[i].  An observation k that takes part adds (ba_pcg_obs_terms) U += Jc^T Jc (the 21 entries r >= c, mirrored) and
//        b += Jc^T (-r); one whose point is also not held adds D += Tm_k W_k^T (the 21 entries r >= c, each (Tm[r][0] W[c][0] +
//        Tm[r][1] W[c][1]) + Tm[r][2] W[c][2], mirrored) and c += Tm_k g_p (the same bracketing).  Each of the 54 sums is R256.  Then
//        (ba_pcg_blocks) Ul = U with its diagonal + lambda * itself - a camera with no observation taking part gets the identity and moves
//        nowhere -, rhs = b - c, M = Ul - D, and (ba_pcg_inverse_column) M^-1 column by column: gs_solve<6> on (M | e_k).  A failed pivot
//        test or an entry of M^-1 that is not finite fails the step (BA_FLAG_STEP_FAILED).
//  7'    q = S p for a vector of 6 F doubles.  Per point not held (ba_pcg_point_z): z_p[m] = z_p[m] + W_l[r][m] p[6 j(l) + r] over its
//        observations l that take part and have a free camera, in order, r = 0 .. 5 inside, from +0.0; a held point has z_p = 0.  Per free
//        camera: s[r] = the R256 sum over the image's observations k that take part with the point not held of (Tm_k[r][0] z[0] +
//        Tm_k[r][1] z[1]) + Tm_k[r][2] z[2] with z = z_p(k) (ba_pcg_obs_tz); q[r] = (row r of Ul times p_f, summed left to right) - s[r].
//  7''   <a, b>: per camera the six products summed left to right (ba_pcg_dot6); the cameras of a block of 256 by ba_block_tree on the
//        zero-padded block; the blocks serially, ascending (rule 3's shape).
//  7'''  PCG (the scalar decisions: ba_pcg_begin, ba_pcg_alpha, ba_pcg_beta).  x = 0, r = rhs, z = M^-1 r (per camera, rows summed left to
//        right), p = z, rho0 = rho = <r, z>.  rho0 not finite or < 0 fails the step; rho0 == 0: done.  For i = 0 .. cg_iters - 1: q = S p;
//        kappa = <p, q>; not kappa > 0 fails the step; alpha = rho / kappa; x = x + alpha p; r = r - alpha q; z = M^-1 r; rho' = <r, z>;
//        used = i + 1; stop iff rho' <= tol^2 rho0; else beta = rho' / rho, p = z + beta p, rho = rho'.  Running out of iterations is no
//        failure: delta_c = x goes to rule 8 and rule 9's cost test judges it.  The log per LM iteration: cg_used = the CG iterations
//        completed, cg_res = the last rho' / rho0 - 1.0 before the first iteration completes, 0.0 when rho0 == 0 or F == 0; a failed step logs
//        what it had reached.
//  limits  1 <= cg_iters <= BA_PCG_MAX_ITERS (256), 0 <= cg_tol < 1 and finite, F <= BA_PCG_MAX_FREE (65536), and rule 11's other limits.
//
// NOT part of this: a preconditioner other than the camera blocks (block Jacobi), an adaptive tolerance (Eisenstat-Walker).
#pragma once
#include "ba_spec.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define BA_PCG_MAX_FREE 65536
#define BA_PCG_MAX_ITERS 256
#define BA_PCG_DEFAULT_ITERS 64
#define BA_PCG_DEFAULT_TOL 1e-6

// the 54 sums of rule 6' in one array: U (21, entry (r, c), c <= r, at r (r + 1) / 2 + c), b (6), D (21, as U), c (6)
#define BA_PCG_OFF_U 0
#define BA_PCG_OFF_B 21
#define BA_PCG_OFF_D 27
#define BA_PCG_OFF_C 48
#define BA_PCG_SUMS 54

// workspace of ba_pcg_inverse_column (doubles, through GsWs)
#define BA_PCG_OFF_A 0            /* [6][7] */
#define BA_PCG_OFF_X 42           /* [6] */
#define BA_PCG_WS_DOUBLES 48

// rule 6', one observation: k (of point p = obs_point[k]) adds its terms to acc; returns whether it takes part.  The indices are
// compile-time ones: acc may live in registers.
BA_HD_FLAT int ba_pcg_obs_terms(const BaView& v, const BaState& s, const BaIter& it, int k, double (&acc)[BA_PCG_SUMS]) {
    if (k < 0 || k >= v.n_obs || !it.part[k]) return 0;
    const int p = v.obs_point[k];
    if (p < 0 || p >= v.T) return 0;
    double res[2], Pu[3], Pv[3], Cu[6], Cv[6];
    if (!ba_obs_jacobian(v, s, k, p, res, Pu, Pv, Cu, Cv)) return 0;
    GS_UNROLL
    for (int r = 0; r < 6; ++r) {
        GS_UNROLL
        for (int c = 0; c <= r; ++c) acc[BA_PCG_OFF_U + r * (r + 1) / 2 + c] = acc[BA_PCG_OFF_U + r * (r + 1) / 2 + c] + (Cu[r] * Cu[c] + Cv[r] * Cv[c]);
        acc[BA_PCG_OFF_B + r] = acc[BA_PCG_OFF_B + r] + (Cu[r] * (-res[0]) + Cv[r] * (-res[1]));
    }
    if (it.hold[p]) return 1;
    const double* Tk = it.Tm + 18 * (size_t)k;
    const double* Wk = it.W + 18 * (size_t)k;
    const double* g = it.g + 3 * (size_t)p;
    GS_UNROLL
    for (int r = 0; r < 6; ++r) {
        GS_UNROLL
        for (int c = 0; c <= r; ++c)
            acc[BA_PCG_OFF_D + r * (r + 1) / 2 + c] =
                acc[BA_PCG_OFF_D + r * (r + 1) / 2 + c] + ((Tk[3 * r] * Wk[3 * c] + Tk[3 * r + 1] * Wk[3 * c + 1]) + Tk[3 * r + 2] * Wk[3 * c + 2]);
        acc[BA_PCG_OFF_C + r] = acc[BA_PCG_OFF_C + r] + ((Tk[3 * r] * g[0] + Tk[3 * r + 1] * g[1]) + Tk[3 * r + 2] * g[2]);
    }
    return 1;
}

// rule 6', after the sums: tot [54] -> Ul [36], M [36] (row-major), rhs [6].  any_part: an observation of the camera takes part.
GS_HD void ba_pcg_blocks(const double* tot, int any_part, double lambda, double* Ul, double* M, double* rhs) {
    for (int r = 0; r < 6; ++r) {
        for (int c = 0; c < 6; ++c) {
            const int e = r >= c ? r * (r + 1) / 2 + c : c * (c + 1) / 2 + r;
            double u = tot[BA_PCG_OFF_U + e];
            if (r == c) u = any_part ? u + lambda * u : 1.0;
            Ul[6 * r + c] = u;
            M[6 * r + c] = u - tot[BA_PCG_OFF_D + e];
        }
        rhs[r] = tot[BA_PCG_OFF_B + r] - tot[BA_PCG_OFF_C + r];
    }
}

// rule 6': column k of M^-1 into Minv [36] (row-major); 0 when the pivot test fails or an entry is not finite
GS_HD int ba_pcg_inverse_column(const double* M, int k, const GsWs& w, double* Minv) {
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < 6; ++j) w(BA_PCG_OFF_A + 7 * i + j) = M[6 * i + j];
        w(BA_PCG_OFF_A + 7 * i + 6) = i == k ? 1.0 : 0.0;
    }
    int ok = gs_solve<6>(w, BA_PCG_OFF_A, BA_PCG_OFF_X);
    for (int i = 0; i < 6; ++i) {
        const double x = ok ? w(BA_PCG_OFF_X + i) : 0.0;
        ok &= tr_finite(x);
        Minv[6 * i + k] = x;
    }
    return ok;
}

// out = A v for a row-major 6 x 6 block, every row summed left to right
GS_HD void ba_pcg_apply6(const double* A, const double* x, double* out) {
    for (int r = 0; r < 6; ++r) {
        double s = A[6 * r] * x[0];
        for (int c = 1; c < 6; ++c) s = s + A[6 * r + c] * x[c];
        out[r] = s;
    }
}

// rule 7'': one camera's share of an inner product
GS_HD double ba_pcg_dot6(const double* a, const double* b) {
    double s = a[0] * b[0];
    for (int r = 1; r < 6; ++r) s = s + a[r] * b[r];
    return s;
}

// rule 7' for point p: z_p = sum W_l^T pv_j(l) into zp [T][3]
GS_HD void ba_pcg_point_z(const BaView& v, const BaIter& it, int p, const double* pv, double* zp) {
    double z[3] = {0.0, 0.0, 0.0};
    if (!it.hold[p]) {
        int b, e;
        ba_point_range(v, p, b, e);
        for (int o = b; o < e; ++o) {
            if (!it.part[o]) continue;
            const int img = v.obs_image[o];
            if (img < 0 || img >= v.n_images) continue;
            const int j = v.cam_free[img];
            if (j < 0 || j >= v.F) continue;
            const double* W = it.W + 18 * (size_t)o;
            for (int r = 0; r < 6; ++r) {
                GS_UNROLL
                for (int m = 0; m < 3; ++m) z[m] = z[m] + W[3 * r + m] * pv[6 * (size_t)j + r];
            }
        }
    }
    GS_UNROLL
    for (int m = 0; m < 3; ++m) zp[3 * (size_t)p + m] = z[m];
}

// rule 7', one observation of a camera's sum: acc += Tm_k z_p(k); nothing for one that takes no part or whose point is held
BA_HD_FLAT void ba_pcg_obs_tz(const BaView& v, const BaIter& it, int k, const double* zp, double (&acc)[6]) {
    if (k < 0 || k >= v.n_obs || !it.part[k]) return;
    const int p = v.obs_point[k];
    if (p < 0 || p >= v.T || it.hold[p]) return;
    const double* Tk = it.Tm + 18 * (size_t)k;
    const double z0 = zp[3 * (size_t)p], z1 = zp[3 * (size_t)p + 1], z2 = zp[3 * (size_t)p + 2];
    GS_UNROLL
    for (int r = 0; r < 6; ++r) acc[r] = acc[r] + ((Tk[3 * r] * z0 + Tk[3 * r + 1] * z1) + Tk[3 * r + 2] * z2);
}

// rule 7''': the scalars of one solve and its decisions
struct BaPcgScalars {
    double rho0, rho, alpha, beta, res;
    int32_t used, done, failed, pad;
};

// after rule 6' and rho0 = <r, z>.  setup_ok: no camera block failed
GS_HD void ba_pcg_begin(BaPcgScalars& c, int setup_ok, double rho0) {
    c.rho0 = rho0; c.rho = rho0; c.alpha = 0.0; c.beta = 0.0; c.res = 1.0;
    c.used = 0; c.done = 0; c.failed = 0;
    if (!setup_ok || !tr_finite(rho0) || rho0 < 0.0) {
        c.failed = 1; c.done = 1;
    } else if (rho0 == 0.0) {
        c.res = 0.0; c.done = 1;
    }
}

// steps 2 - 3 of iteration i: alpha, or the failure
GS_HD void ba_pcg_alpha(BaPcgScalars& c, double kappa) {
    if (!(kappa > 0.0)) {
        c.failed = 1; c.done = 1;
        return;
    }
    c.alpha = c.rho / kappa;
}

// steps 7 - 10 of iteration i: the log, the stopping test, beta
GS_HD void ba_pcg_beta(BaPcgScalars& c, double rho_new, int i, double tol2) {
    c.used = i + 1;
    c.res = rho_new / c.rho0;
    if (rho_new <= tol2 * c.rho0) {
        c.done = 1;
        return;
    }
    c.beta = rho_new / c.rho;
    c.rho = rho_new;
}

// rule 11 with the PCG limits, for both entry points: the message of the first violation, or null
static inline const char* ba_pcg_check_limits(int F, int cg_iters, double cg_tol) {
    if (F > BA_PCG_MAX_FREE) return "more than 65536 free cameras";
    if (cg_iters < 1 || cg_iters > BA_PCG_MAX_ITERS) return "cg_iters must be 1 .. 256";
    if (!(cg_tol >= 0.0 && cg_tol < 1.0)) return "cg_tol must be in [0, 1)";
    return nullptr;
}
