// TEST INFRASTRUCTURE: the serial host form of the absolute-pose RANSAC of k_abspose.hip, compiled from the same abs_solver.h by the
// host C++ compiler (geoformer_amd/build.py: -O2 -ffp-contract=off, no offload) into csrc/_obj/libabspose_host.so.  The tests compare the
// device against it bit for bit; nothing in the package loads it.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../abs_solver.h"

extern "C" {

// uv [3][2] fp64 pixels, X [3][3] fp64 world, K fp32 [9], norm [4] (centre, half the longest side) -> out [4][12]: R row-major, then t in
// WORLD units; returns the number of solutions
int gf_abs_host_p3p(const double* uv, const double* X, const float* K, const double* norm, double* out) {
    double a[3][2], b[3][3], nm[4], ws[AS_WS_DOUBLES];
    for (int i = 0; i < 3; ++i) {
        a[i][0] = uv[2 * i]; a[i][1] = uv[2 * i + 1];
        for (int k = 0; k < 3; ++k) b[i][k] = X[3 * i + k];
    }
    for (int i = 0; i < 4; ++i) nm[i] = norm[i];
    for (int i = 0; i < AS_WS_DOUBLES; ++i) ws[i] = 0.0;
    const GsWs w{ws, 1};
    const int n = as_p3p(a, b, K, nm, w);
    for (int r = 0; r < n; ++r) {
        double S[9], R[9], t[3], tw[3];
        for (int k = 0; k < 9; ++k) S[k] = ws[AS_OFF_SOL + 9 * r + k];
        as_unpack(S, R, t);
        as_to_world(R, t, nm, tw);
        for (int k = 0; k < 9; ++k) out[12 * r + k] = R[k];
        for (int k = 0; k < 3; ++k) out[12 * r + 9 + k] = tw[k];
    }
    return n;
}

// One Gauss-Newton step (step 2 of a round of abs_solver.h) from a given inlier set: uv [n][2], xyz [n][3], every row taken as a surviving
// row, mask [n], K, norm [4]; R [9] and t [3] (CONDITIONED) are updated in place.  Returns 1, or 0 when the step fails (R, t unchanged).
static int abs_gn_step(const float* uv, const float* xyz, int n, const uint8_t* mask, const float* K, const double (&nm)[4], double (&R)[9],
                       double (&t)[3]) {
    std::vector<double> part((size_t)AS_GN_SUMS * FS_REFIT_PARTIALS, 0.0);
    for (int j = 0; j < FS_REFIT_PARTIALS; ++j) {
        double acc[AS_GN_SUMS], Ju[6], Jv[6], res[2];
        for (int e = 0; e < AS_GN_SUMS; ++e) acc[e] = 0.0;
        for (int i = j; i < n; i += FS_REFIT_PARTIALS) {
            if (!mask[i]) continue;
            const AsRow r = as_row(uv + 2 * (size_t)i, xyz + 3 * (size_t)i, nm);
            if (as_gn_row(R, t, K, r, Ju, Jv, res)) as_gn_accum(acc, Ju, Jv, res);
        }
        for (int e = 0; e < AS_GN_SUMS; ++e) part[(size_t)e * FS_REFIT_PARTIALS + j] = acc[e];
    }
    double ws[AS_GN_WS_DOUBLES];
    for (int i = 0; i < AS_GN_WS_DOUBLES; ++i) ws[i] = 0.0;
    for (int e = 0; e < AS_GN_SUMS; ++e) ws[AS_GN_OFF_ACC + e] = fs_refit_tree(part.data() + (size_t)e * FS_REFIT_PARTIALS);
    const GsWs w{ws, 1};
    if (!as_gn_solve(w)) return 0;
    double d[6];
    for (int k = 0; k < 6; ++k) d[k] = ws[AS_GN_OFF_X + k];
    return as_gn_update(d, R, t);
}

// one ROUND's fit (AS_GN_STEPS steps) on a given set; R, t conditioned, in place.  Returns 1, or 0 when a step fails.
int gf_abs_host_refit_once(const float* uv, const float* xyz, int n, const uint8_t* mask, const float* K, const double* norm, double* R_io,
                           double* t_io) {
    double nm[4], R[9], t[3];
    for (int i = 0; i < 4; ++i) nm[i] = norm[i];
    for (int k = 0; k < 9; ++k) R[k] = R_io[k];
    for (int k = 0; k < 3; ++k) t[k] = t_io[k];
    for (int s = 0; s < AS_GN_STEPS; ++s)
        if (!abs_gn_step(uv, xyz, n, mask, K, nm, R, t)) return 0;
    for (int k = 0; k < 9; ++k) R_io[k] = R[k];
    for (int k = 0; k < 3; ++k) t_io[k] = t[k];
    return 1;
}

// maps: P records of (map [H][W][3], H, W) given as parallel arrays; pair_offsets [P + 1]; pts at pts + pts_stride * i (x, y) -> xyz [M][3]
void gf_abs_host_xyz_lookup(const float* const* maps, const int32_t* Hs, const int32_t* Ws, int P, const int32_t* pair_offsets,
                            const float* pts, long pts_stride, int M, float* xyz) {
    for (int i = 0; i < M; ++i) {
        float* o = xyz + 3 * (size_t)i;
        o[0] = o[1] = o[2] = __builtin_nanf("");
        for (int p = 0; p < P; ++p)
            if (pair_offsets[p] <= i && i < pair_offsets[p + 1]) {
                if (maps[p] && Hs[p] > 0 && Ws[p] > 0) as_xyz_sample(maps[p], Hs[p], Ws[p], pts[pts_stride * i], pts[pts_stride * i + 1], o);
                break;
            }
    }
}

// One problem: uv [n][2], xyz [n][3] fp32, scores [n] or NULL, K fp32 [9].  Outputs as gf_abspose_ransac writes them for problem `sample`
// of a launch: R [9], t [3] (world units), hyp [2] (hypothesis, root; -1 when not valid), n_inliers [1], mask [n], rounds [1].  Returns
// valid (0 / 1), or -1 (GF_ERR_INVALID_ARGUMENT) for arguments the device entry point rejects.
int gf_abs_host_ransac(const float* uv, const float* xyz, const float* scores, int n, const float* K, float sc_thres, double pixel_thr,
                       int iters, uint32_t seed, uint32_t sample, int refit_rounds, double* R_out, double* t_out, int32_t* hyp_out,
                       int32_t* n_inliers, uint8_t* mask, int32_t* rounds) {
    if (iters <= 0 || iters % AS_HYP_PER_WG != 0 || n < 0 || !(pixel_thr > 0.0)) return -1;
    if (refit_rounds < 0 || refit_rounds > AS_REFIT_MAX_ROUNDS) return -1;
    *rounds = 0;
    for (int k = 0; k < 9; ++k) R_out[k] = 0.0;
    for (int k = 0; k < 3; ++k) t_out[k] = 0.0;
    hyp_out[0] = hyp_out[1] = -1;
    *n_inliers = 0;
    for (int i = 0; i < n; ++i) mask[i] = 0;
    std::vector<int32_t> rows;
    float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    for (int i = 0; i < n; ++i) {
        if (!as_row_valid(uv + 2 * (size_t)i, xyz + 3 * (size_t)i, scores, i, sc_thres)) continue;
        for (int k = 0; k < 3; ++k) {
            const float c = xyz[3 * (size_t)i + k];
            if (rows.empty() || c < mn[k]) mn[k] = c;
            if (rows.empty() || c > mx[k]) mx[k] = c;
        }
        rows.push_back(i);
    }
    const int cnt = (int)rows.size();
    if (cnt < AS_MIN_ROWS) return 0;
    double nm[4];
    if (!as_box_norm(mn, mx, nm)) return 0;
    const double thr2 = pixel_thr * pixel_thr;
    std::vector<AsRow> cond(cnt);
    for (int i = 0; i < cnt; ++i) cond[i] = as_row(uv + 2 * (size_t)rows[i], xyz + 3 * (size_t)rows[i], nm);
    double ws[AS_WS_DOUBLES];
    const GsWs w{ws, 1};
    int best_cnt = -1, best_t = -1, best_r = -1;
    double best[9];
    for (int t = 0; t < iters; ++t) {
        int idx[3];
        if (!as_draw3(seed, sample, (uint32_t)t, cnt, uv, xyz, rows.data(), idx)) continue;
        double a[3][2], b[3][3];
        for (int k = 0; k < 3; ++k) {
            const float* q = uv + 2 * (size_t)rows[idx[k]];
            const float* x = xyz + 3 * (size_t)rows[idx[k]];
            a[k][0] = (double)q[0]; a[k][1] = (double)q[1];
            b[k][0] = (double)x[0]; b[k][1] = (double)x[1]; b[k][2] = (double)x[2];
        }
        const int nr = as_p3p(a, b, K, nm, w);
        for (int r = 0; r < nr; ++r) {
            double S[9];
            for (int k = 0; k < 9; ++k) S[k] = ws[AS_OFF_SOL + 9 * r + k];
            int c = 0;
            for (int i = 0; i < cnt; ++i) c += as_inlier(S, K, cond[i], thr2);
            if (c > best_cnt) {                       // most inliers, then smallest hypothesis, then smallest root
                best_cnt = c; best_t = t; best_r = r;
                for (int k = 0; k < 9; ++k) best[k] = S[k];
            }
        }
    }
    if (best_cnt < 0) return 0;
    double R[9], tc[3];
    as_unpack(best, R, tc);
    int nin = 0;
    std::vector<uint8_t> set(cnt), cand(cnt);
    for (int i = 0; i < cnt; ++i) {
        set[i] = (uint8_t)as_inlier(best, K, cond[i], thr2);
        nin += set[i];
    }
    if (refit_rounds > 0) {
        std::vector<float> suv(2 * (size_t)cnt), sx(3 * (size_t)cnt);           // the surviving rows, compacted
        for (int i = 0; i < cnt; ++i) {
            for (int k = 0; k < 2; ++k) suv[2 * (size_t)i + k] = uv[2 * (size_t)rows[i] + k];
            for (int k = 0; k < 3; ++k) sx[3 * (size_t)i + k] = xyz[3 * (size_t)rows[i] + k];
        }
        for (int r = 0; r < refit_rounds; ++r) {
            if (nin < AS_REFIT_MIN_INLIERS) break;
            double Rc[9], tcand[3];
            for (int k = 0; k < 9; ++k) Rc[k] = R[k];
            for (int k = 0; k < 3; ++k) tcand[k] = tc[k];
            if (!gf_abs_host_refit_once(suv.data(), sx.data(), cnt, set.data(), K, nm, Rc, tcand)) break;
            int c = 0, differ = 0;
            for (int i = 0; i < cnt; ++i) {
                cand[i] = (uint8_t)as_inlier_rt(Rc, tcand, K, cond[i], thr2);
                c += cand[i];
                differ |= cand[i] != set[i];
            }
            if (c < nin) break;
            for (int k = 0; k < 9; ++k) R[k] = Rc[k];
            for (int k = 0; k < 3; ++k) tc[k] = tcand[k];
            nin = c;
            set.swap(cand);
            ++*rounds;
            if (!differ) break;
        }
    }
    for (int i = 0; i < cnt; ++i) mask[rows[i]] = set[i];
    double tw[3];
    as_to_world(R, tc, nm, tw);
    for (int k = 0; k < 9; ++k) R_out[k] = R[k];
    for (int k = 0; k < 3; ++k) t_out[k] = tw[k];
    hyp_out[0] = best_t; hyp_out[1] = best_r;
    *n_inliers = nin;
    return 1;
}

}   // extern "C"
