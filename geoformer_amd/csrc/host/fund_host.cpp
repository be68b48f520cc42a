// TEST INFRASTRUCTURE: the serial host form of the fundamental-matrix RANSAC of k_fundamental.hip, compiled from the same fund_solver.h
// by the host C++ compiler (geoformer_amd/build.py: -O2 -ffp-contract=off, no offload) into csrc/_obj/libfund_host.so.  The tests compare
// the device against it bit for bit; nothing in the package loads it.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../fund_solver.h"

extern "C" {

// x0, x1 [7][2] fp64 pixels, norm [6] (cx, cy, s of image 0, then of image 1) -> F_out [3][9]; returns the number of solutions
int gf_fund_host_seven_point(const double* x0, const double* x1, const double* norm, double* F_out) {
    double a[7][2], b[7][2], nm[6], ws[FS_WS_DOUBLES];
    for (int i = 0; i < 7; ++i) { a[i][0] = x0[2 * i]; a[i][1] = x0[2 * i + 1]; b[i][0] = x1[2 * i]; b[i][1] = x1[2 * i + 1]; }
    for (int i = 0; i < 6; ++i) nm[i] = norm[i];
    for (int i = 0; i < FS_WS_DOUBLES; ++i) ws[i] = 0.0;
    const GsWs w{ws, 1};
    const int n = fs_seven_point(a, b, nm, w);
    for (int k = 0; k < 9 * n; ++k) F_out[k] = ws[FS_OFF_F + k];
    return n;
}

// the singular members of the pencil of F1, F2 [9] (no conditioning, no change of coordinates) -> F_out [3][9]; returns their number
int gf_fund_host_pencil(const double* F1, const double* F2, double* F_out) {
    double ws[FS_WS_DOUBLES];
    for (int i = 0; i < FS_WS_DOUBLES; ++i) ws[i] = 0.0;
    for (int k = 0; k < 9; ++k) { ws[FS_OFF_BASIS + k] = F1[k]; ws[FS_OFF_BASIS + 9 + k] = F2[k]; }
    const GsWs w{ws, 1};
    const int n = fs_pencil(w);
    for (int k = 0; k < 9 * n; ++k) F_out[k] = ws[FS_OFF_F + k];
    return n;
}

// gs_offsets_range of solver_common.h, the clamp the kernels apply to a device-side offsets array: problem n of a list of M rows -> out [2]
// (first row, number of rows)
void gf_fund_host_offsets_range(const int32_t* offsets, int n, int M, int32_t* out) {
    int off, len;
    gs_offsets_range(offsets, n, M, off, len);
    out[0] = off; out[1] = len;
}

// One refit (steps 2 - 5 of a round of fund_solver.h) from a given inlier set: matches [n][4], every row taken as a surviving row,
// mask [n], norm [6] -> F_out [9] in pixels.  Returns 1, or 0 when the round fails.
int gf_fund_host_refit_once(const float* matches, int n, const uint8_t* mask, const double* norm, double* F_out) {
    double nm[6], ws[FS_REFIT_WS_DOUBLES], F[9];
    for (int i = 0; i < 6; ++i) nm[i] = norm[i];
    std::vector<double> part((size_t)FS_SYM9 * FS_REFIT_PARTIALS, 0.0);
    for (int j = 0; j < FS_REFIT_PARTIALS; ++j) {
        double acc[FS_SYM9], r[9];
        for (int e = 0; e < FS_SYM9; ++e) acc[e] = 0.0;
        for (int i = j; i < n; i += FS_REFIT_PARTIALS) {
            if (!mask[i]) continue;
            fs_refit_row(matches + 4 * (size_t)i, nm, r);
            fs_refit_accum(acc, r);
        }
        for (int e = 0; e < FS_SYM9; ++e) part[(size_t)e * FS_REFIT_PARTIALS + j] = acc[e];
    }
    for (int e = 0; e < FS_SYM9; ++e) ws[FS_REFIT_OFF_ACC + e] = fs_refit_tree(part.data() + (size_t)e * FS_REFIT_PARTIALS);
    const GsWs w{ws, 1};
    if (!fs_refit_solve(w, nm, F)) return 0;
    for (int k = 0; k < 9; ++k) F_out[k] = F[k];
    return 1;
}

// One pair: matches [n][4] fp32 pixels, scores [n] or NULL.  Outputs as gf_fundamental_ransac_lo writes them for pair `sample` of a launch:
// F [9], hyp [2] (hypothesis, root; -1 when not valid), n_inliers [1], mask [n], rounds [1] (the accepted refits; may be NULL when
// refit_rounds is 0).  Returns valid (0 / 1), or -1 (GF_ERR_INVALID_ARGUMENT) for arguments the device entry point rejects.
int gf_fund_host_ransac_lo(const float* matches, const float* scores, int n, float sc_thres, double pixel_thr, int iters, uint32_t seed,
                           uint32_t sample, int refit_rounds, double* F_out, int32_t* hyp_out, int32_t* n_inliers, uint8_t* mask,
                           int32_t* rounds) {
    if (iters <= 0 || iters % FS_HYP_PER_WG != 0 || n < 0 || !(pixel_thr > 0.0)) return -1;
    if (refit_rounds < 0 || refit_rounds > FS_REFIT_MAX_ROUNDS || (refit_rounds > 0 && !rounds)) return -1;
    if (rounds) *rounds = 0;
    for (int k = 0; k < 9; ++k) F_out[k] = 0.0;
    hyp_out[0] = hyp_out[1] = -1;
    *n_inliers = 0;
    for (int i = 0; i < n; ++i) mask[i] = 0;
    std::vector<int32_t> rows;
    float box[8] = {0, 0, 0, 0, 0, 0, 0, 0};          // min, max of x0, y0, x1, y1
    for (int i = 0; i < n; ++i) {
        const float* m = matches + 4 * (size_t)i;
        if (!fs_row_valid(m, scores, i, sc_thres)) continue;
        for (int k = 0; k < 4; ++k) {
            if (rows.empty() || m[k] < box[2 * k]) box[2 * k] = m[k];
            if (rows.empty() || m[k] > box[2 * k + 1]) box[2 * k + 1] = m[k];
        }
        rows.push_back(i);
    }
    const int cnt = (int)rows.size();
    if (cnt < FS_MIN_MATCHES) return 0;
    double nm[6];
    const int ok0 = fs_box_norm(box[0], box[1], box[2], box[3], nm), ok1 = fs_box_norm(box[4], box[5], box[6], box[7], nm + 3);
    if (!ok0 || !ok1) return 0;
    const double thr2 = pixel_thr * pixel_thr;
    double ws[FS_WS_DOUBLES];
    const GsWs w{ws, 1};
    int best_cnt = -1, best_t = -1, best_r = -1;
    double best[9];
    for (int t = 0; t < iters; ++t) {
        int idx[7];
        if (!fs_draw7(seed, sample, (uint32_t)t, cnt, matches, rows.data(), idx)) continue;
        double x0[7][2], x1[7][2];
        for (int k = 0; k < 7; ++k) {
            const float* m = matches + 4 * (size_t)rows[idx[k]];
            x0[k][0] = (double)m[0]; x0[k][1] = (double)m[1]; x1[k][0] = (double)m[2]; x1[k][1] = (double)m[3];
        }
        const int nr = fs_seven_point(x0, x1, nm, w);
        for (int r = 0; r < nr; ++r) {
            double F[9];
            for (int k = 0; k < 9; ++k) F[k] = ws[FS_OFF_F + 9 * r + k];
            int c = 0;
            for (int i = 0; i < cnt; ++i) c += fs_inlier(F, matches + 4 * (size_t)rows[i], thr2);
            if (c > best_cnt) {                       // most inliers, then smallest hypothesis, then smallest root
                best_cnt = c; best_t = t; best_r = r;
                for (int k = 0; k < 9; ++k) best[k] = F[k];
            }
        }
    }
    if (best_cnt < 0) return 0;
    int nin = 0;
    for (int i = 0; i < cnt; ++i) {
        const int in = fs_inlier(best, matches + 4 * (size_t)rows[i], thr2);
        mask[rows[i]] = (uint8_t)in;
        nin += in;
    }
    // ---- refit on the inliers: cur = (best, set, nin) over the surviving rows
    if (refit_rounds > 0) {
        std::vector<float> sm(4 * (size_t)cnt);               // the surviving rows, compacted
        std::vector<uint8_t> set(cnt), cand(cnt);
        for (int i = 0; i < cnt; ++i) {
            for (int k = 0; k < 4; ++k) sm[4 * (size_t)i + k] = matches[4 * (size_t)rows[i] + k];
            set[i] = mask[rows[i]];
        }
        for (int r = 0; r < refit_rounds; ++r) {
            if (nin < FS_REFIT_MIN_INLIERS) break;
            double F[9];
            if (!gf_fund_host_refit_once(sm.data(), cnt, set.data(), nm, F)) break;
            int c = 0, differ = 0;
            for (int i = 0; i < cnt; ++i) {
                cand[i] = (uint8_t)fs_inlier(F, sm.data() + 4 * (size_t)i, thr2);
                c += cand[i];
                differ |= cand[i] != set[i];
            }
            if (c < nin) break;
            for (int k = 0; k < 9; ++k) best[k] = F[k];
            nin = c;
            set.swap(cand);
            ++*rounds;
            if (!differ) break;
        }
        for (int i = 0; i < cnt; ++i) mask[rows[i]] = set[i];
    }
    for (int k = 0; k < 9; ++k) F_out[k] = best[k];
    hyp_out[0] = best_t; hyp_out[1] = best_r;
    *n_inliers = nin;
    return 1;
}

// gf_fundamental_ransac: no refit
int gf_fund_host_ransac(const float* matches, const float* scores, int n, float sc_thres, double pixel_thr, int iters, uint32_t seed,
                        uint32_t sample, double* F_out, int32_t* hyp_out, int32_t* n_inliers, uint8_t* mask) {
    return gf_fund_host_ransac_lo(matches, scores, n, sc_thres, pixel_thr, iters, seed, sample, 0, F_out, hyp_out, n_inliers, mask, nullptr);
}

}   // extern "C"
