// TEST INFRASTRUCTURE: the serial host form of the calibrated two-view RANSAC of k_relpose.hip, compiled from the same rel_solver.h by the
// host C++ compiler (geoformer_amd/build.py: -O2 -ffp-contract=off, no offload) into csrc/_obj/librelpose_host.so.  The tests compare the
// device against it bit for bit; nothing in the package loads it.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../rel_solver.h"

extern "C" {

// the residual of one row (x0, y0, x1, y1 normalised, fp64) under (R, t) and its derivatives by the five parameters; returns rs_gn_row's ok
int gf_rel_host_gn_row(const double* R_in, const double* t_in, const double* row4, double* J_out, double* res_out) {
    double R[9], t[3], E[9], D[5][9], J[5], res = 0.0;
    for (int k = 0; k < 9; ++k) R[k] = R_in[k];
    for (int k = 0; k < 3; ++k) t[k] = t_in[k];
    if (!rs_gn_basis(R, t, D)) return 0;
    rs_E(R, t, E);
    const RsRow q{row4[0], row4[1], row4[2], row4[3]};
    if (!rs_gn_row(E, D, q, J, res)) return 0;
    for (int k = 0; k < 5; ++k) J_out[k] = J[k];
    *res_out = res;
    return 1;
}

// (R, t) <- the update by d [5], in place; returns rs_gn_update's ok
int gf_rel_host_gn_update(const double* d_in, double* R_io, double* t_io) {
    double d[5], R[9], t[3];
    for (int k = 0; k < 5; ++k) d[k] = d_in[k];
    for (int k = 0; k < 9; ++k) R[k] = R_io[k];
    for (int k = 0; k < 3; ++k) t[k] = t_io[k];
    if (!rs_gn_update(d, R, t)) return 0;
    for (int k = 0; k < 9; ++k) R_io[k] = R[k];
    for (int k = 0; k < 3; ++k) t_io[k] = t[k];
    return 1;
}

// one Gauss-Newton step from a given inlier set over n surviving rows
static int rel_gn_step(const RsRow* rows, int n, const uint8_t* mask, double (&R)[9], double (&t)[3]) {
    double E[9], D[5][9];
    if (!rs_gn_basis(R, t, D)) return 0;
    rs_E(R, t, E);
    std::vector<double> part((size_t)RS_GN_SUMS * FS_REFIT_PARTIALS, 0.0);
    for (int j = 0; j < FS_REFIT_PARTIALS; ++j) {
        double acc[RS_GN_SUMS], J[5], res;
        for (int e = 0; e < RS_GN_SUMS; ++e) acc[e] = 0.0;
        for (int i = j; i < n; i += FS_REFIT_PARTIALS) {
            if (!mask[i]) continue;
            if (rs_gn_row(E, D, rows[i], J, res)) rs_gn_accum(acc, J, res);
        }
        for (int e = 0; e < RS_GN_SUMS; ++e) part[(size_t)e * FS_REFIT_PARTIALS + j] = acc[e];
    }
    double ws[RS_GN_WS_DOUBLES];
    for (int i = 0; i < RS_GN_WS_DOUBLES; ++i) ws[i] = 0.0;
    for (int e = 0; e < RS_GN_SUMS; ++e) ws[RS_GN_OFF_ACC + e] = fs_refit_tree(part.data() + (size_t)e * FS_REFIT_PARTIALS);
    const GsWs w{ws, 1};
    if (!rs_gn_solve(w)) return 0;
    double d[5];
    for (int k = 0; k < 5; ++k) d[k] = ws[RS_GN_OFF_X + k];
    return rs_gn_update(d, R, t);
}

// one ROUND's fit (RS_GN_STEPS steps) on a given set: rows4 [n][4] normalised fp64, mask [n]; R, t in place.  Returns 1, or 0 when a step
// fails (R, t unchanged).
int gf_rel_host_refit_once(const double* rows4, int n, const uint8_t* mask, double* R_io, double* t_io) {
    std::vector<RsRow> rows((size_t)(n > 0 ? n : 0));
    for (int i = 0; i < n; ++i) rows[i] = RsRow{rows4[4 * (size_t)i], rows4[4 * (size_t)i + 1], rows4[4 * (size_t)i + 2], rows4[4 * (size_t)i + 3]};
    double R[9], t[3];
    for (int k = 0; k < 9; ++k) R[k] = R_io[k];
    for (int k = 0; k < 3; ++k) t[k] = t_io[k];
    for (int s = 0; s < RS_GN_STEPS; ++s)
        if (!rel_gn_step(rows.data(), n, mask, R, t)) return 0;
    for (int k = 0; k < 9; ++k) R_io[k] = R[k];
    for (int k = 0; k < 3; ++k) t_io[k] = t[k];
    return 1;
}

// One pair: m [n][4] fp32 pixels, scores [n] or NULL, K0, K1 [9] fp32.  Outputs as gf_relpose_ransac_lo writes them for pair `sample` of a
// launch: E [9], R [9], t [3], hyp [2] (hypothesis, root; -1 when not valid), n_inliers [1], n_cheiral [1], mask [n], rounds [1].  Returns
// valid (0 / 1), or -1 (GF_ERR_INVALID_ARGUMENT) for arguments the device entry point rejects.
int gf_rel_host_ransac(const float* m, const float* scores, int n, const float* K0, const float* K1, float sc_thres, double pixel_thr, int iters,
                       uint32_t seed, uint32_t sample, int refit_rounds, double* E_out, double* R_out, double* t_out, int32_t* hyp_out,
                       int32_t* n_inliers, int32_t* n_cheiral, uint8_t* mask, int32_t* rounds) {
    if (iters <= 0 || iters % 64 != 0 || n < 0 || !(pixel_thr > 0.0) || !(pixel_thr < (double)INFINITY)) return -1;
    if (refit_rounds < 0 || refit_rounds > RS_REFIT_MAX_ROUNDS) return -1;
    *rounds = 0;
    for (int k = 0; k < 9; ++k) { E_out[k] = 0.0; R_out[k] = 0.0; }
    for (int k = 0; k < 3; ++k) t_out[k] = 0.0;
    hyp_out[0] = hyp_out[1] = -1;
    *n_inliers = 0;
    *n_cheiral = 0;
    for (int i = 0; i < n; ++i) mask[i] = 0;
    std::vector<int32_t> rows;
    for (int i = 0; i < n; ++i)
        if (fs_row_valid(m + 4 * (size_t)i, scores, i, sc_thres)) rows.push_back(i);
    const int cnt = (int)rows.size();
    if (cnt < RS_MIN_ROWS || !rs_k_valid(K0, K1)) return 0;
    const double thr = ps_threshold(K0, K1, pixel_thr), thr2 = thr * thr;
    std::vector<RsRow> q(cnt);
    for (int i = 0; i < cnt; ++i) q[i] = rs_row(m + 4 * (size_t)rows[i], K0, K1);
    double ws[PS_WS_DOUBLES];
    const PsWs w{ws, 1};
    int best_cnt = -1, best_t = -1, best_r = -1;
    double best[9];
    for (int t = 0; t < iters; ++t) {
        int idx[5];
        if (!gs_draw_distinct<5>(seed, sample, (uint32_t)t, cnt, idx)) continue;
        double x0[5][2], x1[5][2];
        for (int k = 0; k < 5; ++k) {
            x0[k][0] = q[idx[k]].x0; x0[k][1] = q[idx[k]].y0; x1[k][0] = q[idx[k]].x1; x1[k][1] = q[idx[k]].y1;
        }
        const int nr = ps_five_point(x0, x1, w);
        for (int r = 0; r < nr; ++r) {
            double E[9];
            for (int k = 0; k < 9; ++k) E[k] = ws[PS_OFF_E + 9 * r + k];
            int c = 0;
            for (int i = 0; i < cnt; ++i) c += rs_inlier(E, q[i], thr2);
            if (c > best_cnt) {                       // most inliers, then smallest hypothesis, then smallest root
                best_cnt = c; best_t = t; best_r = r;
                for (int k = 0; k < 9; ++k) best[k] = E[k];
            }
        }
    }
    if (best_cnt < RS_MIN_ROWS) return 0;
    // ---- step 6: the pose
    double R1[9], R2[9], tt[3];
    const int dec = ps_decompose(best, R1, R2, tt);
    int votes[4] = {0, 0, 0, 0}, nin = 0;
    std::vector<uint8_t> set(cnt), cand(cnt);
    for (int i = 0; i < cnt; ++i) {
        set[i] = (uint8_t)rs_inlier(best, q[i], thr2);
        nin += set[i];
        if (set[i] && dec)
            for (int c = 0; c < 4; ++c) {
                double R[9], tc[3];
                ps_candidate(c, R1, R2, tt, R, tc);
                votes[c] += ps_cheiral(R, tc, q[i].x0, q[i].y0, q[i].x1, q[i].y1);
            }
    }
    int bc = 0;
    for (int c = 1; c < 4; ++c)
        if (votes[c] > votes[bc]) bc = c;
    if (!dec || votes[bc] <= 0) return 0;
    double E[9], R[9], tc[3];
    for (int k = 0; k < 9; ++k) E[k] = best[k];
    ps_candidate(bc, R1, R2, tt, R, tc);
    // ---- step 7: the refit rounds
    for (int r = 0; r < refit_rounds; ++r) {
        if (nin < RS_REFIT_MIN_INLIERS) break;
        double Rc[9], tcand[3], Ec[9];
        for (int k = 0; k < 9; ++k) Rc[k] = R[k];
        for (int k = 0; k < 3; ++k) tcand[k] = tc[k];
        int ok = 1;
        for (int s = 0; s < RS_GN_STEPS && ok; ++s) ok = rel_gn_step(q.data(), cnt, set.data(), Rc, tcand);
        if (!ok) break;
        rs_E(Rc, tcand, Ec);
        int c = 0, differ = 0;
        for (int i = 0; i < cnt; ++i) {
            cand[i] = (uint8_t)rs_inlier(Ec, q[i], thr2);
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
    if (*rounds > 0 && !rs_E_unit(R, tc, E)) {        // (unit t and a finite R: the norm is sqrt(2); kept as the device's write_refined has it)
        for (int k = 0; k < 9; ++k) E[k] = 0.0;
    }
    for (int i = 0; i < cnt; ++i) mask[rows[i]] = set[i];
    for (int k = 0; k < 9; ++k) { E_out[k] = E[k]; R_out[k] = R[k]; }
    for (int k = 0; k < 3; ++k) t_out[k] = tc[k];
    hyp_out[0] = best_t; hyp_out[1] = best_r;
    *n_inliers = nin;
    *n_cheiral = votes[bc];
    return 1;
}

}   // extern "C"
