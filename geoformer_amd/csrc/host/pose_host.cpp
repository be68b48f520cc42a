// TEST INFRASTRUCTURE: the serial host form of the essential-matrix RANSAC of k_pose.hip, compiled from the same pose_solver.h by
// the host C++ compiler (geoformer_amd/build.py: -O2 -ffp-contract=off, no offload) into csrc/_obj/libpose_host.so.  The tests
// compare the device against it bit for bit; nothing in the package loads it.
#include <stdint.h>
#include <string.h>

#include "../pose_solver.h"

extern "C" {

// x0, x1 [5][2] fp64 normalised coordinates -> E_out [10][9]; returns the number of solutions
int gf_pose_host_five_point(const double* x0, const double* x1, double* E_out) {
    double a[5][2], b[5][2], ws[PS_WS_DOUBLES];
    for (int i = 0; i < 5; ++i) { a[i][0] = x0[2 * i]; a[i][1] = x0[2 * i + 1]; b[i][0] = x1[2 * i]; b[i][1] = x1[2 * i + 1]; }
    for (int i = 0; i < PS_WS_DOUBLES; ++i) ws[i] = 0.0;
    const PsWs w{ws, 1};
    const int n = ps_five_point(a, b, w);
    for (int k = 0; k < 9 * n; ++k) E_out[k] = ws[PS_OFF_E + k];
    return n;
}

// One pair: mk0, mk1 [n][2] fp32 pixels, K0, K1 [9] fp32.  Outputs as gf_pose_essential_ransac writes them for the pair:
// E [9], R [9], t [3], hyp [2] (hypothesis, root; -1 without a pose), n_inliers [1], mask [n].  Returns valid (0 / 1), or -1
// (GF_ERR_INVALID_ARGUMENT) for an iteration count the device entry point rejects.
int gf_pose_host_ransac(const float* mk0, const float* mk1, int n, const float* K0, const float* K1, double pixel_thr, int iters,
                        uint32_t seed, uint32_t sample, double* E_out, double* R_out, double* t_out, int32_t* hyp_out,
                        int32_t* n_inliers, uint8_t* mask) {
    if (iters <= 0 || iters % PS_HYP_PER_WG != 0 || n < 0) return -1;
    for (int k = 0; k < 9; ++k) { E_out[k] = 0.0; R_out[k] = 0.0; }
    for (int k = 0; k < 3; ++k) t_out[k] = 0.0;
    hyp_out[0] = hyp_out[1] = -1;
    *n_inliers = 0;
    for (int i = 0; i < n; ++i) mask[i] = 0;
    if (n < PS_MIN_MATCHES) return 0;
    const double thr = ps_threshold(K0, K1, pixel_thr), thr2 = thr * thr;
    double ws[PS_WS_DOUBLES];
    const PsWs w{ws, 1};
    int best_cnt = -1, best_t = -1, best_r = -1;
    double best[9];
    for (int t = 0; t < iters; ++t) {
        int idx[5];
        if (!gs_draw_distinct<5>(seed, sample, (uint32_t)t, n, idx)) continue;
        double x0[5][2], x1[5][2];
        for (int k = 0; k < 5; ++k) {
            ps_normalise(K0, mk0[2 * idx[k]], mk0[2 * idx[k] + 1], x0[k][0], x0[k][1]);
            ps_normalise(K1, mk1[2 * idx[k]], mk1[2 * idx[k] + 1], x1[k][0], x1[k][1]);
        }
        const int nr = ps_five_point(x0, x1, w);
        for (int r = 0; r < nr; ++r) {
            double E[9];
            for (int k = 0; k < 9; ++k) E[k] = ws[PS_OFF_E + 9 * r + k];
            int c = 0;
            for (int i = 0; i < n; ++i) {
                double a, b, u, v;
                ps_normalise(K0, mk0[2 * i], mk0[2 * i + 1], a, b);
                ps_normalise(K1, mk1[2 * i], mk1[2 * i + 1], u, v);
                c += ps_inlier(E, a, b, u, v, thr2);
            }
            if (c > best_cnt) {                       // most inliers, then smallest hypothesis, then smallest root
                best_cnt = c; best_t = t; best_r = r;
                for (int k = 0; k < 9; ++k) best[k] = E[k];
            }
        }
    }
    if (best_cnt < PS_MIN_MATCHES) return 0;
    double R1[9], R2[9], tt[3];
    const int dec = ps_decompose(best, R1, R2, tt);
    int votes[4] = {0, 0, 0, 0}, nin = 0;
    for (int i = 0; i < n; ++i) {
        double a, b, u, v;
        ps_normalise(K0, mk0[2 * i], mk0[2 * i + 1], a, b);
        ps_normalise(K1, mk1[2 * i], mk1[2 * i + 1], u, v);
        const int in = ps_inlier(best, a, b, u, v, thr2);
        mask[i] = (uint8_t)in;
        nin += in;
        if (in && dec)
            for (int c = 0; c < 4; ++c) {
                double R[9], tc[3];
                ps_candidate(c, R1, R2, tt, R, tc);
                votes[c] += ps_cheiral(R, tc, a, b, u, v);
            }
    }
    int bc = 0;
    for (int c = 1; c < 4; ++c)
        if (votes[c] > votes[bc]) bc = c;
    if (!dec || votes[bc] <= 0) {                     // the reference's `ret is None`
        for (int i = 0; i < n; ++i) mask[i] = 0;
        return 0;
    }
    double R[9], tc[3];
    ps_candidate(bc, R1, R2, tt, R, tc);
    for (int k = 0; k < 9; ++k) { E_out[k] = best[k]; R_out[k] = R[k]; }
    for (int k = 0; k < 3; ++k) t_out[k] = tc[k];
    hyp_out[0] = best_t; hyp_out[1] = best_r;
    *n_inliers = nin;
    return 1;
}

}   // extern "C"
