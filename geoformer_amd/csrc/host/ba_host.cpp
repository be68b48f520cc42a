// TEST INFRASTRUCTURE and CPU reference: the serial host form of the bundle adjustment of k_bundle.hip, compiled from the same ba_spec.h by
// the host C++ compiler (geoformer_amd/build.py: -O2 -ffp-contract=off, no offload) into csrc/_obj/libba_host.so.  The tests compare the
// device against it bit for bit; nothing in the package loads it.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../ba_spec.h"

extern "C" {

// All pointers are host memory.  The arguments and outputs of gf_bundle_adjust (include/geoformer_hip.h) without the workspace and the
// stream.  Returns 0, or -1 (GF_ERR_INVALID_ARGUMENT) for arguments the device entry point rejects.
int gf_ba_host_adjust(const int32_t* obs_off, int T, int n_obs, const int32_t* obs_image, const float* obs_uv, const int32_t* img_off,
                      const int32_t* img_obs, const int32_t* cam_free, int n_images, int F, const float* K, const double* R_in,
                      const double* t_in, const double* X_in, float thr, int iters, double* R_out, double* t_out, double* X_out,
                      uint8_t* inliers, int32_t* n_inliers, double* cost, int32_t* accepted, double* lambda, int32_t* status) {
    if (T < 1 || n_obs < 1 || n_images < 1 || F < 0 || F > BA_MAX_FREE || F > n_images) return -1;
    if (iters < 1 || iters > BA_MAX_ITERS || !(thr > 0.f && thr < INFINITY)) return -1;
    if (ba_check_tables(obs_off, T, n_obs, obs_image, img_off, img_obs, cam_free, n_images, F)) return -1;

    const size_t nI = (size_t)n_images, nT = (size_t)T, nO = (size_t)n_obs;
    const int n = 6 * F, nb = (T + BA_BLOCK - 1) / BA_BLOCK;
    std::vector<int32_t> cam_ok(nI), obs_point(nO), hold(nT, 0);
    std::vector<double> Rs[2] = {std::vector<double>(R_in, R_in + 9 * nI), std::vector<double>(R_in, R_in + 9 * nI)};
    std::vector<double> ts[2] = {std::vector<double>(t_in, t_in + 3 * nI), std::vector<double>(t_in, t_in + 3 * nI)};
    std::vector<double> Xs[2] = {std::vector<double>(X_in, X_in + 3 * nT), std::vector<double>(X_in, X_in + 3 * nT)};
    std::vector<uint8_t> part(nO, 0);
    std::vector<double> W(18 * nO, 0.0), Tm(18 * nO, 0.0), g(3 * nT, 0.0), Ainv(9 * nT, 0.0);
    std::vector<double> S((size_t)n * n, 0.0), rhs((size_t)n, 0.0), dc((size_t)n, 0.0), row(36 * (size_t)(F ? F : 1)), partial(BA_BLOCK);
    int st = 0;
    for (int i = 0; i < n_images; ++i) {
        cam_ok[i] = tr_cam_ok(K + 9 * (size_t)i, R_in + 9 * (size_t)i, t_in + 3 * (size_t)i);
        if (cam_free[i] >= 0 && !cam_ok[i]) st |= BA_FLAG_FREE_NO_POSE;
    }
    for (int p = 0; p < T; ++p)
        for (int o = obs_off[p]; o < obs_off[p + 1]; ++o) obs_point[o] = p;

    BaView v;
    v.obs_off = obs_off; v.obs_image = obs_image; v.obs_uv = obs_uv; v.obs_point = obs_point.data(); v.img_off = img_off; v.img_obs = img_obs;
    v.cam_free = cam_free; v.cam_ok = cam_ok.data(); v.K = K; v.T = T; v.n_obs = n_obs; v.n_images = n_images; v.F = F;
    v.thr2 = (double)thr * (double)thr;
    const BaIter it{part.data(), W.data(), Tm.data(), g.data(), Ainv.data(), hold.data()};
    double ws[BA_PT_WS_DOUBLES];
    for (int i = 0; i < BA_PT_WS_DOUBLES; ++i) ws[i] = 0.0;
    const GsWs w{ws, 1};

    auto state = [&](int c) { return BaState{Rs[c].data(), ts[c].data(), Xs[c].data()}; };
    auto total_cost = [&](const BaState& s) {
        double sum = 0.0;
        for (int b = 0; b < nb; ++b) {
            for (int k = 0; k < BA_BLOCK; ++k) {
                const int p = b * BA_BLOCK + k;
                partial[k] = p < T ? ba_point_cost(v, s, p, nullptr, nullptr) : 0.0;
            }
            sum = sum + ba_block_tree(partial.data());
        }
        return sum;
    };

    int cur = 0;
    double lam = BA_LAMBDA_INIT, cost_cur = total_cost(state(0));
    cost[0] = cost_cur;
    lambda[0] = lam;
    for (int iter = 0; iter < iters; ++iter) {
        const BaState s = state(cur);
        const int cand = 1 - cur;
        int ok = 1;
        for (int p = 0; p < T; ++p)
            if (ba_point_build(v, s, it, p, lam, w)) st |= BA_FLAG_POINT_HELD;
        if (F > 0) {
            for (int i = 0; i < n_images; ++i) {
                const int f = cam_free[i];
                if (f < 0) continue;
                double r6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                for (int e = 0; e < 36 * (f + 1); ++e) row[e] = 0.0;
                ba_camera_row(v, s, it, i, f, lam, row.data(), r6, BaOwnAll{});
                for (int r = 0; r < 6; ++r) {
                    for (int j = 0; j <= f; ++j)
                        for (int c = 0; c < 6; ++c) S[(size_t)(6 * f + r) * n + 6 * j + c] = row[36 * j + 6 * r + c];
                    rhs[6 * f + r] = r6[r];
                }
            }
            for (int c = 0; c < n && ok; ++c) {
                const double* rc = S.data() + (size_t)c * n;
                const double d = ba_chol_chain(rc[c], rc, 1, rc, c);
                if (!(d > 0.0)) { ok = 0; break; }
                const double l = sqrt(d);
                for (int a = c + 1; a < n; ++a) S[(size_t)a * n + c] = ba_chol_chain(S[(size_t)a * n + c], S.data() + (size_t)a * n, 1, rc, c) / l;
                S[(size_t)c * n + c] = l;
            }
            if (!ok) st |= BA_FLAG_STEP_FAILED;
            if (ok) {
                for (int a = 0; a < n; ++a) dc[a] = rhs[a];
                for (int k = 0; k < n; ++k) {
                    dc[k] = dc[k] / S[(size_t)k * n + k];
                    for (int a = k + 1; a < n; ++a) dc[a] = dc[a] - S[(size_t)a * n + k] * dc[k];
                }
                for (int k = n - 1; k >= 0; --k) {
                    dc[k] = dc[k] / S[(size_t)k * n + k];
                    for (int a = 0; a < k; ++a) dc[a] = dc[a] - S[(size_t)k * n + a] * dc[k];
                }
            }
        }
        double cost_cand = cost_cur;
        if (ok) {
            for (int i = 0; i < n_images; ++i)
                if (!ba_camera_delta(v, s, i, dc.data(), Rs[cand].data(), ts[cand].data())) { ok = 0; st |= BA_FLAG_STEP_FAILED; }
            for (int p = 0; p < T; ++p) ba_point_delta(v, s, it, p, dc.data(), Xs[cand].data());
            cost_cand = total_cost(state(cand));
        }
        const int acc = ba_decide_step(ok, cost_cur, cost_cand, lam);
        if (acc) { cur = cand; cost_cur = cost_cand; }
        accepted[iter] = acc;
        cost[iter + 1] = cost_cur;
        lambda[iter + 1] = lam;
    }
    const BaState s = state(cur);
    memcpy(R_out, s.R, 9 * nI * sizeof(double));
    memcpy(t_out, s.t, 3 * nI * sizeof(double));
    memcpy(X_out, s.X, 3 * nT * sizeof(double));
    for (int p = 0; p < T; ++p) ba_point_cost(v, s, p, inliers, n_inliers + p);
    *status = st;
    return 0;
}

}   // extern "C"
