// TEST INFRASTRUCTURE and CPU reference: the serial host form of the bundle adjustment of k_bundle.hip, compiled from the same ba_spec.h
// and ba_pcg_spec.h by the host C++ compiler (geoformer_amd/build.py: -O2 -ffp-contract=off, no offload) into csrc/_obj/libba_host.so.  The
// tests compare the device against it bit for bit; nothing in the package loads it.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../ba_spec.h"
#include "../ba_pcg_spec.h"

// The Levenberg-Marquardt shell, shared by both solvers of the reduced camera system.  pcg = 0: rules 6 and 7 of ba_spec.h (dense Cholesky);
// pcg = 1: the rules of ba_pcg_spec.h.  The arguments have been checked.
static int ba_host_run(const int32_t* obs_off, int T, int n_obs, const int32_t* obs_image, const float* obs_uv, const int32_t* img_off,
                       const int32_t* img_obs, const int32_t* cam_free, int n_images, int F, const float* K, const double* R_in,
                       const double* t_in, const double* X_in, float thr, int iters, double* R_out, double* t_out, double* X_out,
                       uint8_t* inliers, int32_t* n_inliers, double* cost, int32_t* accepted, double* lambda, int32_t* status, int pcg,
                       int cg_iters, double cg_tol, int32_t* cg_used, double* cg_res) {
    const size_t nI = (size_t)n_images, nT = (size_t)T, nO = (size_t)n_obs;
    const int n = 6 * F, nb = (T + BA_BLOCK - 1) / BA_BLOCK;
    std::vector<int32_t> cam_ok(nI), obs_point(nO), hold(nT, 0);
    std::vector<double> Rs[2] = {std::vector<double>(R_in, R_in + 9 * nI), std::vector<double>(R_in, R_in + 9 * nI)};
    std::vector<double> ts[2] = {std::vector<double>(t_in, t_in + 3 * nI), std::vector<double>(t_in, t_in + 3 * nI)};
    std::vector<double> Xs[2] = {std::vector<double>(X_in, X_in + 3 * nT), std::vector<double>(X_in, X_in + 3 * nT)};
    std::vector<uint8_t> part(nO, 0);
    std::vector<double> W(18 * nO, 0.0), Tm(18 * nO, 0.0), g(3 * nT, 0.0), Ainv(9 * nT, 0.0);
    std::vector<double> S(pcg ? 0 : (size_t)n * n, 0.0), rhs((size_t)n, 0.0), dc((size_t)n, 0.0), row(pcg ? 0 : 36 * (size_t)(F ? F : 1)),
        partial(BA_BLOCK);
    // the PCG solver's vectors and blocks: O(F) and O(T), nothing of size F^2
    const size_t nF = pcg ? (size_t)F : 0;
    std::vector<double> Ul(36 * nF), Minv(36 * nF), cr(6 * nF), cz(6 * nF), cp(6 * nF), cq(6 * nF), share(nF), zp(pcg ? 3 * nT : 0),
        sums(pcg ? BA_PCG_SUMS * (size_t)BA_BLOCK : 0);
    std::vector<int32_t> free_img(nF);
    for (int i = 0; i < n_images && pcg; ++i)
        if (cam_free[i] >= 0) free_img[cam_free[i]] = i;
    const double tol2 = cg_tol * cg_tol;
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
    double ws6[BA_PCG_WS_DOUBLES];
    for (int i = 0; i < BA_PCG_WS_DOUBLES; ++i) ws6[i] = 0.0;
    const GsWs w6{ws6, 1};

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
    // the inner product of ba_pcg_spec.h from the cameras' shares
    auto reduce_shares = [&]() {
        double sum = 0.0;
        for (int b = 0; b * BA_BLOCK < F; ++b) {
            for (int k = 0; k < BA_BLOCK; ++k) partial[k] = b * BA_BLOCK + k < F ? share[(size_t)b * BA_BLOCK + k] : 0.0;
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
        if (pcg) {
            cg_used[iter] = 0;
            cg_res[iter] = 0.0;
        }
        if (F > 0 && pcg) {
            int setup_ok = 1;
            for (int f = 0; f < F; ++f) {                              // the camera blocks
                int qb, qlen, any = 0;
                gs_offsets_range(img_off, free_img[f], n_obs, qb, qlen);
                for (size_t e = 0; e < sums.size(); ++e) sums[e] = 0.0;
                for (int q = qb; q < qb + qlen; ++q)
                    any |= ba_pcg_obs_terms(v, s, it, img_obs[q],
                                            *reinterpret_cast<double(*)[BA_PCG_SUMS]>(&sums[BA_PCG_SUMS * (size_t)((q - qb) % BA_BLOCK)]));
                double tot[BA_PCG_SUMS], M[36], r6[6];
                for (int j = 0; j < BA_PCG_SUMS; ++j) {
                    for (int k = 0; k < BA_BLOCK; ++k) partial[k] = sums[BA_PCG_SUMS * (size_t)k + j];
                    tot[j] = ba_block_tree(partial.data());
                }
                ba_pcg_blocks(tot, any, lam, &Ul[36 * (size_t)f], M, r6);
                for (int k = 0; k < 6; ++k) setup_ok &= ba_pcg_inverse_column(M, k, w6, &Minv[36 * (size_t)f]);
                ba_pcg_apply6(&Minv[36 * (size_t)f], r6, &cz[6 * (size_t)f]);
                for (int k = 0; k < 6; ++k) {
                    dc[6 * (size_t)f + k] = 0.0;
                    cr[6 * (size_t)f + k] = r6[k];
                    cp[6 * (size_t)f + k] = cz[6 * (size_t)f + k];
                }
                share[f] = ba_pcg_dot6(r6, &cz[6 * (size_t)f]);
            }
            BaPcgScalars c;
            ba_pcg_begin(c, setup_ok, setup_ok ? reduce_shares() : 0.0);
            for (int i = 0; i < cg_iters && !c.done; ++i) {
                for (int p = 0; p < T; ++p) ba_pcg_point_z(v, it, p, cp.data(), zp.data());
                for (int f = 0; f < F; ++f) {                          // q = S p
                    int qb, qlen;
                    gs_offsets_range(img_off, free_img[f], n_obs, qb, qlen);
                    for (int e = 0; e < 6 * BA_BLOCK; ++e) sums[e] = 0.0;
                    for (int q = qb; q < qb + qlen; ++q)
                        ba_pcg_obs_tz(v, it, img_obs[q], zp.data(), *reinterpret_cast<double(*)[6]>(&sums[6 * (size_t)((q - qb) % BA_BLOCK)]));
                    double u6[6], q6[6];
                    ba_pcg_apply6(&Ul[36 * (size_t)f], &cp[6 * (size_t)f], u6);
                    for (int k = 0; k < 6; ++k) {
                        for (int j = 0; j < BA_BLOCK; ++j) partial[j] = sums[6 * (size_t)j + k];
                        q6[k] = u6[k] - ba_block_tree(partial.data());
                        cq[6 * (size_t)f + k] = q6[k];
                    }
                    share[f] = ba_pcg_dot6(&cp[6 * (size_t)f], q6);
                }
                ba_pcg_alpha(c, reduce_shares());
                if (c.done) break;
                for (int f = 0; f < F; ++f) {
                    const size_t o = 6 * (size_t)f;
                    for (int k = 0; k < 6; ++k) {
                        dc[o + k] = dc[o + k] + c.alpha * cp[o + k];
                        cr[o + k] = cr[o + k] - c.alpha * cq[o + k];
                    }
                    ba_pcg_apply6(&Minv[36 * (size_t)f], &cr[o], &cz[o]);
                    share[f] = ba_pcg_dot6(&cr[o], &cz[o]);
                }
                ba_pcg_beta(c, reduce_shares(), i, tol2);
                if (c.done) break;
                for (size_t e = 0; e < 6 * (size_t)F; ++e) cp[e] = cz[e] + c.beta * cp[e];
            }
            cg_used[iter] = c.used;
            cg_res[iter] = c.res;
            if (c.failed) {
                ok = 0;
                st |= BA_FLAG_STEP_FAILED;
            }
        } else if (F > 0) {
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
    return ba_host_run(obs_off, T, n_obs, obs_image, obs_uv, img_off, img_obs, cam_free, n_images, F, K, R_in, t_in, X_in, thr, iters, R_out, t_out,
                       X_out, inliers, n_inliers, cost, accepted, lambda, status, 0, 0, 0.0, nullptr, nullptr);
}

// The same with the PCG solver (the arguments and outputs of gf_bundle_adjust_pcg): cg_used int32 [iters] and cg_res fp64 [iters] are its logs.
int gf_ba_host_adjust_pcg(const int32_t* obs_off, int T, int n_obs, const int32_t* obs_image, const float* obs_uv, const int32_t* img_off,
                          const int32_t* img_obs, const int32_t* cam_free, int n_images, int F, const float* K, const double* R_in,
                          const double* t_in, const double* X_in, float thr, int iters, int cg_iters, double cg_tol, double* R_out,
                          double* t_out, double* X_out, uint8_t* inliers, int32_t* n_inliers, double* cost, int32_t* accepted, double* lambda,
                          int32_t* status, int32_t* cg_used, double* cg_res) {
    if (T < 1 || n_obs < 1 || n_images < 1 || F < 0 || F > n_images) return -1;
    if (iters < 1 || iters > BA_MAX_ITERS || !(thr > 0.f && thr < INFINITY)) return -1;
    if (ba_pcg_check_limits(F, cg_iters, cg_tol)) return -1;
    if (ba_check_tables(obs_off, T, n_obs, obs_image, img_off, img_obs, cam_free, n_images, F)) return -1;
    return ba_host_run(obs_off, T, n_obs, obs_image, obs_uv, img_off, img_obs, cam_free, n_images, F, K, R_in, t_in, X_in, thr, iters, R_out, t_out,
                       X_out, inliers, n_inliers, cost, accepted, lambda, status, 1, cg_iters, cg_tol, cg_used, cg_res);
}

}   // extern "C"
