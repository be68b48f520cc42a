// TEST INFRASTRUCTURE and CPU reference: the serial host form of the track building and the triangulation of k_triangulate.hip, compiled
// from the same tri_solver.h by the host C++ compiler (geoformer_amd/build.py: -O2 -ffp-contract=off, no offload) into
// csrc/_obj/libtri_host.so.  The tests compare the device against it bit for bit; nothing in the package loads it.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../tri_solver.h"

extern "C" {

int gf_tri_host_hyp_count(int L) { return tr_hyp_count(L); }

// the two positions of hypothesis t of `track` among L effective observations -> out [2]; returns 0 when there is none
int gf_tri_host_pair(uint32_t seed, uint32_t track, int t, int L, int32_t* out) {
    int a, b;
    const int ok = tr_hyp_pair(seed, track, t, L, a, b);
    out[0] = a; out[1] = b;
    return ok;
}

// step 5 for two observations: K fp32 [9], R [9], t [3], uv [2] (fp32 pixels) of each side -> X [3]; returns 0 when there is no solution
int gf_tri_host_midpoint(const float* Ka, const double* Ra, const double* ta, const float* uva, const float* Kb, const double* Rb,
                         const double* tb, const float* uvb, double cos_min, double* X) {
    double oa[3], ob[3], da[3], db[3], Xo[3] = {0.0, 0.0, 0.0};
    X[0] = X[1] = X[2] = 0.0;
    if (!tr_cam_ok(Ka, Ra, ta) || !tr_cam_ok(Kb, Rb, tb)) return 0;
    tr_centre(Ra, ta, oa);
    tr_centre(Rb, tb, ob);
    tr_dir(Ka, Ra, (double)uva[0], (double)uva[1], da);
    tr_dir(Kb, Rb, (double)uvb[0], (double)uvb[1], db);
    const int ok = tr_midpoint(oa, da, ob, db, cos_min, Xo);
    if (ok)
        for (int k = 0; k < 3; ++k) X[k] = Xo[k];
    return ok;
}

// steps 1 and 2, first half: plain union-find with the smallest node as the root -> parent [n_nodes] = the root of every node.  Returns the
// status bits (TR_FLAG_EDGE_RANGE when a row was skipped), or -1 for arguments gf_track_link rejects.
int gf_tri_host_label(const int32_t* ids, const int32_t* id_off, const int32_t* pair_images, int P, int E, const int32_t* kp_off,
                      int n_images, int n_nodes, int32_t* parent) {
    if (P < 0 || E < 0 || n_images < 0 || n_nodes < 0) return -1;
    int status = 0;
    for (int v = 0; v < n_nodes; ++v) parent[v] = v;
    auto root = [&](int x) {
        while (parent[x] != x) x = parent[x];
        return x;
    };
    for (int e = 0; e < E; ++e) {
        int u, v;
        if (!tr_edge_nodes(ids, id_off, pair_images, P, kp_off, n_images, n_nodes, e, u, v)) {
            status |= TR_FLAG_EDGE_RANGE;
            continue;
        }
        const int a = root(u), b = root(v);
        if (a != b) parent[a > b ? a : b] = a > b ? b : a;
    }
    for (int v = 0; v < n_nodes; ++v) parent[v] = root(v);            // (ascending: the parent of v is already a root)
    return status;
}

// step 2, second half: parent (every node's root, the component's smallest node) -> tracks in ascending order of their root, observations
// ascending.  track_off [n_nodes / 2 + 1], obs_node / obs_image / obs_kp [n_nodes] at most; sizes [2] = T, n_obs.
void gf_tri_host_tracks(const int32_t* parent, int n_nodes, const int32_t* kp_off, int n_images, int32_t* track_off, int32_t* obs_node,
                        int32_t* obs_image, int32_t* obs_kp, int32_t* sizes) {
    std::vector<int32_t> count((size_t)n_nodes, 0), start((size_t)n_nodes, 0);
    for (int v = 0; v < n_nodes; ++v) ++count[parent[v]];
    int T = 0, n = 0;
    track_off[0] = 0;
    for (int r = 0; r < n_nodes; ++r)
        if (count[r] >= 2) {
            start[r] = n;
            n += count[r];
            track_off[++T] = n;
        }
    std::vector<int32_t> fill((size_t)n_nodes, 0);
    int img = 0;
    for (int v = 0; v < n_nodes; ++v) {
        while (img + 1 < n_images && kp_off[img + 1] <= v) ++img;     // the last image whose first node is <= v
        const int r = parent[v];
        if (count[r] < 2) continue;
        const int o = start[r] + fill[r]++;
        obs_node[o] = v; obs_image[o] = img; obs_kp[o] = v - kp_off[img];
    }
    sizes[0] = T; sizes[1] = n;
}

// steps 3 - 9 as gf_triangulate writes them.  Returns 0, or -1 (GF_ERR_INVALID_ARGUMENT) for arguments the device entry point rejects.
int gf_tri_host_triangulate(const int32_t* track_off, int T, int n_obs, const int32_t* obs_image, const float* obs_uv, const float* K,
                            const double* R, const double* t, int n_images, float pixel_thr, double cos_min_angle, int min_obs, int refit,
                            uint32_t seed, double* X, int32_t* valid, int32_t* conflict, int32_t* n_inliers, int32_t* hypothesis,
                            int32_t* rounds, double* err2, uint8_t* inliers) {
    if (T < 0 || T > 0x7FFFFFFF / TR_MAX_HYP || n_obs < 0 || n_images < 0) return -1;
    if (!(pixel_thr > 0.f && pixel_thr < INFINITY) || !(cos_min_angle == cos_min_angle) || min_obs < 2) return -1;
    if (refit < 0 || refit > TR_REFIT_MAX_ROUNDS) return -1;
    if (T == 0) return 0;
    if (n_images <= 0 || n_obs <= 0) return -1;
    std::vector<int32_t> cam_ok((size_t)n_images);
    std::vector<double> cam_o(3 * (size_t)n_images);
    for (int i = 0; i < n_images; ++i) {
        double o[3];
        tr_centre(R + 9 * (size_t)i, t + 3 * (size_t)i, o);
        cam_ok[i] = tr_cam_ok(K + 9 * (size_t)i, R + 9 * (size_t)i, t + 3 * (size_t)i);
        for (int k = 0; k < 3; ++k) cam_o[3 * (size_t)i + k] = o[k];
    }
    TrView v;
    v.obs_image = obs_image; v.obs_uv = obs_uv; v.K = K; v.R = R; v.t = t; v.cam_ok = cam_ok.data(); v.cam_o = cam_o.data();
    v.n_images = n_images; v.thr2 = (double)pixel_thr * (double)pixel_thr; v.cos_min = cos_min_angle; v.min_obs = min_obs; v.refit = refit;
    v.seed = seed;
    double ws[TR_GN_WS_DOUBLES];
    for (int i = 0; i < TR_GN_WS_DOUBLES; ++i) ws[i] = 0.0;
    const GsWs w{ws, 1};
    for (int k = 0; k < T; ++k) {
        long b = track_off[k], e = track_off[k + 1];
        b = b < 0 ? 0 : (b > n_obs ? n_obs : b);
        e = e < b ? b : (e > n_obs ? n_obs : e);
        int L, cf;
        tr_track_scan(v, b, e, L, cf);
        const int H = cf ? 0 : tr_hyp_count(L);
        int best_cnt = -1, best_t = -1;
        for (int h = 0; h < H; ++h) {
            const int c = tr_hypothesis(v, (uint32_t)k, b, e, L, h);
            if (c > best_cnt) { best_cnt = c; best_t = h; }           // most inliers, then the smallest hypothesis
        }
        conflict[k] = cf;
        tr_track_finish(v, (uint32_t)k, b, e, L, cf, best_t, w, X + 3 * (size_t)k, valid + k, n_inliers + k, hypothesis + k, rounds + k, err2 + k,
                        inliers);
    }
    return 0;
}

}   // extern "C"
