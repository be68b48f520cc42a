// TEST INFRASTRUCTURE and CPU reference: the serial host form of the covisibility clustering, the 2-D - 3-D rows and the choice of the
// winning cluster of k_covis.hip, compiled from the same covis_spec.h by the host C++ compiler (geoformer_amd/build.py, no offload) into
// csrc/_obj/libcovis_host.so.  The tests compare the device against it byte for byte; nothing in the package loads it.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <utility>
#include <vector>

#include "../covis_spec.h"

extern "C" {

// Step 1 from the pair list: image_q [n_images] = the query index of an image, -1 for a database image.  Outputs: pairs [P][8] and
// pair_row_off [P + 1] (the contributing pairs in pair order), list_off [Q + 1], list_img / sorted_img / sorted_pos [P] at most, sizes [3] =
// C, M0, L_total.  Returns 0, -1 for bad arguments (an image outside [0, n_images) included), -2 for a list above CV_MAX_LIST.
int gf_covis_host_lists(const int32_t* pair_images, const int32_t* id_off, int P, const int32_t* image_q, int n_images, const int32_t* kp_off,
                        const int32_t* pok, int Q, int32_t* pairs, int32_t* pair_row_off, int32_t* list_off, int32_t* list_img,
                        int32_t* sorted_img, int32_t* sorted_pos, int32_t* sizes) {
    if (P < 0 || Q < 0 || n_images < 0) return -1;
    std::vector<char> has_pts((size_t)n_images, 0);
    for (int i = 0; i < n_images; ++i)
        for (int k = kp_off[i]; k < kp_off[i + 1]; ++k)
            if (pok[k] >= 0) { has_pts[i] = 1; break; }
    std::vector<std::vector<int32_t>> lists((size_t)Q);
    std::vector<std::map<int32_t, int32_t>> where((size_t)Q);
    int C = 0;
    long rows = 0;
    pair_row_off[0] = 0;
    for (int p = 0; p < P; ++p) {
        const int i = pair_images[2 * p], j = pair_images[2 * p + 1];
        if (i < 0 || i >= n_images || j < 0 || j >= n_images) return -1;
        for (int side = 0; side < 2; ++side) {
            const int qs = side ? j : i, ds = side ? i : j;
            if (image_q[qs] < 0 || image_q[qs] >= Q || image_q[ds] >= 0 || !has_pts[ds]) continue;
            const int q = image_q[qs];
            auto it = where[q].find(ds);
            if (it == where[q].end()) {
                it = where[q].insert(std::make_pair((int32_t)ds, (int32_t)lists[q].size())).first;
                lists[q].push_back(ds);
            }
            int32_t* o = pairs + (size_t)CV_PAIR_WORDS * C;
            o[CV_Q] = q; o[CV_QIMG] = qs; o[CV_DIMG] = ds; o[CV_RB] = id_off[p]; o[CV_RE] = id_off[p + 1]; o[CV_QCOL] = side; o[CV_POS] = it->second;
            o[7] = 0;
            rows += (long)id_off[p + 1] - id_off[p];
            if (rows > 0x7FFFFFFFl) return -1;
            pair_row_off[++C] = (int32_t)rows;
            break;
        }
    }
    int n = 0;
    list_off[0] = 0;
    for (int q = 0; q < Q; ++q) {
        const int L = (int)lists[q].size();
        if (L > CV_MAX_LIST) return -2;
        std::vector<std::pair<int32_t, int32_t>> s;
        for (int a = 0; a < L; ++a) s.push_back(std::make_pair(lists[q][a], (int32_t)a));
        std::sort(s.begin(), s.end());
        for (int a = 0; a < L; ++a) {
            list_img[n + a] = lists[q][a];
            sorted_img[n + a] = s[a].first;
            sorted_pos[n + a] = s[a].second;
        }
        n += L;
        list_off[q + 1] = n;
    }
    sizes[0] = C; sizes[1] = (int32_t)rows; sizes[2] = n;
    return 0;
}

// Steps 2 and 3 as gf_covis_cluster writes them.  Returns the status bits, -1 for arguments the device entry point rejects (-2: a list
// above CV_MAX_LIST).
int gf_covis_host_cluster(const int32_t* kp_off, int n_images, const int32_t* pok, int n_nodes, const int32_t* obs_offsets, int T,
                          const int32_t* obs_image, int n_obs, const int32_t* list_off, const int32_t* list_img, const int32_t* sorted_img,
                          const int32_t* sorted_pos, int Q, int L_total, int enable, int32_t* cluster, int32_t* n_clusters) {
    if (Q < 0 || L_total < 0 || n_images < 0 || n_nodes < 0 || T < 0 || n_obs < 0) return -1;
    if (Q == 0) return 0;
    if (list_off[0] != 0 || list_off[Q] != L_total) return -1;
    for (int q = 0; q < Q; ++q) {
        if (list_off[q + 1] < list_off[q]) return -1;
        if (list_off[q + 1] - list_off[q] > CV_MAX_LIST) return -2;
    }
    for (int i = 0; i < L_total; ++i)
        if (list_img[i] < 0 || list_img[i] >= n_images) return -1;
    const CvView v{kp_off, pok, obs_offsets, obs_image, n_images, n_nodes, T, n_obs};
    int flags = 0;
    std::vector<int32_t> parent(CV_MAX_LIST), spos(CV_MAX_LIST);
    for (int q = 0; q < Q; ++q) {
        const int base = list_off[q], L = list_off[q + 1] - base;
        for (int i = 0; i < L; ++i) {
            parent[i] = i;
            spos[i] = cv_clamp(sorted_pos[base + i], 0, L - 1);
            if (sorted_pos[base + i] < 0 || sorted_pos[base + i] >= L) flags |= CV_FLAG_LIST_RANGE;
        }
        auto root = [&](int x) {
            while (parent[x] != x) x = parent[x];
            return x;
        };
        auto unite = [&](int a, int b) {
            const int ra = root(a), rb = root(b);
            if (ra != rb) parent[ra > rb ? ra : rb] = ra > rb ? rb : ra;
        };
        if (enable && !(flags & CV_FLAG_LIST_RANGE))
            for (int a = 0; a < L; ++a) {
                const int img = list_img[base + a];
                const int nb = cv_clamp(kp_off[img], 0, n_nodes), ne = cv_clamp(kp_off[img + 1], nb, n_nodes);
                for (int node = nb; node < ne; ++node) flags |= cv_point_star(v, sorted_img + base, spos.data(), L, a, node, unite);
            }
        int C = 0;
        std::vector<int32_t> number((size_t)L, 0);
        for (int i = 0; i < L; ++i) {                                  // ascending: the root of i is numbered before i is
            const int r = enable ? root(i) : 0;
            if (r == i) number[i] = C++;
            cluster[base + i] = number[r];
        }
        n_clusters[q] = C;
    }
    return flags;
}

// Steps 4 and 5 as gf_sparse_rows and the ordering behind it write them.  Per original row r (M0 of them): row_kp, row_pt, row_prob, keep,
// first_of (an original row; -1: dropped in step 4), slot (the RANSAC row of first_of[r]; -1).  sel [M0] at most: the original rows of the
// RANSAC rows in order; prob_off [N + 1]; sizes [1] = M.  Returns the status bits, or -1 for arguments the device entry point rejects.
int gf_covis_host_rows(const int32_t* pairs, const int32_t* pair_row_off, int C, int M0, const int32_t* ids, int E, const int32_t* kp_off,
                       int n_images, const int32_t* pok, int n_nodes, int T, const int32_t* list_off, const int32_t* cluster, int L_total,
                       const int32_t* prob_base, int Q, int N, int dedup, int32_t* row_kp, int32_t* row_pt, int32_t* row_prob, uint8_t* keep,
                       int32_t* first_of, int32_t* slot, int32_t* sel, int32_t* prob_off, int32_t* sizes) {
    if (C < 0 || M0 < 0 || E < 0 || n_images < 0 || n_nodes < 0 || T < 0 || L_total < 0 || Q < 0 || N < 0) return -1;
    for (int k = 0; k <= N; ++k) prob_off[k] = 0;
    sizes[0] = 0;
    if (M0 == 0) return 0;
    if (C == 0 || Q == 0) return -1;
    long rows = 0;
    for (int c = 0; c < C; ++c) {
        const int32_t* p = pairs + (size_t)CV_PAIR_WORDS * c;
        if (p[CV_Q] < 0 || p[CV_Q] >= Q || p[CV_QIMG] < 0 || p[CV_QIMG] >= n_images || p[CV_DIMG] < 0 || p[CV_DIMG] >= n_images) return -1;
        if (p[CV_RB] < 0 || p[CV_RE] < p[CV_RB] || p[CV_RE] > E || (p[CV_QCOL] != 0 && p[CV_QCOL] != 1)) return -1;
        if (p[CV_POS] < 0 || p[CV_POS] >= CV_MAX_LIST) return -1;
        rows += (long)p[CV_RE] - p[CV_RB];
    }
    if (rows != M0) return -1;
    const CvView v{kp_off, pok, nullptr, nullptr, n_images, n_nodes, T, 0};
    int flags = 0;
    std::vector<std::vector<int32_t>> of_prob((size_t)N);
    for (int r = 0; r < M0; ++r) {
        int qnode, pt, prob;
        keep[r] = (uint8_t)cv_row(pairs, pair_row_off, C, ids, E, v, list_off, cluster, L_total, prob_base, Q, r, qnode, pt, prob, flags);
        row_kp[r] = qnode; row_pt[r] = pt; row_prob[r] = prob;
        first_of[r] = slot[r] = -1;
        if (keep[r] && prob >= 0 && prob < N) of_prob[prob].push_back(r);
    }
    int M = 0;
    for (int k = 0; k < N; ++k) {
        std::map<std::pair<int32_t, int32_t>, int32_t> seen;            // (query keypoint, point) -> the first row that had it
        for (int32_t r : of_prob[k]) {
            int32_t first = r;
            if (dedup) {
                auto ins = seen.insert(std::make_pair(std::make_pair(row_kp[r], row_pt[r]), r));
                first = ins.first->second;
            }
            first_of[r] = first;
            if (first == r) {
                sel[M] = r;
                slot[r] = M++;
            } else {
                slot[r] = slot[first];
            }
        }
        prob_off[k + 1] = M;
    }
    sizes[0] = M;
    return flags;
}

// Steps 8 and 9 as gf_covis_select writes them.
void gf_covis_host_select(const int32_t* prob_base, int Q, int N, const int32_t* valid, const int32_t* n_inliers, const double* R, const double* t,
                          const int32_t* rounds, const uint8_t* inliers, int M, const int32_t* row_prob, const int32_t* slot, int M0,
                          int min_inliers, int32_t* winner, int32_t* localized, double* Rq, double* tq, int32_t* nin_q, int32_t* rounds_q,
                          uint8_t* is_win, uint8_t* mask) {
    for (int k = 0; k < N; ++k) is_win[k] = 0;
    for (int q = 0; q < Q; ++q) {
        const int b = cv_clamp(prob_base[q], 0, N), e = cv_clamp(prob_base[q + 1], b, N);
        const int w = cv_select(valid, n_inliers, b, e);
        winner[q] = w < 0 ? -1 : w - b;
        localized[q] = w >= 0 && n_inliers[w] >= min_inliers;
        nin_q[q] = w < 0 ? 0 : n_inliers[w];
        rounds_q[q] = w < 0 ? 0 : rounds[w];
        for (int i = 0; i < 9; ++i) Rq[9 * (size_t)q + i] = w < 0 ? 0.0 : R[9 * (size_t)w + i];
        for (int i = 0; i < 3; ++i) tq[3 * (size_t)q + i] = w < 0 ? 0.0 : t[3 * (size_t)w + i];
        if (w >= 0) is_win[w] = 1;
    }
    for (int r = 0; r < M0; ++r) mask[r] = cv_mask(is_win, inliers, N, M, row_prob[r], slot[r]);
}

}   // extern "C"
