// Stand-alone run of the host form of the covisibility rule on random graphs, for sanitizer builds of the rule's text:
//   c++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all covis_host.cpp covis_host_selftest.cpp -o t && ./t
// Buffers are exactly as large as the entry points say they must be, so a write past one is an error here.  It checks what needs no second
// implementation: a chain of 1024 is one cluster, 1025 is refused, clusters are numbered in ascending order of their smallest position,
// linked positions share a cluster, and with dedup the kept rows of a problem are distinct.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <utility>
#include <vector>

extern "C" int gf_covis_host_lists(const int32_t* pair_images, const int32_t* id_off, int P, const int32_t* image_q, int n_images, const int32_t* kp_off,
                                   const int32_t* pok, int Q, int32_t* pairs, int32_t* pair_row_off, int32_t* list_off, int32_t* list_img,
                                   int32_t* sorted_img, int32_t* sorted_pos, int32_t* sizes);
extern "C" int gf_covis_host_cluster(const int32_t* kp_off, int n_images, const int32_t* pok, int n_nodes, const int32_t* obs_offsets, int T,
                                     const int32_t* obs_image, int n_obs, const int32_t* list_off, const int32_t* list_img, const int32_t* sorted_img,
                                     const int32_t* sorted_pos, int Q, int L_total, int enable, int32_t* cluster, int32_t* n_clusters);
extern "C" int gf_covis_host_rows(const int32_t* pairs, const int32_t* pair_row_off, int C, int M0, const int32_t* ids, int E, const int32_t* kp_off,
                                  int n_images, const int32_t* pok, int n_nodes, int T, const int32_t* list_off, const int32_t* cluster, int L_total,
                                  const int32_t* prob_base, int Q, int N, int dedup, int32_t* row_kp, int32_t* row_pt, int32_t* row_prob,
                                  uint8_t* keep, int32_t* first_of, int32_t* slot, int32_t* sel, int32_t* prob_off, int32_t* sizes);
extern "C" void gf_covis_host_select(const int32_t* prob_base, int Q, int N, const int32_t* valid, const int32_t* n_inliers, const double* R,
                                     const double* t, const int32_t* rounds, const uint8_t* inliers, int M, const int32_t* row_prob,
                                     const int32_t* slot, int M0, int min_inliers, int32_t* winner, int32_t* localized, double* Rq, double* tq,
                                     int32_t* nin_q, int32_t* rounds_q, uint8_t* is_win, uint8_t* mask);

static uint64_t g_state = 12345;
static int below(int n) {                              // uniform in [0, n)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (int)((g_state >> 33) % (uint64_t)n);
}

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c);      \
            exit(1);                                                    \
        }                                                               \
    } while (0)

struct Graph {
    int n_images, Q, T;
    std::vector<int32_t> image_q, kp_off, pok, obs_off, obs_img, pair_images, id_off, ids;
};

// images 0 .. Q - 1 are the queries (4 keypoints, no point); a database image's keypoints are its observations, then one without a point
static Graph make(int Q, int n_db, const std::vector<std::vector<int>>& tracks, const std::vector<std::pair<int, int>>& pairs, int rows) {
    Graph g;
    g.n_images = Q + n_db; g.Q = Q; g.T = (int)tracks.size();
    g.image_q.assign((size_t)g.n_images, -1);
    for (int q = 0; q < Q; ++q) g.image_q[q] = q;
    std::vector<std::vector<int>> per((size_t)g.n_images);
    g.obs_off.push_back(0);
    for (int t = 0; t < g.T; ++t) {
        std::set<int> s(tracks[t].begin(), tracks[t].end());
        for (int i : s) { per[i].push_back(t); g.obs_img.push_back(i); }
        g.obs_off.push_back((int32_t)g.obs_img.size());
    }
    g.kp_off.push_back(0);
    for (int i = 0; i < g.n_images; ++i) {
        for (int t : per[i]) g.pok.push_back(t);
        for (int k = 0; k < (i < Q ? 4 : 1); ++k) g.pok.push_back(-1);
        g.kp_off.push_back((int32_t)g.pok.size());
    }
    g.id_off.push_back(0);
    for (auto& p : pairs) {
        g.pair_images.push_back(p.first); g.pair_images.push_back(p.second);
        for (int r = 0; r < rows; ++r) {
            g.ids.push_back(below(g.kp_off[p.first + 1] - g.kp_off[p.first]));
            g.ids.push_back(below(g.kp_off[p.second + 1] - g.kp_off[p.second]));
        }
        g.id_off.push_back((int32_t)(g.ids.size() / 2));
    }
    return g;
}

// the whole host chain on g with exact-size buffers; returns the number of clusters of query 0 (-2: the list was refused)
static int run(const Graph& g, int enable, int dedup) {
    const int P = (int)g.pair_images.size() / 2, Q = g.Q;
    std::vector<int32_t> pairs((size_t)8 * P), pro((size_t)P + 1), loff((size_t)Q + 1), limg((size_t)P), simg((size_t)P), spos((size_t)P), sizes(3);
    const int rc = gf_covis_host_lists(g.pair_images.data(), g.id_off.data(), P, g.image_q.data(), g.n_images, g.kp_off.data(), g.pok.data(), Q,
                                       pairs.data(), pro.data(), loff.data(), limg.data(), simg.data(), spos.data(), sizes.data());
    if (rc == -2) return -2;
    CHECK(rc == 0);
    const int C = sizes[0], M0 = sizes[1], Lt = sizes[2];
    limg.resize((size_t)Lt); simg.resize((size_t)Lt); spos.resize((size_t)Lt);
    std::vector<int32_t> cluster((size_t)Lt), ncl((size_t)Q);
    CHECK(gf_covis_host_cluster(g.kp_off.data(), g.n_images, g.pok.data(), (int)g.pok.size(), g.obs_off.data(), g.T, g.obs_img.data(),
                                (int)g.obs_img.size(), loff.data(), limg.data(), simg.data(), spos.data(), Q, Lt, enable, cluster.data(),
                                ncl.data()) == 0);
    std::vector<int32_t> prob_base((size_t)Q + 1, 0);
    for (int q = 0; q < Q; ++q) {
        const int b = loff[q], e = loff[q + 1];
        int next = 0;                                                   // ascending label order: a new number is the next one
        for (int i = b; i < e; ++i) {
            CHECK(cluster[i] >= 0 && cluster[i] <= next);
            if (cluster[i] == next) ++next;
        }
        CHECK(next == ncl[q] && (enable || next == (e > b)));
        prob_base[q + 1] = prob_base[q] + ncl[q];
        if (enable)                                                     // two listed images that share a point share a cluster
            for (int t = 0; t < g.T; ++t) {
                int first = -1;
                for (int o = g.obs_off[t]; o < g.obs_off[t + 1]; ++o)
                    for (int i = b; i < e; ++i)
                        if (limg[i] == g.obs_img[o]) {
                            if (first < 0) first = cluster[i];
                            CHECK(cluster[i] == first);
                        }
            }
    }
    const int N = prob_base[Q];
    std::vector<int32_t> kp((size_t)M0), pt((size_t)M0), prob((size_t)M0), first((size_t)M0), slot((size_t)M0), sel((size_t)M0), poff((size_t)N + 1), m(1);
    std::vector<uint8_t> keep((size_t)M0);
    CHECK(gf_covis_host_rows(pairs.data(), pro.data(), C, M0, g.ids.data(), (int)g.ids.size() / 2, g.kp_off.data(), g.n_images, g.pok.data(),
                             (int)g.pok.size(), g.T, loff.data(), cluster.data(), Lt, prob_base.data(), Q, N, dedup, kp.data(), pt.data(),
                             prob.data(), keep.data(), first.data(), slot.data(), sel.data(), poff.data(), m.data()) == 0);
    const int M = m[0];
    CHECK(poff[N] == M);
    std::set<std::pair<int, std::pair<int, int>>> seen;
    for (int k = 0; k < M; ++k) {
        const int r = sel[k];
        CHECK(r >= 0 && r < M0 && keep[r] && slot[r] == k && first[r] == r && (k == 0 || prob[sel[k - 1]] <= prob[r]));
        if (dedup) CHECK(seen.insert(std::make_pair(prob[r], std::make_pair(kp[r], pt[r]))).second);
    }
    for (int r = 0; r < M0; ++r) {
        CHECK((keep[r] != 0) == (first[r] >= 0) && (keep[r] != 0) == (slot[r] >= 0));
        if (keep[r]) CHECK(first[r] <= r && kp[first[r]] == kp[r] && pt[first[r]] == pt[r] && prob[first[r]] == prob[r] && (dedup || first[r] == r));
    }
    // steps 8 and 9 on made-up RANSAC outputs
    std::vector<int32_t> valid((size_t)N), nin((size_t)N), rounds((size_t)N), win((size_t)Q), loc((size_t)Q), ninq((size_t)Q), rq((size_t)Q);
    std::vector<double> R((size_t)9 * N, 1.0), t((size_t)3 * N, 2.0), Rq((size_t)9 * Q), tq((size_t)3 * Q);
    std::vector<uint8_t> inl((size_t)M), is_win((size_t)N), mask((size_t)M0);
    for (int k = 0; k < N; ++k) { valid[k] = below(4) != 0; nin[k] = below(30); rounds[k] = below(3); }
    for (int k = 0; k < M; ++k) inl[k] = (uint8_t)below(2);
    gf_covis_host_select(prob_base.data(), Q, N, valid.data(), nin.data(), R.data(), t.data(), rounds.data(), inl.data(), M, prob.data(), slot.data(),
                         M0, 12, win.data(), loc.data(), Rq.data(), tq.data(), ninq.data(), rq.data(), is_win.data(), mask.data());
    for (int q = 0; q < Q; ++q) {
        int best = -1;
        for (int k = prob_base[q]; k < prob_base[q + 1]; ++k)
            if (valid[k] && (best < 0 || nin[k] > nin[best])) best = k;
        CHECK(win[q] == (best < 0 ? -1 : best - prob_base[q]) && loc[q] == (best >= 0 && nin[best] >= 12));
    }
    for (int r = 0; r < M0; ++r) CHECK(mask[r] == (keep[r] && is_win[prob[r]] && inl[slot[r]]));
    return Q ? ncl[0] : 0;
}

static Graph chain(int L) {                              // one query, database images 1 .. L linked k - (k + 1), the far end paired first
    std::vector<std::vector<int>> tracks;
    for (int k = 1; k < L; ++k) tracks.push_back({k, k + 1});
    std::vector<std::pair<int, int>> pairs;
    for (int i = L; i >= 1; --i) pairs.push_back({0, i});
    return make(1, L, tracks, pairs, 1);
}

int main() {
    CHECK(run(chain(1024), 1, 1) == 1);
    CHECK(run(chain(1024), 0, 0) == 1);
    CHECK(run(chain(1025), 1, 0) == -2);
    CHECK(run(make(1, 2, {}, {}, 0), 1, 1) == 0);                       // no pairs
    int graphs = 0;
    for (int it = 0; it < 200; ++it) {
        const int Q = 1 + below(6), n_db = 1 + below(40), T = below(201);
        std::vector<std::vector<int>> tracks((size_t)T);
        for (auto& tr : tracks)
            for (int k = 2 + below(7); k > 0; --k) tr.push_back(Q + below(n_db));
        std::vector<std::pair<int, int>> pairs;
        for (int q = 0; q < Q; ++q)
            for (int k = 1 + below(n_db); k > 0; --k) {
                const int d = Q + below(n_db);
                pairs.push_back(below(2) ? std::make_pair(q, d) : std::make_pair(d, q));
            }
        pairs.push_back({Q, Q + n_db - 1});                             // a database - database pair contributes nothing
        const Graph g = make(Q, n_db, tracks, pairs, below(12));
        for (int mode = 0; mode < 4; ++mode) run(g, mode & 1, mode >> 1);
        ++graphs;
    }
    printf("covis host selftest ok: chains of 1024 and 1025, %d random graphs x 4 modes\n", graphs);
    return 0;
}
