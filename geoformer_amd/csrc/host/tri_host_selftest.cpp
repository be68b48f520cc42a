// Stand-alone run of the host form of the track building and the triangulation on planted scenes, for sanitizer builds of the solver text:
//   c++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tri_host.cpp tri_host_selftest.cpp -o t && ./t
// (cameras and points planted with a small LCG; libm is used HERE only, to plant the scenes).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

extern "C" int gf_tri_host_hyp_count(int L);
extern "C" int gf_tri_host_pair(uint32_t seed, uint32_t track, int t, int L, int32_t* out);
extern "C" int gf_tri_host_midpoint(const float* Ka, const double* Ra, const double* ta, const float* uva, const float* Kb, const double* Rb,
                                    const double* tb, const float* uvb, double cos_min, double* X);
extern "C" int gf_tri_host_label(const int32_t* ids, const int32_t* id_off, const int32_t* pair_images, int P, int E, const int32_t* kp_off,
                                 int n_images, int n_nodes, int32_t* parent);
extern "C" void gf_tri_host_tracks(const int32_t* parent, int n_nodes, const int32_t* kp_off, int n_images, int32_t* track_off, int32_t* obs_node,
                                   int32_t* obs_image, int32_t* obs_kp, int32_t* sizes);
extern "C" int gf_tri_host_triangulate(const int32_t* track_off, int T, int n_obs, const int32_t* obs_image, const float* obs_uv, const float* K,
                                       const double* R, const double* t, int n_images, float pixel_thr, double cos_min_angle, int min_obs,
                                       int refit, uint32_t seed, double* X, int32_t* valid, int32_t* conflict, int32_t* n_inliers,
                                       int32_t* hypothesis, int32_t* rounds, double* err2, uint8_t* inliers);

static uint64_t g_state;
static double uni() {                                  // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}
static double gauss() { return sqrt(-2.0 * log(1.0 - uni())) * cos(6.283185307179586 * uni()); }

static const int NCAM = 24;
static const double FOC = 800, CX = 800, CY = 600;
static const double COS_MIN = 0.99965732497555726;     // cos(1.5 deg)

// camera i on an arc of 8 units, looking along +z with a small rotation about y towards the scene's middle
static void camera(int i, double* R, double* t) {
    const double c[3] = {-4.0 + 8.0 * i / (NCAM - 1), uni() - 0.5, uni() - 0.5};
    const double th = atan2(-c[0], 7.0), s = sin(th), co = cos(th);
    const double Rm[9] = {co, 0, -s, 0, 1, 0, s, 0, co};
    for (int k = 0; k < 9; ++k) R[k] = Rm[k];
    for (int k = 0; k < 3; ++k) t[k] = -(Rm[3 * k] * c[0] + Rm[3 * k + 1] * c[1] + Rm[3 * k + 2] * c[2]);
}

static void project(const double* R, const double* t, const double* X, double* px) {
    double Y[3];
    for (int i = 0; i < 3; ++i) Y[i] = R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2] + t[i];
    px[0] = FOC * Y[0] / Y[2] + CX; px[1] = FOC * Y[1] / Y[2] + CY;
}

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

int main() {
    g_state = 1;
    std::vector<float> K(9 * NCAM, 0.f);
    std::vector<double> R(9 * NCAM), t(3 * NCAM);
    for (int i = 0; i < NCAM; ++i) {
        K[9 * i] = (float)FOC; K[9 * i + 2] = (float)CX; K[9 * i + 4] = (float)FOC; K[9 * i + 5] = (float)CY; K[9 * i + 8] = 1.f;
        camera(i, &R[9 * i], &t[3 * i]);
    }
    // ---- hypothesis pairs: every pair once up to 11, distinct draws above
    for (int L = 0; L <= 40; ++L) {
        const int H = gf_tri_host_hyp_count(L);
        CHECK(H == (L < 2 ? 0 : (L <= 11 ? L * (L - 1) / 2 : 64)), "L %d: %d hypotheses", L, H);
        int32_t prev[2] = {0, 0}, p[2];
        for (int h = 0; h < H; ++h) {
            CHECK(gf_tri_host_pair(7, 3, h, L, p) == 1 && p[0] >= 0 && p[1] >= 0 && p[0] < L && p[1] < L && p[0] != p[1], "L %d t %d: %d %d", L, h, p[0], p[1]);
            if (L <= 11 && h > 0) CHECK(p[0] < p[1] && (p[0] > prev[0] || (p[0] == prev[0] && p[1] == prev[1] + 1)), "L %d t %d not lexicographic", L, h);
            prev[0] = p[0]; prev[1] = p[1];
        }
        CHECK(gf_tri_host_pair(7, 3, H, L, p) == 0 && gf_tri_host_pair(7, 3, -1, L, p) == 0, "L %d: a hypothesis past the last", L);
    }
    // ---- the two-view solver and its clean failures
    {
        const double X[3] = {0.3, -0.4, 7.0};
        double a[2], b[2], out[3];
        project(&R[0], &t[0], X, a);
        project(&R[9 * 15], &t[3 * 15], X, b);
        const float fa[2] = {(float)a[0], (float)a[1]}, fb[2] = {(float)b[0], (float)b[1]}, nanpx[2] = {NAN, 5.f};
        CHECK(gf_tri_host_midpoint(&K[0], &R[0], &t[0], fa, &K[0], &R[9 * 15], &t[3 * 15], fb, COS_MIN, out) == 1 &&
              fabs(out[0] - X[0]) + fabs(out[1] - X[1]) + fabs(out[2] - X[2]) < 1e-4, "exact recovery: %g %g %g", out[0], out[1], out[2]);
        CHECK(gf_tri_host_midpoint(&K[0], &R[0], &t[0], fa, &K[0], &R[0], &t[0], fa, COS_MIN, out) == 0, "equal camera centres");
        CHECK(gf_tri_host_midpoint(&K[0], &R[0], &t[0], fa, &K[0], &R[9 * 15], &t[3 * 15], fb, -1.0, out) == 0, "every angle below the threshold");
        CHECK(gf_tri_host_midpoint(&K[0], &R[0], &t[0], nanpx, &K[0], &R[9 * 15], &t[3 * 15], fb, COS_MIN, out) == 0, "NaN pixel");
        double tn[3] = {NAN, 0, 0};
        CHECK(gf_tri_host_midpoint(&K[0], &R[0], tn, fa, &K[0], &R[9 * 15], &t[3 * 15], fb, COS_MIN, out) == 0, "NaN pose");
    }
    // ---- labelling and the track list: a chain listed backwards, a star, a self-loop, duplicates, a row out of range, an empty image
    {
        const int n_images = 60;
        std::vector<int32_t> kp_off(n_images + 1);
        for (int i = 0; i <= n_images; ++i) kp_off[i] = i <= 50 ? i : 50 + 3 * (i - 51);      // one keypoint each, image 50 empty, then three each
        const int n_nodes = kp_off[n_images];
        std::vector<int32_t> ids, id_off(1, 0), pim;
        for (int i = 48; i >= 0; --i) { pim.push_back(i); pim.push_back(i + 1); ids.push_back(0); ids.push_back(0); id_off.push_back((int)ids.size() / 2); }
        pim.push_back(51); pim.push_back(52);
        const int32_t rows[] = {0, 0, 0, 1, 0, 1, 0, 2, 2, 2, 5, 0, 0, -1};          // a star from (51, 0), a duplicate, two rows out of range
        for (int32_t v : rows) ids.push_back(v);
        id_off.push_back((int)ids.size() / 2);
        pim.push_back(53); pim.push_back(53); ids.push_back(1); ids.push_back(1); id_off.push_back((int)ids.size() / 2);      // a self-loop
        const int P = (int)pim.size() / 2, E = (int)ids.size() / 2;
        std::vector<int32_t> parent(n_nodes), toff(n_nodes + 2), node(n_nodes), img(n_nodes), kp(n_nodes);
        int32_t sizes[2];
        const int st = gf_tri_host_label(ids.data(), id_off.data(), pim.data(), P, E, kp_off.data(), n_images, n_nodes, parent.data());
        gf_tri_host_tracks(parent.data(), n_nodes, kp_off.data(), n_images, toff.data(), node.data(), img.data(), kp.data(), sizes);
        int chain = 1;
        for (int v = 0; v < 50; ++v) chain &= parent[v] == 0;
        CHECK(st == 1 && chain && sizes[0] == 2 && sizes[1] == 55 && toff[1] == 50 && toff[2] == 55, "status %d chain %d tracks %d obs %d", st, chain, sizes[0], sizes[1]);
        CHECK(node[50] == 50 && node[51] == 52 && node[52] == 53 && node[53] == 54 && node[54] == 55 && img[51] == 51 && img[52] == 52 && kp[53] == 1 && parent[57] == 57,
              "the star: %d %d %d %d", node[50], node[51], node[52], node[53]);
        CHECK(gf_tri_host_label(ids.data(), id_off.data(), pim.data(), P, -1, kp_off.data(), n_images, n_nodes, parent.data()) == -1, "E < 0");
        gf_tri_host_tracks(parent.data(), 0, kp_off.data(), 0, toff.data(), node.data(), img.data(), kp.data(), sizes);
        CHECK(sizes[0] == 0 && sizes[1] == 0, "no nodes");
    }
    // ---- triangulation: every length on both sides of the switch to draws, outliers, a conflict, a pose-less image, refit 0 .. 8
    {
        const int lengths[] = {2, 3, 5, 8, 11, 12, 13, 20, 24, 2, 3, 3};
        const int T = (int)(sizeof lengths / sizeof lengths[0]);
        std::vector<int32_t> toff(1, 0), img;
        std::vector<float> uv;
        std::vector<uint8_t> planted;
        std::vector<double> Xp;
        for (int k = 0; k < T; ++k) {
            const double X[3] = {4 * uni() - 2, 3 * uni() - 1.5, 5 + 4 * uni()};
            const int L = lengths[k], step = NCAM / L;
            for (int j = 0; j < L; ++j) {
                const int c = j * step + (int)(uni() * step);
                double px[2];
                project(&R[9 * c], &t[3 * c], X, px);
                const int bad = L >= 5 && j % 5 == 2;
                img.push_back(c);
                uv.push_back((float)(bad ? 1600 * uni() : px[0] + 0.5 * gauss()));
                uv.push_back((float)(bad ? 1200 * uni() : px[1] + 0.5 * gauss()));
                planted.push_back(!bad);
            }
            toff.push_back((int)img.size());
            for (int i = 0; i < 3; ++i) Xp.push_back(X[i]);
        }
        const int n_obs = (int)img.size();
        img[toff[10] + 1] = img[toff[10]];                               // track 10: an image twice
        std::vector<double> Rn(R);
        const int lost = img[toff[9]];
        for (int k = 0; k < 9; ++k) Rn[9 * lost + k] = NAN;              // track 9 (length 2) keeps one effective observation
        std::vector<double> X0(3 * T);
        std::vector<int32_t> nin0(T), hyp0(T);
        for (int refit = 0; refit <= 8; ++refit) {
            std::vector<double> X(3 * T), err2(T);
            std::vector<int32_t> valid(T), conflict(T), nin(T), hyp(T), rounds(T);
            std::vector<uint8_t> inl(n_obs);
            const int rc = gf_tri_host_triangulate(toff.data(), T, n_obs, img.data(), uv.data(), K.data(), Rn.data(), t.data(), NCAM, 4.f, COS_MIN, 2,
                                                   refit, 0x5EED, X.data(), valid.data(), conflict.data(), nin.data(), hyp.data(), rounds.data(),
                                                   err2.data(), inl.data());
            CHECK(rc == 0, "refit %d: rc %d", refit, rc);
            if (refit == 0) { X0 = X; nin0 = nin; hyp0 = hyp; }
            int kept_outliers = 0;
            double worst = 0;
            for (int k = 0; k < T; ++k) {
                int cnt = 0;
                for (int i = toff[k]; i < toff[k + 1]; ++i) {
                    cnt += inl[i];
                    kept_outliers += inl[i] && !planted[i] && k != 10;
                    CHECK(!inl[i] || img[i] != lost, "a pose-less observation is an inlier");
                }
                CHECK(conflict[k] == (k == 10) && valid[k] == (k != 9 && k != 10), "track %d refit %d: conflict %d valid %d", k, refit, conflict[k], valid[k]);
                CHECK(cnt == (valid[k] ? nin[k] : 0) && nin[k] >= nin0[k] && hyp[k] == hyp0[k] && rounds[k] >= 0 && rounds[k] <= refit,
                      "track %d refit %d: mask %d inliers %d (midpoint %d) rounds %d", k, refit, cnt, nin[k], nin0[k], rounds[k]);
                CHECK(rounds[k] > 0 || (X[3 * k] == X0[3 * k] && X[3 * k + 1] == X0[3 * k + 1] && X[3 * k + 2] == X0[3 * k + 2]), "track %d: rounds 0 but not the midpoint", k);
                if (valid[k]) {
                    const double e = sqrt(pow(X[3 * k] - Xp[3 * k], 2) + pow(X[3 * k + 1] - Xp[3 * k + 1], 2) + pow(X[3 * k + 2] - Xp[3 * k + 2], 2));
                    worst = fmax(worst, e);
                    CHECK(err2[k] >= 0 && err2[k] < 16.0, "track %d: err2 %g", k, err2[k]);
                } else {
                    CHECK(X[3 * k] == 0 && X[3 * k + 1] == 0 && X[3 * k + 2] == 0 && err2[k] == 0, "track %d is not valid but has a point", k);
                }
            }
            CHECK(kept_outliers == 0 && worst < 0.25, "refit %d: %d outliers kept, worst 3-D error %g", refit, kept_outliers, worst);
            printf("triangulate refit %d: worst 3-D error %.4f units over %d tracks\n", refit, worst, T);
        }
        std::vector<double> X(3 * T), err2(T);
        std::vector<int32_t> a(T), b(T), c(T), d(T), e(T);
        std::vector<uint8_t> inl(n_obs);
        for (int which = 0; which < 5; ++which) {
            const int rc = gf_tri_host_triangulate(toff.data(), which == 4 ? -1 : T, n_obs, img.data(), uv.data(), K.data(), R.data(), t.data(), NCAM,
                                                   which == 0 ? 0.f : 4.f, which == 1 ? (double)NAN : COS_MIN, which == 2 ? 1 : 2, which == 3 ? 9 : 0, 1,
                                                   X.data(), a.data(), b.data(), c.data(), d.data(), e.data(), err2.data(), inl.data());
            CHECK(rc == -1, "argument error %d: rc %d", which, rc);
        }
        CHECK(gf_tri_host_triangulate(toff.data(), 0, 0, nullptr, nullptr, K.data(), R.data(), t.data(), NCAM, 4.f, COS_MIN, 2, 0, 1, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0, "zero tracks");
        // offsets past the buffers are clamped, not followed
        int32_t wild[3] = {-5, 3, 1 << 30};
        CHECK(gf_tri_host_triangulate(wild, 2, n_obs, img.data(), uv.data(), K.data(), R.data(), t.data(), NCAM, 4.f, COS_MIN, 2, 2, 1, X.data(), a.data(),
                                      b.data(), c.data(), d.data(), e.data(), err2.data(), inl.data()) == 0, "wild offsets");
    }
    printf(g_fail ? "%d check(s) FAILED\n" : "all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
}
