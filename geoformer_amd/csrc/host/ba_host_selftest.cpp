// Stand-alone run of the host form of the bundle adjustment on planted scenes, for sanitizer builds of the rule's text:
//   c++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all ba_host.cpp ba_host_selftest.cpp -o t && ./t
// (cameras and points planted with a small LCG; libm is used HERE only, to plant the scenes).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

extern "C" int gf_ba_host_adjust(const int32_t* obs_off, int T, int n_obs, const int32_t* obs_image, const float* obs_uv, const int32_t* img_off,
                                 const int32_t* img_obs, const int32_t* cam_free, int n_images, int F, const float* K, const double* R_in,
                                 const double* t_in, const double* X_in, float thr, int iters, double* R_out, double* t_out, double* X_out,
                                 uint8_t* inliers, int32_t* n_inliers, double* cost, int32_t* accepted, double* lambda, int32_t* status);
extern "C" int gf_ba_host_adjust_pcg(const int32_t* obs_off, int T, int n_obs, const int32_t* obs_image, const float* obs_uv, const int32_t* img_off,
                                     const int32_t* img_obs, const int32_t* cam_free, int n_images, int F, const float* K, const double* R_in,
                                     const double* t_in, const double* X_in, float thr, int iters, int cg_iters, double cg_tol, double* R_out,
                                     double* t_out, double* X_out, uint8_t* inliers, int32_t* n_inliers, double* cost, int32_t* accepted,
                                     double* lambda, int32_t* status, int32_t* cg_used, double* cg_res);

static uint64_t g_state;
static double uni() {                                  // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}
static double gauss() { return sqrt(-2.0 * log(1.0 - uni())) * cos(6.283185307179586 * uni()); }

static const double FOC = 500, CX = 320, CY = 240;
static int g_fail = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++g_fail; } \
    } while (0)

struct Scene {
    int n, T;
    std::vector<float> K, uv;
    std::vector<double> R, t, Rtrue, ttrue, X;
    std::vector<int32_t> off, img, img_off, img_obs, cam_free;
    int F;
};

// the image-major index: a stable counting sort
static void index_images(Scene& s) {
    s.img_off.assign((size_t)s.n + 1, 0);
    for (int32_t i : s.img) ++s.img_off[(size_t)i + 1];
    for (int i = 0; i < s.n; ++i) s.img_off[(size_t)i + 1] += s.img_off[i];
    s.img_obs.resize(s.img.size());
    std::vector<int32_t> fill(s.img_off.begin(), s.img_off.end() - 1);
    for (size_t o = 0; o < s.img.size(); ++o) s.img_obs[fill[s.img[o]]++] = (int32_t)o;
}

// rotation about y by th, then a small rotation about x by ph
static void rot(double th, double ph, double* R) {
    const double s = sin(th), c = cos(th), sp = sin(ph), cp = cos(ph);
    const double Ry[9] = {c, 0, -s, 0, 1, 0, s, 0, c}, Rx[9] = {1, 0, 0, 0, cp, -sp, 0, sp, cp};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = Rx[3 * i] * Ry[j] + Rx[3 * i + 1] * Ry[3 + j] + Rx[3 * i + 2] * Ry[6 + j];
}

// n cameras on an arc looking at the points, `fixed_ends` of them fixed at their true poses, the rest perturbed; poseless: an image of NaN
static Scene plant(uint64_t seed, int n, int T, double noise, double rot_err, int fixed_ends, int poseless, double outliers) {
    g_state = seed;
    Scene s;
    s.n = n; s.T = 0;
    s.K.assign(9 * (size_t)n, 0.f);
    s.R.resize(9 * (size_t)n); s.t.resize(3 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        float* K = &s.K[9 * (size_t)i];
        K[0] = (float)FOC; K[2] = (float)CX; K[4] = (float)FOC; K[5] = (float)CY; K[8] = 1.f;
        const double c[3] = {-3.0 + 6.0 * i / (n > 1 ? n - 1 : 1), 0.3 * (uni() - 0.5), 0.3 * (uni() - 0.5)};
        double R[9];
        rot(atan2(-c[0], 6.0), 0.0, R);
        for (int k = 0; k < 9; ++k) s.R[9 * (size_t)i + k] = R[k];
        for (int k = 0; k < 3; ++k) s.t[3 * (size_t)i + k] = -(R[3 * k] * c[0] + R[3 * k + 1] * c[1] + R[3 * k + 2] * c[2]);
    }
    s.Rtrue = s.R; s.ttrue = s.t;
    s.off.push_back(0);
    for (int p = 0; p < T; ++p) {
        const double X[3] = {4.0 * (uni() - 0.5), 3.0 * (uni() - 0.5), 4.0 + 4.0 * uni()};
        size_t first = s.img.size();
        for (int i = 0; i < n; ++i) {
            const double* R = &s.R[9 * (size_t)i];
            double Y[3];
            for (int k = 0; k < 3; ++k) Y[k] = R[3 * k] * X[0] + R[3 * k + 1] * X[1] + R[3 * k + 2] * X[2] + s.t[3 * (size_t)i + k];
            double u = FOC * Y[0] / Y[2] + CX + noise * gauss(), v = FOC * Y[1] / Y[2] + CY + noise * gauss();
            if (!(Y[2] > 0) || u < 0 || u >= 640 || v < 0 || v >= 480 || uni() < 0.25) continue;
            if (uni() < outliers) { u += 40.0; v -= 30.0; }
            s.img.push_back(i); s.uv.push_back((float)u); s.uv.push_back((float)v);
        }
        if (s.img.size() - first < 2) {
            s.img.resize(first); s.uv.resize(2 * first);
            continue;
        }
        for (int k = 0; k < 3; ++k) s.X.push_back(X[k] + 0.02 * gauss());
        s.off.push_back((int32_t)s.img.size());
        ++s.T;
    }
    s.cam_free.assign((size_t)n, -1);
    s.F = 0;
    for (int i = 0; i < n; ++i) {
        if (i < fixed_ends / 2 + fixed_ends % 2 || i >= n - fixed_ends / 2) continue;
        if (i == poseless) {
            for (int k = 0; k < 9; ++k) s.R[9 * (size_t)i + k] = NAN;
            for (int k = 0; k < 3; ++k) s.t[3 * (size_t)i + k] = NAN;
            continue;
        }
        s.cam_free[i] = s.F++;
        double dR[9], Rn[9];
        rot(rot_err * (uni() - 0.5), rot_err * (uni() - 0.5), dR);
        const double* R = &s.R[9 * (size_t)i];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) Rn[3 * a + b] = dR[3 * a] * R[b] + dR[3 * a + 1] * R[3 + b] + dR[3 * a + 2] * R[6 + b];
        for (int k = 0; k < 9; ++k) s.R[9 * (size_t)i + k] = Rn[k];
        for (int k = 0; k < 3; ++k) s.t[3 * (size_t)i + k] += 0.03 * (uni() - 0.5);
    }
    index_images(s);
    return s;
}

// surgery for the PCG scenes: one more camera (free or fixed) at pose (R, t); one more point with its observations (ascending images)
static int add_camera(Scene& s, const double* R, const double* t, int is_free) {
    const float K[9] = {(float)FOC, 0.f, (float)CX, 0.f, (float)FOC, (float)CY, 0.f, 0.f, 1.f};
    s.K.insert(s.K.end(), K, K + 9);
    s.R.insert(s.R.end(), R, R + 9); s.Rtrue.insert(s.Rtrue.end(), R, R + 9);
    s.t.insert(s.t.end(), t, t + 3); s.ttrue.insert(s.ttrue.end(), t, t + 3);
    s.cam_free.push_back(is_free ? s.F++ : -1);
    return s.n++;
}
struct Seen { int image; double u, v; };
static void add_point(Scene& s, const double* X, const std::vector<Seen>& seen) {
    for (const Seen& o : seen) { s.img.push_back(o.image); s.uv.push_back((float)o.u); s.uv.push_back((float)o.v); }
    s.X.insert(s.X.end(), X, X + 3);
    s.off.push_back((int32_t)s.img.size());
    ++s.T;
    index_images(s);
}
static void project(const Scene& s, int i, const double* X, double& u, double& v) {
    const double* R = &s.R[9 * (size_t)i];
    double Y[3];
    for (int k = 0; k < 3; ++k) Y[k] = R[3 * k] * X[0] + R[3 * k + 1] * X[1] + R[3 * k + 2] * X[2] + s.t[3 * (size_t)i + k];
    u = FOC * Y[0] / Y[2] + CX; v = FOC * Y[1] / Y[2] + CY;
}

struct Out {
    std::vector<double> R, t, X, cost, lambda;
    std::vector<uint8_t> inl;
    std::vector<int32_t> nin, acc, used;
    std::vector<double> res;
    int32_t status;
    int rc;
};

static Out run(const Scene& s, float thr, int iters) {
    Out o;
    o.R.resize(s.R.size()); o.t.resize(s.t.size()); o.X.resize(s.X.size()); o.inl.resize(s.img.size()); o.nin.resize((size_t)s.T);
    o.cost.resize((size_t)iters + 1); o.lambda.resize((size_t)iters + 1); o.acc.resize((size_t)iters);
    o.status = 0;
    o.rc = gf_ba_host_adjust(s.off.data(), s.T, (int)s.img.size(), s.img.data(), s.uv.data(), s.img_off.data(), s.img_obs.data(), s.cam_free.data(),
                             s.n, s.F, s.K.data(), s.R.data(), s.t.data(), s.X.data(), thr, iters, o.R.data(), o.t.data(), o.X.data(), o.inl.data(),
                             o.nin.data(), o.cost.data(), o.acc.data(), o.lambda.data(), &o.status);
    return o;
}

static Out run_pcg(const Scene& s, float thr, int iters, int cg_iters = 64, double cg_tol = 1e-6) {
    Out o;
    o.R.resize(s.R.size()); o.t.resize(s.t.size()); o.X.resize(s.X.size()); o.inl.resize(s.img.size()); o.nin.resize((size_t)s.T);
    o.cost.resize((size_t)iters + 1); o.lambda.resize((size_t)iters + 1); o.acc.resize((size_t)iters);
    o.used.assign((size_t)iters, -1); o.res.assign((size_t)iters, -1.0);
    o.status = 0;
    o.rc = gf_ba_host_adjust_pcg(s.off.data(), s.T, (int)s.img.size(), s.img.data(), s.uv.data(), s.img_off.data(), s.img_obs.data(),
                                 s.cam_free.data(), s.n, s.F, s.K.data(), s.R.data(), s.t.data(), s.X.data(), thr, iters, cg_iters, cg_tol, o.R.data(),
                                 o.t.data(), o.X.data(), o.inl.data(), o.nin.data(), o.cost.data(), o.acc.data(), o.lambda.data(), &o.status,
                                 o.used.data(), o.res.data());
    return o;
}

static double rot_err(const Scene& s, const std::vector<double>& R) {
    double worst = 0;
    for (int i = 0; i < s.n; ++i)
        if (s.cam_free[i] >= 0)
            for (int k = 0; k < 9; ++k) worst = fmax(worst, fabs(R[9 * (size_t)i + k] - s.Rtrue[9 * (size_t)i + k]));
    return worst;
}

static void invariants(const Scene& s, const Out& o, int iters, int pcg = 0) {
    CHECK(o.rc == 0);
    for (int k = 0; k < iters; ++k) {
        CHECK(o.cost[k + 1] <= o.cost[k]);
        if (!o.acc[k]) CHECK(o.cost[k + 1] == o.cost[k] && o.lambda[k + 1] > o.lambda[k]);
    }
    for (int i = 0; i < s.n; ++i)
        if (s.cam_free[i] < 0) {
            CHECK(memcmp(&o.R[9 * (size_t)i], &s.R[9 * (size_t)i], 72) == 0);
            CHECK(memcmp(&o.t[3 * (size_t)i], &s.t[3 * (size_t)i], 24) == 0);
        }
    const Out again = pcg ? run_pcg(s, 20.f, iters) : run(s, 20.f, iters);
    if (pcg) {
        CHECK(again.used == o.used && memcmp(again.res.data(), o.res.data(), 8 * o.res.size()) == 0);
        for (int k = 0; k < iters; ++k) CHECK(o.used[k] >= 0 && o.used[k] <= 64 && (o.used[k] == 64 || (o.status & 1) || o.res[k] <= 1e-12));
    }
    CHECK(memcmp(again.X.data(), o.X.data(), 8 * o.X.size()) == 0 && memcmp(again.cost.data(), o.cost.data(), 8 * o.cost.size()) == 0);
}

int main() {
    {   // 8 cameras, two fixed, noise: converges towards the truth
        const Scene s = plant(11, 8, 200, 0.5, 0.03, 2, -1, 0.0);
        const Out o = run(s, 20.f, 16);
        invariants(s, o, 16);
        int nacc = 0;
        for (int a : o.acc) nacc += a;
        CHECK(s.F == 6 && nacc >= 3 && o.cost[16] < 0.05 * o.cost[0]);
        CHECK(rot_err(s, o.R) < 0.2 * rot_err(s, s.R));
        printf("scene 1: %d points, %zu observations, cost %.6g -> %.6g, %d accepted, rotation error %.2e -> %.2e\n", s.T, s.img.size(), o.cost[0],
               o.cost[16], nacc, rot_err(s, s.R), rot_err(s, o.R));
    }
    {   // an image without a pose, outliers, one fixed camera only
        const Scene s = plant(12, 6, 150, 0.5, 0.02, 1, 3, 0.1);
        const Out o = run(s, 20.f, 12);
        invariants(s, o, 12);
        for (size_t k = 0; k < s.img.size(); ++k)
            if (s.img[k] == 3) CHECK(o.inl[k] == 0);
        printf("scene 2: %d points, %zu observations, %d free, cost %.6g -> %.6g, status %d\n", s.T, s.img.size(), s.F, o.cost[0], o.cost[12], o.status);
    }
    {   // no free camera: points only; and the limits
        Scene s = plant(13, 5, 60, 0.5, 0.0, 5, -1, 0.0);
        CHECK(s.F == 0);
        const Out o = run(s, 20.f, 4);
        invariants(s, o, 4);
        CHECK(run(s, 20.f, 0).rc == -1 && run(s, 20.f, 65).rc == -1 && run(s, 0.f, 4).rc == -1);
        s.off[1] = s.off[2] + 1;
        CHECK(run(s, 20.f, 4).rc == -1);
        printf("scene 3: %d points, cost %.6g -> %.6g\n", s.T, o.cost[0], o.cost[4]);
    }
    {   // PCG: 130 free cameras - more than the dense solver takes
        const Scene s = plant(14, 132, 300, 0.5, 0.02, 2, -1, 0.0);
        CHECK(s.F == 130 && run(s, 20.f, 2).rc == -1);
        const Out o = run_pcg(s, 20.f, 8);
        invariants(s, o, 8, 1);
        int nacc = 0, most = 0;
        for (int k = 0; k < 8; ++k) { nacc += o.acc[k]; most = o.used[k] > most ? o.used[k] : most; }
        CHECK(nacc >= 3 && o.cost[8] < 0.05 * o.cost[0] && o.status == 0 && rot_err(s, o.R) < 0.5 * rot_err(s, s.R));
        printf("scene 4 (pcg): %d free, %d points, %zu observations, cost %.6g -> %.6g, %d accepted, at most %d CG iterations, rotation error %.2e -> %.2e\n",
               s.F, s.T, s.img.size(), o.cost[0], o.cost[8], nacc, most, rot_err(s, s.R), rot_err(s, o.R));
    }
    {   // PCG: a free camera with no observation taking part (all of its pixels 100 px off), and a held point (two fixed cameras on one ray)
        Scene s = plant(15, 8, 200, 0.5, 0.03, 2, -1, 0.0);
        for (size_t k = 0; k < s.img.size(); ++k)
            if (s.img[k] == 3) s.uv[2 * k] += 100.f;
        const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t0[3] = {0, 0, 0}, t1[3] = {0, 0, 1}, X[3] = {0, 0, 5};
        const int a = add_camera(s, I, t0, 0), b = add_camera(s, I, t1, 0);
        add_point(s, X, {{a, CX, CY}, {b, CX, CY}});
        const Out o = run_pcg(s, 20.f, 8);
        invariants(s, o, 8, 1);
        CHECK(memcmp(&o.R[27], &s.R[27], 72) == 0 && memcmp(&o.t[9], &s.t[9], 24) == 0);      // camera 3 moved nowhere
        for (size_t k = 0; k < s.img.size(); ++k)
            if (s.img[k] == 3) CHECK(o.inl[k] == 0);
        CHECK((o.status & 2) && memcmp(&o.X[3 * (size_t)(s.T - 1)], X, 24) == 0);               // the held point stayed
        CHECK(o.acc[0] && o.cost[8] < o.cost[0]);                                                // (camera 3's observations cost thr^2 each, to the end)
        printf("scene 5 (pcg): %d free, one without inliers, one held point, cost %.6g -> %.6g, status %d\n", s.F, o.cost[0], o.cost[8], o.status);
    }
    {   // PCG: a breakdown - a free camera whose only observation lies on its optical axis has a singular block at every lambda
        Scene s = plant(16, 6, 100, 0.5, 0.02, 2, -1, 0.0);
        const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t0[3] = {0, 0, 0}, X[3] = {0, 0, 5};
        const int a = add_camera(s, I, t0, 1);
        double u, v;
        project(s, 0, X, u, v);
        add_point(s, X, {{0, u, v}, {a, CX, CY}});
        const Out o = run_pcg(s, 20.f, 5);
        invariants(s, o, 5, 1);
        CHECK((o.status & 1) && memcmp(o.X.data(), s.X.data(), 8 * s.X.size()) == 0 && memcmp(o.R.data(), s.R.data(), 8 * s.R.size()) == 0);
        for (int k = 0; k < 5; ++k) CHECK(!o.acc[k] && o.used[k] == 0 && o.res[k] == 1.0 && o.lambda[k + 1] > o.lambda[k]);
        // and the limits of the PCG arguments
        CHECK(run_pcg(s, 20.f, 2, 0).rc == -1 && run_pcg(s, 20.f, 2, 257).rc == -1 && run_pcg(s, 20.f, 2, 64, -1.0).rc == -1 &&
              run_pcg(s, 20.f, 2, 64, 1.0).rc == -1 && run_pcg(s, 20.f, 2, 64, NAN).rc == -1 && run_pcg(s, 20.f, 2, 1, 0.0).rc == 0);
        printf("scene 6 (pcg): breakdown, %d of 5 steps accepted, lambda %.3g -> %.3g, status %d\n", 0, o.lambda[0], o.lambda[5], o.status);
    }
    printf(g_fail ? "ba_host_selftest: %d checks FAILED\n" : "ba_host_selftest: all checks passed\n", g_fail);
    return g_fail != 0;
}
