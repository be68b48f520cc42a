// Stand-alone run of the host form of the essential-matrix RANSAC on planted scenes, for sanitizer builds of the solver text:
//   c++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all pose_host.cpp pose_host_selftest.cpp -o t && ./t
// (the scene generator of tests/pose_cases.py restated with a small LCG; libm is used HERE only, to plant the scenes).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

extern "C" int gf_pose_host_five_point(const double* x0, const double* x1, double* E_out);
extern "C" int gf_pose_host_ransac(const float* mk0, const float* mk1, int n, const float* K0, const float* K1, double pixel_thr, int iters,
                                   uint32_t seed, uint32_t sample, double* E_out, double* R_out, double* t_out, int32_t* hyp_out,
                                   int32_t* n_inliers, uint8_t* mask);

static uint64_t g_state;
static double uni() {                                  // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}
static double gauss() { return sqrt(-2.0 * log(1.0 - uni())) * cos(6.283185307179586 * uni()); }

struct Pose { double R[9], t[3], E[9]; };

static Pose random_pose() {
    Pose p;
    double v[3] = {gauss() * 0.20943951, gauss() * 0.20943951, gauss() * 0.20943951};      // 12 degrees
    const double th = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double k[3] = {v[0] / th, v[1] / th, v[2] / th}, s = sin(th), c = 1 - cos(th);
    const double Kx[9] = {0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double kk = 0;
            for (int m = 0; m < 3; ++m) kk += Kx[3 * i + m] * Kx[3 * m + j];
            p.R[3 * i + j] = (i == j) + s * Kx[3 * i + j] + c * kk;
        }
    double t[3] = {gauss(), gauss(), gauss()};
    const double n = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    for (int i = 0; i < 3; ++i) p.t[i] = t[i] / n;
    const double Tx[9] = {0, -p.t[2], p.t[1], p.t[2], 0, -p.t[0], -p.t[1], p.t[0], 0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            p.E[3 * i + j] = 0;
            for (int m = 0; m < 3; ++m) p.E[3 * i + j] += Tx[3 * i + m] * p.R[3 * m + j];
        }
    return p;
}

static void project(const Pose& p, double (&x0)[2], double (&x1)[2]) {
    const double X[3] = {uni() * 5 - 2.5, uni() * 4 - 2, 4 + uni() * 6};
    double Y[3];
    for (int i = 0; i < 3; ++i) Y[i] = p.R[3 * i] * X[0] + p.R[3 * i + 1] * X[1] + p.R[3 * i + 2] * X[2] + p.t[i];
    x0[0] = X[0] / X[2]; x0[1] = X[1] / X[2]; x1[0] = Y[0] / Y[2]; x1[1] = Y[1] / Y[2];
}

static double sampson_px(const Pose& p, double a, double b, double u, double v) {
    const double* E = p.E;
    const double a0 = E[0] * a + E[1] * b + E[2], a1 = E[3] * a + E[4] * b + E[5], a2 = E[6] * a + E[7] * b + E[8];
    const double b0 = E[0] * u + E[3] * v + E[6], b1 = E[1] * u + E[4] * v + E[7];
    const double num = u * a0 + v * a1 + a2;
    return sqrt(num * num / (a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1)) * 500.0;
}

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

int main() {
    const float K[9] = {500, 0, 320, 0, 500, 240, 0, 0, 1};
    // ---- minimal solver: the planted E among the roots
    g_state = 1;
    double worst = 0;
    for (int s = 0; s < 300; ++s) {
        const Pose p = random_pose();
        double x0[10], x1[10], Es[90];
        for (int i = 0; i < 5; ++i) { double a[2], b[2]; project(p, a, b); x0[2 * i] = a[0]; x0[2 * i + 1] = a[1]; x1[2 * i] = b[0]; x1[2 * i + 1] = b[1]; }
        const int n = gf_pose_host_five_point(x0, x1, Es);
        CHECK(n >= 2 && n <= 10 && n % 2 == 0, "scene %d: %d roots", s, n);
        double en = 0, best = 1e9;
        for (int k = 0; k < 9; ++k) en += p.E[k] * p.E[k];
        en = sqrt(en);
        for (int r = 0; r < n; ++r) {
            double dp = 0, dm = 0;
            for (int k = 0; k < 9; ++k) { const double e = p.E[k] / en; dp += (Es[9 * r + k] - e) * (Es[9 * r + k] - e); dm += (Es[9 * r + k] + e) * (Es[9 * r + k] + e); }
            best = fmin(best, sqrt(fmin(dp, dm)));
        }
        worst = fmax(worst, best);
    }
    CHECK(worst < 1e-6, "worst distance to the planted E %.3e", worst);
    printf("five-point: worst distance to the planted E over 300 scenes %.3e\n", worst);
    // ---- RANSAC on planted scenes: 300 matches, 30 %% outliers; then the gates
    for (int seed = 0; seed < 8; ++seed) {
        g_state = 100 + seed;
        const Pose p = random_pose();
        const int n = 300;
        std::vector<float> m0(2 * n), m1(2 * n);
        std::vector<uint8_t> outlier(n), mask(n);
        for (int i = 0; i < n; ++i) {
            double a[2], b[2];
            project(p, a, b);
            m0[2 * i] = (float)(a[0] * 500 + 320); m0[2 * i + 1] = (float)(a[1] * 500 + 240);
            m1[2 * i] = (float)(b[0] * 500 + 320); m1[2 * i + 1] = (float)(b[1] * 500 + 240);
            outlier[i] = uni() < 0.3;
            for (int redraw = 0; outlier[i]; ++redraw) {
                if (redraw == 200) { outlier[i] = 0; break; }      // a keypoint on the epipole: no point is 10 px from its "line"
                const float u = (float)(uni() * 640), v = (float)(uni() * 480);
                if (sampson_px(p, ((double)m0[2 * i] - 320) / 500, ((double)m0[2 * i + 1] - 240) / 500, ((double)u - 320) / 500, ((double)v - 240) / 500) > 10.0) {
                    m1[2 * i] = u; m1[2 * i + 1] = v;
                    break;
                }
            }
        }
        double E[9], R[9], t[3];
        int32_t hyp[2], nin;
        int rc = gf_pose_host_ransac(m0.data(), m1.data(), n, K, K, 0.5, 256, (uint32_t)seed, 0, E, R, t, hyp, &nin, mask.data());
        int same = 1, planted = 0;
        for (int i = 0; i < n; ++i) { same &= (mask[i] != 0) == (outlier[i] == 0); planted += !outlier[i]; }
        double tr = 0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) tr += R[3 * i + j] * p.R[3 * i + j];
        const double rerr = acos(fmax(-1.0, fmin(1.0, (tr - 1) / 2))) * 57.29577951308232;
        CHECK(rc == 1 && same && nin == planted && rerr < 0.05, "seed %d: rc %d mask equal %d inliers %d / %d R_err %.3e", seed, rc, same, nin, planted, rerr);
        printf("ransac seed %d: valid %d, %d inliers (planted %d), R_err %.2e deg, hypothesis %d root %d\n", seed, rc, nin, planted, rerr, hyp[0], hyp[1]);
        if (seed == 0) {
            for (int cnt : {5, 4, 0}) {                 // exact matches only
                std::vector<float> a, b;
                for (int i = 0; i < n && (int)a.size() < 2 * cnt; ++i)
                    if (!outlier[i]) { a.push_back(m0[2 * i]); a.push_back(m0[2 * i + 1]); b.push_back(m1[2 * i]); b.push_back(m1[2 * i + 1]); }
                a.resize(2 * cnt + 2); b.resize(2 * cnt + 2);
                std::vector<uint8_t> mk(cnt + 1);
                rc = gf_pose_host_ransac(a.data(), b.data(), cnt, K, K, 0.5, 256, 7, 0, E, R, t, hyp, &nin, mk.data());
                CHECK(rc == (cnt >= 5) && nin == (cnt >= 5 ? 5 : 0), "%d matches: rc %d, %d inliers", cnt, rc, nin);
            }
            m1[2 * 17] = NAN;
            rc = gf_pose_host_ransac(m0.data(), m1.data(), n, K, K, 0.5, 256, 3, 0, E, R, t, hyp, &nin, mask.data());
            CHECK(rc == 1 && mask[17] == 0 && nin >= planted - 1, "NaN keypoint: rc %d mask %d inliers %d", rc, mask[17], nin);
            CHECK(gf_pose_host_ransac(m0.data(), m1.data(), n, K, K, 0.5, 100, 3, 0, E, R, t, hyp, &nin, mask.data()) == -1, "iters 100");
            CHECK(gf_pose_host_ransac(m0.data(), m1.data(), n, K, K, 0.5, 0, 3, 0, E, R, t, hyp, &nin, mask.data()) == -1, "iters 0");
        }
    }
    printf(g_fail ? "%d check(s) FAILED\n" : "all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
}
