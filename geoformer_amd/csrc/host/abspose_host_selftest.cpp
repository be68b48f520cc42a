// Stand-alone run of the host form of the absolute-pose RANSAC and of the 3-D map lookup on planted scenes, for sanitizer builds of the solver text:
//   c++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all abspose_host.cpp abspose_host_selftest.cpp -o t && ./t
// (the scene generator of tests/abspose_cases.py restated with a small LCG; libm is used HERE only, to plant the scenes).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

extern "C" int gf_abs_host_p3p(const double* uv, const double* X, const float* K, const double* norm, double* out);
extern "C" int gf_abs_host_refit_once(const float* uv, const float* xyz, int n, const uint8_t* mask, const float* K, const double* norm,
                                      double* R_io, double* t_io);
extern "C" void gf_abs_host_xyz_lookup(const float* const* maps, const int32_t* Hs, const int32_t* Ws, int P, const int32_t* pair_offsets,
                                       const float* pts, long pts_stride, int M, float* xyz);
extern "C" int gf_abs_host_ransac(const float* uv, const float* xyz, const float* scores, int n, const float* K, float sc_thres, double pixel_thr,
                                  int iters, uint32_t seed, uint32_t sample, int refit_rounds, double* R_out, double* t_out, int32_t* hyp_out,
                                  int32_t* n_inliers, uint8_t* mask, int32_t* rounds);

static uint64_t g_state;
static double uni() {                                  // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}
static double gauss() { return sqrt(-2.0 * log(1.0 - uni())) * cos(6.283185307179586 * uni()); }

struct Pose { double R[9], t[3]; };
static const double FOC = 500, CX = 320, CY = 240;
static const float K9[9] = {500, 0, 320, 0, 500, 240, 0, 0, 1};

static Pose random_pose() {
    Pose p;
    double k[3];
    for (int i = 0; i < 3; ++i) k[i] = gauss();
    const double n = sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2]);
    for (int i = 0; i < 3; ++i) k[i] /= n;
    const double th = 0.05 + 1.15 * uni(), s = sin(th), c = 1 - cos(th);
    const double Kx[9] = {0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double kk = 0;
            for (int m = 0; m < 3; ++m) kk += Kx[3 * i + m] * Kx[3 * m + j];
            p.R[3 * i + j] = (i == j) + s * Kx[3 * i + j] + c * kk;
        }
    const double C[3] = {120 + 4 * uni() - 2, -45 + 4 * uni() - 2, 30 + 4 * uni() - 2};
    for (int i = 0; i < 3; ++i) p.t[i] = -(p.R[3 * i] * C[0] + p.R[3 * i + 1] * C[1] + p.R[3 * i + 2] * C[2]);
    return p;
}

// a uniform pixel at depth 3 .. 8, taken to the world frame
static void plant(const Pose& p, double (&px)[2], double (&X)[3]) {
    px[0] = uni() * 640; px[1] = uni() * 480;
    const double z = 3 + 5 * uni();
    const double Y[3] = {(px[0] - CX) / FOC * z - p.t[0], (px[1] - CY) / FOC * z - p.t[1], z - p.t[2]};
    for (int i = 0; i < 3; ++i) X[i] = p.R[i] * Y[0] + p.R[3 + i] * Y[1] + p.R[6 + i] * Y[2];
}

static double reproj_px(const double* R, const double* t, const double* px, const double* X) {
    double Y[3];
    for (int i = 0; i < 3; ++i) Y[i] = R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2] + t[i];
    if (!(Y[2] > 0)) return 1e30;
    return hypot(Y[0] / Y[2] * FOC + CX - px[0], Y[1] / Y[2] * FOC + CY - px[1]);
}

static double centre_error(const double* R, const double* t, const Pose& p) {
    double e = 0;
    for (int i = 0; i < 3; ++i) {
        const double a = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]), b = -(p.R[i] * p.t[0] + p.R[3 + i] * p.t[1] + p.R[6 + i] * p.t[2]);
        e += (a - b) * (a - b);
    }
    return sqrt(e);
}

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

int main() {
    // ---- minimal solver: the planted pose is among the solutions, every solution reprojects its three points
    g_state = 1;
    double worst_fit = 0, worst_pose = 0;
    int total = 0;
    for (int s = 0; s < 300; ++s) {
        const Pose p = random_pose();
        double px[6], X[9], out[48], lo[3] = {1e9, 1e9, 1e9}, hi[3] = {-1e9, -1e9, -1e9};
        for (int i = 0; i < 40; ++i) {
            double a[2], b[3];
            plant(p, a, b);
            if (i < 3) { px[2 * i] = a[0]; px[2 * i + 1] = a[1]; X[3 * i] = b[0]; X[3 * i + 1] = b[1]; X[3 * i + 2] = b[2]; }
            for (int k = 0; k < 3; ++k) { lo[k] = fmin(lo[k], b[k]); hi[k] = fmax(hi[k], b[k]); }
        }
        const double nm[4] = {0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2]),
                              0.5 * fmax(hi[0] - lo[0], fmax(hi[1] - lo[1], hi[2] - lo[2]))};
        const int n = gf_abs_host_p3p(px, X, K9, nm, out);
        CHECK(n >= 1 && n <= 4, "scene %d: %d solutions", s, n);
        total += n;
        double best = 1e9;
        for (int r = 0; r < n; ++r) {
            for (int i = 0; i < 3; ++i) worst_fit = fmax(worst_fit, reproj_px(out + 12 * r, out + 12 * r + 9, px + 2 * i, X + 3 * i));
            best = fmin(best, centre_error(out + 12 * r, out + 12 * r + 9, p));
        }
        worst_pose = fmax(worst_pose, best);
    }
    CHECK(worst_fit < 1e-3 && worst_pose < 1e-4, "worst reprojection %.3e px, worst centre error %.3e", worst_fit, worst_pose);
    printf("p3p: %d solutions in 300 scenes, worst reprojection of a solution's own points %.3e px, worst centre error of the best %.3e\n", total,
           worst_fit, worst_pose);
    // ---- clean failures
    {
        double out[48];
        const double nm[4] = {0, 0, 0, 1};
        const double px[6] = {100, 100, 300, 200, 500, 400}, line[9] = {1, 2, 3, 2, 4, 6, 4, 8, 12}, tri[9] = {1, 0, 5, 0, 1, 6, -1, -1, 7};
        double bad[9], same[6] = {100, 100, 100, 100, 500, 400};
        CHECK(gf_abs_host_p3p(px, line, K9, nm, out) == 0, "collinear points");
        CHECK(gf_abs_host_p3p(same, tri, K9, nm, out) == 0, "two equal bearings");
        for (int i = 0; i < 9; ++i) bad[i] = tri[i];
        bad[4] = NAN;
        CHECK(gf_abs_host_p3p(px, bad, K9, nm, out) == 0, "NaN input");
        const double zero[4] = {0, 0, 0, 0};
        CHECK(gf_abs_host_p3p(px, tri, K9, zero, out) == 0, "a box without extent");
    }
    // ---- RANSAC with and without the refit: noisy scenes at the edges of the four-row and six-inlier minimum and of the 256 partial sums
    for (int n : {0, 3, 4, 5, 6, 7, 257, 600}) {
        g_state = 500 + n;
        const Pose p = random_pose();
        std::vector<float> uv(2 * n + 2), xyz(3 * n + 3), sc(n + 1, 1.f);
        std::vector<uint8_t> outlier(n + 1, 0);
        for (int i = 0; i < n; ++i) {
            double a[2], b[3];
            plant(p, a, b);
            outlier[i] = n >= 257 && uni() < 0.3;
            if (outlier[i]) { a[0] = uni() * 640; a[1] = uni() * 480; }
            const double sg = n >= 257 ? 0.5 : 0.0;
            uv[2 * i] = (float)(a[0] + sg * gauss()); uv[2 * i + 1] = (float)(a[1] + sg * gauss());
            for (int k = 0; k < 3; ++k) xyz[3 * i + k] = (float)b[k];
        }
        double R0[9], t0[3];
        int32_t hyp0[2] = {0, 0}, nin0 = 0;
        std::vector<uint8_t> mask0(n + 1);
        for (int rr : {0, 1, 8}) {
            double R[9], t[3];
            int32_t hyp[2], nin = 0, rounds = -1;
            std::vector<uint8_t> mask(n + 1);
            const int rc = gf_abs_host_ransac(uv.data(), xyz.data(), nullptr, n, K9, 0.25f, 2.0, 128, 11, 0, rr, R, t, hyp, &nin, mask.data(), &rounds);
            int cnt = 0, finite = 1, same = 1, extra = 0;
            for (int i = 0; i < n; ++i) { cnt += mask[i]; extra += mask[i] && outlier[i]; }
            for (int k = 0; k < 9; ++k) finite &= isfinite(R[k]) != 0;
            if (rr == 0) {
                for (int k = 0; k < 9; ++k) R0[k] = R[k];
                for (int k = 0; k < 3; ++k) t0[k] = t[k];
                hyp0[0] = hyp[0]; hyp0[1] = hyp[1]; nin0 = nin; mask0 = mask;
            }
            for (int k = 0; k < 9; ++k) same &= R[k] == R0[k];
            for (int k = 0; k < 3; ++k) same &= t[k] == t0[k];
            for (int i = 0; i < n; ++i) same &= mask[i] == mask0[i];
            CHECK(rc == (n >= 4) && finite && cnt == nin && nin >= nin0 && rounds >= 0 && rounds <= rr && hyp[0] == hyp0[0] && hyp[1] == hyp0[1],
                  "%d rows R %d: rc %d finite %d mask %d inliers %d (p3p %d) rounds %d", n, rr, rc, finite, cnt, nin, nin0, rounds);
            CHECK(rounds > 0 || (same && nin == nin0), "%d rows R %d: rounds 0 but not the p3p winner", n, rr);
            CHECK(n >= 6 || rounds == 0, "refit of %d rows: rounds %d", n, rounds);
            CHECK(n < 4 || n >= 257 || nin == n, "%d exact rows: %d inliers", n, nin);
            CHECK(extra <= 2, "%d rows: %d outliers accepted", n, extra);
            if (rc == 1)
                printf("ransac %3d rows R %d: %d -> %d inliers in %d round(s), centre error %.3e\n", n, rr, nin0, nin, rounds, centre_error(R, t, p));
        }
        if (n == 600) {
            double R[9], t[3];
            int32_t hyp[2], nin, rounds;
            std::vector<uint8_t> mask(n);
            uv[2 * 17] = NAN; xyz[3 * 18 + 2] = INFINITY; sc[40] = 0.1f; sc[41] = NAN;
            const int rc = gf_abs_host_ransac(uv.data(), xyz.data(), sc.data(), n, K9, 0.25f, 2.0, 128, 3, 0, 4, R, t, hyp, &nin, mask.data(), &rounds);
            CHECK(rc == 1 && !mask[17] && !mask[18] && !mask[40] && !mask[41], "filtered rows: rc %d masks %d %d %d %d", rc, mask[17], mask[18], mask[40], mask[41]);
            CHECK(gf_abs_host_ransac(uv.data(), xyz.data(), nullptr, n, K9, 0.25f, 2.0, 100, 3, 0, 0, R, t, hyp, &nin, mask.data(), &rounds) == -1, "iters 100");
            CHECK(gf_abs_host_ransac(uv.data(), xyz.data(), nullptr, n, K9, 0.25f, 0.0, 128, 3, 0, 0, R, t, hyp, &nin, mask.data(), &rounds) == -1, "thr 0");
            CHECK(gf_abs_host_ransac(uv.data(), xyz.data(), nullptr, n, K9, 0.25f, 2.0, 128, 3, 0, 9, R, t, hyp, &nin, mask.data(), &rounds) == -1, "refit 9");
            // one round alone on an empty set: a singular system, the pose stays
            std::vector<uint8_t> none(n, 0);
            const double nm[4] = {120, -45, 30, 10};
            double Rk[9], tk[3];
            for (int k = 0; k < 9; ++k) Rk[k] = p.R[k];
            for (int k = 0; k < 3; ++k) tk[k] = 0.1 * k;
            CHECK(gf_abs_host_refit_once(uv.data(), xyz.data(), n, none.data(), K9, nm, Rk, tk) == 0 && Rk[4] == p.R[4] && tk[2] == 0.2, "empty set");
        }
    }
    // ---- the lookup: exact map sizes, every edge
    {
        const int H = 5, W = 7;
        std::vector<float> map(3 * H * W);
        for (size_t i = 0; i < map.size(); ++i) map[i] = (float)(uni() * 100 - 50);
        map[3 * (2 * W + 3) + 1] = NAN;
        const float* maps[2] = {map.data(), nullptr};
        const int32_t Hs[2] = {H, 0}, Ws[2] = {W, 0}, off[3] = {0, 9, 11};
        const float pts[24] = {0, 0, 6, 4, 6.f, 3.5f, 5.5f, 4, 6.001f, 1, 1, 4.001f, -0.001f, 1, NAN, 1, 3, 2, 1, 1, 2, 2, 3, 3};
        float out[36];
        gf_abs_host_xyz_lookup(maps, Hs, Ws, 2, off, pts, 2, 12, out);
        CHECK(out[0] == map[0] && out[3] == map[3 * (4 * W + 6)], "integer coordinates are the pixel's own value");
        CHECK(isfinite(out[6]) && isfinite(out[9]), "the last column and the last row");
        for (int i = 4; i < 12; ++i) CHECK(isnan(out[3 * i]) && isnan(out[3 * i + 2]), "row %d should have no 3-D point", i);
    }
    printf(g_fail ? "%d check(s) FAILED\n" : "all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
}
