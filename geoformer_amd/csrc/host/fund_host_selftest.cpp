// Stand-alone run of the host form of the fundamental-matrix RANSAC on planted scenes, for sanitizer builds of the solver text:
//   c++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all fund_host.cpp fund_host_selftest.cpp -o t && ./t
// (the scene generator of tests/fund_cases.py restated with a small LCG; libm is used HERE only, to plant the scenes).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

extern "C" int gf_fund_host_seven_point(const double* x0, const double* x1, const double* norm, double* F_out);
extern "C" int gf_fund_host_pencil(const double* F1, const double* F2, double* F_out);
extern "C" void gf_fund_host_offsets_range(const int32_t* offsets, int n, int M, int32_t* out);
extern "C" int gf_fund_host_ransac(const float* matches, const float* scores, int n, float sc_thres, double pixel_thr, int iters, uint32_t seed,
                                   uint32_t sample, double* F_out, int32_t* hyp_out, int32_t* n_inliers, uint8_t* mask);
extern "C" int gf_fund_host_ransac_lo(const float* matches, const float* scores, int n, float sc_thres, double pixel_thr, int iters, uint32_t seed,
                                      uint32_t sample, int refit_rounds, double* F_out, int32_t* hyp_out, int32_t* n_inliers, uint8_t* mask,
                                      int32_t* rounds);

static uint64_t g_state;
static double uni() {                                  // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}
static double gauss() { return sqrt(-2.0 * log(1.0 - uni())) * cos(6.283185307179586 * uni()); }
static void unit(double (&v)[3]) {
    for (int i = 0; i < 3; ++i) v[i] = gauss();
    const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int i = 0; i < 3; ++i) v[i] /= n;
}

struct Geo { double R[9], t[3], F[9]; };
static const double FOC = 500, CX = 320, CY = 240;

static Geo random_geo() {
    Geo p;
    double k[3], d[3];
    unit(k);
    const double th = 0.05 + 0.35 * uni(), s = sin(th), c = 1 - cos(th);
    const double Kx[9] = {0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double kk = 0;
            for (int m = 0; m < 3; ++m) kk += Kx[3 * i + m] * Kx[3 * m + j];
            p.R[3 * i + j] = (i == j) + s * Kx[3 * i + j] + c * kk;
        }
    unit(d);
    const double b = 0.3 + 0.7 * uni();
    for (int i = 0; i < 3; ++i) p.t[i] = d[i] * b;
    const double Tx[9] = {0, -p.t[2], p.t[1], p.t[2], 0, -p.t[0], -p.t[1], p.t[0], 0};
    double E[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            E[3 * i + j] = 0;
            for (int m = 0; m < 3; ++m) E[3 * i + j] += Tx[3 * i + m] * p.R[3 * m + j];
        }
    // F = K^-T E K^-1 with K^-1 = [[1/f, 0, -cx/f], [0, 1/f, -cy/f], [0, 0, 1]]
    const double Ki[9] = {1 / FOC, 0, -CX / FOC, 0, 1 / FOC, -CY / FOC, 0, 0, 1};
    double EK[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            EK[3 * i + j] = 0;
            for (int m = 0; m < 3; ++m) EK[3 * i + j] += E[3 * i + m] * Ki[3 * m + j];
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            p.F[3 * i + j] = 0;
            for (int m = 0; m < 3; ++m) p.F[3 * i + j] += Ki[3 * m + i] * EK[3 * m + j];
        }
    return p;
}

// one correspondence visible in both 640 x 480 images, depth 3 .. 8
static void project(const Geo& p, double (&x0)[2], double (&x1)[2]) {
    for (;;) {
        const double u = uni() * 640, v = uni() * 480, z = 3 + 5 * uni();
        const double X[3] = {(u - CX) / FOC * z, (v - CY) / FOC * z, z};
        double Y[3];
        for (int i = 0; i < 3; ++i) Y[i] = p.R[3 * i] * X[0] + p.R[3 * i + 1] * X[1] + p.R[3 * i + 2] * X[2] + p.t[i];
        if (Y[2] <= 0.1) continue;
        const double a = Y[0] / Y[2] * FOC + CX, b = Y[1] / Y[2] * FOC + CY;
        if (!(a >= 0 && a < 640 && b >= 0 && b < 480)) continue;
        x0[0] = u; x0[1] = v; x1[0] = a; x1[1] = b;
        return;
    }
}

static double sampson_px(const double* F, double a, double b, double u, double v) {
    const double a0 = F[0] * a + F[1] * b + F[2], a1 = F[3] * a + F[4] * b + F[5], a2 = F[6] * a + F[7] * b + F[8];
    const double b0 = F[0] * u + F[3] * v + F[6], b1 = F[1] * u + F[4] * v + F[7];
    const double num = u * a0 + v * a1 + a2;
    return fabs(num) / sqrt(a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1);
}

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

int main() {
    // ---- minimal solver: the best root fits 50 held-out correspondences
    g_state = 1;
    double worst = 0;
    int three = 0;
    for (int s = 0; s < 300; ++s) {
        const Geo p = random_geo();
        double x0[114], x1[114], Fs[27], box[8] = {1e9, -1e9, 1e9, -1e9, 1e9, -1e9, 1e9, -1e9};
        for (int i = 0; i < 57; ++i) {
            double a[2], b[2];
            project(p, a, b);
            x0[2 * i] = a[0]; x0[2 * i + 1] = a[1]; x1[2 * i] = b[0]; x1[2 * i + 1] = b[1];
            const double c[4] = {a[0], a[1], b[0], b[1]};
            for (int k = 0; k < 4; ++k) { box[2 * k] = fmin(box[2 * k], c[k]); box[2 * k + 1] = fmax(box[2 * k + 1], c[k]); }
        }
        const double nm[6] = {0.5 * (box[0] + box[1]), 0.5 * (box[2] + box[3]), 0.5 * fmax(box[1] - box[0], box[3] - box[2]),
                              0.5 * (box[4] + box[5]), 0.5 * (box[6] + box[7]), 0.5 * fmax(box[5] - box[4], box[7] - box[6])};
        const int n = gf_fund_host_seven_point(x0, x1, nm, Fs);
        CHECK(n == 1 || n == 3, "scene %d: %d roots", s, n);
        three += n == 3;
        double best = 1e9;
        for (int r = 0; r < n; ++r) {
            double w = 0;
            for (int i = 7; i < 57; ++i) w = fmax(w, sampson_px(Fs + 9 * r, x0[2 * i], x0[2 * i + 1], x1[2 * i], x1[2 * i + 1]));
            best = fmin(best, w);
        }
        worst = fmax(worst, best);
    }
    CHECK(worst < 2e-6, "worst held-out Sampson distance %.3e px", worst);
    printf("seven-point: worst held-out Sampson distance over 300 scenes %.3e px, %d scenes with three roots\n", worst, three);
    // ---- clean failures and the vanishing leading coefficient
    {
        double x[14], Fs[27];
        const double unitn[6] = {0, 0, 1, 0, 0, 1};
        for (int i = 0; i < 14; ++i) x[i] = 0;
        CHECK(gf_fund_host_seven_point(x, x, unitn, Fs) == 0, "all-zero input");
        for (int i = 0; i < 14; ++i) x[i] = 100 + i;
        x[5] = NAN;
        CHECK(gf_fund_host_seven_point(x, x, unitn, Fs) == 0, "NaN input");
        const double F1[9] = {1, 2, 3, 4, 5, 6, 0, 0, 0}, F2[9] = {2, -1, 0, 1, 3, -2, 0, 1, 4}, F3[9] = {0, 0, 0, 1, 2, 3, 4, 5, 6};
        const int n = gf_fund_host_pencil(F1, F2, Fs);
        int finite = 1;
        for (int k = 0; k < 9 * n; ++k) finite &= isfinite(Fs[k]) != 0;
        CHECK((n == 1 || n == 3) && finite, "vanishing leading coefficient: %d solutions, finite %d", n, finite);
        CHECK(gf_fund_host_pencil(F1, F3, Fs) == 0, "both ends singular");
    }
    // ---- RANSAC on planted scenes: 300 matches, 30 %% outliers; then the gates
    for (int seed = 0; seed < 8; ++seed) {
        g_state = 100 + seed;
        const Geo p = random_geo();
        const int n = 300;
        std::vector<float> m(4 * n), sc(n, 1.f);
        std::vector<uint8_t> outlier(n), mask(n);
        int planted = 0;
        for (int i = 0; i < n; ++i) {
            double a[2], b[2];
            project(p, a, b);
            outlier[i] = uni() < 0.3;
            if (outlier[i]) { b[0] = uni() * 640; b[1] = uni() * 480; }
            m[4 * i] = (float)a[0]; m[4 * i + 1] = (float)a[1]; m[4 * i + 2] = (float)b[0]; m[4 * i + 3] = (float)b[1];
            planted += !outlier[i];
        }
        double F[9];
        int32_t hyp[2], nin;
        int rc = gf_fund_host_ransac(m.data(), nullptr, n, 0.25f, 1.0, 256, (uint32_t)seed, 0, F, hyp, &nin, mask.data());
        int missed = 0, extra = 0;
        for (int i = 0; i < n; ++i) { missed += !outlier[i] && !mask[i]; extra += outlier[i] && mask[i]; }
        CHECK(rc == 1 && missed == 0 && extra <= 6 && nin == planted + extra, "seed %d: rc %d missed %d extra %d inliers %d / %d", seed, rc, missed,
              extra, nin, planted);
        printf("ransac seed %d: valid %d, %d inliers (planted %d, %d missed, %d extra), hypothesis %d root %d\n", seed, rc, nin, planted, missed, extra,
               hyp[0], hyp[1]);
        if (seed == 0) {
            for (int cnt : {7, 6, 0}) {                 // exact matches only
                std::vector<float> a;
                for (int i = 0; i < n && (int)a.size() < 4 * cnt; ++i)
                    if (!outlier[i]) a.insert(a.end(), m.begin() + 4 * i, m.begin() + 4 * i + 4);
                std::vector<uint8_t> mk(cnt + 1);
                rc = gf_fund_host_ransac(a.data(), nullptr, cnt, 0.25f, 1.0, 256, 7, 0, F, hyp, &nin, mk.data());
                CHECK(rc == (cnt >= 7) && nin == (cnt >= 7 ? 7 : 0), "%d matches: rc %d, %d inliers", cnt, rc, nin);
            }
            m[4 * 17 + 2] = NAN; sc[40] = 0.1f; sc[41] = NAN;
            rc = gf_fund_host_ransac(m.data(), sc.data(), n, 0.25f, 1.0, 256, 3, 0, F, hyp, &nin, mask.data());
            CHECK(rc == 1 && mask[17] == 0 && mask[40] == 0 && mask[41] == 0 && nin >= planted - 3, "filtered rows: rc %d masks %d %d %d inliers %d", rc,
                  mask[17], mask[40], mask[41], nin);
            CHECK(gf_fund_host_ransac(m.data(), nullptr, n, 0.25f, 1.0, 100, 3, 0, F, hyp, &nin, mask.data()) == -1, "iters 100");
            CHECK(gf_fund_host_ransac(m.data(), nullptr, n, 0.25f, 1.0, 0, 3, 0, F, hyp, &nin, mask.data()) == -1, "iters 0");
        }
    }
    // ---- the refit on the inliers: noisy scenes (sigma 0.5 px) at the edges of the eight-inlier minimum and of the 256 partial sums
    for (int n : {7, 8, 9, 257, 600}) {
        g_state = 500 + n;
        const Geo p = random_geo();
        std::vector<float> m(4 * n);
        for (int i = 0; i < n; ++i) {
            double a[2], b[2];
            project(p, a, b);
            if (n >= 257 && uni() < 0.3) { b[0] = uni() * 640; b[1] = uni() * 480; }
            m[4 * i] = (float)(a[0] + 0.5 * gauss()); m[4 * i + 1] = (float)(a[1] + 0.5 * gauss());
            m[4 * i + 2] = (float)(b[0] + 0.5 * gauss()); m[4 * i + 3] = (float)(b[1] + 0.5 * gauss());
        }
        double F0[9];
        int32_t hyp0[2], nin0 = 0;
        std::vector<uint8_t> mask0(n);
        for (int R : {0, 1, 8}) {
            double F[9];
            int32_t hyp[2], nin = 0, rounds = -1;
            std::vector<uint8_t> mask(n);
            const int rc = gf_fund_host_ransac_lo(m.data(), nullptr, n, 0.25f, 1.0, 64, 11, 0, R, F, hyp, &nin, mask.data(), &rounds);
            int cnt = 0, finite = 1, same = 1;
            for (int i = 0; i < n; ++i) cnt += mask[i];
            for (int k = 0; k < 9; ++k) finite &= isfinite(F[k]) != 0;
            if (R == 0) {
                for (int k = 0; k < 9; ++k) F0[k] = F[k];
                hyp0[0] = hyp[0]; hyp0[1] = hyp[1]; nin0 = nin; mask0 = mask;
            }
            for (int k = 0; k < 9; ++k) same &= F[k] == F0[k];
            for (int i = 0; i < n; ++i) same &= mask[i] == mask0[i];
            CHECK(rc == 1 && finite && cnt == nin && nin >= nin0 && rounds >= 0 && rounds <= R && hyp[0] == hyp0[0] && hyp[1] == hyp0[1],
                  "refit %d rows R %d: rc %d finite %d mask %d inliers %d (seven-point %d) rounds %d", n, R, rc, finite, cnt, nin, nin0, rounds);
            CHECK(rounds > 0 || (same && nin == nin0), "refit %d rows R %d: rounds 0 but not the seven-point winner", n, R);
            CHECK(n != 7 || rounds == 0, "refit of seven inliers: rounds %d", rounds);
            printf("refit %3d rows R %d: %d -> %d inliers in %d round(s)\n", n, R, nin0, nin, rounds);
        }
        double F[9];
        int32_t hyp[2], nin, rounds;
        std::vector<uint8_t> mask(n);
        CHECK(gf_fund_host_ransac_lo(m.data(), nullptr, n, 0.25f, 1.0, 64, 11, 0, 9, F, hyp, &nin, mask.data(), &rounds) == -1, "refit_rounds 9");
        CHECK(gf_fund_host_ransac_lo(m.data(), nullptr, n, 0.25f, 1.0, 64, 11, 0, -1, F, hyp, &nin, mask.data(), &rounds) == -1, "refit_rounds -1");
    }
    // ---- the offsets clamp, M = 200: o = clamp(offsets[n], 0, M), e = clamp(max(offsets[n + 1], o), 0, M)
    {
        const int M = 200;
        const int32_t cases[][4] = {{0, 0, 0, 0},       {0, 7, 0, 7},     {7, 64, 7, 57},   {199, 200, 199, 1},          // in range, ascending
                                    {-5, 30, 0, 30},    {-9, 0, 0, 0},    {INT32_MIN, 200, 0, 200},                      // a negative start
                                    {150, 201, 150, 50}, {0, INT32_MAX, 0, 200},                                         // an end past M
                                    {120, 40, 120, 0},  {200, 0, 200, 0}, {50, -3, 50, 0},                               // a descending pair
                                    {201, 300, 200, 0}, {300, 201, 200, 0}, {INT32_MAX, INT32_MAX, 200, 0}};             // both past M
        for (const auto& c : cases) {
            const int32_t offs[3] = {-77, c[0], c[1]};
            int32_t out[2] = {-1, -1};
            gf_fund_host_offsets_range(offs, 1, M, out);
            const int o = c[0] < 0 ? 0 : c[0] > M ? M : c[0];
            int e = c[1] < o ? o : c[1];
            e = e > M ? M : e;
            CHECK(out[0] == c[2] && out[1] == c[3] && out[0] == o && out[1] == e - o, "offsets (%d, %d): (%d, %d), expected (%d, %d)", c[0], c[1],
                  out[0], out[1], c[2], c[3]);
        }
        printf("offsets clamp: %d cases\n", (int)(sizeof(cases) / sizeof(cases[0])));
    }
    printf(g_fail ? "%d check(s) FAILED\n" : "all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
}
