// Stand-alone run of the host form of the calibrated two-view RANSAC on planted pairs, for sanitizer builds of the solver text:
//   c++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all relpose_host.cpp relpose_host_selftest.cpp -o t && ./t
// (the scene generator of tests/pose_cases.py restated with a small LCG; libm is used HERE only, to plant the scenes).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

extern "C" int gf_rel_host_gn_row(const double* R_in, const double* t_in, const double* row4, double* J_out, double* res_out);
extern "C" int gf_rel_host_gn_update(const double* d_in, double* R_io, double* t_io);
extern "C" int gf_rel_host_refit_once(const double* rows4, int n, const uint8_t* mask, double* R_io, double* t_io);
extern "C" int gf_rel_host_ransac(const float* m, const float* scores, int n, const float* K0, const float* K1, float sc_thres, double pixel_thr,
                                  int iters, uint32_t seed, uint32_t sample, int refit_rounds, double* E_out, double* R_out, double* t_out,
                                  int32_t* hyp_out, int32_t* n_inliers, int32_t* n_cheiral, uint8_t* mask, int32_t* rounds);

static uint64_t g_state;
static double uni() {                                  // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}
static double gauss() { return sqrt(-2.0 * log(1.0 - uni())) * cos(6.283185307179586 * uni()); }

static const float K0[9] = {500, 0, 320, 0, 500, 240, 0, 0, 1};
static const float K1[9] = {460, 0, 300, 0, 540, 250, 0, 0, 1};

static int g_fail = 0;
#define CHECK(cond, ...)                                                \
    do {                                                                \
        if (!(cond)) { printf("FAIL: " __VA_ARGS__); printf("\n"); ++g_fail; } \
    } while (0)

struct Scene { std::vector<float> m, sc; double R[9], t[3]; };

// n matches of a random pose (rotation up to ~12 degrees, unit t), 30 % outliers from 10 rows on, 0.3 px noise
static Scene plant(int n) {
    Scene s;
    double k[3];
    for (int i = 0; i < 3; ++i) k[i] = gauss();
    const double nk = sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2]);
    for (int i = 0; i < 3; ++i) k[i] /= nk;
    const double th = 0.05 + 0.25 * uni(), sn = sin(th), cs = 1 - cos(th);
    const double Kx[9] = {0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double kk = 0;
            for (int q = 0; q < 3; ++q) kk += Kx[3 * i + q] * Kx[3 * q + j];
            s.R[3 * i + j] = (i == j) + sn * Kx[3 * i + j] + cs * kk;
        }
    double nt = 0;
    for (int i = 0; i < 3; ++i) { s.t[i] = gauss(); nt += s.t[i] * s.t[i]; }
    for (int i = 0; i < 3; ++i) s.t[i] /= sqrt(nt);
    s.m.resize(4 * (size_t)n);
    s.sc.assign((size_t)n, 1.f);
    for (int i = 0; i < n; ++i) {
        const double X[3] = {-2.5 + 5 * uni(), -2 + 4 * uni(), 4 + 6 * uni()};
        double Y[3];
        for (int r = 0; r < 3; ++r) Y[r] = s.R[3 * r] * X[0] + s.R[3 * r + 1] * X[1] + s.R[3 * r + 2] * X[2] + s.t[r];
        s.m[4 * i + 0] = (float)(K0[0] * X[0] / X[2] + K0[2]);
        s.m[4 * i + 1] = (float)(K0[4] * X[1] / X[2] + K0[5]);
        s.m[4 * i + 2] = (float)(K1[0] * Y[0] / Y[2] + K1[2] + 0.3 * gauss());
        s.m[4 * i + 3] = (float)(K1[4] * Y[1] / Y[2] + K1[5] + 0.3 * gauss());
        if (n >= 10 && uni() < 0.3) { s.m[4 * i + 2] = (float)(640 * uni()); s.m[4 * i + 3] = (float)(480 * uni()); }
    }
    return s;
}

struct Out { int valid; double E[9], R[9], t[3]; int32_t hyp[2], nin, nch, rounds; std::vector<uint8_t> mask; };

static Out run(const Scene& s, int n, bool scores, int refit, uint32_t sample) {
    Out o;
    o.mask.assign((size_t)(n > 0 ? n : 1), 7);
    o.valid = gf_rel_host_ransac(s.m.data(), scores ? s.sc.data() : nullptr, n, K0, K1, 0.25f, 1.0, 128, 0x5EEDu, sample, refit, o.E, o.R, o.t, o.hyp,
                                 &o.nin, &o.nch, o.mask.data(), &o.rounds);
    return o;
}

static void invariants(const Out& o, int n, const char* what) {
    int c = 0;
    for (int i = 0; i < n; ++i) c += o.mask[i];
    CHECK(c == o.nin, "%s: mask count %d != n_inliers %d", what, c, (int)o.nin);
    if (!o.valid) {
        CHECK(o.nin == 0 && o.hyp[0] == -1 && o.rounds == 0 && o.nch == 0, "%s: an invalid pair with outputs", what);
        for (int k = 0; k < 9; ++k) CHECK(o.E[k] == 0.0 && o.R[k] == 0.0, "%s: an invalid pair with a model", what);
        return;
    }
    double ne = 0, nt = 0;
    for (int k = 0; k < 9; ++k) ne += o.E[k] * o.E[k];
    for (int k = 0; k < 3; ++k) nt += o.t[k] * o.t[k];
    CHECK(fabs(sqrt(ne) - 1) < 1e-12, "%s: |E| = %.17g", what, sqrt(ne));
    CHECK(fabs(sqrt(nt) - 1) < 1e-12, "%s: |t| = %.17g", what, sqrt(nt));
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double d = 0;
            for (int q = 0; q < 3; ++q) d += o.R[3 * i + q] * o.R[3 * j + q];
            CHECK(fabs(d - (i == j)) < 1e-9, "%s: R R^T [%d][%d] = %.17g", what, i, j, d);
        }
    const double* R = o.R;
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    CHECK(fabs(det - 1) < 1e-9, "%s: det R = %.17g", what, det);
    CHECK(o.nch > 0 && o.nch <= o.nin + 0 * n, "%s: n_cheiral %d of %d", what, (int)o.nch, (int)o.nin);
}

int main() {
    g_state = 0x1234567ull;
    const int sizes[5] = {0, 4, 5, 65, 300};
    for (int si = 0; si < 5; ++si) {
        const int n = sizes[si];
        Scene s = plant(n);
        char what[64];
        snprintf(what, sizeof what, "n = %d", n);
        const Out a = run(s, n, false, 0, (uint32_t)si), b = run(s, n, false, 4, (uint32_t)si);
        invariants(a, n, what);
        invariants(b, n, what);
        CHECK(n >= 5 || !a.valid, "%s: valid below five rows", what);
        CHECK(n < 65 || a.valid, "%s: no pose", what);
        CHECK(b.valid == a.valid && b.nin >= a.nin && b.hyp[0] == a.hyp[0] && b.hyp[1] == a.hyp[1], "%s: refit %d -> %d inliers", what, (int)a.nin,
              (int)b.nin);
        if (b.valid && b.rounds == 0)
            for (int k = 0; k < 9; ++k) CHECK(a.E[k] == b.E[k] && a.R[k] == b.R[k], "%s: rounds = 0 but other bits", what);
        // filtered rows: low and NaN scores, non-finite coordinates; the result is that of the list without them
        if (n >= 65) {
            Scene f = s;
            std::vector<int> gone = {0, 31, 32, 63, 64, n - 1};
            f.sc[0] = 0.1f; f.sc[31] = NAN; f.m[4 * 32 + 1] = NAN; f.m[4 * 63 + 2] = INFINITY; f.m[4 * 64] = -INFINITY; f.sc[n - 1] = 0.2f;
            Scene g;
            for (int i = 0; i < n; ++i) {
                bool out = false;
                for (int j : gone) out |= j == i;
                if (out) continue;
                for (int k = 0; k < 4; ++k) g.m.push_back(s.m[4 * i + k]);
                g.sc.push_back(1.f);
            }
            for (int refit = 0; refit <= 4; refit += 4) {
                const Out x = run(f, n, true, refit, 3), y = run(g, (int)g.sc.size(), true, refit, 3);
                invariants(x, n, "filtered");
                CHECK(x.valid == y.valid && x.nin == y.nin && x.rounds == y.rounds && x.hyp[0] == y.hyp[0], "filtered: another result");
                for (int k = 0; k < 9; ++k) CHECK(x.E[k] == y.E[k] && x.R[k] == y.R[k], "filtered: other bits");
                for (int j : gone) CHECK(x.mask[j] == 0, "filtered: row %d is an inlier", j);
            }
            for (int i = 0; i < n; ++i) f.sc[i] = 0.f;
            const Out z = run(f, n, true, 4, 0);
            invariants(z, n, "all filtered");
            CHECK(!z.valid, "all filtered: valid");
        }
    }
    // the refit pieces on their own: a step from the planted pose on exact rows stays there; identical rows fail the fit
    {
        Scene s = plant(9);
        double rows[40 * 4], R[9], t[3];
        uint8_t mask[40];
        for (int i = 0; i < 40; ++i) {
            const double X[3] = {-2.5 + 5 * uni(), -2 + 4 * uni(), 4 + 6 * uni()};
            double Y[3];
            for (int r = 0; r < 3; ++r) Y[r] = s.R[3 * r] * X[0] + s.R[3 * r + 1] * X[1] + s.R[3 * r + 2] * X[2] + s.t[r];
            rows[4 * i] = X[0] / X[2]; rows[4 * i + 1] = X[1] / X[2]; rows[4 * i + 2] = Y[0] / Y[2]; rows[4 * i + 3] = Y[1] / Y[2];
            mask[i] = 1;
        }
        for (int k = 0; k < 9; ++k) R[k] = s.R[k];
        for (int k = 0; k < 3; ++k) t[k] = s.t[k];
        CHECK(gf_rel_host_refit_once(rows, 40, mask, R, t) == 1, "refit_once failed on exact rows");
        for (int k = 0; k < 9; ++k) CHECK(fabs(R[k] - s.R[k]) < 1e-9, "refit_once left the planted R");
        for (int k = 0; k < 3; ++k) CHECK(fabs(t[k] - s.t[k]) < 1e-9, "refit_once left the planted t");
        for (int i = 1; i < 40; ++i)
            for (int k = 0; k < 4; ++k) rows[4 * i + k] = rows[k];
        rows[2] += 1e-3;
        CHECK(gf_rel_host_refit_once(rows, 40, mask, R, t) == 0, "identical rows: the fit did not fail");
        double J[5], res, d[5] = {1e-3, -2e-3, 5e-4, 1e-3, 2e-3};
        CHECK(gf_rel_host_gn_row(R, t, rows, J, &res) == 1, "gn_row failed");
        CHECK(gf_rel_host_gn_update(d, R, t) == 1, "gn_update failed");
        CHECK(gf_rel_host_refit_once(rows, 0, mask, R, t) == 0, "no rows: the fit did not fail");
    }
    if (g_fail) { printf("%d check(s) failed\n", g_fail); return 1; }
    printf("relpose_host_selftest: ok\n");
    return 0;
}
