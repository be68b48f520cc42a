// Stand-alone run of the host form of the lens-distortion rule on planted points, for sanitizer builds of the rule's text:
//   c++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all camera_host.cpp camera_host_selftest.cpp -o t && ./t
// (points planted with a small LCG).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

extern "C" int gf_camera_host_points(const float* pts, long pts_stride, int P, const int32_t* seg_off, const int32_t* seg_camera, int S,
                                     const double* cameras, int C, int inverse, float* out, uint8_t* status, int32_t* flags);
extern "C" int gf_camera_host_undistort(const double* camera, double tx, double ty, double* xy, int32_t* steps);
extern "C" int gf_camera_host_distort(const double* camera, double x, double y, double* xy, double* j);

static uint64_t g_state;
static double uni() {                                  // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static const int NCAM = 7;
static const double CAMS[NCAM][8] = {
    {800, 800, 800, 600, 0, 0, 0, 0},                  // both pinhole models
    {800, 800, 800, 600, 0.1, 0, 0, 0},                // SIMPLE_RADIAL
    {800, 800, 800, 600, -0.1, 0, 0, 0},
    {800, 800, 800, 600, -0.3, 0, 0, 0},
    {1000, 1000, 640, 480, -0.2, 0.05, 0, 0},          // RADIAL
    {900, 950, 700, 500, -0.25, 0.08, 1e-3, -2e-3},    // OPENCV
    {800, 800, 800, 600, -0.0, 0, 0, 0},               // a negative zero is no distortion
};

int main() {
    g_state = 1;
    // ---- in-domain points of every camera: distort, undistort, compare in normalised units; the step statistics
    for (int c = 0; c < NCAM; ++c) {
        int most = 0, n = 0;
        long total = 0;
        double worst = 0;
        for (int k = 0; k < 4000; ++k) {
            const double x = 1.2 * uni() - 0.6, y = 1.2 * uni() - 0.6;
            double d[2], j[4], back[2];
            int32_t steps;
            if (!gf_camera_host_distort(CAMS[c], x, y, d, j)) continue;          // beyond the fold
            ++n;
            CHECK(gf_camera_host_undistort(CAMS[c], d[0], d[1], back, &steps) == 1, "camera %d point %g %g: no pre-image", c, x, y);
            worst = fmax(worst, fmax(fabs(back[0] - x), fabs(back[1] - y)));
            most = steps > most ? steps : most;
            total += steps;
        }
        CHECK(n > 3000 && worst < 1e-8 && most <= 32, "camera %d: %d points, worst %g, %d steps", c, n, worst, most);
        printf("camera %d: %d points, worst |x - x'| %.3g, steps at most %d, mean %.2f\n", c, n, worst, most, (double)total / (n ? n : 1));
    }
    // ---- the list form: several cameras, empty segments, both strides, failures and non-finite rows
    {
        const int32_t seg_off[] = {0, 0, 1, 64, 128, 128, 193, 450, 460};
        const int32_t seg_cam[] = {1, 0, 0, 3, 2, 4, 5, 6};
        const int S = 8, P = 460;
        std::vector<float> block(4 * P), flat(2 * P);
        for (int i = 0; i < P; ++i) {
            block[4 * i] = (float)(1600 * uni()); block[4 * i + 1] = (float)(1200 * uni());
            block[4 * i + 2] = (float)(400 + 800 * uni()); block[4 * i + 3] = (float)(300 + 600 * uni());
        }
        block[4 * 70 + 2] = NAN; block[4 * 71 + 3] = INFINITY; block[4 * 72 + 2] = -INFINITY; block[4 * 0 + 2] = NAN;
        block[4 * 80 + 2] = 800 + 800 * 0.69f; block[4 * 80 + 3] = 600;
        block[4 * 81 + 2] = 800 + 800 * 0.71f; block[4 * 81 + 3] = 600;
        block[4 * 82 + 2] = 800 + 800 * 2.0f; block[4 * 82 + 3] = 600;
        for (int i = 0; i < P; ++i) { flat[2 * i] = block[4 * i + 2]; flat[2 * i + 1] = block[4 * i + 3]; }
        std::vector<float> a(2 * P), b(2 * P), d(2 * P);
        std::vector<uint8_t> sa(P), sb(P);
        int32_t flags[2] = {0, 0};
        CHECK(gf_camera_host_points(&block[2], 4, P, seg_off, seg_cam, S, &CAMS[0][0], NCAM, 1, a.data(), sa.data(), flags) == 0, "stride 4");
        CHECK(gf_camera_host_points(flat.data(), 2, P, seg_off, seg_cam, S, &CAMS[0][0], NCAM, 1, b.data(), sb.data(), flags) == 0, "stride 2");
        CHECK(memcmp(a.data(), b.data(), 8 * P) == 0 && memcmp(sa.data(), sb.data(), P) == 0 && !flags[0] && !flags[1], "strides differ or flags %d %d", flags[0], flags[1]);
        CHECK(sa[0] == 1 && sa[70] == 1 && sa[71] == 1 && sa[72] == 1 && sa[80] == 0 && sa[81] == 2 && sa[82] == 2, "status %d %d %d %d %d %d %d", sa[0],
              sa[70], sa[71], sa[72], sa[80], sa[81], sa[82]);
        CHECK(a[2 * 81] != a[2 * 81] && a[2 * 81 + 1] != a[2 * 81 + 1] && a[2 * 70] != a[2 * 70] && a[2 * 70 + 1] != a[2 * 70 + 1], "a failed row is not NaN");
        for (int i = 1; i < 64; ++i) CHECK(memcmp(&a[2 * i], &flat[2 * i], 8) == 0 && sa[i] == 0, "row %d of a pinhole camera changed", i);
        for (int i = 450; i < 460; ++i) CHECK(memcmp(&a[2 * i], &flat[2 * i], 8) == 0, "row %d of a -0.0 camera changed", i);
        // the round trip of the rows that have a pre-image
        CHECK(gf_camera_host_points(a.data(), 2, P, seg_off, seg_cam, S, &CAMS[0][0], NCAM, 0, d.data(), nullptr, flags) == 0, "distort");
        double worst = 0;
        for (int i = 0; i < P; ++i)
            if (sa[i] == 0) worst = fmax(worst, fmax(fabs((double)d[2 * i] - flat[2 * i]), fabs((double)d[2 * i + 1] - flat[2 * i + 1])));
        CHECK(worst < 1e-3, "round trip: %g px", worst);
        printf("list form: round trip within %.3g px\n", worst);
        // what is reported and never followed
        const int32_t bad_cam[] = {1, 0, 0, 9, 2, 4, -1, 6};
        int32_t f2[2] = {0, 0};
        CHECK(gf_camera_host_points(flat.data(), 2, P, seg_off, bad_cam, S, &CAMS[0][0], NCAM, 1, b.data(), sb.data(), f2) == 0 && f2[0] == 0 && f2[1] == 1 &&
              sb[64] == 3 && sb[127] == 3 && sb[193] == 3 && sb[128] == 0 && b[2 * 64] != b[2 * 64], "a camera index outside the table");
        const int32_t bad_off[] = {0, 0, 1, 64, 40, 128, 193, 450, 455};
        int32_t f3[2] = {0, 0};
        CHECK(gf_camera_host_points(flat.data(), 2, P, bad_off, seg_cam, S, &CAMS[0][0], NCAM, 1, b.data(), sb.data(), f3) == 0 && f3[0] == 1 && f3[1] == 0 &&
              sb[459] == 3, "offsets that do not ascend");
        const int32_t wild[] = {-5, 1 << 30, 3};
        const int32_t wc[] = {0, 1};
        int32_t f4[2] = {0, 0};
        CHECK(gf_camera_host_points(flat.data(), 2, P, wild, wc, 2, &CAMS[0][0], NCAM, 1, b.data(), sb.data(), f4) == 0 && f4[0] == 1, "wild offsets");
        CHECK(gf_camera_host_points(flat.data(), 2, -1, seg_off, seg_cam, S, &CAMS[0][0], NCAM, 1, b.data(), sb.data(), flags) == -1, "P < 0");
        CHECK(gf_camera_host_points(flat.data(), 2, P, seg_off, seg_cam, S, &CAMS[0][0], 0, 1, b.data(), sb.data(), flags) == -1, "C == 0 with points");
        CHECK(gf_camera_host_points(flat.data(), 1, P, seg_off, seg_cam, S, &CAMS[0][0], NCAM, 1, b.data(), sb.data(), flags) == -1, "stride 1");
        CHECK(gf_camera_host_points(nullptr, 2, 0, nullptr, nullptr, 0, nullptr, 0, 1, nullptr, nullptr, nullptr) == 0, "an empty call");
    }
    printf(g_fail ? "%d check(s) FAILED\n" : "all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
}
