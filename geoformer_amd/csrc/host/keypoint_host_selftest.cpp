// TEST INFRASTRUCTURE: a stand-alone sanitizer run of keypoint_host.cpp (keypoint_spec.h on the host):
//   c++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all keypoint_host.cpp keypoint_host_selftest.cpp -o t && ./t
// empty input (no pairs; pairs without rows), one point, a cell with hundreds of centres (a 1-pixel lattice under dthres 0.5), boundary
// coordinates (k * psize and one ulp on either side, 0, -0.0, +-KP_MAX_COORD), denormals, huge coordinates (beyond KP_MAX_COORD: reported
// in the status word of the quantised mode, plain keys in the exact mode; FLT_MAX; non-finite rows and NaN scores are dropped), an image
// index out of range, equal scores under the filter, and the argument checks.  Prints "ok" and a checksum; the sanitizers abort on any
// out-of-range conversion, overflow or out-of-bounds access.
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

extern "C" float gf_keypoint_host_cell(float x, float psize);
extern "C" int gf_keypoint_host_filter(const int* ids, const float* scores, int n, unsigned char* keep);
extern "C" int gf_keypoint_host_consolidate(const float* matches, const float* scores, const int* pair_offsets, const int* pair_images, int P,
                                            int n_images, float sc_thres, float psize, float dthres, int unique, float* keypoints,
                                            int* kp_offsets, int* ids, int* pair_offsets_out, long long* stats);

static unsigned long g_sum = 0;
static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); g_fail = 1; } } while (0)

struct Out {
    std::vector<float> kp;
    std::vector<int> kpo, ids, po;
    long long st[8];
    int rc;
};

static Out run(const std::vector<float>& m, const std::vector<float>& s, const std::vector<int>& off, const std::vector<int>& im, int n_images,
               float thr, float psize, float dthres, int unique) {
    Out o;
    const int P = (int)off.size() - 1, M = off.back();
    o.kp.assign(4 * (size_t)M + 2, -7.f), o.kpo.assign(n_images + 1, -7), o.ids.assign(2 * (size_t)M + 2, -7), o.po.assign(P + 1, -7);
    o.rc = gf_keypoint_host_consolidate(m.data(), s.data(), off.data(), im.data(), P, n_images, thr, psize, dthres, unique, o.kp.data(),
                                        o.kpo.data(), o.ids.data(), o.po.data(), o.st);
    if (o.rc == 0) {
        for (long long k = 0; k < 2 * o.st[6]; ++k) { uint32_t u; memcpy(&u, &o.kp[k], 4); g_sum += u; }
        for (long long k = 0; k < 2 * o.st[7]; ++k) g_sum += (unsigned)o.ids[k];
    }
    return o;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // empty input
    { Out o = run({}, {}, {0}, {}, 0, 0.25f, 48.f, 4.f, 1); EXPECT(o.rc == 0 && o.st[6] == 0 && o.st[7] == 0); }
    { Out o = run({}, {}, {0, 0, 0}, {0, 1, 1, 2}, 3, 0.25f, 48.f, 4.f, 1); EXPECT(o.rc == 0 && o.kpo[3] == 0 && o.po[2] == 0); }
    // one point
    { Out o = run({1.5f, 2.5f, 3.5f, 4.5f}, {0.9f}, {0, 1}, {0, 1}, 2, 0.25f, 48.f, 4.f, 1);
      EXPECT(o.rc == 0 && o.st[6] == 2 && o.st[7] == 1 && o.kp[0] == 1.5f && o.kp[3] == 4.5f && o.ids[0] == 0 && o.ids[1] == 0); }
    // a cell with hundreds of centres: the 1-pixel lattice of a 48 x 48 cell, dthres 0.5 (nothing merges), then every point again (all merge)
    {
        std::vector<float> m, s;
        for (int rep = 0; rep < 2; ++rep)
            for (int k = 0; k < 2304; ++k) {
                const int j = (k * 1013) % 2304;
                m.insert(m.end(), {(float)(j % 48), (float)(j / 48), 96.f + (float)(j % 48), (float)(j / 48) + 0.25f * rep});
                s.push_back(0.3f + 1e-4f * (float)(k + 2304 * rep));
            }
        Out o = run(m, s, {0, 4608}, {0, 0}, 1, 0.25f, 48.f, 0.5f, 0);
        EXPECT(o.rc == 0 && o.st[4] == 2304 && o.st[6] == 2 * 2304 && o.st[7] == 4608);
        Out u = run(m, s, {0, 4608}, {0, 0}, 1, 0.25f, 48.f, 0.5f, 1);
        EXPECT(u.rc == 0 && u.st[7] == 2304 && u.st[5] == 2304);
    }
    // boundary coordinates, denormals, huge coordinates
    {
        std::vector<float> xs = {0.f, -0.f, FLT_MIN, -FLT_MIN, 1e-45f, -1e-45f, 4194304.f, -4194304.f, nextafterf(4194304.f, 0.f), 4194304.5f, 1e30f, FLT_MAX,
                                 -FLT_MAX, inf, -inf, nan};
        for (float p : {16.f, 48.f})
            for (int k : {1, 2, 3, 199, 200, 87381})
                for (float v : {p * (float)k, nextafterf(p * (float)k, 0.f), nextafterf(p * (float)k, inf), -p * (float)k, nextafterf(-p * (float)k, -inf)}) xs.push_back(v);
        for (float p : {16.f, 48.f, 2.0000002f, 0.3f * 48.f})
            for (float v : xs)
                if (fabsf(v) <= 4194304.f) {
                    const float c = gf_keypoint_host_cell(v, p);
                    EXPECT(c == floorf(c) && (double)c * (double)p <= (double)v && (double)v < ((double)c + 1.0) * (double)p);
                    EXPECT(fabsf(c) <= 2097152.f);
                }
        std::vector<float> m, s;
        for (size_t i = 0; i < xs.size(); ++i) {
            m.insert(m.end(), {xs[i], xs[(i * 7 + 3) % xs.size()], xs[(i * 5 + 1) % xs.size()], xs[(i * 3 + 2) % xs.size()]});
            s.push_back(i % 11 == 5 ? nan : i % 7 == 3 ? 0.1f : 0.5f);
        }
        const int n = (int)s.size();
        for (int unique = 0; unique < 2; ++unique) {
            Out q = run(m, s, {0, n / 2, n}, {0, 1, 1, 0}, 2, 0.25f, 48.f, 4.f, unique);
            EXPECT(q.rc == 0 && (q.st[0] & 1) && q.st[7] <= n);
            Out q2 = run(m, s, {0, n / 2, n}, {0, 1, 1, 0}, 2, 0.25f, 16.f, 6.f, unique);
            EXPECT(q2.rc == 0);
        }
        Out x = run(m, s, {0, n / 2, n}, {0, 1, 1, 0}, 2, 0.25f, 0.f, 0.f, 1);
        EXPECT(x.rc == 0 && x.st[0] == 0);
        Out y = run(m, s, {0, n / 2, n}, {0, 1, 1, 0}, 2, 0.25f, 48.f, -1.f, 1);
        EXPECT(y.rc == 0 && y.st[7] == x.st[7]);
        // an image index out of range: the pair's rows are dropped and the status word says so
        Out z = run(m, s, {0, n / 2, n}, {0, 1, 2, 0}, 2, 0.25f, 48.f, 4.f, 1);
        EXPECT(z.rc == 0 && (z.st[0] & 2) && z.po[2] == z.po[1]);
        Out w = run(m, s, {0, n / 2, n}, {0, -1, 1, 0}, 2, 0.25f, 0.f, 0.f, 1);
        EXPECT(w.rc == 0 && (w.st[0] & 2) && w.po[1] == 0);
    }
    // exact mode: +-0.0 and repeated points
    { Out o = run({0.f, 0.f, 5.f, 5.f, -0.f, 0.f, 5.f, 5.f, 0.f, -0.f, 6.f, 5.f}, {0.5f, 0.6f, 0.7f}, {0, 3}, {0, 1}, 2, 0.25f, -1.f, -1.f, 1);
      EXPECT(o.rc == 0 && o.st[6] == 3 && o.st[7] == 3 && o.ids[0] == 0 && o.ids[2] == 0 && o.ids[4] == 0 && o.ids[5] == 1); }
    // equal scores under the filter: the lower row wins
    { const int ids[] = {3, 4, 3, 5, 6, 5, 7, 8}; const float sc[] = {0.5f, 0.5f, 0.5f, 0.1f}; unsigned char keep[4];
      EXPECT(gf_keypoint_host_filter(ids, sc, 4, keep) == 0 && keep[0] == 1 && keep[1] == 0 && keep[2] == 0 && keep[3] == 1);
      EXPECT(gf_keypoint_host_filter(nullptr, nullptr, 0, nullptr) == 0); }
    // argument checks
    { Out o = run({1.f, 1.f, 1.f, 1.f}, {0.9f}, {0, 1}, {0, 0}, 1, 0.25f, 2.f, 4.f, 1); EXPECT(o.rc == -1); }
    { Out o = run({1.f, 1.f, 1.f, 1.f}, {0.9f}, {0, 1}, {0, 0}, 1, 0.25f, inf, 4.f, 1); EXPECT(o.rc == -1); }
    { Out o = run({1.f, 1.f, 1.f, 1.f}, {0.9f}, {0, 1}, {0, 0}, 524289, 0.25f, 48.f, 4.f, 1); EXPECT(o.rc == -1); }
    { Out o = run({1.f, 1.f, 1.f, 1.f}, {0.9f}, {0, 1}, {0, 0}, 1, 0.25f, 48.f, inf, 1); EXPECT(o.rc == 0 && o.st[6] == 1); }
    if (g_fail) return 1;
    printf("ok %lu\n", g_sum);
    return 0;
}
