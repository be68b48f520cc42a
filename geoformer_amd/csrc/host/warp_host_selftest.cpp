// TEST INFRASTRUCTURE: a stand-alone sanitizer run of warp_host.cpp (warp_spec.h on the host) over matrices chosen to reach every guard:
//   c++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all warp_host.cpp warp_host_selftest.cpp -o t && ./t
// identity, all-outside, a horizon inside the image (W == 0 on a row), overflowing and underflowing entries, W == 0 everywhere, negative
// positions, denormal W (32 / W = inf, 0 * inf = NaN), positions beyond int32, an infinite entry; and the brightness / contrast rule far
// outside [0, 255].  Prints "ok" and a checksum; the sanitizers abort on any out-of-range conversion, overflow or out-of-bounds read.
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include <limits>
extern "C" int gf_warp_host_perspective_u8(const uint8_t* src, int hs, int ws, long long stride, const double* minv, int h, int w, uint8_t* dst);
extern "C" void gf_warp_host_brightness_contrast(uint8_t* v, int n, float alpha, float beta);
int main() {
    const int hs = 37, ws = 53;
    std::vector<uint8_t> src(hs * ws), dst(64 * 80);
    for (size_t i = 0; i < src.size(); ++i) src[i] = (uint8_t)(i * 37 + 11);
    const double inf = std::numeric_limits<double>::infinity();
    double ms[][9] = {{1,0,0,0,1,0,0,0,1}, {1,0,-1000,0,1,-1000,0,0,1}, {1,0,0,0,1,0,0,-0.05,1}, {1e300,0,0,0,1e300,0,0,0,1e-300},
                      {1.3,0,-4.3,0,1.3,-2.6,0,0,1}, {0,0,0,0,0,0,0,0,0}, {1e308,1e308,1e308,-1e308,-1e308,-1e308,1e-320,0,0},
                      {1,0,0,0,1,0,0,0,5e-324}, {-1,0,1e9,0,-1,-1e9,0,0,1}, {inf,0,0,0,1,0,0,0,1}};
    unsigned long sum = 0;
    for (auto& m : ms) {
        if (gf_warp_host_perspective_u8(src.data(), hs, ws, ws, m, 64, 80, dst.data()) != 0) return 1;
        for (uint8_t v : dst) sum += v;
    }
    uint8_t v[256];
    for (float a : {1.f, 1.3f, 0.7f, 1e30f, -1e30f}) for (float b : {0.f, 0.2f, -0.2f, 1e30f}) { for (int i = 0; i < 256; ++i) v[i] = (uint8_t)i; gf_warp_host_brightness_contrast(v, 256, a, b); sum += v[7]; }
    printf("ok %lu\n", sum);
    return 0;
}
