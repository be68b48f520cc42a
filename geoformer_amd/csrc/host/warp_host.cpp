// TEST INFRASTRUCTURE: warp_spec.h (the text k_homo_pair.hip compiles for the device) compiled by the host C++ compiler
// (geoformer_amd/build.py: -O2 -ffp-contract=off, no offload) into csrc/_obj/libwarp_host.so.  The CPU tests compare the numpy
// restatement (train/homo_data.py) against it bit for bit; nothing in the package loads it.
#include <stdint.h>

#include "../warp_spec.h"

extern "C" {

// cv2.warpPerspective(src, M, (w, h)) for a gray uint8 image: src [hs][ws], rows `stride` bytes apart; minv [9] = inv(M); dst dense [h][w].
// Returns 0, or -1 for a null pointer or a size < 1.
int gf_warp_host_perspective_u8(const uint8_t* src, int hs, int ws, long long stride, const double* minv, int h, int w, uint8_t* dst) {
    if (!src || !minv || !dst || hs < 1 || ws < 1 || h < 1 || w < 1 || stride < ws) return -1;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            dst[(size_t)y * w + x] =
                (uint8_t)ws_warp_pixel(minv, x, y, hs, ws, [src, stride](int sx, int sy) { return (int)src[(size_t)sy * stride + sx]; });
    return 0;
}

// the source position (X, Y) of destination pixel (x, y) in 1/32 pixels
void gf_warp_host_position(const double* minv, int x, int y, int32_t* XY) {
    int X, Y;
    ws_position(minv, x, y, X, Y);
    XY[0] = X;
    XY[1] = Y;
}

// n values through the brightness / contrast rule, in place
void gf_warp_host_brightness_contrast(uint8_t* v, int n, float alpha, float beta) {
    const float b255 = beta * 255.f;
    for (int i = 0; i < n; ++i) v[i] = (uint8_t)ws_brightness_contrast(v[i], alpha, b255);
}

}   // extern "C"
