// Perspective warp of an 8-bit image and the brightness / contrast rule of the homography-pair generator: the arithmetic, stated once
// for the device (k_homo_pair.hip), the host build (host/warp_host.cpp) and, line for line, numpy (train/homo_data.py:
// cv2_warp_perspective_u8, brightness_contrast_u8).
//
// ws_warp_pixel states cv2.warpPerspective(src_u8, M, (w, h)) with the defaults homodataset/HomoDataset.py:96 uses - INTER_LINEAR,
// BORDER_CONSTANT 0, a forward M - in the form of OpenCV's published 8-bit path (imgproc/imgwarp.cpp, WarpPerspectiveInvoker +
// remapBilinear<FixedPtCast<int, uchar, 15>>).  The caller inverts M in fp64 and passes Minv.  For destination pixel (x, y), in fp64
// with contraction off and the sums taken left to right:
//     W  = Minv[6] * x + Minv[7] * y + Minv[8];   W = W ? 32 / W : 0              (INTER_TAB_SIZE = 32)
//     fX = max(INT_MIN, min(INT_MAX, (Minv[0] * x + Minv[1] * y + Minv[2]) * W)),  fY likewise from Minv[3..5]
//          (std::min / std::max as comparisons: a NaN product - 0 * inf - becomes INT_MAX, never a NaN-derived index)
//     X  = lrint(fX), Y = lrint(fY)                                                round half to even
//     sx = X >> 5, ax = X & 31, sy = Y >> 5, ay = Y & 31                           arithmetic shift: negative positions floor
//     dst = ((32 - ax) (32 - ay) p00 + ax (32 - ay) p01 + (32 - ax) ay p10 + ax ay p11 + 512) >> 10
// with p00 = src[sy][sx], p01 = src[sy][sx + 1], p10 = src[sy + 1][sx], p11 = src[sy + 1][sx + 1], a tap outside the source
// counting 0, each of the four tested on its own.  The last line IS OpenCV's 15-bit weight table with its (+ (1 << 14)) >> 15
// rounding: for the bilinear table every weight 32 (32 - ax) (32 - ay) is an exact integer, the table's sum-to-32768 fix-up never
// fires, and the common factor 32 cancels against the shift - so no table.
//
// ONE STATED DEVIATION.  OpenCV evaluates the three numerators incrementally over 16 x 64 blocks (X0 + M[0] * x1 with X0 carried per
// block row), so its result depends on the block and thread split; here they are evaluated per pixel.  The two can differ where an
// fp64 rounding crosses a 1/32-pixel boundary.  OpenCV is absent from the build container: parity with cv2 is UNPINNED, as at every
// OpenCV boundary of this project; what is pinned is the arithmetic written here (hand-derived vectors in tests/test_homo_data_cpu.py).
//
// ws_brightness_contrast is albumentations' look-up-table rule for uint8 images (RandomBrightness / RandomContrast,
// brightness_contrast_adjust with beta_by_max): v -> clip(trunc(fp32(v) * alpha + beta * 255), 0, 255), every operation in fp32 and
// unfused (alpha, beta fp32; b255 = beta * 255 is formed once, in fp32).  It applies to the RESIZED uint8 image, before the division.
#pragma once
#include <limits.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define WS_HD __host__ __device__ inline
#else
#define WS_HD static inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define WS_TAB_BITS 5                               /* INTER_BITS: positions in 1/32 pixel */
#define WS_TAB_SIZE (1 << WS_TAB_BITS)

// source position of destination pixel (x, y) in 1/32 pixels
WS_HD void ws_position(const double* Minv, int x, int y, int& X, int& Y) {
    const double dx = (double)x, dy = (double)y;
    double W = Minv[6] * dx + Minv[7] * dy + Minv[8];
    W = W != 0.0 ? (double)WS_TAB_SIZE / W : 0.0;
    double fX = (Minv[0] * dx + Minv[1] * dy + Minv[2]) * W;
    double fY = (Minv[3] * dx + Minv[4] * dy + Minv[5]) * W;
    fX = fX < (double)INT_MAX ? fX : (double)INT_MAX;            // std::min((double)INT_MAX, fX): a NaN lands here
    fX = (double)INT_MIN < fX ? fX : (double)INT_MIN;            // std::max((double)INT_MIN, .)
    fY = fY < (double)INT_MAX ? fY : (double)INT_MAX;
    fY = (double)INT_MIN < fY ? fY : (double)INT_MIN;
    X = (int)rint(fX);
    Y = (int)rint(fY);
}

// fetch(sx, sy) -> the 8-bit value of source pixel (sx, sy); called for pixels inside [0, ws) x [0, hs) only
template <class Fetch>
WS_HD int ws_tap(const Fetch& fetch, int sx, int sy, int hs, int ws) {
    return (unsigned)sx < (unsigned)ws && (unsigned)sy < (unsigned)hs ? fetch(sx, sy) : 0;
}

// the warped image's pixel (x, y), 0 .. 255
template <class Fetch>
WS_HD int ws_warp_pixel(const double* Minv, int x, int y, int hs, int ws, const Fetch& fetch) {
    int X, Y;
    ws_position(Minv, x, y, X, Y);
    const int sx = X >> WS_TAB_BITS, ax = X & (WS_TAB_SIZE - 1), sy = Y >> WS_TAB_BITS, ay = Y & (WS_TAB_SIZE - 1);
    if (sx < -1 || sx >= ws || sy < -1 || sy >= hs) return 0;   // all four taps outside (also keeps sx + 1, sy + 1 from overflowing)
    const int p00 = ws_tap(fetch, sx, sy, hs, ws), p01 = ws_tap(fetch, sx + 1, sy, hs, ws);
    const int p10 = ws_tap(fetch, sx, sy + 1, hs, ws), p11 = ws_tap(fetch, sx + 1, sy + 1, hs, ws);
    const int bx = WS_TAB_SIZE - ax, by = WS_TAB_SIZE - ay;
    return (bx * by * p00 + ax * by * p01 + bx * ay * p10 + ax * ay * p11 + 512) >> 10;
}

// v in 0 .. 255, b255 = beta * 255.f
WS_HD int ws_brightness_contrast(int v, float alpha, float b255) {
    const float t = truncf((float)v * alpha + b255);
    return t < 0.f ? 0 : t > 255.f ? 255 : (int)t;
}
