// The 8-bit resize of the image kernels (k_image_pre.hip, k_homo_pair.hip), shared: gray conversion of a tap, the three resize forms of
// matcher.cv2_resize_linear_u8 over an abstract pixel source, the output conversions and the kernel + launch scaffolding.
//   gray    (R*4899 + G*9617 + B*1868 + 2^13) >> 14, computed on the fly for the <= 2x2 source pixels of an output pixel;
//   resize  same size: copy;  exact 2x decimation in both directions: (a + b + c + d + 2) >> 2;  otherwise OpenCV's
//           fixed-point bilinear: 11-bit weights, horizontally index and fraction clamped together, vertically only the
//           row indices, dst = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2.
// The weights are computed per thread (no table to upload per shape) with the roundings of matcher._linear_coeffs:
// (d + 0.5) * scale - 0.5 as TWO fp64 roundings - a fused multiply-add rounds once and moves a weight by one unit for some
// (size, position) pairs, hence the contraction pragma - then fp32, floor, fp32 fraction, rint of f * 2048 and (1 - f) * 2048.
// Every intermediate fits int32: row terms <= 255 * 2048, b * (r >> 4) <= 2048 * 32640.
// Each thread produces 4 consecutive pixels of one output row; a block is 64 x 4 threads = 256 x 4 pixels.
//
// A pixel SOURCE is a struct with  Row row(int y) const  and  int at(Row& r, int x) const  (the 8-bit value of pixel (x, y), both
// inside the source's extent): a row pointer and a load for a decoded image, the row number and warp_spec.h's sample for a warped one.
#pragma once
#include <type_traits>

#include "gf_common.h"
#include "warp_spec.h"

namespace {

enum { kCopy = 0, kArea2 = 1, kLinear = 2 };
constexpr int kPix = 4;       // output pixels per thread

struct ResizeGeom {
    int hs, ws, ht, wt;        // extent of the pixel source, extent of the output
    double sx, sy;             // double(ws) / double(wt), double(hs) / double(ht)
};

struct ImgOut {
    void* dst;                 // dense [ht][wt]
    int vec;                   // dst rows take one aligned 4-pixel store per thread
    int bc;                    // apply ws_brightness_contrast(v, alpha, b255) to the resized value
    float alpha, b255;
};

__host__ __device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

template <int CH>
__host__ __device__ __forceinline__ int gray_at(const uint8_t* row, int x) {
    if constexpr (CH == 1) {
        return row[x];
    } else {
        const uint8_t* p = row + 3 * x;
        return (p[0] * 4899 + p[1] * 9617 + p[2] * 1868 + (1 << 13)) >> 14;
    }
}

// a decoded image in memory: uint8 [hs][ws][CH], rows `stride` bytes apart
template <int CH>
struct PlainSource {
    using Row = const uint8_t*;
    const uint8_t* src;
    long long stride;
    __host__ __device__ __forceinline__ Row row(int y) const { return src + (size_t)y * stride; }
    __host__ __device__ __forceinline__ int at(Row& r, int x) const { return gray_at<CH>(r, x); }
};

// source index and the two 11-bit weights of destination position d (matcher._linear_coeffs)
__host__ __device__ __forceinline__ void linear_coeff(int d, double scale, int ssize, bool clamp_index, int& s, int& w0, int& w1) {
#pragma clang fp contract(off)
    const double t = ((double)d + 0.5) * scale;
    float f = (float)(t - 0.5);
    const float fl = floorf(f);
    s = (int)fl;
    f = f - fl;
    if (clamp_index) {
        if (s < 0) { s = 0; f = 0.f; }
        if (s >= ssize - 1) { s = ssize - 1; f = 0.f; }
    }
    w1 = (int)rintf(f * 2048.f);
    w0 = (int)rintf((1.f - f) * 2048.f);
}

// the gray values (0 .. 255) of output pixels x0 .. x0 + 3 of output row y; positions beyond wt give 0 and read nothing
template <int MODE, class SRC>
__host__ __device__ __forceinline__ void pixels4(const SRC& s, const ResizeGeom& g, int x0, int y, int (&v)[kPix]) {
    if constexpr (MODE == kCopy) {
        typename SRC::Row r = s.row(y);
#pragma unroll
        for (int k = 0; k < kPix; ++k) v[k] = x0 + k < g.wt ? s.at(r, x0 + k) : 0;
    } else if constexpr (MODE == kArea2) {
        typename SRC::Row r0 = s.row(2 * y), r1 = s.row(2 * y + 1);
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            const int x = 2 * (x0 + k);
            v[k] = x0 + k < g.wt ? (s.at(r0, x) + s.at(r0, x + 1) + s.at(r1, x) + s.at(r1, x + 1) + 2) >> 2 : 0;
        }
    } else {
        int sy, b0, b1;
        linear_coeff(y, g.sy, g.hs, false, sy, b0, b1);
        typename SRC::Row r0 = s.row(clampi(sy, 0, g.hs - 1)), r1 = s.row(clampi(sy + 1, 0, g.hs - 1));
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            v[k] = 0;
            if (x0 + k < g.wt) {
                int sx, a0, a1;
                linear_coeff(x0 + k, g.sx, g.ws, true, sx, a0, a1);
                const int sx1 = sx + 1 < g.ws ? sx + 1 : g.ws - 1;
                const int t0 = s.at(r0, sx) * a0 + s.at(r0, sx1) * a1;
                const int t1 = s.at(r1, sx) * a0 + s.at(r1, sx1) * a1;
                v[k] = clampi((((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2, 0, 255);
            }
        }
    }
}

// GF_IMAGE_F32_NORMALISED: the correctly rounded quotient (v_div_scale / v_div_fmas / v_div_fixup: hipcc's default for fp32 division), what
// torch gives on the CPU.  GF_IMAGE_F32_NORMALISED_RCP: the product with fp32(1 / 255) - torch's DEVICE kernel for `tensor / 255.0` (a Python
// scalar divisor) multiplies by the rounded reciprocal, so this is what matcher.load_gray_scale_tensor's host path returns for a GPU;
// the two differ in the last bit for 126 of the 256 byte values.
template <int KIND>
__device__ __forceinline__ std::conditional_t<KIND == GF_IMAGE_U8, uint8_t, float> out_value(int v) {
    if constexpr (KIND == GF_IMAGE_U8) return (uint8_t)v;
    else if constexpr (KIND == GF_IMAGE_F32_NORMALISED) return (float)v / 255.0f;
    else return (float)v * (float)(1.0 / 255.0);
}

// BC: the kernel can apply the brightness / contrast rule (o.bc decides at run time); false compiles it out
template <class SRC, int MODE, int KIND, bool BC>
__global__ __launch_bounds__(256) void image_pre(SRC s, ResizeGeom g, ImgOut o) {
    using TO = std::conditional_t<KIND == GF_IMAGE_U8, uint8_t, float>;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * kPix;
    const int y = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= g.wt || y >= g.ht) return;
    int v[kPix];
    pixels4<MODE>(s, g, x0, y, v);
    if constexpr (BC) {
        if (o.bc) {
#pragma unroll
            for (int k = 0; k < kPix; ++k) v[k] = ws_brightness_contrast(v[k], o.alpha, o.b255);
        }
    }
    TO* out = (TO*)o.dst + (size_t)y * g.wt + x0;
    if (o.vec) {
        gf_vec<TO, kPix> w;
#pragma unroll
        for (int k = 0; k < kPix; ++k) w[k] = out_value<KIND>(v[k]);
        *reinterpret_cast<gf_vec<TO, kPix>*>(out) = w;
    } else {
#pragma unroll
        for (int k = 0; k < kPix; ++k)
            if (x0 + k < g.wt) out[k] = out_value<KIND>(v[k]);
    }
}

template <class SRC, int KIND, bool BC>
void launch_modes(const SRC& s, const ResizeGeom& g, const ImgOut& o, hipStream_t st) {
    const dim3 grid((g.wt + 64 * kPix - 1) / (64 * kPix), (g.ht + 3) / 4), block(64, 4);
    if (g.ws == g.wt && g.hs == g.ht) image_pre<SRC, kCopy, KIND, BC><<<grid, block, 0, st>>>(s, g, o);      // as cv2_resize_linear_u8 selects
    else if (g.ws == 2 * g.wt && g.hs == 2 * g.ht) image_pre<SRC, kArea2, KIND, BC><<<grid, block, 0, st>>>(s, g, o);
    else image_pre<SRC, kLinear, KIND, BC><<<grid, block, 0, st>>>(s, g, o);
}

template <class SRC, bool BC>
void launch_kinds(const SRC& s, const ResizeGeom& g, const ImgOut& o, int dst_kind, hipStream_t st) {
    if (dst_kind == GF_IMAGE_U8) launch_modes<SRC, GF_IMAGE_U8, BC>(s, g, o, st);
    else if (dst_kind == GF_IMAGE_F32_NORMALISED) launch_modes<SRC, GF_IMAGE_F32_NORMALISED, BC>(s, g, o, st);
    else launch_modes<SRC, GF_IMAGE_F32_NORMALISED_RCP, BC>(s, g, o, st);
}

inline ResizeGeom resize_geom(int hs, int ws, int ht, int wt) { return ResizeGeom{hs, ws, ht, wt, (double)ws / (double)wt, (double)hs / (double)ht}; }

inline ImgOut image_out(void* dst, int dst_kind, int wt) {
    const size_t store = dst_kind == GF_IMAGE_U8 ? kPix : kPix * sizeof(float);
    return ImgOut{dst, wt % kPix == 0 && (uintptr_t)dst % store == 0, 0, 1.f, 0.f};
}

}   // namespace
