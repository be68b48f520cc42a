// Image preprocessing of the matcher, one launch: decoded uint8 image -> gray -> resize -> [ht, wt] uint8 or fp32 / 255 (two roundings, below)
// (load_gray_scale_tensor_cv, eval_tool/immatch/utils/data_io.py:48-62: cv2.imread(IMREAD_GRAYSCALE), cv2.resize, to_tensor).
// Bit-identical to the host restatement in geoformer_amd/matcher.py (cv2_gray_u8 + cv2_resize_linear_u8):
//   gray    (R*4899 + G*9617 + B*1868 + 2^13) >> 14, computed on the fly for the <= 2x2 source pixels of an output pixel;
//   resize  same size: copy;  exact 2x decimation in both directions: (a + b + c + d + 2) >> 2;  otherwise OpenCV's
//           fixed-point bilinear: 11-bit weights, horizontally index and fraction clamped together, vertically only the
//           row indices, dst = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2.
// The weights are computed per thread (no table to upload per shape) with the roundings of matcher._linear_coeffs:
// (d + 0.5) * scale - 0.5 as TWO fp64 roundings - a fused multiply-add rounds once and moves a weight by one unit for some
// (size, position) pairs, hence the contraction pragma - then fp32, floor, fp32 fraction, rint of f * 2048 and (1 - f) * 2048.
// Every intermediate fits int32: row terms <= 255 * 2048, b * (r >> 4) <= 2048 * 32640.
// Each thread produces 4 consecutive pixels of one output row; a block is 64 x 4 threads = 256 x 4 pixels.
#include <type_traits>

#include "gf_common.h"

namespace {

enum { kCopy = 0, kArea2 = 1, kLinear = 2 };
constexpr int kPix = 4;       // output pixels per thread

struct ImgArgs {
    const uint8_t* src;
    long long stride;          // bytes between source rows
    void* dst;                 // dense [ht][wt]
    int hs, ws, ht, wt;
    double sx, sy;             // double(ws) / double(wt), double(hs) / double(ht)
    int vec;                   // dst rows take one aligned 4-pixel store per thread
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
template <int CH, int MODE>
__host__ __device__ __forceinline__ void pixels4(const ImgArgs& a, int x0, int y, int (&v)[kPix]) {
    if constexpr (MODE == kCopy) {
        const uint8_t* r = a.src + (size_t)y * a.stride;
#pragma unroll
        for (int k = 0; k < kPix; ++k) v[k] = x0 + k < a.wt ? gray_at<CH>(r, x0 + k) : 0;
    } else if constexpr (MODE == kArea2) {
        const uint8_t* r0 = a.src + (size_t)(2 * y) * a.stride;
        const uint8_t* r1 = r0 + a.stride;
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            const int x = 2 * (x0 + k);
            v[k] = x0 + k < a.wt ? (gray_at<CH>(r0, x) + gray_at<CH>(r0, x + 1) + gray_at<CH>(r1, x) + gray_at<CH>(r1, x + 1) + 2) >> 2 : 0;
        }
    } else {
        int sy, b0, b1;
        linear_coeff(y, a.sy, a.hs, false, sy, b0, b1);
        const uint8_t* r0 = a.src + (size_t)clampi(sy, 0, a.hs - 1) * a.stride;
        const uint8_t* r1 = a.src + (size_t)clampi(sy + 1, 0, a.hs - 1) * a.stride;
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            v[k] = 0;
            if (x0 + k < a.wt) {
                int sx, a0, a1;
                linear_coeff(x0 + k, a.sx, a.ws, true, sx, a0, a1);
                const int sx1 = sx + 1 < a.ws ? sx + 1 : a.ws - 1;
                const int t0 = gray_at<CH>(r0, sx) * a0 + gray_at<CH>(r0, sx1) * a1;
                const int t1 = gray_at<CH>(r1, sx) * a0 + gray_at<CH>(r1, sx1) * a1;
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

template <int CH, int MODE, int KIND>
__global__ __launch_bounds__(256) void image_pre(ImgArgs a) {
    using TO = std::conditional_t<KIND == GF_IMAGE_U8, uint8_t, float>;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * kPix;
    const int y = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= a.wt || y >= a.ht) return;
    int v[kPix];
    pixels4<CH, MODE>(a, x0, y, v);
    TO* o = (TO*)a.dst + (size_t)y * a.wt + x0;
    if (a.vec) {
        gf_vec<TO, kPix> w;
#pragma unroll
        for (int k = 0; k < kPix; ++k) w[k] = out_value<KIND>(v[k]);
        *reinterpret_cast<gf_vec<TO, kPix>*>(o) = w;
    } else {
#pragma unroll
        for (int k = 0; k < kPix; ++k)
            if (x0 + k < a.wt) o[k] = out_value<KIND>(v[k]);
    }
}

template <int CH, int KIND>
void launch_modes(const ImgArgs& a, int mode, hipStream_t st) {
    const dim3 grid((a.wt + 64 * kPix - 1) / (64 * kPix), (a.ht + 3) / 4), block(64, 4);
    if (mode == kCopy) image_pre<CH, kCopy, KIND><<<grid, block, 0, st>>>(a);
    else if (mode == kArea2) image_pre<CH, kArea2, KIND><<<grid, block, 0, st>>>(a);
    else image_pre<CH, kLinear, KIND><<<grid, block, 0, st>>>(a);
}

template <int KIND>
void launch_channels(const ImgArgs& a, int channels, int mode, hipStream_t st) {
    if (channels == 1) launch_modes<1, KIND>(a, mode, st);
    else launch_modes<3, KIND>(a, mode, st);
}

}   // namespace

extern "C" int gf_image_gray_resize(const void* src, int channels, int hs, int ws, long long src_row_stride_bytes, void* dst,
                                    int dst_kind, int ht, int wt, void* stream) {
    GF_CHECK_ARG(src, "src is a null pointer");
    GF_CHECK_ARG(dst, "dst is a null pointer");
    GF_CHECK_ARG(channels == 1 || channels == 3, "channels must be 1 or 3");
    GF_CHECK_ARG(hs > 0 && ws > 0, "hs and ws must be positive");
    GF_CHECK_ARG(ht > 0 && wt > 0, "ht and wt must be positive");
    GF_CHECK_ARG(src_row_stride_bytes >= (long long)ws * channels, "src_row_stride_bytes is smaller than ws * channels");
    GF_CHECK_ARG(dst_kind >= GF_IMAGE_U8 && dst_kind <= GF_IMAGE_F32_NORMALISED_RCP, "unknown dst_kind");
    GF_CHECK_ARG(ht <= 4 * 65535, "ht is larger than 262140");
    ImgArgs a{(const uint8_t*)src, src_row_stride_bytes, dst, hs, ws, ht, wt, (double)ws / (double)wt, (double)hs / (double)ht, 0};
    const int mode = (ws == wt && hs == ht) ? kCopy : (ws == 2 * wt && hs == 2 * ht) ? kArea2 : kLinear;      // as cv2_resize_linear_u8 selects
    const size_t store = dst_kind == GF_IMAGE_U8 ? kPix : kPix * sizeof(float);
    a.vec = wt % kPix == 0 && (uintptr_t)dst % store == 0;
    hipStream_t st = (hipStream_t)stream;
    if (dst_kind == GF_IMAGE_U8) launch_channels<GF_IMAGE_U8>(a, channels, mode, st);
    else if (dst_kind == GF_IMAGE_F32_NORMALISED) launch_channels<GF_IMAGE_F32_NORMALISED>(a, channels, mode, st);
    else launch_channels<GF_IMAGE_F32_NORMALISED_RCP>(a, channels, mode, st);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
