// One image of a homography training pair, one launch: decoded uint8 image -> gray -> cv2.warpPerspective at the warp's own
// resolution -> cv2.resize -> brightness / contrast -> [ht, wt] uint8 or fp32 / 255 (homodataset/HomoDataset.py:83-123, get_pair).
// No warped image ever exists: the resize of image_resize.h (what gf_image_gray_resize runs) reads its <= 2x2 "source pixels" from a
// WarpSource, which computes each one in registers by warp_spec.h (the 8-bit bilinear warp, gray taken per tap), so the result has
// the bits of the two-stage form matcher.cv2_resize_linear_u8(homo_data.cv2_warp_perspective_u8(cv2_gray_u8(src), M, w, h), wt, ht).
// A gather over a source of at most a few MB (it sits in L2 after the first touch); per warped pixel ~14 fp64 operations and one fp64
// division, so the kernel is bound by neither: no LDS staging.  Thread shape as image_pre: 4 consecutive output pixels per thread.
// In the bilinear branch neighbouring output pixels share warped columns (always when enlarging, every other one when reducing by
// less than 2): each of the thread's two warped rows remembers its last two (column, value) pairs and samples a column once.
#include <math.h>

#include "image_resize.h"

namespace {

template <int CH>
struct WarpSource {
    struct Row {
        int y;
        int c0, v0, c1, v1;        // the last two columns sampled in this row
    };
    const uint8_t* src;            // uint8 [hs][ws][CH], rows `stride` bytes apart
    long long stride;
    int hs, ws;
    double minv[9];
    __host__ __device__ __forceinline__ Row row(int y) const { return Row{y, INT_MIN, 0, INT_MIN, 0}; }
    __host__ __device__ __forceinline__ int at(Row& r, int x) const {
        if (x == r.c1) return r.v1;
        if (x == r.c0) return r.v0;
        const uint8_t* s = src;
        const long long st = stride;
        const int v = ws_warp_pixel(minv, x, r.y, hs, ws, [s, st](int sx, int sy) { return gray_at<CH>(s + (size_t)sy * st, sx); });
        r.c0 = r.c1; r.v0 = r.v1;
        r.c1 = x; r.v1 = v;
        return v;
    }
};

template <int CH>
void launch_warp(const void* src, long long stride, int hs, int ws, const double* minv, const ResizeGeom& g, const ImgOut& o, int dst_kind,
                 hipStream_t st) {
    WarpSource<CH> s{(const uint8_t*)src, stride, hs, ws, {}};
    for (int k = 0; k < 9; ++k) s.minv[k] = minv[k];
    launch_kinds<WarpSource<CH>, true>(s, g, o, dst_kind, st);
}

}   // namespace

extern "C" int gf_image_warp_resize(const void* src, int channels, int hs, int ws, long long src_row_stride_bytes, const double* minv,
                                    int warp_h, int warp_w, void* dst, int dst_kind, int ht, int wt, const float* brightness_contrast,
                                    void* stream) {
    GF_CHECK_ARG(src, "src is a null pointer");
    GF_CHECK_ARG(dst, "dst is a null pointer");
    GF_CHECK_ARG(minv, "minv is a null pointer");
    GF_CHECK_ARG(channels == 1 || channels == 3, "channels must be 1 or 3");
    GF_CHECK_ARG(hs > 0 && ws > 0, "hs and ws must be positive");
    GF_CHECK_ARG(warp_h > 0 && warp_w > 0, "warp_h and warp_w must be positive");
    GF_CHECK_ARG(ht > 0 && wt > 0, "ht and wt must be positive");
    GF_CHECK_ARG(src_row_stride_bytes >= (long long)ws * channels, "src_row_stride_bytes is smaller than ws * channels");
    GF_CHECK_ARG(dst_kind >= GF_IMAGE_U8 && dst_kind <= GF_IMAGE_F32_NORMALISED_RCP, "unknown dst_kind");
    GF_CHECK_ARG(ht <= 4 * 65535, "ht is larger than 262140");
    bool finite = true, identity = true;
    for (int k = 0; k < 9; ++k) {
        finite = finite && isfinite(minv[k]);
        identity = identity && minv[k] == (k % 4 == 0 ? 1.0 : 0.0);
    }
    GF_CHECK_ARG(finite, "minv has a non-finite entry");
    ResizeGeom g = resize_geom(warp_h, warp_w, ht, wt);
    ImgOut o = image_out(dst, dst_kind, wt);
    if (brightness_contrast) {
        GF_CHECK_ARG(isfinite(brightness_contrast[0]) && isfinite(brightness_contrast[1]), "brightness_contrast has a non-finite entry");
        o.bc = 1;
        o.alpha = brightness_contrast[0];
        o.b255 = brightness_contrast[1] * 255.f;
    }
    hipStream_t st = (hipStream_t)stream;
    if (identity && warp_h == hs && warp_w == ws) {
        // image 0 of a pair: the identity warp at the source's size returns the source (X = 32 x: one tap of weight 1024), so the
        // plain source of gf_image_gray_resize gives the same bits without the warp arithmetic
        if (channels == 1) launch_kinds<PlainSource<1>, true>(PlainSource<1>{(const uint8_t*)src, src_row_stride_bytes}, g, o, dst_kind, st);
        else launch_kinds<PlainSource<3>, true>(PlainSource<3>{(const uint8_t*)src, src_row_stride_bytes}, g, o, dst_kind, st);
    } else if (channels == 1) {
        launch_warp<1>(src, src_row_stride_bytes, hs, ws, minv, g, o, dst_kind, st);
    } else {
        launch_warp<3>(src, src_row_stride_bytes, hs, ws, minv, g, o, dst_kind, st);
    }
    GF_CHECK_LAUNCH();
    return GF_OK;
}
