// Image preprocessing of the matcher, one launch: decoded uint8 image -> gray -> resize -> [ht, wt] uint8 or fp32 / 255 (two roundings, below)
// (load_gray_scale_tensor_cv, eval_tool/immatch/utils/data_io.py:48-62: cv2.imread(IMREAD_GRAYSCALE), cv2.resize, to_tensor).
// Bit-identical to the host restatement in geoformer_amd/matcher.py (cv2_gray_u8 + cv2_resize_linear_u8):
//   gray    (R*4899 + G*9617 + B*1868 + 2^13) >> 14, computed on the fly for the <= 2x2 source pixels of an output pixel;
//   resize  same size: copy;  exact 2x decimation in both directions: (a + b + c + d + 2) >> 2;  otherwise OpenCV's
//           fixed-point bilinear: 11-bit weights, horizontally index and fraction clamped together, vertically only the
//           row indices, dst = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2.
// The resize arithmetic, the kernel and its launch scaffolding live in image_resize.h, shared with k_homo_pair.hip (the same resize
// over a perspective-warped source); this file instantiates them for a decoded image in memory, without the brightness / contrast step.
#include "image_resize.h"

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
    const ResizeGeom g = resize_geom(hs, ws, ht, wt);
    const ImgOut o = image_out(dst, dst_kind, wt);
    hipStream_t st = (hipStream_t)stream;
    if (channels == 1) launch_kinds<PlainSource<1>, false>(PlainSource<1>{(const uint8_t*)src, src_row_stride_bytes}, g, o, dst_kind, st);
    else launch_kinds<PlainSource<3>, false>(PlainSource<3>{(const uint8_t*)src, src_row_stride_bytes}, g, o, dst_kind, st);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
