// Lens distortion on the device: match coordinates of real cameras -> pixels of an ideal pinhole camera with the same fx, fy, cx, cy
// (gf_undistort_points), and back (gf_distort_points), before any geometry runs.  The kernel runs, operation for operation and in fp64 with
// contraction off, the rule stated in camera_spec.h, which host/camera_host.cpp compiles for the CPU: every output can be checked bit
// for bit.
//
//   camera_points : one thread per point; thread j <= S also checks boundary j of the segment offsets and segment j's camera index.  The
//                   point's segment by bisection of the offsets, its camera record from the table in device memory, cm_point.  The Newton
//                   loop's trip count differs per lane: a wave runs until its last lane is done, at most CM_MAX_STEPS steps.  A point's
//                   outputs are written by its own thread only; the two flag words only ever receive the value 1 (plain stores: no
//                   atomics, no dependency between workgroups).  One launch serves all segments of one point list.
// No host synchronisation; every output is the same in every run.
#include "gf_common.h"
#include "camera_spec.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void camera_points(const float* pts, long pts_stride, int P, const int32_t* seg_off, const int32_t* seg_camera,
                                                     int S, const double* cameras, int C, int inverse, float* out, uint8_t* status,
                                                     int32_t* flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i <= S) cm_check_segment(seg_off, seg_camera, S, C, P, (int)i, flags);
    if (i >= P) return;
    float o[2] = {__builtin_nanf(""), __builtin_nanf("")};
    int st = CM_ST_ARGS;
    const double* cam = cm_camera_of(seg_off, seg_camera, S, cameras, C, (int)i, flags);
    if (cam) {
        double c[CM_REC];
        for (int k = 0; k < CM_REC; ++k) c[k] = cam[k];
        st = cm_point(c, pts[pts_stride * i], pts[pts_stride * i + 1], inverse, o);
    }
    out[2 * (size_t)i] = o[0]; out[2 * (size_t)i + 1] = o[1];
    if (status) status[i] = (uint8_t)st;
}

int camera_run(const char* name, const float* pts, long pts_stride, int P, const int32_t* seg_off, const int32_t* seg_camera, int S,
               const double* cameras, int C, int inverse, float* out, uint8_t* status, int32_t* flags, void* stream) {
    if (P < 0 || S < 0 || C < 0 || S == 0x7FFFFFFF) {
        gf_set_error("%s: need P >= 0, 0 <= S < 2^31 - 1 and C >= 0", name);
        return GF_ERR_INVALID_ARGUMENT;
    }
    if (P == 0) return GF_OK;
    if (S == 0 || C == 0 || pts_stride < 2) {
        gf_set_error("%s: points without a segment or a camera, or pts_stride < 2", name);
        return GF_ERR_INVALID_ARGUMENT;
    }
    if (!(pts && seg_off && seg_camera && cameras && out && flags) || (inverse && !status)) {
        gf_set_error("%s: null pointer", name);
        return GF_ERR_INVALID_ARGUMENT;
    }
    const long n = P > S + 1 ? (long)P : (long)S + 1;
    camera_points<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(pts, pts_stride, P, seg_off, seg_camera, S, cameras, C, inverse,
                                                                                 out, status, flags);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        gf_set_error("%s: launch failed: %s", name, hipGetErrorString(e));
        return GF_ERR_LAUNCH;
    }
    return GF_OK;
}

}   // namespace

extern "C" int gf_undistort_points(const float* pts, long pts_stride, int P, const int32_t* seg_offsets, const int32_t* seg_camera, int S,
                                   const double* cameras, int C, float* out, uint8_t* status, int32_t* flags, void* stream) {
    return camera_run("gf_undistort_points", pts, pts_stride, P, seg_offsets, seg_camera, S, cameras, C, 1, out, status, flags, stream);
}

extern "C" int gf_distort_points(const float* pts, long pts_stride, int P, const int32_t* seg_offsets, const int32_t* seg_camera, int S,
                                 const double* cameras, int C, float* out, uint8_t* status, int32_t* flags, void* stream) {
    return camera_run("gf_distort_points", pts, pts_stride, P, seg_offsets, seg_camera, S, cameras, C, 0, out, status, flags, stream);
}
