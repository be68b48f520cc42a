// TEST INFRASTRUCTURE and CPU reference: the serial host form of k_camera.hip, compiled from the same camera_spec.h by the host C++
// compiler (geoformer_amd/build.py: -O2 -ffp-contract=off, no offload) into csrc/_obj/libcamera_host.so.  The tests compare the device
// against it bit for bit; nothing in the package loads it.
#include <stdint.h>

#include "../camera_spec.h"

extern "C" {

// gf_undistort_points (inverse = 1) / gf_distort_points (inverse = 0) as the device writes them: out [P][2], status [P] (may be null),
// flags [CM_FLAG_WORDS] (only ever set to 1).  Returns 0, or -1 (GF_ERR_INVALID_ARGUMENT) for arguments the device entry points reject.
int gf_camera_host_points(const float* pts, long pts_stride, int P, const int32_t* seg_off, const int32_t* seg_camera, int S,
                          const double* cameras, int C, int inverse, float* out, uint8_t* status, int32_t* flags) {
    if (P < 0 || S < 0 || C < 0 || S == 0x7FFFFFFF) return -1;
    if (P == 0) return 0;
    if (S == 0 || C == 0 || pts_stride < 2) return -1;
    if (!(pts && seg_off && seg_camera && cameras && out && flags) || (inverse && !status)) return -1;
    for (int j = 0; j <= S; ++j) cm_check_segment(seg_off, seg_camera, S, C, P, j, flags);
    for (int i = 0; i < P; ++i) {
        float o[2] = {__builtin_nanf(""), __builtin_nanf("")};
        int st = CM_ST_ARGS;
        const double* cam = cm_camera_of(seg_off, seg_camera, S, cameras, C, i, flags);
        if (cam) st = cm_point(cam, pts[pts_stride * (long)i], pts[pts_stride * (long)i + 1], inverse, o);
        out[2 * (size_t)i] = o[0]; out[2 * (size_t)i + 1] = o[1];
        if (status) status[i] = (uint8_t)st;
    }
    return 0;
}

// step 5 alone, for the tests' statistics: target (tx, ty) in normalised units -> xy [2], steps [1]; returns 1 when accepted
int gf_camera_host_undistort(const double* camera, double tx, double ty, double* xy, int32_t* steps) {
    int n = 0;
    const int ok = cm_undistort(camera, tx, ty, xy[0], xy[1], &n);
    steps[0] = n;
    return ok;
}

// step 4 alone, with the Jacobian: (x, y) -> xy [2], j [4]; returns 1 when the determinant is > 0
int gf_camera_host_distort(const double* camera, double x, double y, double* xy, double* j) {
    cm_distort(camera, x, y, xy[0], xy[1]);
    return cm_jacobian(camera, x, y, j) > 0.0;
}

}   // extern "C"
