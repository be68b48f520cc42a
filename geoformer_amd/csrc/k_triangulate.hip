// On-device triangulation of database tracks from known poses: the connected components of the keypoint match graph (tracks), then one
// 3-D point per track.  The kernels run, operation for operation and in fp64 with contraction off, the algorithm stated in tri_solver.h,
// which host/tri_host.cpp compiles for the CPU: every output can be checked bit for bit.  COLMAP parity is UNPINNED.
//
//   track_init    : one thread per node: parent[v] = v.
//   track_link    : one thread per edge, a lock-free union-find.  Both roots by path halving (a parent is only ever replaced by one of
//                   its ancestors, through atomicMin: parents never increase).  While the roots differ, atomicCAS(&parent[hi], hi, lo) with
//                   hi > lo; on failure the walk continues from the value read.  A failed CAS means another thread linked hi: global
//                   progress, so the loop ends, and it is no spin lock - lock-step lanes of one wave cannot deadlock in it.  Every link
//                   points to a smaller node, so a root is its tree's minimum, and the final partition and every component's root do not
//                   depend on the order of execution.
//   track_flatten : one thread per node: parent[v] = root(v).  A concurrent writer only replaces a parent by that node's root: either
//                   value leads to the same root.
//   (the track list between the two halves is torch's: a stable sort of the nodes by root and scans - ops.build_tracks.)
//   tri_cams      : one thread per image: tr_cam_ok and the camera centre.
//   tri_prepare   : one thread per track: effective length, conflict, the number of hypotheses H (0 for a conflict), best = -1; the
//                   exclusive scan of H inside the block of 256 tracks through LDS, and the block's sum.
//   tri_scan      : one workgroup: the exclusive scan of the block sums, 256 at a time.
//   tri_hypotheses: the dense form - one thread per (track, hypothesis) SLOT, no wave per track: most tracks have two or three
//                   observations and one to three hypotheses.  A slot finds its block of tracks by bisection of the block offsets and its
//                   track by bisection of the block's scan.  The thread solves the two-view midpoint, scores it over the track's
//                   observations (a loop over global memory, no cap on the length) and does atomicMax(best + track, rt_key(count, t)):
//                   keys of different hypotheses are distinct, so the maximum does not depend on the order.  The number of slots is only
//                   known on the device: the grid covers min(64 T, 6 n_obs) >= the sum of H (H <= 6 L for every L), and a thread past the
//                   sum leaves after one load.
//   tri_finish    : one thread per track: the winner again from its key, the refit rounds with the 3 x 3 solve in an LDS tile interleaved
//                   across the threads, the outputs and the observation mask (tr_track_finish).
// All on the caller's stream, no host synchronisation; integer atomics only, so every output is the same in every run.
#include "gf_common.h"
#include "tri_solver.h"
#include "ransac_tile.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ int tk_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x, halving the path on the way
__device__ __forceinline__ int tk_find(int32_t* parent, int x) {
    int p = tk_load(parent + x);
    while (p != x) {
        const int gp = tk_load(parent + p);
        if (gp != p) atomicMin(parent + x, gp);
        x = p;
        p = gp;
    }
    return x;
}

__global__ __launch_bounds__(256) void track_init(int32_t* parent, int n_nodes, int32_t* status) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v == 0) *status = 0;
    if (v < n_nodes) parent[v] = (int)v;
}

__global__ __launch_bounds__(256) void track_link(const int32_t* ids, const int32_t* id_off, const int32_t* pair_images, int P, int E,
                                                  const int32_t* kp_off, int n_images, int n_nodes, int32_t* parent, int32_t* status) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    int u, v;
    if (!tr_edge_nodes(ids, id_off, pair_images, P, kp_off, n_images, n_nodes, (int)e, u, v)) {      // (u, v in [0, n_nodes) otherwise)
        atomicOr(status, TR_FLAG_EDGE_RANGE);
        return;
    }
    int a = tk_find(parent, u), b = tk_find(parent, v);
    while (a != b) {
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int seen = atomicCAS(parent + hi, hi, lo);
        if (seen == hi) break;                                         // linked
        a = tk_find(parent, seen);                                     // hi had been linked below itself by another thread
        b = tk_find(parent, lo);
    }
}

__global__ __launch_bounds__(256) void track_flatten(int32_t* parent, int n_nodes) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_nodes) return;
    int x = (int)v, p = tk_load(parent + x);
    while (p != x) {
        x = p;
        p = tk_load(parent + x);
    }
    parent[v] = x;
}

struct TriArgs {
    TrView v;
    const int32_t* track_off;    // [T + 1]
    int T, n_obs, nb;            // nb: blocks of 256 tracks
    int32_t* cam_ok;             // [n_images]
    double* cam_o;               // [n_images][3]
    int32_t* leff;               // [T]
    int32_t* slot_loc;           // [T]       exclusive scan of H inside the track's block
    int32_t* nhyp;               // [T]
    int32_t* blk_off;            // [nb + 1]  block sums, then their exclusive scan (the last entry: all slots)
    long long* best;             // [T]
    double* X;
    int32_t *valid, *conflict, *n_inliers, *hypothesis, *rounds;
    double* err2;
    uint8_t* inliers;
};

__global__ __launch_bounds__(256) void tri_cams(TriArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.v.n_images) return;
    const double* R = a.v.R + 9 * (size_t)i;
    const double* t = a.v.t + 3 * (size_t)i;
    double o[3];
    tr_centre(R, t, o);
    a.cam_ok[i] = tr_cam_ok(a.v.K + 9 * (size_t)i, R, t);
    a.cam_o[3 * (size_t)i] = o[0]; a.cam_o[3 * (size_t)i + 1] = o[1]; a.cam_o[3 * (size_t)i + 2] = o[2];
}

__global__ __launch_bounds__(256) void tri_prepare(TriArgs a) {
    __shared__ int s_scan[256];
    const int tid = threadIdx.x, k = blockIdx.x * 256 + tid;
    int H = 0;
    if (k < a.T) {
        int off, len, L, conflict;
        gs_offsets_range(a.track_off, k, a.n_obs, off, len);         // (offsets come from device memory: clamped into the buffers)
        tr_track_scan(a.v, off, off + len, L, conflict);
        H = conflict ? 0 : tr_hyp_count(L);
        a.leff[k] = L;
        a.conflict[k] = conflict;
        a.nhyp[k] = H;
        a.best[k] = -1ll;
    }
    s_scan[tid] = H;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {                                // inclusive scan (integers: order-free)
        const int add = tid >= s ? s_scan[tid - s] : 0;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    if (k < a.T) a.slot_loc[k] = s_scan[tid] - H;
    if (tid == 255) a.blk_off[blockIdx.x] = s_scan[255];
}

__global__ __launch_bounds__(256) void tri_scan(TriArgs a) {
    __shared__ int s_scan[256];
    __shared__ int s_base;
    const int tid = threadIdx.x;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < a.nb; i0 += 256) {
        const int i = i0 + tid;
        const int h = i < a.nb ? a.blk_off[i] : 0;
        s_scan[tid] = h;
        __syncthreads();
        for (int s = 1; s < 256; s <<= 1) {
            const int add = tid >= s ? s_scan[tid - s] : 0;
            __syncthreads();
            s_scan[tid] += add;
            __syncthreads();
        }
        const int base = s_base;
        if (i < a.nb) a.blk_off[i] = base + s_scan[tid] - h;
        __syncthreads();
        if (tid == 255) s_base = base + s_scan[255];
        __syncthreads();
    }
    if (tid == 0) a.blk_off[a.nb] = s_base;
}

__global__ __launch_bounds__(256) void tri_hypotheses(TriArgs a) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long)a.blk_off[a.nb]) return;
    int lo = 0, hi = a.nb;                                             // the last block of tracks whose first slot is <= g
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((long)a.blk_off[mid] <= g) lo = mid; else hi = mid;
    }
    const int r = (int)(g - a.blk_off[lo]);
    int klo = lo * 256, khi = min(klo + 256, a.T);                     // the last track of the block whose first slot is <= r
    while (khi - klo > 1) {
        const int mid = klo + ((khi - klo) >> 1);
        if (a.slot_loc[mid] <= r) klo = mid; else khi = mid;
    }
    const int k = klo, t = r - a.slot_loc[k];
    if (t < 0 || t >= a.nhyp[k]) return;                               // (cannot happen for consistent scans)
    int off, len;
    gs_offsets_range(a.track_off, k, a.n_obs, off, len);
    const int c = tr_hypothesis(a.v, (uint32_t)k, off, off + len, a.leff[k], t);
    if (c >= 0) atomicMax(a.best + k, rt_key(c, t));
}

__global__ __launch_bounds__(256) void tri_finish(TriArgs a) {
    __shared__ double ws[TR_GN_WS_DOUBLES * 256];
    const int tid = threadIdx.x, k = blockIdx.x * 256 + tid;
    if (k >= a.T) return;
    int off, len;
    gs_offsets_range(a.track_off, k, a.n_obs, off, len);
    tr_track_finish(a.v, (uint32_t)k, off, off + len, a.leff[k], a.conflict[k], rt_key_hyp(a.best[k]), GsWs{ws + tid, 256}, a.X + 3 * (size_t)k,
                    a.valid + k, a.n_inliers + k, a.hypothesis + k, a.rounds + k, a.err2 + k, a.inliers);
}

}   // namespace

extern "C" int gf_track_link(const int32_t* ids, const int32_t* id_off, const int32_t* pair_images, int P, int E, const int32_t* kp_off,
                             int n_images, int n_nodes, int32_t* parent, int32_t* status, void* stream) {
    GF_CHECK_ARG(id_off && kp_off && parent && status && (E == 0 || (ids && pair_images)), "null pointer");
    GF_CHECK_ARG(P >= 0 && E >= 0 && n_images >= 0 && n_nodes >= 0, "need P, E, n_images, n_nodes >= 0 (each below 2^31)");
    hipStream_t st = (hipStream_t)stream;
    void* tok = gf_prof_begin("track_link", st, (double)E);
    track_init<<<(unsigned)(((long)n_nodes + 255) / 256 + (n_nodes == 0)), 256, 0, st>>>(parent, n_nodes, status);
    if (E > 0) track_link<<<(unsigned)(((long)E + 255) / 256), 256, 0, st>>>(ids, id_off, pair_images, P, E, kp_off, n_images, n_nodes, parent, status);
    gf_prof_end("track_link", tok, st);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_track_flatten(int32_t* parent, int n_nodes, void* stream) {
    GF_CHECK_ARG(parent, "null pointer");
    GF_CHECK_ARG(n_nodes >= 0, "need n_nodes >= 0");
    if (n_nodes == 0) return GF_OK;
    hipStream_t st = (hipStream_t)stream;
    void* tok = gf_prof_begin("track_flatten", st, (double)n_nodes);
    track_flatten<<<(unsigned)(((long)n_nodes + 255) / 256), 256, 0, st>>>(parent, n_nodes);
    gf_prof_end("track_flatten", tok, st);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" size_t gf_triangulate_workspace_bytes(int T, int n_images) {
    if (T <= 0 || n_images <= 0) return 0;
    const size_t nb = ((size_t)T + 255) / 256;
    return gf_align_up((size_t)n_images * sizeof(int32_t), 256) + gf_align_up((size_t)n_images * 3 * sizeof(double), 256) +
           3 * gf_align_up((size_t)T * sizeof(int32_t), 256) + gf_align_up((nb + 1) * sizeof(int32_t), 256) +
           gf_align_up((size_t)T * sizeof(long long), 256);
}

extern "C" int gf_triangulate(const int32_t* track_off, int T, int n_obs, const int32_t* obs_image, const float* obs_uv, const float* K,
                              const double* R, const double* t, int n_images, float pixel_thr, double cos_min_angle, int min_obs, int refit,
                              uint32_t seed, double* X, int32_t* valid, int32_t* conflict, int32_t* n_inliers, int32_t* hypothesis,
                              int32_t* rounds, double* err2, uint8_t* inliers, void* workspace, size_t workspace_bytes, void* stream) {
    GF_CHECK_ARG(T >= 0 && T <= 0x7FFFFFFF / TR_MAX_HYP, "need 0 <= T and T * 64 < 2^31");
    GF_CHECK_ARG(n_obs >= 0 && n_images >= 0, "need n_obs >= 0 and n_images >= 0");
    GF_CHECK_ARG(pixel_thr > 0.f && pixel_thr < INFINITY, "pixel_thr must be positive and finite");
    GF_CHECK_ARG(cos_min_angle == cos_min_angle, "cos_min_angle is NaN");
    GF_CHECK_ARG(min_obs >= 2, "min_obs must be at least 2");
    GF_CHECK_ARG(refit >= 0 && refit <= TR_REFIT_MAX_ROUNDS, "refit must be 0 .. 8");
    if (T == 0) return GF_OK;
    GF_CHECK_ARG(track_off && obs_image && obs_uv && K && R && t && X && valid && conflict && n_inliers && hypothesis && rounds && err2 && inliers,
                 "null pointer");
    GF_CHECK_ARG(n_images > 0 && n_obs > 0, "tracks but no images or no observations");
    if (workspace == nullptr || workspace_bytes < gf_triangulate_workspace_bytes(T, n_images)) {
        gf_set_error("gf_triangulate: workspace too small");
        return GF_ERR_WORKSPACE;
    }
    TriArgs a;
    a.track_off = track_off; a.T = T; a.n_obs = n_obs; a.nb = (T + 255) / 256;
    GfCarver cv(workspace);
    a.cam_ok = cv.take<int32_t>((size_t)n_images);
    a.cam_o = cv.take<double>((size_t)n_images * 3);
    a.leff = cv.take<int32_t>((size_t)T);
    a.slot_loc = cv.take<int32_t>((size_t)T);
    a.nhyp = cv.take<int32_t>((size_t)T);
    a.blk_off = cv.take<int32_t>((size_t)a.nb + 1);
    a.best = cv.take<long long>((size_t)T);
    a.v.obs_image = obs_image; a.v.obs_uv = obs_uv; a.v.K = K; a.v.R = R; a.v.t = t; a.v.cam_ok = a.cam_ok; a.v.cam_o = a.cam_o;
    a.v.n_images = n_images; a.v.thr2 = (double)pixel_thr * (double)pixel_thr; a.v.cos_min = cos_min_angle; a.v.min_obs = min_obs;
    a.v.refit = refit; a.v.seed = seed;
    a.X = X; a.valid = valid; a.conflict = conflict; a.n_inliers = n_inliers; a.hypothesis = hypothesis; a.rounds = rounds; a.err2 = err2;
    a.inliers = inliers;
    const long long cap_t = (long long)T * TR_MAX_HYP, cap_o = 6ll * n_obs;          // H <= 64 and H <= 6 L for every track
    const long long slots = cap_t < cap_o ? cap_t : cap_o;
    hipStream_t st = (hipStream_t)stream;
    tri_cams<<<(unsigned)((n_images + 255) / 256), 256, 0, st>>>(a);
    tri_prepare<<<(unsigned)a.nb, 256, 0, st>>>(a);
    tri_scan<<<1, 256, 0, st>>>(a);
    void* tok = gf_prof_begin("triangulate", st, (double)T);
    tri_hypotheses<<<(unsigned)((slots + 255) / 256), 256, 0, st>>>(a);
    tri_finish<<<(unsigned)a.nb, 256, 0, st>>>(a);
    gf_prof_end("triangulate", tok, st);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
