// Covisibility clustering, the 2-D - 3-D rows and the choice of the winning cluster for sparse localisation, on the device.  The kernels
// run the rule stated in covis_spec.h, which host/covis_host.cpp compiles for the CPU: integer work only, every output can be checked bit
// for bit.
//
//   covis_cluster : one workgroup of 1024 threads per query (a query is one workgroup's work whatever the load: sixteen waves hide the
//                   latency of the dependent loads of a walk).  The list's image ids, sorted, with their positions sit in LDS for a binary
//                   search, and so does parent[L_q] (L_q <= 1024: 20 KiB with the labels and the scan).  For every position the threads
//                   stride over the image's keypoints; a keypoint with a point walks the point's observations from the position that is the point's
//                   first listed observer and unites every other listed observer with it (a star per point: linear in the track length).
//                   The union is gf_track_link's, on LDS: both roots by path halving (atomicMin: parents never increase), then
//                   atomicCAS(&parent[hi], hi, lo) with hi > lo; a failed CAS means another thread linked hi, so the loop makes global
//                   progress and lock-step lanes cannot deadlock in it.  Every link points to a smaller position, so a component's root
//                   is its smallest position whatever the arrival order.  Then a flatten into a second array, and the rank of the roots by
//                   a block scan (one position per thread): the cluster number per position and C_q.
//   sparse_rows   : one thread per match row of the contributing pairs (cv_row): the query keypoint's node, the point, the problem, keep.
//   (the stable order by problem and the dedup between the kernels are torch's sorts and scans - ops.sparse_rows.)
//   covis_select  : one thread per query over its problems (cv_select): the winner, its pose and counts, is_win per problem.
//   covis_mask    : one thread per original row (cv_mask).
// All on the caller's stream, no host synchronisation; integer atomics only, so every output is the same in every run.
#include "gf_common.h"
#include "covis_spec.h"

namespace {

__device__ __forceinline__ int cl_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// the root of x in the LDS forest, halving the path on the way
__device__ __forceinline__ int cl_find(int32_t* parent, int x) {
    int p = cl_load(parent + x);
    while (p != x) {
        const int gp = cl_load(parent + p);
        if (gp != p) atomicMin(parent + x, gp);
        x = p;
        p = gp;
    }
    return x;
}

struct ClUnite {
    int32_t* parent;
    __device__ void operator()(int u, int v) const {
        int a = cl_find(parent, u), b = cl_find(parent, v);
        while (a != b) {
            const int hi = a > b ? a : b, lo = a > b ? b : a;
            const int seen = atomicCAS(parent + hi, hi, lo);
            if (seen == hi) break;                                     // linked
            a = cl_find(parent, seen);                                 // hi had been linked below itself by another thread
            b = cl_find(parent, lo);
        }
    }
};

__global__ __launch_bounds__(CV_MAX_LIST) void covis_cluster(CvView v, const int32_t* list_off, const int32_t* list_img, const int32_t* sorted_img,
                                                     const int32_t* sorted_pos, int L_total, int enable, int32_t* cluster, int32_t* n_clusters,
                                                     int32_t* status) {
    __shared__ int32_t s_img[CV_MAX_LIST], s_pos[CV_MAX_LIST], s_parent[CV_MAX_LIST], s_label[CV_MAX_LIST];
    __shared__ int s_scan[CV_MAX_LIST];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int base = cv_clamp(list_off[q], 0, L_total);
    int L = cv_clamp(list_off[q + 1], base, L_total) - base;
    int flags = 0;
    if (L > CV_MAX_LIST) {                                             // (the entry point has refused such a list: nothing wraps)
        flags |= CV_FLAG_LIST_RANGE;
        L = 0;
    }
    for (int i = tid; i < L; i += CV_MAX_LIST) {
        s_img[i] = sorted_img[base + i];
        const int pos = sorted_pos[base + i];
        s_pos[i] = cv_clamp(pos, 0, L - 1);                            // (an index into s_parent: never outside it)
        if (pos < 0 || pos >= L) flags |= CV_FLAG_LIST_RANGE;
        s_parent[i] = i;
    }
    __syncthreads();
    if (enable && !flags) {                                            // (flags of this thread only: a bad table skips its own work)
        for (int a = 0; a < L; ++a) {
            const int img = list_img[base + a];
            if (img < 0 || img >= v.n_images) {
                flags |= CV_FLAG_IMAGE_RANGE;
                continue;
            }
            const int nb = cv_clamp(v.kp_off[img], 0, v.n_nodes), ne = cv_clamp(v.kp_off[img + 1], nb, v.n_nodes);
            for (int node = nb + tid; node < ne; node += CV_MAX_LIST) flags |= cv_point_star(v, s_img, s_pos, L, a, node, ClUnite{s_parent});
        }
    }
    __syncthreads();
    for (int i = tid; i < L; i += CV_MAX_LIST) {                       // flatten: s_parent is only read from here on
        int x = i, p = s_parent[x];
        while (p != x) {
            x = p;
            p = s_parent[x];
        }
        s_label[i] = enable ? x : 0;
    }
    __syncthreads();
    // the rank of every root among the roots: one position per thread, an inclusive block scan of the root flags
    const int mine = tid < L && s_label[tid] == tid;
    s_scan[tid] = mine;
    __syncthreads();
    for (int s = 1; s < CV_MAX_LIST; s <<= 1) {
        const int add = tid >= s ? s_scan[tid - s] : 0;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    if (mine) s_parent[tid] = s_scan[tid] - 1;                         // (a root's own entry now holds its cluster number)
    __syncthreads();
    for (int i = tid; i < L; i += CV_MAX_LIST) cluster[base + i] = s_parent[s_label[i]];
    if (tid == 0) n_clusters[q] = s_scan[CV_MAX_LIST - 1];
    if (flags) atomicOr(status, flags);
}

__global__ __launch_bounds__(256) void sparse_rows(const int32_t* pairs, const int32_t* pair_row_off, int C, int M0, const int32_t* ids, int E,
                                                   CvView v, const int32_t* list_off, const int32_t* cluster, int L_total,
                                                   const int32_t* prob_base, int Q, int32_t* row_kp, int32_t* row_pt, int32_t* row_prob,
                                                   uint8_t* keep, int32_t* status) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= M0) return;
    int qnode, pt, prob, flags = 0;
    const int k = cv_row(pairs, pair_row_off, C, ids, E, v, list_off, cluster, L_total, prob_base, Q, (int)r, qnode, pt, prob, flags);
    row_kp[r] = qnode; row_pt[r] = pt; row_prob[r] = prob; keep[r] = (uint8_t)k;
    if (flags) atomicOr(status, flags);
}

__global__ __launch_bounds__(256) void covis_select(const int32_t* prob_base, int Q, int N, const int32_t* valid, const int32_t* n_inliers,
                                                    const double* R, const double* t, const int32_t* rounds, int min_inliers, int32_t* winner,
                                                    int32_t* localized, double* Rq, double* tq, int32_t* nin_q, int32_t* rounds_q,
                                                    uint8_t* is_win) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const int b = cv_clamp(prob_base[q], 0, N), e = cv_clamp(prob_base[q + 1], b, N);
    for (int k = b; k < e; ++k) is_win[k] = 0;
    const int w = cv_select(valid, n_inliers, b, e);
    winner[q] = w < 0 ? -1 : w - b;
    localized[q] = w >= 0 && n_inliers[w] >= min_inliers;
    nin_q[q] = w < 0 ? 0 : n_inliers[w];
    rounds_q[q] = w < 0 ? 0 : rounds[w];
    for (int i = 0; i < 9; ++i) Rq[9 * (size_t)q + i] = w < 0 ? 0.0 : R[9 * (size_t)w + i];
    for (int i = 0; i < 3; ++i) tq[3 * (size_t)q + i] = w < 0 ? 0.0 : t[3 * (size_t)w + i];
    if (w >= 0) is_win[w] = 1;
}

__global__ __launch_bounds__(256) void covis_mask(const uint8_t* is_win, const uint8_t* inliers, int N, int M, const int32_t* row_prob,
                                                  const int32_t* slot, int M0, uint8_t* mask) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r < M0) mask[r] = cv_mask(is_win, inliers, N, M, row_prob[r], slot[r]);
}

}   // namespace

extern "C" int gf_covis_cluster(const int32_t* kp_off, int n_images, const int32_t* point_of_keypoint, int n_nodes, const int32_t* obs_offsets,
                                int T, const int32_t* obs_image, int n_obs, const int32_t* list_off_host, const int32_t* list_img_host,
                                const int32_t* list_off, const int32_t* list_img, const int32_t* sorted_img, const int32_t* sorted_pos, int Q,
                                int L_total, int enable, int32_t* cluster, int32_t* n_clusters, int32_t* status, void* stream) {
    GF_CHECK_ARG(Q >= 0 && L_total >= 0 && n_images >= 0 && n_nodes >= 0 && T >= 0 && n_obs >= 0,
                 "need Q, L_total, n_images, n_nodes, T, n_obs >= 0 (each below 2^31)");
    if (Q == 0) return GF_OK;
    GF_CHECK_ARG(list_off_host && list_off && n_clusters && status && kp_off && obs_offsets, "null pointer");
    GF_CHECK_ARG(L_total == 0 || (list_img_host && list_img && sorted_img && sorted_pos && cluster), "null pointer");
    GF_CHECK_ARG(n_nodes == 0 || point_of_keypoint, "null pointer");
    GF_CHECK_ARG(n_obs == 0 || obs_image, "null pointer");
    GF_CHECK_ARG(list_off_host[0] == 0 && list_off_host[Q] == L_total, "list_off must start at 0 and end at L_total");
    for (int q = 0; q < Q; ++q) {
        const long len = (long)list_off_host[q + 1] - list_off_host[q];
        GF_CHECK_ARG(len >= 0, "list_off must ascend");
        GF_CHECK_ARG(len <= CV_MAX_LIST, "a query with more than 1024 database images");
    }
    for (int i = 0; i < L_total; ++i) GF_CHECK_ARG(list_img_host[i] >= 0 && list_img_host[i] < n_images, "a list names an image outside [0, n_images)");
    CvView v{kp_off, point_of_keypoint, obs_offsets, obs_image, n_images, n_nodes, T, n_obs};
    hipStream_t st = (hipStream_t)stream;
    void* tok = gf_prof_begin("covis_cluster", st, (double)L_total);
    covis_cluster<<<(unsigned)Q, CV_MAX_LIST, 0, st>>>(v, list_off, list_img, sorted_img, sorted_pos, L_total, enable != 0, cluster, n_clusters, status);
    gf_prof_end("covis_cluster", tok, st);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_sparse_rows(const int32_t* pairs_host, const int32_t* pairs, const int32_t* pair_row_off, int C, int M0, const int32_t* ids,
                              int E, const int32_t* kp_off, int n_images, const int32_t* point_of_keypoint, int n_nodes, int T,
                              const int32_t* list_off, const int32_t* cluster, int L_total, const int32_t* prob_base, int Q, int32_t* row_kp,
                              int32_t* row_pt, int32_t* row_prob, uint8_t* keep, int32_t* status, void* stream) {
    GF_CHECK_ARG(C >= 0 && M0 >= 0 && E >= 0 && n_images >= 0 && n_nodes >= 0 && T >= 0 && L_total >= 0 && Q >= 0,
                 "need C, M0, E, n_images, n_nodes, T, L_total, Q >= 0 (each below 2^31)");
    if (M0 == 0) return GF_OK;
    GF_CHECK_ARG(pairs_host && pairs && pair_row_off && ids && kp_off && point_of_keypoint && list_off && cluster && prob_base && row_kp && row_pt &&
                 row_prob && keep && status, "null pointer");
    GF_CHECK_ARG(C > 0 && Q > 0, "rows but no pairs or no queries");
    long rows = 0;
    for (int c = 0; c < C; ++c) {
        const int32_t* p = pairs_host + (size_t)CV_PAIR_WORDS * c;
        GF_CHECK_ARG(p[CV_Q] >= 0 && p[CV_Q] < Q, "a pair names a query outside [0, Q)");
        GF_CHECK_ARG(p[CV_QIMG] >= 0 && p[CV_QIMG] < n_images && p[CV_DIMG] >= 0 && p[CV_DIMG] < n_images, "a pair names an image outside [0, n_images)");
        GF_CHECK_ARG(p[CV_RB] >= 0 && p[CV_RE] >= p[CV_RB] && p[CV_RE] <= E, "a pair's rows lie outside ids");
        GF_CHECK_ARG(p[CV_QCOL] == 0 || p[CV_QCOL] == 1, "a pair's query column is neither 0 nor 1");
        GF_CHECK_ARG(p[CV_POS] >= 0 && p[CV_POS] < CV_MAX_LIST, "a pair's list position lies outside [0, 1024)");
        rows += (long)p[CV_RE] - p[CV_RB];
    }
    GF_CHECK_ARG(rows == M0, "M0 is not the number of rows of the pairs");
    CvView v{kp_off, point_of_keypoint, nullptr, nullptr, n_images, n_nodes, T, 0};
    hipStream_t st = (hipStream_t)stream;
    void* tok = gf_prof_begin("sparse_rows", st, (double)M0);
    sparse_rows<<<(unsigned)(((long)M0 + 255) / 256), 256, 0, st>>>(pairs, pair_row_off, C, M0, ids, E, v, list_off, cluster, L_total, prob_base, Q,
                                                                    row_kp, row_pt, row_prob, keep, status);
    gf_prof_end("sparse_rows", tok, st);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_covis_select(const int32_t* prob_base, int Q, int N, const int32_t* valid, const int32_t* n_inliers, const double* R,
                               const double* t, const int32_t* rounds, const uint8_t* inliers, int M, const int32_t* row_prob,
                               const int32_t* slot, int M0, int min_inliers, int32_t* winner, int32_t* localized, double* Rq, double* tq,
                               int32_t* nin_q, int32_t* rounds_q, uint8_t* is_win, uint8_t* mask, void* stream) {
    GF_CHECK_ARG(Q >= 0 && N >= 0 && M >= 0 && M0 >= 0, "need Q, N, M, M0 >= 0 (each below 2^31)");
    if (Q == 0 && M0 == 0) return GF_OK;
    GF_CHECK_ARG(Q == 0 || (prob_base && winner && localized && Rq && tq && nin_q && rounds_q), "null pointer");
    GF_CHECK_ARG(N == 0 || (valid && n_inliers && R && t && rounds && is_win), "null pointer");
    GF_CHECK_ARG(M0 == 0 || (row_prob && slot && mask), "null pointer");
    GF_CHECK_ARG(M == 0 || inliers, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (Q > 0)
        covis_select<<<(unsigned)((Q + 255) / 256), 256, 0, st>>>(prob_base, Q, N, valid, n_inliers, R, t, rounds, min_inliers, winner, localized, Rq,
                                                                 tq, nin_q, rounds_q, is_win);
    if (M0 > 0) covis_mask<<<(unsigned)(((long)M0 + 255) / 256), 256, 0, st>>>(is_win, inliers, N, M, row_prob, slot, M0, mask);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
