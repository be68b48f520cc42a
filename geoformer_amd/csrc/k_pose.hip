// On-device relative pose for validation: essential-matrix RANSAC + pose recovery (replaces the cv2.findEssentialMat /
// cv2.recoverPose host round trip of model/loftr_src/utils/metrics.py:72-98) and the symmetric epipolar error of every match
// (metrics.py:30-69).  OpenCV parity is UNPINNED (no OpenCV in the reference tree, no test fixing its output); these kernels run,
// operation for operation and in fp64 with contraction off, the algorithm stated in pose_solver.h, which host/pose_host.cpp compiles
// for the CPU: valid, the chosen hypothesis, the inlier mask, E, R and t can be checked bit for bit.
//
//   pose_score : grid (iters / 32, N), 256 threads.  Threads 0..31 each draw the 5 matches of one hypothesis (k_ransac's hash) and run
//                the five-point solver with EVERYTHING it indexes at run time - the 5x9 system, the 10x20 elimination, the
//                polynomials, the roots, the up to 10 solutions - in an LDS tile of PS_WS_DOUBLES doubles per hypothesis,
//                interleaved across the 32 solver lanes (element i of hypothesis h at ws[32 i + h]: lanes hit 32 consecutive
//                doubles, conflict-free).  Nothing of the elimination lives in a lane's scratch memory (k_ransac.hip's header
//                records what that cost the homography kernel).  Then all four waves score: wave w owns hypotheses 8w .. 8w + 7, walks
//                the pair's matches 64 at a time, and counts the Sampson inliers of every root with one ballot + popcount - a
//                wave-uniform count, no shuffle reduction and no cross-wave traffic.  Per hypothesis: the best root (most inliers,
//                then smallest root index), its E and its count.
//   pose_final : grid N.  Best hypothesis (most inliers, then smallest index), inlier mask, E -> (R1, R2, +-t), cheirality vote over
//                the inliers (integer counts through LDS atomics: order-free), outputs.
//   epipolar_errors : one thread per match, fp64 arithmetic, one rounding to fp32.
// No host synchronisation: match counts are read from device memory (rt_counts_range).  pose_score is the scoring stage that ransac_tile.h
// states as rt_score<Model>, kept hand-written with per-hypothesis results: on rt_score's per-block winners it measured 1 - 3.5 % slower
// (profiles/ransac_tile.txt).
#include "gf_common.h"
#include "pose_solver.h"
#include "ransac_tile.h"

#pragma clang fp contract(off)

namespace {

struct PoseArgs {
    const float* mk0;        // [cap][2] matched keypoints (px), sorted by pair
    const float* mk1;
    const int32_t* counts;   // [1+N]: total, per pair
    const float* K0;         // [N][9]
    const float* K1;
    int N, iters, capacity;
    double pixel_thr;
    uint32_t seed;
    double* hyp;             // [N][iters][9]   best root of every hypothesis
    int32_t* hyp_cnt;        // [N][iters]      its inlier count (-1: no solution)
    int32_t* hyp_root;       // [N][iters]
    double* E;               // [N][9]
    double* R;               // [N][9]
    double* t;               // [N][3]
    int32_t* valid;          // [N]
    int32_t* n_inliers;      // [N]
    int32_t* best;           // [N][2] hypothesis, root (-1 without a pose)
    uint8_t* inliers;        // [cap]
};

__global__ __launch_bounds__(256) void pose_score(PoseArgs a) {
    __shared__ double ws[PS_WS_DOUBLES * PS_HYP_PER_WG];
    __shared__ int s_nroot[PS_HYP_PER_WG];
    __shared__ int s_cnt[PS_HYP_PER_WG * PS_MAX_ROOTS];
    const int n = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int off, cnt;
    rt_counts_range(a.counts, n, a.capacity, off, cnt);
    if (cnt < PS_MIN_MATCHES) return;                                  // (uniform per block; pose_final does not read hyp_* then)
    const float* k0 = a.mk0 + 2 * (size_t)off;
    const float* k1 = a.mk1 + 2 * (size_t)off;
    const float* K0 = a.K0 + 9 * n;
    const float* K1 = a.K1 + 9 * n;
    const double thr = ps_threshold(K0, K1, a.pixel_thr), thr2 = thr * thr;
    for (int i = tid; i < PS_HYP_PER_WG * PS_MAX_ROOTS; i += 256) s_cnt[i] = 0;
    if (tid < PS_HYP_PER_WG) {
        const int t = blockIdx.x * PS_HYP_PER_WG + tid;                // < iters: iters is a multiple of PS_HYP_PER_WG
        int idx[5], nr = 0;
        if (gs_draw_distinct<5>(a.seed, (uint32_t)n, (uint32_t)t, cnt, idx)) {
            double x0[5][2], x1[5][2];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                ps_normalise(K0, k0[2 * idx[k]], k0[2 * idx[k] + 1], x0[k][0], x0[k][1]);
                ps_normalise(K1, k1[2 * idx[k]], k1[2 * idx[k] + 1], x1[k][0], x1[k][1]);
            }
            nr = ps_five_point(x0, x1, PsWs{ws + tid, PS_HYP_PER_WG});
        }
        s_nroot[tid] = nr;
    }
    __syncthreads();
    // ---- scoring: this wave's 8 hypotheses against every match of the pair
    for (int i0 = 0; i0 < cnt; i0 += 64) {
        const int i = i0 + lane;
        const bool have = i < cnt;
        double x0 = 0.0, y0 = 0.0, x1 = 0.0, y1 = 0.0;
        if (have) {
            ps_normalise(K0, k0[2 * i], k0[2 * i + 1], x0, y0);
            ps_normalise(K1, k1[2 * i], k1[2 * i + 1], x1, y1);
        }
        for (int g = 0; g < PS_HYP_PER_WG / 4; ++g) {
            const int h = wave * (PS_HYP_PER_WG / 4) + g, nr = s_nroot[h];
            for (int r = 0; r < nr; ++r) {
                double E[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) E[k] = ws[(PS_OFF_E + 9 * r + k) * PS_HYP_PER_WG + h];
                const int in = have && ps_inlier(E, x0, y0, x1, y1, thr2);
                const int pc = __popcll(__ballot(in));
                if (lane == 0) s_cnt[h * PS_MAX_ROOTS + r] += pc;     // this wave alone touches its hypotheses' counters
            }
        }
    }
    __syncthreads();
    if (tid < PS_HYP_PER_WG) {
        const int t = blockIdx.x * PS_HYP_PER_WG + tid, nr = s_nroot[tid];
        int bc = -1, br = -1;
        for (int r = 0; r < nr; ++r) {
            const int c = s_cnt[tid * PS_MAX_ROOTS + r];
            if (c > bc) { bc = c; br = r; }
        }
        const size_t o = (size_t)n * a.iters + t;
        a.hyp_cnt[o] = bc;
        a.hyp_root[o] = br;
        if (br >= 0)
            for (int k = 0; k < 9; ++k) a.hyp[o * 9 + k] = ws[(PS_OFF_E + 9 * br + k) * PS_HYP_PER_WG + tid];
    }
}

__global__ __launch_bounds__(256) void pose_final(PoseArgs a) {
    __shared__ long long sh_key[256];
    __shared__ double sh_E[9];
    __shared__ int sh_votes[4], sh_nin;
    const int n = blockIdx.x, t = threadIdx.x;
    int off, cnt;
    rt_counts_range(a.counts, n, a.capacity, off, cnt);
    uint8_t* mask = a.inliers + off;
    const float* k0 = a.mk0 + 2 * (size_t)off;
    const float* k1 = a.mk1 + 2 * (size_t)off;
    const float* K0 = a.K0 + 9 * n;
    const float* K1 = a.K1 + 9 * n;
    // ---- best hypothesis: most inliers, then the smallest index (rt_key)
    long long key = -1;
    if (cnt >= PS_MIN_MATCHES)
        for (int i = t; i < a.iters; i += 256) {
            const int c = a.hyp_cnt[(size_t)n * a.iters + i];
            if (c >= 0) {
                const long long kk = rt_key(c, i);
                key = kk > key ? kk : key;
            }
        }
    sh_key[t] = key;
    if (t < 4) sh_votes[t] = 0;
    if (t == 0) sh_nin = 0;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (t < s) sh_key[t] = sh_key[t] > sh_key[t + s] ? sh_key[t] : sh_key[t + s];
        __syncthreads();
    }
    key = sh_key[0];
    const int best_cnt = rt_key_count(key), best_t = rt_key_hyp(key);
    bool have = best_cnt >= PS_MIN_MATCHES;                            // (uniform: every thread holds the same key)
    double E[9], R1[9], R2[9], tt[3];
    int dec = 0;
    if (have) {
        if (t < 9) sh_E[t] = a.hyp[((size_t)n * a.iters + best_t) * 9 + t];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = sh_E[k];
        dec = ps_decompose(E, R1, R2, tt);
        const double thr = ps_threshold(K0, K1, a.pixel_thr), thr2 = thr * thr;
        int votes[4] = {0, 0, 0, 0}, nin = 0;
        for (int i = t; i < cnt; i += 256) {
            double x0, y0, x1, y1;
            ps_normalise(K0, k0[2 * i], k0[2 * i + 1], x0, y0);
            ps_normalise(K1, k1[2 * i], k1[2 * i + 1], x1, y1);
            const int in = ps_inlier(E, x0, y0, x1, y1, thr2);
            mask[i] = (uint8_t)in;
            nin += in;
            if (in && dec) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    double R[9], tc[3];
                    ps_candidate(c, R1, R2, tt, R, tc);
                    votes[c] += ps_cheiral(R, tc, x0, y0, x1, y1);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (votes[c]) atomicAdd(&sh_votes[c], votes[c]);
        if (nin) atomicAdd(&sh_nin, nin);
        __syncthreads();
    }
    int bc = 0;
    if (have) {
#pragma unroll
        for (int c = 1; c < 4; ++c)
            if (sh_votes[c] > sh_votes[bc]) bc = c;
        have = dec && sh_votes[bc] > 0;                                // no candidate in front of both cameras: no pose
    }
    if (!have) {                                                       // the reference's `ret is None`: all-zero mask
        for (int i = t; i < cnt; i += 256) mask[i] = 0;
        if (t == 0) {
            for (int k = 0; k < 9; ++k) { a.E[9 * n + k] = 0.0; a.R[9 * n + k] = 0.0; }
            for (int k = 0; k < 3; ++k) a.t[3 * n + k] = 0.0;
            a.valid[n] = 0; a.n_inliers[n] = 0; a.best[2 * n] = -1; a.best[2 * n + 1] = -1;
        }
        return;
    }
    if (t == 0) {
        double R[9], tc[3];
        ps_candidate(bc, R1, R2, tt, R, tc);
        for (int k = 0; k < 9; ++k) { a.E[9 * n + k] = E[k]; a.R[9 * n + k] = R[k]; }
        for (int k = 0; k < 3; ++k) a.t[3 * n + k] = tc[k];
        a.valid[n] = 1; a.n_inliers[n] = sh_nin;
        a.best[2 * n] = best_t; a.best[2 * n + 1] = a.hyp_root[(size_t)n * a.iters + best_t];
    }
}

struct EpiArgs {
    const float* mk0;        // [M][2]
    const float* mk1;
    const int64_t* bids;     // [M] pair of every match
    const float* T;          // [N][16] T_0to1
    const float* K0;         // [N][9]
    const float* K1;
    int M, N;
    float* out;              // [M]
};

// metrics.py:30-47 with E = [t]x R (:55-56): the squared symmetric epipolar distance in normalised coordinates
__global__ __launch_bounds__(256) void epipolar_errors(EpiArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.M) return;
    const long long b = a.bids[i];
    if (b < 0 || b >= a.N) { a.out[i] = __builtin_nanf(""); return; }
    const float* T = a.T + 16 * b;
    double R[9], t[3], E[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (double)T[4 * r + c];
        t[r] = (double)T[4 * r + 3];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        E[0 + c] = t[1] * R[6 + c] - t[2] * R[3 + c];
        E[3 + c] = t[2] * R[0 + c] - t[0] * R[6 + c];
        E[6 + c] = t[0] * R[3 + c] - t[1] * R[0 + c];
    }
    double x0, y0, x1, y1;
    ps_normalise(a.K0 + 9 * b, a.mk0[2 * i], a.mk0[2 * i + 1], x0, y0);
    ps_normalise(a.K1 + 9 * b, a.mk1[2 * i], a.mk1[2 * i + 1], x1, y1);
    const double a0 = (E[0] * x0 + E[1] * y0) + E[2], a1 = (E[3] * x0 + E[4] * y0) + E[5], a2 = (E[6] * x0 + E[7] * y0) + E[8];
    const double b0 = (E[0] * x1 + E[3] * y1) + E[6], b1 = (E[1] * x1 + E[4] * y1) + E[7];
    const double num = (x1 * a0 + y1 * a1) + a2;
    a.out[i] = (float)((num * num) * (1.0 / (a0 * a0 + a1 * a1) + 1.0 / (b0 * b0 + b1 * b1)));
}

}   // namespace

extern "C" size_t gf_pose_workspace_bytes(int N, int iters) {
    if (N <= 0 || iters <= 0) return 0;
    return gf_align_up((size_t)N * iters * 9 * sizeof(double), 256) + 2 * gf_align_up((size_t)N * iters * sizeof(int32_t), 256);
}

extern "C" int gf_pose_essential_ransac(const float* mkpts0, const float* mkpts1, const int32_t* counts, int N, int capacity,
                                        const float* K0, const float* K1, float pixel_thr, int iters, uint32_t seed, double* E,
                                        double* R, double* t, int32_t* valid, int32_t* n_inliers, int32_t* best, uint8_t* inliers,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    GF_CHECK_ARG(mkpts0 && mkpts1 && counts && K0 && K1 && E && R && t && valid && n_inliers && best && inliers, "null pointer");
    GF_CHECK_ARG(N > 0 && capacity > 0, "need N, capacity > 0");
    GF_CHECK_ARG(iters > 0 && iters % PS_HYP_PER_WG == 0, "iters must be a positive multiple of 32 (the hypotheses of one workgroup)");
    GF_CHECK_ARG(pixel_thr > 0.f, "pixel_thr must be positive");
    if (workspace == nullptr || workspace_bytes < gf_pose_workspace_bytes(N, iters)) {
        gf_set_error("gf_pose_essential_ransac: workspace too small");
        return GF_ERR_WORKSPACE;
    }
    PoseArgs a;
    a.mk0 = mkpts0; a.mk1 = mkpts1; a.counts = counts; a.K0 = K0; a.K1 = K1; a.N = N; a.iters = iters; a.capacity = capacity;
    a.pixel_thr = (double)pixel_thr; a.seed = seed;
    GfCarver cv(workspace);
    a.hyp = cv.take<double>((size_t)N * iters * 9);
    a.hyp_cnt = cv.take<int32_t>((size_t)N * iters);
    a.hyp_root = cv.take<int32_t>((size_t)N * iters);
    a.E = E; a.R = R; a.t = t; a.valid = valid; a.n_inliers = n_inliers; a.best = best; a.inliers = inliers;
    hipStream_t st = (hipStream_t)stream;
    pose_score<<<dim3(iters / PS_HYP_PER_WG, N), 256, 0, st>>>(a);
    pose_final<<<N, 256, 0, st>>>(a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_epipolar_errors(const float* mkpts0, const float* mkpts1, const int64_t* m_bids, int M, const float* T_0to1,
                                  const float* K0, const float* K1, int N, float* epi_errs, void* stream) {
    GF_CHECK_ARG(N > 0 && M >= 0, "need N > 0 and M >= 0");
    if (M == 0) return GF_OK;
    GF_CHECK_ARG(mkpts0 && mkpts1 && m_bids && T_0to1 && K0 && K1 && epi_errs, "null pointer");
    EpiArgs a;
    a.mk0 = mkpts0; a.mk1 = mkpts1; a.bids = m_bids; a.T = T_0to1; a.K0 = K0; a.K1 = K1; a.M = M; a.N = N; a.out = epi_errs;
    epipolar_errors<<<(M + 255) / 256, 256, 0, (hipStream_t)stream>>>(a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
