// On-device localisation of query images: absolute-pose (P3P) RANSAC for every query of a 2-D - 3-D correspondence list in three launches,
// and a fourth when the winner is refitted on its inliers (refit_rounds > 0); and the lookup that makes the 3-D side of the list.  The
// kernels run, operation for operation and in fp64 with contraction off, the algorithm stated in abs_solver.h, which
// host/abspose_host.cpp compiles for the CPU: every output can be checked bit for bit.  pycolmap parity is UNPINNED.
//
// The four stages - compaction and conditioning, scoring, the winner over the original rows, the refit rounds - and the entry point around
// them are ransac_tile.h's (rt_prepare, rt_score, rt_final, rt_refit, rt_run); problems are addressed by an offsets array [N + 1] in DEVICE
// memory.  This file holds what is the absolute pose's:
//
//   AbsModel     : rows are valid by as_row_valid, the box of the surviving 3-D points conditions them (as_box_norm, 3 coordinates, 4
//                  doubles).  solve: a lane of wave 0 draws the 3 rows of one hypothesis and runs as_p3p - the quartic, its roots, the up
//                  to 4 poses - in the LDS tile (64 x 53 x 8 B = 27,136 B); inliers by the reprojection error.  A pose travels as the
//                  template's 9 doubles: two rows of R and t' (as_unpack rebuilds the third row, here as on the host).  The outputs are R
//                  and t in world units; the winner's 9 doubles are kept in the workspace for the refit.
//   AbsModel::fit : AS_GN_STEPS Gauss-Newton steps of the refit rule of abs_solver.h.  Thread j holds partial j of the 27 sums of a step in
//                  registers, rt_block_sums leaves their block sum in LDS; the 6 x 6 solve and the Cayley update run on thread 0 with the
//                  workspace in LDS.
//   xyz_lookup   : one thread per row.  The row's pair by bisection of the pair offsets (a row outside every pair gets NaN), the pair's map
//                  through a device table of gf_xyz_map records, as_xyz_sample.
// No host synchronisation; every output is the same in every run.
#include "gf_common.h"
#include "abs_solver.h"
#include "ransac_tile.h"

#pragma clang fp contract(off)

namespace {

struct AbsArgs {
    const float* uv;         // [M][2] query pixels, sorted by problem
    const float* xyz;        // [M][3] world points
    const float* scores;     // [M] or null
    const int32_t* offsets;  // [N + 1]
    const float* K;          // [N][9]
    int N, M;
    float sc_thres;
    double thr2;
    uint32_t seed;
    int32_t* rows;           // [M]        per problem: the surviving rows (relative to the problem's first), ascending
    int32_t* use;            // [N]        surviving rows where the problem can be estimated (>= 4, a box with an extent), else 0
    double* norm;            // [N][4]
    double* win;             // [N][9]     the winner's solution in conditioned coordinates
    RtBlocks blk;            // every block's best solution
    double* R;               // [N][9]
    double* t;               // [N][3]
    int32_t* valid;          // [N]
    int32_t* n_inliers;      // [N]
    int32_t* best;           // [N][2] hypothesis, root (-1 when not valid)
    uint8_t* inliers;        // [M]
    // rt_refit only
    int refit_rounds;
    uint8_t* set[2];         // [M] each: per problem (at its offset) the current and the candidate inlier set over its SURVIVING rows
    int32_t* rounds;         // [N] accepted refits
};

// the absolute-pose model of the stages of ransac_tile.h: rows are reached through the compacted list, 3-D points are conditioned by the
// problem's box
struct AbsModel {
    static constexpr int HYP = AS_HYP_PER_WG, ROOTS = AS_MAX_ROOTS, WS = AS_WS_DOUBLES, OFF_SOL = AS_OFF_SOL;
    static constexpr int BOX = 3, NORM = 4, MIN_INLIERS = AS_REFIT_MIN_INLIERS, MAX_ROUNDS = AS_REFIT_MAX_ROUNDS;
    typedef AbsArgs Args;
    typedef AsRow Row;
    struct Cand { double R[9], t[3]; };                                // in conditioned coordinates
    const float* uv;         // the problem's pixels
    const float* xyz;        // and 3-D points
    const float* sc;         // and scores, or null
    const int32_t* rows;     // its surviving rows
    const float* K;          // [9]
    double nm[4];
    uint32_t seed, n;
    int cnt;
    float sc_thres;
    double thr2;
    __device__ __forceinline__ void bind(const AbsArgs& a, int prob, int off) {
        uv = a.uv + 2 * (size_t)off; xyz = a.xyz + 3 * (size_t)off; sc = a.scores ? a.scores + off : nullptr; rows = a.rows + off;
        K = a.K + 9 * (size_t)prob;
        seed = a.seed; n = (uint32_t)prob; sc_thres = a.sc_thres; thr2 = a.thr2;
    }
    __device__ __forceinline__ int init(const AbsArgs& a, int prob) {
        int off, len;
        gs_offsets_range(a.offsets, prob, a.M, off, len);
        bind(a, prob, off);
#pragma unroll
        for (int k = 0; k < 4; ++k) nm[k] = a.norm[4 * (size_t)prob + k];
        return cnt = min(a.use[prob], len);
    }
    static void take(AbsArgs& a, GfCarver& cv) { a.win = cv.take<double>((size_t)a.N * 9); }
    __device__ __forceinline__ Row row(size_t j) const { return as_row(uv + 2 * j, xyz + 3 * j, nm); }
    // ---- rt_prepare
    __device__ __forceinline__ bool row_valid(int i) const { return as_row_valid(uv + 2 * (size_t)i, xyz + 3 * (size_t)i, sc, i, sc_thres); }
    __device__ __forceinline__ float coord(int i, int k) const { return xyz[3 * (size_t)i + k]; }
    __device__ __forceinline__ int condition(int base, const float (&lo)[3], const float (&hi)[3], double (&norm)[4]) const {
        return base >= AS_MIN_ROWS && as_box_norm(lo, hi, norm);
    }
    // ---- rt_score
    __device__ __forceinline__ Row load(int i, bool have) const {
        Row r = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (have) r = row((size_t)rows[i]);
        return r;
    }
    __device__ __forceinline__ int solve(int t, const GsWs& w) const {
        int idx[3];
        if (!as_draw3(seed, n, (uint32_t)t, cnt, uv, xyz, rows, idx)) return 0;
        double p[3][2], X[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const size_t j = (size_t)rows[idx[k]];
            p[k][0] = (double)uv[2 * j]; p[k][1] = (double)uv[2 * j + 1];
            X[k][0] = (double)xyz[3 * j]; X[k][1] = (double)xyz[3 * j + 1]; X[k][2] = (double)xyz[3 * j + 2];
        }
        return as_p3p(p, X, K, nm, w);
    }
    __device__ __forceinline__ int inlier(const double (&S)[9], const Row& r) const { return as_inlier(S, K, r, thr2); }
    // ---- rt_final: R and t in world units; the winner's 9 doubles are kept in the workspace for load_winner
    __device__ __forceinline__ int original_inlier(const double (&S)[9], int i) const {
        return row_valid(i) ? as_inlier(S, K, row((size_t)i), thr2) : 0;
    }
    __device__ __forceinline__ void write_invalid(const AbsArgs& a, int prob) const {
        for (int k = 0; k < 9; ++k) { a.R[9 * (size_t)prob + k] = 0.0; a.win[9 * (size_t)prob + k] = 0.0; }
        for (int k = 0; k < 3; ++k) a.t[3 * (size_t)prob + k] = 0.0;
    }
    __device__ __forceinline__ void write_pose(const AbsArgs& a, int prob, const double (&R)[9], const double (&tc)[3]) const {
        double tw[3];
        as_to_world(R, tc, nm, tw);
        for (int k = 0; k < 9; ++k) a.R[9 * (size_t)prob + k] = R[k];
        for (int k = 0; k < 3; ++k) a.t[3 * (size_t)prob + k] = tw[k];
    }
    __device__ __forceinline__ void write_solution(const AbsArgs& a, int prob, const double (&S)[9]) const {
        double R[9], tc[3];
        as_unpack(S, R, tc);
        write_pose(a, prob, R, tc);
        for (int k = 0; k < 9; ++k) a.win[9 * (size_t)prob + k] = S[k];
    }
    // ---- rt_refit
    __device__ __forceinline__ Cand load_winner(const AbsArgs& a, int prob) const {
        double S[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) S[k] = a.win[9 * (size_t)prob + k];
        Cand c;
        as_unpack(S, c.R, c.t);
        return c;
    }
    // AS_GN_STEPS Gauss-Newton steps from the pose in c on the set `cur` over the surviving rows: the 27 sums by all threads, the 6 x 6
    // solve and the Cayley update on thread 0 with the workspace in LDS
    __device__ __forceinline__ int fit(const uint8_t* cur, int cnt, Cand& c) const {
        __shared__ double sh_ws[AS_GN_WS_DOUBLES];
        __shared__ double sh_part[4][AS_GN_SUMS];
        __shared__ double sh_pose[12];
        __shared__ int sh_ok;
        const int t = threadIdx.x;
        for (int step = 0; step < AS_GN_STEPS; ++step) {
            // ---- partial t, ascending rows
            double acc[AS_GN_SUMS];
#pragma unroll
            for (int e = 0; e < AS_GN_SUMS; ++e) acc[e] = 0.0;
            for (int i = t; i < cnt; i += 256) {
                if (!cur[i]) continue;
                double Ju[6], Jv[6], res[2];
                if (as_gn_row(c.R, c.t, K, row((size_t)rows[i]), Ju, Jv, res)) as_gn_accum(acc, Ju, Jv, res);
            }
            rt_block_sums<AS_GN_SUMS>(acc, sh_part, sh_ws + AS_GN_OFF_ACC);
            if (t == 0) {
                int good = as_gn_solve(GsWs{sh_ws, 1});
                if (good) {
                    double d[6], Rn[9], tt[3];
#pragma unroll
                    for (int k = 0; k < 6; ++k) d[k] = sh_ws[AS_GN_OFF_X + k];
#pragma unroll
                    for (int k = 0; k < 9; ++k) Rn[k] = c.R[k];
#pragma unroll
                    for (int k = 0; k < 3; ++k) tt[k] = c.t[k];
                    good = as_gn_update(d, Rn, tt);
#pragma unroll
                    for (int k = 0; k < 9; ++k) sh_pose[k] = Rn[k];
#pragma unroll
                    for (int k = 0; k < 3; ++k) sh_pose[9 + k] = tt[k];
                }
                sh_ok = good;
            }
            __syncthreads();                                           // (the next step writes both again behind rt_block_sums' barriers)
            if (!sh_ok) return 0;                                      // (uniform)
#pragma unroll
            for (int k = 0; k < 9; ++k) c.R[k] = sh_pose[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) c.t[k] = sh_pose[9 + k];
        }
        return 1;
    }
    __device__ __forceinline__ int cand_inlier(const Cand& c, int i) const { return as_inlier_rt(c.R, c.t, K, row((size_t)rows[i]), thr2); }
    __device__ __forceinline__ void write_refined(const AbsArgs& a, int prob, const Cand& c) const { write_pose(a, prob, c.R, c.t); }
};

__global__ __launch_bounds__(256) void xyz_lookup(const gf_xyz_map* table, int P, const int32_t* pair_offsets, const float* pts, long pts_stride,
                                                  int M, float* xyz) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    int lo = 0, hi = P;                                                // the last pair whose first row is <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pair_offsets[mid] <= i) lo = mid; else hi = mid;
    }
    float o[3] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
    if (pair_offsets[lo] <= i && i < pair_offsets[lo + 1]) {
        const gf_xyz_map r = table[lo];
        if (r.base && r.h > 0 && r.w > 0) as_xyz_sample(r.base, r.h, r.w, pts[pts_stride * i], pts[pts_stride * i + 1], o);
    }
    xyz[3 * (size_t)i] = o[0]; xyz[3 * (size_t)i + 1] = o[1]; xyz[3 * (size_t)i + 2] = o[2];
}

}   // namespace

extern "C" size_t gf_abspose_workspace_bytes(int N, int M, int iters) {
    if (N <= 0 || M < 0 || iters <= 0) return 0;
    const size_t nb = (size_t)N * ((size_t)(iters + AS_HYP_PER_WG - 1) / AS_HYP_PER_WG);
    return gf_align_up((size_t)M * sizeof(int32_t), 256) + gf_align_up((size_t)N * sizeof(int32_t), 256) +
           gf_align_up((size_t)N * 4 * sizeof(double), 256) + gf_align_up((size_t)N * 9 * sizeof(double), 256) + rt_blocks_bytes(nb) +
           2 * gf_align_up((size_t)M, 256);
}

extern "C" int gf_abspose_ransac(const float* p2d, const float* p3d, const float* scores, const int32_t* offsets, int N, int M, const float* K,
                                 float sc_thres, float pixel_thr, int iters, uint32_t seed, int refit_rounds, double* R, double* t,
                                 int32_t* valid, int32_t* n_inliers, int32_t* best, int32_t* rounds, uint8_t* inliers, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    AbsArgs a;
    a.uv = p2d; a.xyz = p3d; a.scores = scores; a.offsets = offsets; a.K = K; a.N = N; a.M = M; a.sc_thres = sc_thres; a.seed = seed;
    a.R = R; a.t = t; a.valid = valid; a.n_inliers = n_inliers; a.best = best; a.inliers = inliers; a.rounds = rounds;
    return rt_run<AbsModel>("gf_abspose_ransac", "abspose_ransac", a,
                            p2d && p3d && offsets && K && R && t && valid && n_inliers && best && rounds && inliers, pixel_thr, iters, true,
                            refit_rounds, workspace, workspace_bytes, gf_abspose_workspace_bytes(N, M, iters), stream);
}

extern "C" int gf_xyz_lookup(const gf_xyz_map* table, int P, const int32_t* pair_offsets, const float* pts, long pts_stride, int M,
                             float* xyz, void* stream) {
    GF_CHECK_ARG(table && pair_offsets && pts && xyz, "null pointer");
    GF_CHECK_ARG(P > 0 && M > 0 && pts_stride >= 2, "need P > 0, M > 0 and pts_stride >= 2");
    xyz_lookup<<<(unsigned)((M + 255) / 256), 256, 0, (hipStream_t)stream>>>(table, P, pair_offsets, pts, pts_stride, M, xyz);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        gf_set_error("gf_xyz_lookup: launch failed: %s", hipGetErrorString(e));
        return GF_ERR_LAUNCH;
    }
    return GF_OK;
}
