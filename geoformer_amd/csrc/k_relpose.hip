// On-device calibrated two-view verification: essential-matrix RANSAC with pose recovery for every pair of a match list in four launches,
// and a fifth when the pose is refitted on its inliers (gf_relpose_ransac_lo, refit_rounds > 0).  The kernels run, operation for operation
// and in fp64 with contraction off, the algorithm stated in rel_solver.h, which host/relpose_host.cpp compiles for the CPU: valid, the chosen
// hypothesis, the inlier mask, E, R, t, n_cheiral and rounds can be checked bit for bit.  OpenCV parity is UNPINNED.
//
// The stages - compaction, scoring, the winner over the original rows, the pose, the refit rounds - and the entry point around them are
// ransac_tile.h's (rt_prepare, rt_score, rt_final, rt_pose, rt_refit, rt_run); pairs are addressed by an offsets array [N + 1] in DEVICE
// memory (the layout consolidate_matches uploads).  This file holds what is the essential matrix's:
//
//   RelModel     : rows are valid by fs_row_valid and travel in normalised coordinates (rs_row); a pair can be estimated with 5 surviving
//                  rows and finite positive focal lengths, nothing else (the template's box is computed and not looked at; norm holds the
//                  pair's thr^2).  solve: a lane of the first 32 draws the 5 rows of one hypothesis and runs ps_five_point in the LDS tile.
//                  RS_HYP_PER_WG = 32: the tile is 32 x 236 x 8 B = 60,416 B (pose_score's); 64 hypotheses (120,832 B) would pass the
//                  64 KiB a kernel may declare statically.  iters stays a multiple of 64: a pair runs an even number of workgroups.
//   RelModel::pose : step 6 of rel_solver.h with the whole workgroup behind rt_final: ps_decompose on every thread, the winner's inliers
//                  vote through integer LDS atomics (order-free), thread 0 writes R, t, n_cheiral; without a pose valid, mask and
//                  outputs are withdrawn.
//   RelModel::fit : RS_GN_STEPS Gauss-Newton steps of the refit rule.  Thread j holds partial j of the 20 sums of a step in registers
//                  (every index compile-time), rt_block_sums leaves their block sum in LDS; the 5 x 5 solve and the update run on
//                  thread 0 with the workspace in LDS.
// No host synchronisation; every output is the same in every run; a pair's result depends on its index in the call, not on its neighbours.
// Measured on an MI355X, 120 pairs x 1889 rows, 512 hypotheses, between device events (profiles/relative_pose.txt): the four launches
// 4.90 ms (4.87 .. 4.96) against 4.94 ms (4.90 .. 4.99) for pose_score + pose_final on the same rows - the tile form is not slower than
// pose_score by more than the run's spread; with refit_rounds = 4 the five launches 5.18 ms, 5.27 ms on rows with 0.5 px noise.
#include "gf_common.h"
#include "rel_solver.h"
#include "ransac_tile.h"

#pragma clang fp contract(off)

namespace {

struct RelArgs {
    const float* m;          // [M][4] x0, y0, x1, y1 (px), sorted by pair
    const float* scores;     // [M] or null
    const int32_t* offsets;  // [N + 1]
    const float* K0;         // [N][9]
    const float* K1;
    int N, M;
    float sc_thres;
    double thr2;             // (rt_run's pixel_thr^2: not used, the threshold is per pair)
    double pixel_thr;
    uint32_t seed;
    int32_t* rows;           // [M]        per pair: the surviving rows (relative to the pair's first), ascending
    int32_t* use;            // [N]        surviving rows where the pair can be estimated (>= 5, focal lengths finite and positive), else 0
    double* norm;            // [N]        the pair's thr^2 in normalised coordinates
    RtBlocks blk;            // every block's best E
    double* E;               // [N][9]
    double* R;               // [N][9]
    double* t;               // [N][3]
    int32_t* valid;          // [N]
    int32_t* n_inliers;      // [N]
    int32_t* n_cheiral;      // [N]
    int32_t* best;           // [N][2] hypothesis, root (-1 when not valid)
    uint8_t* inliers;        // [M]
    // rt_refit only
    int refit_rounds;
    uint8_t* set[2];         // [M] each: per pair (at its offset) the current and the candidate inlier set over its SURVIVING rows
    int32_t* rounds;         // [N] accepted refits
};

struct RelModel {
    static constexpr int HYP = RS_HYP_PER_WG, ROOTS = PS_MAX_ROOTS, WS = PS_WS_DOUBLES, OFF_SOL = PS_OFF_E;
    static constexpr int BOX = 1, NORM = 1, MIN_INLIERS = RS_REFIT_MIN_INLIERS, MAX_ROUNDS = RS_REFIT_MAX_ROUNDS;
    typedef RelArgs Args;
    typedef RsRow Row;
    struct Cand { double R[9], t[3], E[9]; };                          // E = [t]x R as rs_E builds it
    const float* m;          // the pair's matches
    const float* sc;         // and scores, or null
    const int32_t* rows;     // its surviving rows
    const float* K0;         // [9]
    const float* K1;
    uint8_t* mask;           // the pair's slice of the inlier bytes
    uint32_t seed, n;
    int cnt;
    float sc_thres;
    double pixel_thr, thr2;
    __device__ __forceinline__ void bind(const RelArgs& a, int pair, int off) {
        m = a.m + 4 * (size_t)off; sc = a.scores ? a.scores + off : nullptr; rows = a.rows + off; mask = a.inliers + off;
        K0 = a.K0 + 9 * (size_t)pair; K1 = a.K1 + 9 * (size_t)pair;
        seed = a.seed; n = (uint32_t)pair; sc_thres = a.sc_thres; pixel_thr = a.pixel_thr;
    }
    __device__ __forceinline__ int init(const RelArgs& a, int pair) {
        int off, len;
        gs_offsets_range(a.offsets, pair, a.M, off, len);
        bind(a, pair, off);
        thr2 = a.norm[pair];
        return cnt = min(a.use[pair], len);
    }
    static void take(RelArgs&, GfCarver&) {}
    __device__ __forceinline__ Row row(size_t j) const { return rs_row(m + 4 * j, K0, K1); }
    // ---- rt_prepare
    __device__ __forceinline__ bool row_valid(int i) const { return fs_row_valid(m + 4 * (size_t)i, sc, i, sc_thres); }
    __device__ __forceinline__ float coord(int i, int) const { return m[4 * (size_t)i]; }
    __device__ __forceinline__ int condition(int base, const float (&)[1], const float (&)[1], double (&nm)[1]) const {
        if (base < RS_MIN_ROWS || !rs_k_valid(K0, K1)) return 0;
        const double thr = ps_threshold(K0, K1, pixel_thr);
        nm[0] = thr * thr;
        return 1;
    }
    // ---- rt_score
    __device__ __forceinline__ Row load(int i, bool have) const {
        Row r = {0.0, 0.0, 0.0, 0.0};
        if (have) r = row((size_t)rows[i]);
        return r;
    }
    __device__ __forceinline__ int solve(int t, const GsWs& w) const {
        int idx[5];
        if (!gs_draw_distinct<5>(seed, n, (uint32_t)t, cnt, idx)) return 0;
        double x0[5][2], x1[5][2];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const Row r = row((size_t)rows[idx[k]]);
            x0[k][0] = r.x0; x0[k][1] = r.y0; x1[k][0] = r.x1; x1[k][1] = r.y1;
        }
        return ps_five_point(x0, x1, w);
    }
    __device__ __forceinline__ int inlier(const double (&E)[9], const Row& r) const { return rs_inlier(E, r, thr2); }
    // ---- rt_final
    __device__ __forceinline__ int original_inlier(const double (&E)[9], int i) const {
        return row_valid(i) ? rs_inlier(E, row((size_t)i), thr2) : 0;
    }
    __device__ __forceinline__ void write_invalid(const RelArgs& a, int pair) const {
        for (int k = 0; k < 9; ++k) { a.E[9 * (size_t)pair + k] = 0.0; a.R[9 * (size_t)pair + k] = 0.0; }
        for (int k = 0; k < 3; ++k) a.t[3 * (size_t)pair + k] = 0.0;
        a.n_cheiral[pair] = 0;
    }
    __device__ __forceinline__ void write_solution(const RelArgs& a, int pair, const double (&E)[9]) const {
        for (int k = 0; k < 9; ++k) a.E[9 * (size_t)pair + k] = E[k];
    }
    // ---- rt_pose: step 6 on what rt_final wrote.  A filtered row has a zero mask byte, so only the winner's inliers vote.
    __device__ __forceinline__ void pose(const RelArgs& a, int pair, int len) const {
        __shared__ int sh_votes[4];
        const int t = threadIdx.x;
        if (!a.valid[pair]) return;                                    // (uniform; rt_final wrote the zeros)
        if (t < 4) sh_votes[t] = 0;
        __syncthreads();
        double E[9], R1[9], R2[9], tt[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = a.E[9 * (size_t)pair + k];
        const int dec = ps_decompose(E, R1, R2, tt);
        int votes[4] = {0, 0, 0, 0};
        if (dec)
            for (int i = t; i < len; i += 256) {
                if (!mask[i]) continue;
                const Row r = row((size_t)i);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    double R[9], tc[3];
                    ps_candidate(c, R1, R2, tt, R, tc);
                    votes[c] += ps_cheiral(R, tc, r.x0, r.y0, r.x1, r.y1);
                }
            }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (votes[c]) atomicAdd(&sh_votes[c], votes[c]);
        __syncthreads();
        int bc = 0;
#pragma unroll
        for (int c = 1; c < 4; ++c)
            if (sh_votes[c] > sh_votes[bc]) bc = c;
        const int nch = sh_votes[bc];
        if (!(a.n_inliers[pair] >= RS_MIN_ROWS && dec && nch > 0)) {   // (uniform) no pose: the pair is withdrawn
            for (int i = t; i < len; i += 256) mask[i] = 0;
            if (t == 0) {
                write_invalid(a, pair);
                a.valid[pair] = 0; a.n_inliers[pair] = 0; a.best[2 * pair] = -1; a.best[2 * pair + 1] = -1;
            }
            return;
        }
        if (t == 0) {
            double R[9], tc[3];
            ps_candidate(bc, R1, R2, tt, R, tc);
            for (int k = 0; k < 9; ++k) a.R[9 * (size_t)pair + k] = R[k];
            for (int k = 0; k < 3; ++k) a.t[3 * (size_t)pair + k] = tc[k];
            a.n_cheiral[pair] = nch;
        }
    }
    // ---- rt_refit
    __device__ __forceinline__ Cand load_winner(const RelArgs& a, int pair) const {
        Cand c;
#pragma unroll
        for (int k = 0; k < 9; ++k) c.R[k] = a.R[9 * (size_t)pair + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) c.t[k] = a.t[3 * (size_t)pair + k];
        rs_E(c.R, c.t, c.E);
        return c;
    }
    // RS_GN_STEPS Gauss-Newton steps from the pose in c on the set `cur` over the surviving rows: the 20 sums by all threads, the 5 x 5
    // solve and the update on thread 0 with the workspace in LDS
    __device__ __forceinline__ int fit(const uint8_t* cur, int cnt, Cand& c) const {
        __shared__ double sh_ws[RS_GN_WS_DOUBLES];
        __shared__ double sh_part[4][RS_GN_SUMS];
        __shared__ double sh_pose[12];
        __shared__ int sh_ok;
        const int t = threadIdx.x;
        for (int step = 0; step < RS_GN_STEPS; ++step) {
            double D[5][9];
            const int basis = rs_gn_basis(c.R, c.t, D);                // (uniform: every thread holds the same pose)
            // ---- partial t, ascending rows
            double acc[RS_GN_SUMS];
#pragma unroll
            for (int e = 0; e < RS_GN_SUMS; ++e) acc[e] = 0.0;
            if (basis)
                for (int i = t; i < cnt; i += 256) {
                    if (!cur[i]) continue;
                    double J[5], res;
                    if (rs_gn_row(c.E, D, row((size_t)rows[i]), J, res)) rs_gn_accum(acc, J, res);
                }
            rt_block_sums<RS_GN_SUMS>(acc, sh_part, sh_ws + RS_GN_OFF_ACC);
            if (t == 0) {
                int good = basis && rs_gn_solve(GsWs{sh_ws, 1});
                if (good) {
                    double d[5], Rn[9], tn[3];
#pragma unroll
                    for (int k = 0; k < 5; ++k) d[k] = sh_ws[RS_GN_OFF_X + k];
#pragma unroll
                    for (int k = 0; k < 9; ++k) Rn[k] = c.R[k];
#pragma unroll
                    for (int k = 0; k < 3; ++k) tn[k] = c.t[k];
                    good = rs_gn_update(d, Rn, tn);
#pragma unroll
                    for (int k = 0; k < 9; ++k) sh_pose[k] = Rn[k];
#pragma unroll
                    for (int k = 0; k < 3; ++k) sh_pose[9 + k] = tn[k];
                }
                sh_ok = good;
            }
            __syncthreads();                                           // (the next step writes both again behind rt_block_sums' barriers)
            if (!sh_ok) return 0;                                      // (uniform)
#pragma unroll
            for (int k = 0; k < 9; ++k) c.R[k] = sh_pose[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) c.t[k] = sh_pose[9 + k];
            rs_E(c.R, c.t, c.E);
        }
        return 1;
    }
    __device__ __forceinline__ int cand_inlier(const Cand& c, int i) const { return rs_inlier(c.E, row((size_t)rows[i]), thr2); }
    __device__ __forceinline__ void write_refined(const RelArgs& a, int pair, const Cand& c) const {
        double E[9];
        if (!rs_E_unit(c.R, c.t, E))
            for (int k = 0; k < 9; ++k) E[k] = 0.0;
        for (int k = 0; k < 9; ++k) { a.E[9 * (size_t)pair + k] = E[k]; a.R[9 * (size_t)pair + k] = c.R[k]; }
        for (int k = 0; k < 3; ++k) a.t[3 * (size_t)pair + k] = c.t[k];
    }
};

}   // namespace

extern "C" size_t gf_relpose_workspace_bytes(int N, int M, int iters) {
    if (N <= 0 || M < 0 || iters <= 0) return 0;
    const size_t nb = (size_t)N * ((size_t)(iters + RS_HYP_PER_WG - 1) / RS_HYP_PER_WG);
    return gf_align_up((size_t)M * sizeof(int32_t), 256) + gf_align_up((size_t)N * sizeof(int32_t), 256) +
           gf_align_up((size_t)N * sizeof(double), 256) + rt_blocks_bytes(nb);
}

extern "C" size_t gf_relpose_lo_workspace_bytes(int N, int M, int iters) {
    const size_t base = gf_relpose_workspace_bytes(N, M, iters);
    return base ? base + 2 * gf_align_up((size_t)M, 256) : 0;
}

// both entries; lo = 0: gf_relpose_ransac (no refit stage, no `rounds`, its own workspace size)
static int rel_run(const char* name, bool lo, const float* matches, const float* scores, const int32_t* offsets, int N, int M, const float* K0,
                   const float* K1, float sc_thres, float pixel_thr, int iters, uint32_t seed, double* E, double* R, double* t, int32_t* valid,
                   int32_t* n_inliers, int32_t* n_cheiral, int32_t* best, uint8_t* inliers, int refit_rounds, int32_t* rounds, void* workspace,
                   size_t workspace_bytes, void* stream) {
    RelArgs a;
    a.m = matches; a.scores = scores; a.offsets = offsets; a.K0 = K0; a.K1 = K1; a.N = N; a.M = M; a.sc_thres = sc_thres; a.seed = seed;
    a.pixel_thr = (double)pixel_thr;
    a.E = E; a.R = R; a.t = t; a.valid = valid; a.n_inliers = n_inliers; a.n_cheiral = n_cheiral; a.best = best; a.inliers = inliers;
    a.rounds = rounds;
    return rt_run<RelModel>(name, "rel_ransac", a,
                            matches && offsets && K0 && K1 && E && R && t && valid && n_inliers && n_cheiral && best && inliers && (!lo || rounds),
                            pixel_thr, iters, lo, refit_rounds, workspace, workspace_bytes,
                            lo ? gf_relpose_lo_workspace_bytes(N, M, iters) : gf_relpose_workspace_bytes(N, M, iters), stream);
}

extern "C" int gf_relpose_ransac(const float* matches, const float* scores, const int32_t* offsets, int N, int M, const float* K0, const float* K1,
                                 float sc_thres, float pixel_thr, int iters, uint32_t seed, double* E, double* R, double* t, int32_t* valid,
                                 int32_t* n_inliers, int32_t* n_cheiral, int32_t* best, uint8_t* inliers, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    return rel_run("gf_relpose_ransac", false, matches, scores, offsets, N, M, K0, K1, sc_thres, pixel_thr, iters, seed, E, R, t, valid, n_inliers,
                   n_cheiral, best, inliers, 0, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int gf_relpose_ransac_lo(const float* matches, const float* scores, const int32_t* offsets, int N, int M, const float* K0,
                                    const float* K1, float sc_thres, float pixel_thr, int iters, uint32_t seed, double* E, double* R, double* t,
                                    int32_t* valid, int32_t* n_inliers, int32_t* n_cheiral, int32_t* best, uint8_t* inliers, int refit_rounds,
                                    int32_t* rounds, void* workspace, size_t workspace_bytes, void* stream) {
    return rel_run("gf_relpose_ransac_lo", true, matches, scores, offsets, N, M, K0, K1, sc_thres, pixel_thr, iters, seed, E, R, t, valid, n_inliers,
                   n_cheiral, best, inliers, refit_rounds, rounds, workspace, workspace_bytes, stream);
}
