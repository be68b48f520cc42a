// On-device two-view verification without intrinsics: fundamental-matrix RANSAC for every pair of a match list in three launches, and
// a fourth when the winner is refitted on its inliers (gf_fundamental_ransac_lo, refit_rounds > 0).  The kernels run, operation for
// operation and in fp64 with contraction off, the algorithm stated in fund_solver.h, which host/fund_host.cpp compiles for the CPU: valid, the chosen hypothesis, the inlier mask and F can be checked bit for bit.  OpenCV parity is UNPINNED.
//
// The four stages - compaction and conditioning, scoring, the winner over the original rows, the refit rounds - and the entry point around
// them are ransac_tile.h's (rt_prepare, rt_score, rt_final, rt_refit, rt_run); pairs are addressed by an offsets array [N + 1] in DEVICE
// memory (the layout consolidate_matches uploads).  This file holds what is the fundamental matrix's:
//
//   FundModel    : rows are valid by fs_row_valid, the boxes of both images condition the samples (fs_box_norm, 4 coordinates, 6 doubles).
//                  solve: a lane of wave 0 draws the 7 rows of one hypothesis and runs the seven-point solver - the 7x9 system, the null
//                  space, the cubic, its roots, the up to 3 solutions - in the LDS tile; inliers by the Sampson distance.
//                  FS_HYP_PER_WG = 64: the tile is 64 x 81 x 8 B = 41,472 B; 128 hypotheses (82,944 B) would pass the 64 KiB a kernel may
//                  declare statically - the static LDS limit bound the choice - and 64 is also exactly one wave of solver lanes.
//   FundModel::fit : steps 2 - 5 of a round of the refit rule of fund_solver.h.  Thread j holds partial j of the 45 entries of the normal
//                  matrix in registers (every index compile-time), rt_block_sums leaves their block sum in LDS.  A [45][256] fp64 tree in
//                  LDS would be 92 KB, past the 64 KiB a kernel may declare statically.  fs_refit_solve follows with
//                  its workspace in LDS (225 doubles): the 9 x 9 Jacobi iteration - 360 sequential rotations - with the elements of a
//                  rotation on nine lanes of wave 0 (fund_jacobi9_wave), the rest - the 3 x 3 iteration, the rank-2 step, the way back
//                  to pixels - on thread 0.  Measured on an MI355X, 120 pairs x 1889 rows, 512 hypotheses, all four launches between
//                  device events: no refit 1.05 ms; R = 1 / 4 / 8 with everything on thread 0 1.60 / 3.15 / 4.90 ms, with the nine lanes
//                  1.36 / 2.23 / 3.38 ms (the same bits): about 0.31 ms per round run instead of 0.55, so the nine lanes stayed.
// No host synchronisation; every output is the same in every run.
#include "gf_common.h"
#include "fund_solver.h"
#include "ransac_tile.h"

#pragma clang fp contract(off)

namespace {

struct FundArgs {
    const float* m;          // [M][4] x0, y0, x1, y1 (px), sorted by pair
    const float* scores;     // [M] or null
    const int32_t* offsets;  // [N + 1]
    int N, M;
    float sc_thres;
    double thr2;
    uint32_t seed;
    int32_t* rows;           // [M]        per pair: the surviving rows (relative to the pair's first), ascending
    int32_t* use;            // [N]        surviving rows where the pair can be estimated (>= 7, both boxes with an extent), else 0
    double* norm;            // [N][6]
    RtBlocks blk;            // every block's best F
    double* F;               // [N][9]
    int32_t* valid;          // [N]
    int32_t* n_inliers;      // [N]
    int32_t* best;           // [N][2] hypothesis, root (-1 when not valid)
    uint8_t* inliers;        // [M]
    // rt_refit only
    int refit_rounds;
    uint8_t* set[2];         // [M] each: per pair (at its offset) the current and the candidate inlier set over its SURVIVING rows
    int32_t* rounds;         // [N] accepted refits
};

// gs_jacobi_sym<9> of fs_refit_solve with the elements of a rotation spread over the first nine lanes of a wave (lane k: row k of A and of
// V), all 64 lanes of the wave calling.  Every lane computes (c, s, t) from the same three numbers with the expressions of gs_jacobi_sym,
// every element is the same arithmetic: the same bits.  The wave runs in lockstep and its LDS operations complete in program order; the
// volatile accesses keep the compiler to that order, reads of a rotation before its writes.
__device__ __forceinline__ void fund_jacobi9_wave(volatile double* A, volatile double* V, int lane) {
    const int k = lane < 9 ? lane : 0;
    if (lane < 9)
        for (int j = 0; j < 9; ++j) V[9 * k + j] = k == j ? 1.0 : 0.0;
    for (int sw = 0; sw < FS_JACOBI9_SWEEPS; ++sw)
        for (int p = 0; p < 8; ++p)
            for (int q = p + 1; q < 9; ++q) {
                const double apq = A[9 * p + q];
                if (apq == 0.0) continue;                              // (uniform: every lane read the same number)
                const double app = A[9 * p + p], aqq = A[9 * q + q];
                const double akp = A[9 * k + p], akq = A[9 * k + q], vkp = V[9 * k + p], vkq = V[9 * k + q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double mag = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double t = theta < 0.0 ? -mag : mag;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                if (lane < 9) {
                    if (k == p) {
                        A[9 * p + p] = app - t * apq;
                        A[9 * p + q] = 0.0;
                    } else if (k == q) {
                        A[9 * q + q] = aqq + t * apq;
                        A[9 * q + p] = 0.0;
                    } else {
                        const double np = c * akp - s * akq, nq = s * akp + c * akq;
                        A[9 * k + p] = np; A[9 * p + k] = np;
                        A[9 * k + q] = nq; A[9 * q + k] = nq;
                    }
                    V[9 * k + p] = c * vkp - s * vkq;
                    V[9 * k + q] = s * vkp + c * vkq;
                }
            }
}

// the fundamental-matrix model of the stages of ransac_tile.h: rows are reached through the compacted list, samples are conditioned by the
// pair's boxes
struct FundModel {
    static constexpr int HYP = FS_HYP_PER_WG, ROOTS = FS_MAX_ROOTS, WS = FS_WS_DOUBLES, OFF_SOL = FS_OFF_F;
    static constexpr int BOX = 4, NORM = 6, MIN_INLIERS = FS_REFIT_MIN_INLIERS, MAX_ROUNDS = FS_REFIT_MAX_ROUNDS;
    typedef FundArgs Args;
    struct Row { float q[4]; };
    struct Cand { double F[9]; };
    const float* m;          // the pair's matches
    const float* sc;         // and scores, or null
    const int32_t* rows;     // its surviving rows
    const double* norm;      // [6]
    uint32_t seed, n;
    int cnt;
    float sc_thres;
    double thr2;
    __device__ __forceinline__ void bind(const FundArgs& a, int pair, int off) {
        m = a.m + 4 * (size_t)off; sc = a.scores ? a.scores + off : nullptr; rows = a.rows + off; norm = a.norm + 6 * (size_t)pair;
        seed = a.seed; n = (uint32_t)pair; sc_thres = a.sc_thres; thr2 = a.thr2;
    }
    __device__ __forceinline__ int init(const FundArgs& a, int pair) {
        int off, len;
        gs_offsets_range(a.offsets, pair, a.M, off, len);
        bind(a, pair, off);
        return cnt = a.use[pair];
    }
    static void take(FundArgs&, GfCarver&) {}
    // ---- rt_prepare
    __device__ __forceinline__ bool row_valid(int i) const { return fs_row_valid(m + 4 * (size_t)i, sc, i, sc_thres); }
    __device__ __forceinline__ float coord(int i, int k) const { return m[4 * (size_t)i + k]; }
    __device__ __forceinline__ int condition(int base, const float (&lo)[4], const float (&hi)[4], double (&nm)[6]) const {
        if (base < FS_MIN_MATCHES) return 0;
        const int ok0 = fs_box_norm(lo[0], hi[0], lo[1], hi[1], nm);
        const int ok1 = fs_box_norm(lo[2], hi[2], lo[3], hi[3], nm + 3);
        return ok0 && ok1;
    }
    // ---- rt_score
    __device__ __forceinline__ Row load(int i, bool have) const {
        Row r = {{0.f, 0.f, 0.f, 0.f}};
        if (have) {
            const float* p = m + 4 * (size_t)rows[i];
            r.q[0] = p[0]; r.q[1] = p[1]; r.q[2] = p[2]; r.q[3] = p[3];
        }
        return r;
    }
    __device__ __forceinline__ int solve(int t, const GsWs& w) const {
        int idx[7];
        if (!fs_draw7(seed, n, (uint32_t)t, cnt, m, rows, idx)) return 0;
        double x0[7][2], x1[7][2], nm[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) nm[k] = norm[k];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const Row r = load(idx[k], true);
            x0[k][0] = (double)r.q[0]; x0[k][1] = (double)r.q[1]; x1[k][0] = (double)r.q[2]; x1[k][1] = (double)r.q[3];
        }
        return fs_seven_point(x0, x1, nm, w);
    }
    __device__ __forceinline__ int inlier(const double (&F)[9], const Row& r) const { return fs_inlier(F, r.q, thr2); }
    // ---- rt_final
    __device__ __forceinline__ int original_inlier(const double (&F)[9], int i) const {
        return row_valid(i) && fs_inlier(F, m + 4 * (size_t)i, thr2);
    }
    __device__ __forceinline__ void write_invalid(const FundArgs& a, int pair) const {
        for (int k = 0; k < 9; ++k) a.F[9 * (size_t)pair + k] = 0.0;
    }
    __device__ __forceinline__ void write_solution(const FundArgs& a, int pair, const double (&F)[9]) const {
        for (int k = 0; k < 9; ++k) a.F[9 * (size_t)pair + k] = F[k];
    }
    // ---- rt_refit
    __device__ __forceinline__ Cand load_winner(const FundArgs& a, int pair) const {
        Cand c;
#pragma unroll
        for (int k = 0; k < 9; ++k) c.F[k] = a.F[9 * (size_t)pair + k];
        return c;
    }
    // steps 2 - 5 of a round of fund_solver.h on the set `cur` over the surviving rows (what c held is not used)
    __device__ __forceinline__ int fit(const uint8_t* cur, int cnt, Cand& c) const {
        __shared__ double sh_ws[FS_REFIT_WS_DOUBLES];
        __shared__ double sh_part[4][FS_SYM9];
        __shared__ double sh_F[9];
        __shared__ int sh_ok;
        const int t = threadIdx.x;
        double nm[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) nm[k] = norm[k];
        // ---- the normal matrix: partial t, ascending rows
        double acc[FS_SYM9];
#pragma unroll
        for (int e = 0; e < FS_SYM9; ++e) acc[e] = 0.0;
        for (int i = t; i < cnt; i += 256) {
            if (!cur[i]) continue;
            double row[9];
            fs_refit_row(m + 4 * (size_t)rows[i], nm, row);
            fs_refit_accum(acc, row);
        }
        rt_block_sums<FS_SYM9>(acc, sh_part, sh_ws + FS_REFIT_OFF_ACC);
        // ---- eigenvector, rank 2, back to pixels
        if (t < 64) {                                                  // fs_refit_solve, its middle part across nine lanes
            if (t == 0) fs_refit_fill(GsWs{sh_ws, 1});
            fund_jacobi9_wave(sh_ws + FS_REFIT_OFF_A, sh_ws + FS_REFIT_OFF_V, t);
        }
        if (t == 0) {
            double G[9];
            sh_ok = fs_refit_finish(GsWs{sh_ws, 1}, nm, G);
#pragma unroll
            for (int k = 0; k < 9; ++k) sh_F[k] = G[k];
        }
        __syncthreads();
        if (!sh_ok) return 0;                                          // (uniform)
#pragma unroll
        for (int k = 0; k < 9; ++k) c.F[k] = sh_F[k];
        return 1;
    }
    __device__ __forceinline__ int cand_inlier(const Cand& c, int i) const { return fs_inlier(c.F, m + 4 * (size_t)rows[i], thr2); }
    __device__ __forceinline__ void write_refined(const FundArgs& a, int pair, const Cand& c) const { write_solution(a, pair, c.F); }
};

}   // namespace

extern "C" size_t gf_fundamental_workspace_bytes(int N, int M, int iters) {
    if (N <= 0 || M < 0 || iters <= 0) return 0;
    const size_t nb = (size_t)N * ((size_t)(iters + FS_HYP_PER_WG - 1) / FS_HYP_PER_WG);
    return gf_align_up((size_t)M * sizeof(int32_t), 256) + gf_align_up((size_t)N * sizeof(int32_t), 256) +
           gf_align_up((size_t)N * 6 * sizeof(double), 256) + rt_blocks_bytes(nb);
}

extern "C" size_t gf_fundamental_lo_workspace_bytes(int N, int M, int iters) {
    const size_t base = gf_fundamental_workspace_bytes(N, M, iters);
    return base ? base + 2 * gf_align_up((size_t)M, 256) : 0;
}

// both entries; lo = 0: gf_fundamental_ransac (no refit stage, no `rounds`, its own workspace size)
static int fund_run(const char* name, bool lo, const float* matches, const float* scores, const int32_t* offsets, int N, int M, float sc_thres,
                    float pixel_thr, int iters, uint32_t seed, double* F, int32_t* valid, int32_t* n_inliers, int32_t* best, uint8_t* inliers,
                    int refit_rounds, int32_t* rounds, void* workspace, size_t workspace_bytes, void* stream) {
    FundArgs a;
    a.m = matches; a.scores = scores; a.offsets = offsets; a.N = N; a.M = M; a.sc_thres = sc_thres; a.seed = seed;
    a.F = F; a.valid = valid; a.n_inliers = n_inliers; a.best = best; a.inliers = inliers; a.rounds = rounds;
    return rt_run<FundModel>(name, "fund_ransac", a, matches && offsets && F && valid && n_inliers && best && inliers && (!lo || rounds), pixel_thr,
                             iters, lo, refit_rounds, workspace, workspace_bytes,
                             lo ? gf_fundamental_lo_workspace_bytes(N, M, iters) : gf_fundamental_workspace_bytes(N, M, iters), stream);
}

extern "C" int gf_fundamental_ransac(const float* matches, const float* scores, const int32_t* offsets, int N, int M, float sc_thres,
                                     float pixel_thr, int iters, uint32_t seed, double* F, int32_t* valid, int32_t* n_inliers,
                                     int32_t* best, uint8_t* inliers, void* workspace, size_t workspace_bytes, void* stream) {
    return fund_run("gf_fundamental_ransac", false, matches, scores, offsets, N, M, sc_thres, pixel_thr, iters, seed, F, valid, n_inliers, best,
                    inliers, 0, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int gf_fundamental_ransac_lo(const float* matches, const float* scores, const int32_t* offsets, int N, int M, float sc_thres,
                                        float pixel_thr, int iters, uint32_t seed, double* F, int32_t* valid, int32_t* n_inliers,
                                        int32_t* best, uint8_t* inliers, int refit_rounds, int32_t* rounds, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    return fund_run("gf_fundamental_ransac_lo", true, matches, scores, offsets, N, M, sc_thres, pixel_thr, iters, seed, F, valid, n_inliers, best,
                    inliers, refit_rounds, rounds, workspace, workspace_bytes, stream);
}
