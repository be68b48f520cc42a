// On-device localisation of query images: absolute-pose (P3P) RANSAC for every query of a 2-D - 3-D correspondence list in three launches,
// and a fourth when the winner is refitted on its inliers (refit_rounds > 0); and the lookup that makes the 3-D side of the list.  The
// kernels run, operation for operation and in fp64 with contraction off, the algorithm stated in abs_solver.h, which
// host/abspose_host.cpp compiles for the CPU: every output can be checked bit for bit.  pycolmap parity is UNPINNED.
//
// Problems are addressed by an offsets array [N + 1] in DEVICE memory: a block reads its two entries.  Offsets are clamped to [0, M] and
// to ascending order before anything is indexed with them.  This is the pattern of k_fundamental.hip.
//
//   abs_prepare  : grid N, 256 threads.  Stable compaction of the problem's surviving rows (as_row_valid) into the workspace, 256 rows at
//                  a time: ballot per wave, prefix = popcount of the lower lanes + the counts of the lower waves, in row order.  Min / max
//                  of the surviving 3-D points through an LDS tree (order-free), then as_box_norm.
//   rt_score<AbsModel> : grid N * (iters / 64), 256 threads: the scoring kernel of ransac_tile.h.  The 64 lanes of wave 0 each draw the 3
//                  rows of one hypothesis and run as_p3p - the quartic, its roots, the up to 4 poses - in the LDS tile (64 x 53 x 8 B =
//                  27,136 B); the four waves count the reprojection inliers of every root over the problem's surviving rows.  A pose
//                  travels as the template's 9 doubles: two rows of R and t' (as_unpack rebuilds the third row, here as on the host).
//   abs_final    : grid N, 256 threads.  Best block, then the winner's inlier set over the problem's ORIGINAL rows (filtered rows 0), the
//                  count through ballot + popcount and an integer LDS atomic (order-free), R and t in world units, valid, best; the
//                  winner's 9 doubles are kept in the workspace for abs_refit.
//   abs_refit    : grid N, 256 threads, launched only when refit_rounds > 0: the three launches above and their bits do not know of it.
//                  One workgroup runs all rounds of the refit rule of abs_solver.h for its problem.  Thread j holds partial j of the 27
//                  sums of a Gauss-Newton step in registers; a wave's xor butterfly leaves the block sum of 64 partials in lane 0 with the
//                  bits of fs_refit_tree, the four block sums meet in LDS as (b0 + b1) + (b2 + b3).  The 6 x 6 solve and the Cayley update
//                  run on thread 0 with the workspace in LDS.  The candidate is scored by all threads as abs_final scores; "set
//                  unchanged" is a block-wide OR.  The current and the candidate inlier sets over the surviving rows live in the
//                  workspace, one byte per row each, and change places when a candidate is accepted.  The last pass writes R, t,
//                  n_inliers and the mask at the surviving rows - nothing when no round was accepted.
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
    // abs_refit only
    int refit_rounds;
    uint8_t* set[2];         // [M] each: per problem (at its offset) the current and the candidate inlier set over its SURVIVING rows
    int32_t* rounds;         // [N] accepted refits
};

// the problem's slice of the list (offsets come from device memory: clamped into the buffers)
__device__ __forceinline__ void abs_range(const AbsArgs& a, int n, int& off, int& len) {
    int o = a.offsets[n], e = a.offsets[n + 1];
    o = min(max(o, 0), a.M);
    e = min(max(e, o), a.M);
    off = o;
    len = e - o;
}

__global__ __launch_bounds__(256) void abs_prepare(AbsArgs a) {
    __shared__ int s_wave[4];
    __shared__ float s_red[6][256];
    const int n = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int off, len;
    abs_range(a, n, off, len);
    const float* uv = a.uv + 2 * (size_t)off;
    const float* xyz = a.xyz + 3 * (size_t)off;
    const float* sc = a.scores ? a.scores + off : nullptr;
    int32_t* rows = a.rows + off;
    float mn[3], mx[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { mn[k] = INFINITY; mx[k] = -INFINITY; }
    int base = 0;
    for (int i0 = 0; i0 < len; i0 += 256) {
        const int i = i0 + tid;
        const bool v = i < len && as_row_valid(uv + 2 * (size_t)i, xyz + 3 * (size_t)i, sc, i, a.sc_thres);
        const unsigned long long b = __ballot(v);
        if (lane == 0) s_wave[wave] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            before += k < wave ? s_wave[k] : 0;
            total += s_wave[k];
        }
        if (v) {
            rows[base + before + __popcll(b & ((1ull << lane) - 1ull))] = i;      // < len: one slot per surviving row, in row order
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float c = xyz[3 * (size_t)i + k];
                mn[k] = c < mn[k] ? c : mn[k];
                mx[k] = c > mx[k] ? c : mx[k];
            }
        }
        base += total;
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { s_red[2 * k][tid] = mn[k]; s_red[2 * k + 1][tid] = mx[k]; }
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float p = s_red[2 * k][tid + s], q = s_red[2 * k + 1][tid + s];
                if (p < s_red[2 * k][tid]) s_red[2 * k][tid] = p;
                if (q > s_red[2 * k + 1][tid]) s_red[2 * k + 1][tid] = q;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        double nm[4] = {0.0, 0.0, 0.0, 0.0};
        int ok = 0;
        if (base >= AS_MIN_ROWS) {
            const float lo[3] = {s_red[0][0], s_red[2][0], s_red[4][0]}, hi[3] = {s_red[1][0], s_red[3][0], s_red[5][0]};
            ok = as_box_norm(lo, hi, nm);
        }
        a.use[n] = ok ? base : 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) a.norm[4 * (size_t)n + k] = nm[k];
    }
}

// the absolute-pose model of rt_score: rows are reached through the compacted list, 3-D points are conditioned by the problem's box
struct AbsModel {
    static constexpr int HYP = AS_HYP_PER_WG, ROOTS = AS_MAX_ROOTS, WS = AS_WS_DOUBLES, OFF_SOL = AS_OFF_SOL;
    typedef AbsArgs Args;
    typedef AsRow Row;
    const float* uv;         // the problem's pixels
    const float* xyz;        // and 3-D points
    const int32_t* rows;     // its surviving rows
    const float* K;          // [9]
    double nm[4];
    uint32_t seed, n;
    int cnt;
    double thr2;
    __device__ __forceinline__ int init(const AbsArgs& a, int prob) {
        int off, len;
        abs_range(a, prob, off, len);
        uv = a.uv + 2 * (size_t)off; xyz = a.xyz + 3 * (size_t)off; rows = a.rows + off; K = a.K + 9 * (size_t)prob;
#pragma unroll
        for (int k = 0; k < 4; ++k) nm[k] = a.norm[4 * (size_t)prob + k];
        seed = a.seed; n = (uint32_t)prob; thr2 = a.thr2;
        return cnt = min(a.use[prob], len);
    }
    __device__ __forceinline__ Row load(int i, bool have) const {
        Row r = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (have) {
            const size_t j = (size_t)rows[i];
            r = as_row(uv + 2 * j, xyz + 3 * j, nm);
        }
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
};

__global__ __launch_bounds__(256) void abs_final(AbsArgs a) {
    __shared__ double sh_S[9];
    __shared__ int sh_nin;
    const int n = blockIdx.x, t = threadIdx.x, lane = t & 63;
    int off, len;
    abs_range(a, n, off, len);
    uint8_t* mask = a.inliers + off;
    const float* uv = a.uv + 2 * (size_t)off;
    const float* xyz = a.xyz + 3 * (size_t)off;
    const float* sc = a.scores ? a.scores + off : nullptr;
    const float* K = a.K + 9 * (size_t)n;
    if (t == 0) sh_nin = 0;
    // ---- best block: most inliers, then the smallest hypothesis
    size_t o;
    const long long key = rt_best_block(a.blk, n, a.use[n] > 0, o);
    if (key < 0) {                                                     // (uniform: every thread holds the same key)
        for (int i = t; i < len; i += 256) mask[i] = 0;
        if (t == 0) {
            for (int k = 0; k < 9; ++k) { a.R[9 * (size_t)n + k] = 0.0; a.win[9 * (size_t)n + k] = 0.0; }
            for (int k = 0; k < 3; ++k) a.t[3 * (size_t)n + k] = 0.0;
            a.valid[n] = 0; a.n_inliers[n] = 0; a.best[2 * n] = -1; a.best[2 * n + 1] = -1;
        }
        return;
    }
    if (t < 9) sh_S[t] = a.blk.sol[o * 9 + t];
    __syncthreads();
    double S[9], nm[4];
#pragma unroll
    for (int k = 0; k < 9; ++k) S[k] = sh_S[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) nm[k] = a.norm[4 * (size_t)n + k];
    for (int i0 = 0; i0 < len; i0 += 256) {
        const int i = i0 + t;
        int in = 0;
        if (i < len && as_row_valid(uv + 2 * (size_t)i, xyz + 3 * (size_t)i, sc, i, a.sc_thres))
            in = as_inlier(S, K, as_row(uv + 2 * (size_t)i, xyz + 3 * (size_t)i, nm), a.thr2);
        if (i < len) mask[i] = (uint8_t)in;
        const int pc = __popcll(__ballot(in));
        if (lane == 0 && pc) atomicAdd(&sh_nin, pc);
    }
    __syncthreads();
    if (t == 0) {
        double R[9], tc[3], tw[3];
        as_unpack(S, R, tc);
        as_to_world(R, tc, nm, tw);
        for (int k = 0; k < 9; ++k) { a.R[9 * (size_t)n + k] = R[k]; a.win[9 * (size_t)n + k] = S[k]; }
        for (int k = 0; k < 3; ++k) a.t[3 * (size_t)n + k] = tw[k];
        a.valid[n] = 1; a.n_inliers[n] = sh_nin;
        a.best[2 * n] = rt_key_hyp(key); a.best[2 * n + 1] = a.blk.root[o];
    }
}

__global__ __launch_bounds__(256) void abs_refit(AbsArgs a) {
    __shared__ double sh_ws[AS_GN_WS_DOUBLES];
    __shared__ double sh_part[4][AS_GN_SUMS];
    __shared__ double sh_pose[12];
    __shared__ int sh_ok, sh_nin, sh_diff;
    const int n = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    int off, len;
    abs_range(a, n, off, len);
    const int cnt = min(a.use[n], len);                                // (uniform; the compacted list has at most len entries)
    if (!a.valid[n] || cnt == 0) {
        if (t == 0) a.rounds[n] = 0;
        return;
    }
    const float* uv = a.uv + 2 * (size_t)off;
    const float* xyz = a.xyz + 3 * (size_t)off;
    const float* K = a.K + 9 * (size_t)n;
    const int32_t* rows = a.rows + off;
    uint8_t* mask = a.inliers + off;
    uint8_t* cur = a.set[0] + off;
    uint8_t* cand = a.set[1] + off;
    double nm[4], S[9], R[9], tc[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) nm[k] = a.norm[4 * (size_t)n + k];
#pragma unroll
    for (int k = 0; k < 9; ++k) S[k] = a.win[9 * (size_t)n + k];
    as_unpack(S, R, tc);
    int nin = a.n_inliers[n], rounds = 0;
    // every thread reads and writes the sets at its own rows only (i = t, t + 256, ..): no fence between the rounds
    for (int i = t; i < cnt; i += 256) cur[i] = mask[rows[i]];
    for (int r = 0; r < a.refit_rounds; ++r) {
        if (nin < AS_REFIT_MIN_INLIERS) break;
        double Rc[9], tn[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rc[k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) tn[k] = tc[k];
        int ok = 1;
        for (int step = 0; step < AS_GN_STEPS; ++step) {
            // ---- the 27 sums: partial t, ascending rows
            double acc[AS_GN_SUMS];
#pragma unroll
            for (int e = 0; e < AS_GN_SUMS; ++e) acc[e] = 0.0;
            for (int i = t; i < cnt; i += 256) {
                if (!cur[i]) continue;
                const size_t j = (size_t)rows[i];
                double Ju[6], Jv[6], res[2];
                if (as_gn_row(Rc, tn, K, as_row(uv + 2 * j, xyz + 3 * j, nm), Ju, Jv, res)) as_gn_accum(acc, Ju, Jv, res);
            }
#pragma unroll
            for (int e = 0; e < AS_GN_SUMS; ++e) {
#pragma unroll
                for (int stride = 32; stride >= 1; stride >>= 1) acc[e] = acc[e] + __shfl_xor(acc[e], stride, 64);
                if (lane == 0) sh_part[wave][e] = acc[e];
            }
            __syncthreads();
            if (t < AS_GN_SUMS) sh_ws[AS_GN_OFF_ACC + t] = (sh_part[0][t] + sh_part[1][t]) + (sh_part[2][t] + sh_part[3][t]);
            __syncthreads();
            // ---- the 6 x 6 solve and the Cayley update
            if (t == 0) {
                const GsWs w{sh_ws, 1};
                int good = as_gn_solve(w);
                if (good) {
                    double d[6], Rn[9], tt[3];
#pragma unroll
                    for (int k = 0; k < 6; ++k) d[k] = sh_ws[AS_GN_OFF_X + k];
#pragma unroll
                    for (int k = 0; k < 9; ++k) Rn[k] = Rc[k];
#pragma unroll
                    for (int k = 0; k < 3; ++k) tt[k] = tn[k];
                    good = as_gn_update(d, Rn, tt);
#pragma unroll
                    for (int k = 0; k < 9; ++k) sh_pose[k] = Rn[k];
#pragma unroll
                    for (int k = 0; k < 3; ++k) sh_pose[9 + k] = tt[k];
                }
                sh_ok = good;
            }
            __syncthreads();
            ok = sh_ok;
            if (ok) {
#pragma unroll
                for (int k = 0; k < 9; ++k) Rc[k] = sh_pose[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) tn[k] = sh_pose[9 + k];
            }
            if (t == 0) { sh_nin = 0; sh_diff = 0; }
            __syncthreads();                                           // (sh_ok, sh_pose and sh_part are written again in the next step)
            if (!ok) break;                                            // (uniform)
        }
        if (!ok) break;
        // ---- re-selection over all surviving rows
        int differ = 0;
        for (int i0 = 0; i0 < cnt; i0 += 256) {
            const int i = i0 + t;
            int in = 0;
            if (i < cnt) {
                const size_t j = (size_t)rows[i];
                in = as_inlier_rt(Rc, tn, K, as_row(uv + 2 * j, xyz + 3 * j, nm), a.thr2);
                cand[i] = (uint8_t)in;
                differ |= in != (int)cur[i];
            }
            const int pc = __popcll(__ballot(in));
            if (lane == 0 && pc) atomicAdd(&sh_nin, pc);
        }
        if (__ballot(differ) != 0ull && lane == 0) atomicOr(&sh_diff, 1);
        __syncthreads();
        const int c = sh_nin, changed = sh_diff;
        __syncthreads();                                               // (both are reset after the next round's steps)
        if (c < nin) break;
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = Rc[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) tc[k] = tn[k];
        nin = c;
        uint8_t* tmp = cur; cur = cand; cand = tmp;
        ++rounds;
        if (!changed) break;
    }
    if (rounds > 0) {
        for (int i = t; i < cnt; i += 256) mask[rows[i]] = cur[i];
        if (t == 0) {
            double tw[3];
            as_to_world(R, tc, nm, tw);
            for (int k = 0; k < 9; ++k) a.R[9 * (size_t)n + k] = R[k];
            for (int k = 0; k < 3; ++k) a.t[3 * (size_t)n + k] = tw[k];
            a.n_inliers[n] = nin;
        }
    }
    if (t == 0) a.rounds[n] = rounds;
}

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

#define ABS_CHECK_ARG(cond, msg)                                  \
    do {                                                          \
        if (!(cond)) {                                            \
            gf_set_error("gf_abspose_ransac: %s", msg);           \
            return GF_ERR_INVALID_ARGUMENT;                       \
        }                                                         \
    } while (0)

extern "C" int gf_abspose_ransac(const float* p2d, const float* p3d, const float* scores, const int32_t* offsets, int N, int M, const float* K,
                                 float sc_thres, float pixel_thr, int iters, uint32_t seed, int refit_rounds, double* R, double* t,
                                 int32_t* valid, int32_t* n_inliers, int32_t* best, int32_t* rounds, uint8_t* inliers, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    ABS_CHECK_ARG(p2d && p3d && offsets && K && R && t && valid && n_inliers && best && rounds && inliers, "null pointer");
    ABS_CHECK_ARG(M >= 0, "need M >= 0");
    ABS_CHECK_ARG(iters > 0 && iters % AS_HYP_PER_WG == 0, "iters must be a positive multiple of 64 (the hypotheses of one workgroup)");
    ABS_CHECK_ARG(N > 0 && (long long)N * (iters / AS_HYP_PER_WG) <= RT_MAX_BLOCKS,
                  "N out of range: need N > 0 and N * (iters / 64) <= 16777216 workgroups in one launch");
    ABS_CHECK_ARG(pixel_thr > 0.f && pixel_thr < INFINITY, "pixel_thr must be positive and finite");
    ABS_CHECK_ARG(refit_rounds >= 0 && refit_rounds <= AS_REFIT_MAX_ROUNDS, "refit_rounds must be 0 .. 8");
    if (workspace == nullptr || workspace_bytes < gf_abspose_workspace_bytes(N, M, iters)) {
        gf_set_error("gf_abspose_ransac: workspace too small");
        return GF_ERR_WORKSPACE;
    }
    AbsArgs a;
    a.uv = p2d; a.xyz = p3d; a.scores = scores; a.offsets = offsets; a.K = K; a.N = N; a.M = M;
    a.sc_thres = sc_thres; a.thr2 = (double)pixel_thr * (double)pixel_thr; a.seed = seed;
    GfCarver cv(workspace);
    a.rows = cv.take<int32_t>((size_t)M);
    a.use = cv.take<int32_t>((size_t)N);
    a.norm = cv.take<double>((size_t)N * 4);
    a.win = cv.take<double>((size_t)N * 9);
    a.blk = rt_blocks_take(cv, N, iters / AS_HYP_PER_WG);
    a.set[0] = cv.take<uint8_t>((size_t)M);
    a.set[1] = cv.take<uint8_t>((size_t)M);
    a.R = R; a.t = t; a.valid = valid; a.n_inliers = n_inliers; a.best = best; a.inliers = inliers;
    a.refit_rounds = refit_rounds; a.rounds = rounds;
    hipStream_t st = (hipStream_t)stream;
    void* tok = gf_prof_begin("abspose_ransac", st, (double)N * iters);
    abs_prepare<<<N, 256, 0, st>>>(a);
    rt_score<AbsModel><<<(unsigned)N * a.blk.nblk, 256, 0, st>>>(a);
    abs_final<<<N, 256, 0, st>>>(a);
    if (refit_rounds > 0) abs_refit<<<N, 256, 0, st>>>(a);
    gf_prof_end("abspose_ransac", tok, st);
    if (refit_rounds == 0 && hipMemsetAsync(rounds, 0, (size_t)N * sizeof(int32_t), st) != hipSuccess) {
        gf_set_error("gf_abspose_ransac: hipMemsetAsync failed");
        return GF_ERR_LAUNCH;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        gf_set_error("gf_abspose_ransac: launch failed: %s", hipGetErrorString(e));
        return GF_ERR_LAUNCH;
    }
    return GF_OK;
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
