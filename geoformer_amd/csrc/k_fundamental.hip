// On-device two-view verification without intrinsics: fundamental-matrix RANSAC for every pair of a match list in three launches, and
// a fourth when the winner is refitted on its inliers (gf_fundamental_ransac_lo, refit_rounds > 0).  The
// kernels run, operation for operation and in fp64 with contraction off, the algorithm stated in fund_solver.h, which host/fund_host.cpp
// compiles for the CPU: valid, the chosen hypothesis, the inlier mask and F can be checked bit for bit.  OpenCV parity is UNPINNED.
//
// Pairs are addressed by an offsets array [N + 1] in DEVICE memory (the layout consolidate_matches uploads): a block reads its two
// entries, no prefix loop.  Offsets are clamped to [0, M] and to ascending order before anything is indexed with them.
//
//   fund_prepare : grid N, 256 threads.  Stable compaction of the pair's surviving rows (fs_row_valid) into the workspace, 256 rows at a
//                  time: ballot per wave, prefix = popcount of the lower lanes + the counts of the lower waves, in row order.  Min / max
//                  of the surviving points per image through an LDS tree (order-free: min and max are exact), then fs_box_norm.
//   rt_score<FundModel> : grid N * (iters / 64), 256 threads: the scoring kernel of ransac_tile.h.  The 64 lanes of wave 0 each draw the
//                  7 rows of one hypothesis and run the seven-point solver - the 7x9 system, the null space, the cubic, its roots, the up
//                  to 3 solutions - in the LDS tile; the four waves count the Sampson inliers of every root over the pair's surviving
//                  rows.  The block's best (most inliers, smallest hypothesis, smallest root) goes to the workspace with its F: 11 words
//                  per block, not per hypothesis.
//                  FS_HYP_PER_WG = 64: the tile is 64 x 81 x 8 B = 41,472 B; 128 hypotheses (82,944 B) would pass the 64 KiB a kernel may
//                  declare statically - the static LDS limit bound the choice - and 64 is also exactly one wave of solver lanes.
//   fund_final   : grid N, 256 threads.  Best block (same order), then the winner's inlier set over the pair's ORIGINAL rows (filtered
//                  rows 0), the count through ballot + popcount and an integer LDS atomic (order-free), F, valid, best.
//   fund_refit   : grid N, 256 threads, launched only when refit_rounds > 0: the three launches above and their bits do not know of it.
//                  One workgroup runs all rounds of the refit rule of fund_solver.h for its pair.  Thread j holds partial j of the 45
//                  entries of the normal matrix in registers (every index compile-time); a wave's xor butterfly leaves the block sum of
//                  64 partials in lane 0 with the bits of fs_refit_tree, the four block sums meet in LDS as (b0 + b1) + (b2 + b3).  A
//                  [45][256] fp64 tree in LDS would be 92 KB, past the 64 KiB a kernel may declare statically.  fs_refit_solve follows with
//                  its workspace in LDS (225 doubles): the 9 x 9 Jacobi iteration - 360 sequential rotations - with the elements of a
//                  rotation on nine lanes of wave 0 (fund_jacobi9_wave), the rest - the 3 x 3 iteration, the rank-2 step, the way back
//                  to pixels - on thread 0.  Measured on an MI355X, 120 pairs x 1889 rows, 512 hypotheses, all four launches between
//                  device events: no refit 1.05 ms; R = 1 / 4 / 8 with everything on thread 0 1.60 / 3.15 / 4.90 ms, with the nine lanes
//                  1.36 / 2.23 / 3.38 ms (the same bits): about 0.31 ms per round run instead of 0.55, so the nine lanes stayed.
//                  The candidate is scored by all threads as fund_final scores (ballot + popcount + an integer LDS atomic),
//                  "set unchanged" is a block-wide OR.  The current and the candidate inlier sets over the surviving rows live in the
//                  workspace, one byte per row each, and change places when a candidate is accepted.  The last pass writes F, n_inliers
//                  and the mask at the surviving rows (filtered rows stay 0 from fund_final) - nothing when no round was accepted.
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
    // fund_refit only
    int refit_rounds;
    uint8_t* set[2];         // [M] each: per pair (at its offset) the current and the candidate inlier set over its SURVIVING rows
    int32_t* rounds;         // [N] accepted refits
};

// the pair's slice of the match list (offsets come from device memory: clamped into the buffers)
__device__ __forceinline__ void fund_range(const FundArgs& a, int n, int& off, int& len) {
    int o = a.offsets[n], e = a.offsets[n + 1];
    o = min(max(o, 0), a.M);
    e = min(max(e, o), a.M);
    off = o;
    len = e - o;
}

__global__ __launch_bounds__(256) void fund_prepare(FundArgs a) {
    __shared__ int s_wave[4];
    __shared__ float s_red[8][256];
    const int n = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int off, len;
    fund_range(a, n, off, len);
    const float* m = a.m + 4 * (size_t)off;
    const float* sc = a.scores ? a.scores + off : nullptr;
    int32_t* rows = a.rows + off;
    float mn[4], mx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { mn[k] = INFINITY; mx[k] = -INFINITY; }
    int base = 0;
    for (int i0 = 0; i0 < len; i0 += 256) {
        const int i = i0 + tid;
        const bool v = i < len && fs_row_valid(m + 4 * (size_t)i, sc, i, a.sc_thres);
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
            for (int k = 0; k < 4; ++k) {
                const float c = m[4 * (size_t)i + k];
                mn[k] = c < mn[k] ? c : mn[k];
                mx[k] = c > mx[k] ? c : mx[k];
            }
        }
        base += total;
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { s_red[2 * k][tid] = mn[k]; s_red[2 * k + 1][tid] = mx[k]; }
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float p = s_red[2 * k][tid + s], q = s_red[2 * k + 1][tid + s];
                if (p < s_red[2 * k][tid]) s_red[2 * k][tid] = p;
                if (q > s_red[2 * k + 1][tid]) s_red[2 * k + 1][tid] = q;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        double nm[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int ok = 0;
        if (base >= FS_MIN_MATCHES) {
            const int ok0 = fs_box_norm(s_red[0][0], s_red[1][0], s_red[2][0], s_red[3][0], nm);
            const int ok1 = fs_box_norm(s_red[4][0], s_red[5][0], s_red[6][0], s_red[7][0], nm + 3);
            ok = ok0 && ok1;
        }
        a.use[n] = ok ? base : 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) a.norm[6 * (size_t)n + k] = nm[k];
    }
}

// the fundamental-matrix model of rt_score: rows are reached through the compacted list, samples are conditioned by the pair's boxes
struct FundModel {
    static constexpr int HYP = FS_HYP_PER_WG, ROOTS = FS_MAX_ROOTS, WS = FS_WS_DOUBLES, OFF_SOL = FS_OFF_F;
    typedef FundArgs Args;
    struct Row { float q[4]; };
    const float* m;          // the pair's matches
    const int32_t* rows;     // its surviving rows
    const double* norm;      // [6]
    uint32_t seed, n;
    int cnt;
    double thr2;
    __device__ __forceinline__ int init(const FundArgs& a, int pair) {
        int off, len;
        fund_range(a, pair, off, len);
        m = a.m + 4 * (size_t)off; rows = a.rows + off; norm = a.norm + 6 * (size_t)pair;
        seed = a.seed; n = (uint32_t)pair; thr2 = a.thr2;
        return cnt = a.use[pair];
    }
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
};

__global__ __launch_bounds__(256) void fund_final(FundArgs a) {
    __shared__ double sh_F[9];
    __shared__ int sh_nin;
    const int n = blockIdx.x, t = threadIdx.x, lane = t & 63;
    int off, len;
    fund_range(a, n, off, len);
    uint8_t* mask = a.inliers + off;
    const float* m = a.m + 4 * (size_t)off;
    const float* sc = a.scores ? a.scores + off : nullptr;
    if (t == 0) sh_nin = 0;
    // ---- best block: most inliers, then the smallest hypothesis
    size_t o;
    const long long key = rt_best_block(a.blk, n, a.use[n] > 0, o);
    if (key < 0) {                                                     // (uniform: every thread holds the same key)
        for (int i = t; i < len; i += 256) mask[i] = 0;
        if (t == 0) {
            for (int k = 0; k < 9; ++k) a.F[9 * (size_t)n + k] = 0.0;
            a.valid[n] = 0; a.n_inliers[n] = 0; a.best[2 * n] = -1; a.best[2 * n + 1] = -1;
        }
        return;
    }
    if (t < 9) sh_F[t] = a.blk.sol[o * 9 + t];
    __syncthreads();
    double F[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = sh_F[k];
    for (int i0 = 0; i0 < len; i0 += 256) {
        const int i = i0 + t;
        const int in = i < len && fs_row_valid(m + 4 * (size_t)i, sc, i, a.sc_thres) && fs_inlier(F, m + 4 * (size_t)i, a.thr2);
        if (i < len) mask[i] = (uint8_t)in;
        const int pc = __popcll(__ballot(in));
        if (lane == 0 && pc) atomicAdd(&sh_nin, pc);
    }
    __syncthreads();
    if (t == 0) {
        for (int k = 0; k < 9; ++k) a.F[9 * (size_t)n + k] = F[k];
        a.valid[n] = 1; a.n_inliers[n] = sh_nin;
        a.best[2 * n] = rt_key_hyp(key); a.best[2 * n + 1] = a.blk.root[o];
    }
}

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

__global__ __launch_bounds__(256) void fund_refit(FundArgs a) {
    __shared__ double sh_ws[FS_REFIT_WS_DOUBLES];
    __shared__ double sh_part[4][FS_SYM9];
    __shared__ double sh_F[9];
    __shared__ int sh_ok, sh_nin, sh_diff;
    const int n = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    int off, len;
    fund_range(a, n, off, len);
    const int cnt = min(a.use[n], len);                                // (uniform; the compacted list has at most len entries)
    if (!a.valid[n] || cnt == 0) {
        if (t == 0) a.rounds[n] = 0;
        return;
    }
    const float* m = a.m + 4 * (size_t)off;
    const int32_t* rows = a.rows + off;
    uint8_t* mask = a.inliers + off;
    uint8_t* cur = a.set[0] + off;
    uint8_t* cand = a.set[1] + off;
    double nm[6], F[9];
#pragma unroll
    for (int k = 0; k < 6; ++k) nm[k] = a.norm[6 * (size_t)n + k];
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = a.F[9 * (size_t)n + k];
    int nin = a.n_inliers[n], rounds = 0;
    // every thread reads and writes the sets at its own rows only (i = t, t + 256, ..): no fence between the rounds
    for (int i = t; i < cnt; i += 256) cur[i] = mask[rows[i]];
    for (int r = 0; r < a.refit_rounds; ++r) {
        if (nin < FS_REFIT_MIN_INLIERS) break;
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
#pragma unroll
        for (int e = 0; e < FS_SYM9; ++e) {
#pragma unroll
            for (int stride = 32; stride >= 1; stride >>= 1) acc[e] = acc[e] + __shfl_xor(acc[e], stride, 64);
            if (lane == 0) sh_part[wave][e] = acc[e];
        }
        if (t == 0) { sh_nin = 0; sh_diff = 0; }
        __syncthreads();
        if (t < FS_SYM9) sh_ws[FS_REFIT_OFF_ACC + t] = (sh_part[0][t] + sh_part[1][t]) + (sh_part[2][t] + sh_part[3][t]);
        __syncthreads();
        // ---- eigenvector, rank 2, back to pixels
        if (wave == 0) {                                               // fs_refit_solve, its middle part across nine lanes
            if (t == 0) fs_refit_fill(GsWs{sh_ws, 1});
            fund_jacobi9_wave(sh_ws + FS_REFIT_OFF_A, sh_ws + FS_REFIT_OFF_V, lane);
        }
        if (t == 0) {
            double G[9];
            const int ok = fs_refit_finish(GsWs{sh_ws, 1}, nm, G);
            sh_ok = ok;
#pragma unroll
            for (int k = 0; k < 9; ++k) sh_F[k] = G[k];
        }
        __syncthreads();
        if (!sh_ok) break;                                             // (uniform)
        double G[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) G[k] = sh_F[k];
        // ---- re-selection over all surviving rows
        int differ = 0;
        for (int i0 = 0; i0 < cnt; i0 += 256) {
            const int i = i0 + t;
            int in = 0;
            if (i < cnt) {
                in = fs_inlier(G, m + 4 * (size_t)rows[i], a.thr2);
                cand[i] = (uint8_t)in;
                differ |= in != (int)cur[i];
            }
            const int pc = __popcll(__ballot(in));
            if (lane == 0 && pc) atomicAdd(&sh_nin, pc);
        }
        if (__ballot(differ) != 0ull && lane == 0) atomicOr(&sh_diff, 1);
        __syncthreads();
        const int c = sh_nin, changed = sh_diff;
        __syncthreads();                                               // (both are reset at the top of the next round)
        if (c < nin) break;
#pragma unroll
        for (int k = 0; k < 9; ++k) F[k] = G[k];
        nin = c;
        uint8_t* tmp = cur; cur = cand; cand = tmp;
        ++rounds;
        if (!changed) break;
    }
    if (rounds > 0) {
        for (int i = t; i < cnt; i += 256) mask[rows[i]] = cur[i];
        if (t == 0) {
            for (int k = 0; k < 9; ++k) a.F[9 * (size_t)n + k] = F[k];
            a.n_inliers[n] = nin;
        }
    }
    if (t == 0) a.rounds[n] = rounds;
}

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

#define FUND_CHECK_ARG(cond, msg)                                 \
    do {                                                          \
        if (!(cond)) {                                            \
            gf_set_error("%s: %s", name, msg);                    \
            return GF_ERR_INVALID_ARGUMENT;                       \
        }                                                         \
    } while (0)

// both entries; refit_rounds < 0: gf_fundamental_ransac (no refit, no `rounds`, its own workspace size), `name` goes into the messages
static int fund_run(const char* name, const float* matches, const float* scores, const int32_t* offsets, int N, int M, float sc_thres,
                    float pixel_thr, int iters, uint32_t seed, double* F, int32_t* valid, int32_t* n_inliers, int32_t* best, uint8_t* inliers,
                    int refit_rounds, int32_t* rounds, void* workspace, size_t workspace_bytes, void* stream) {
    const bool lo = refit_rounds >= 0;
    FUND_CHECK_ARG(matches && offsets && F && valid && n_inliers && best && inliers && (!lo || rounds), "null pointer");
    FUND_CHECK_ARG(M >= 0, "need M >= 0");
    FUND_CHECK_ARG(iters > 0 && iters % FS_HYP_PER_WG == 0, "iters must be a positive multiple of 64 (the hypotheses of one workgroup)");
    FUND_CHECK_ARG(N > 0 && (long long)N * (iters / FS_HYP_PER_WG) <= RT_MAX_BLOCKS,
                 "N out of range: need N > 0 and N * (iters / 64) <= 16777216 workgroups in one launch");
    FUND_CHECK_ARG(pixel_thr > 0.f && pixel_thr < INFINITY, "pixel_thr must be positive and finite");
    if (workspace == nullptr || workspace_bytes < (lo ? gf_fundamental_lo_workspace_bytes(N, M, iters) : gf_fundamental_workspace_bytes(N, M, iters))) {
        gf_set_error("%s: workspace too small", name);
        return GF_ERR_WORKSPACE;
    }
    FundArgs a;
    a.m = matches; a.scores = scores; a.offsets = offsets; a.N = N; a.M = M;
    a.sc_thres = sc_thres; a.thr2 = (double)pixel_thr * (double)pixel_thr; a.seed = seed;
    GfCarver cv(workspace);
    a.rows = cv.take<int32_t>((size_t)M);
    a.use = cv.take<int32_t>((size_t)N);
    a.norm = cv.take<double>((size_t)N * 6);
    a.blk = rt_blocks_take(cv, N, iters / FS_HYP_PER_WG);
    a.F = F; a.valid = valid; a.n_inliers = n_inliers; a.best = best; a.inliers = inliers;
    a.refit_rounds = lo ? refit_rounds : 0; a.rounds = rounds;
    a.set[0] = a.set[1] = nullptr;
    if (lo) { a.set[0] = cv.take<uint8_t>((size_t)M); a.set[1] = cv.take<uint8_t>((size_t)M); }
    hipStream_t st = (hipStream_t)stream;
    void* tok = gf_prof_begin("fund_ransac", st, (double)N * iters);
    fund_prepare<<<N, 256, 0, st>>>(a);
    rt_score<FundModel><<<(unsigned)N * a.blk.nblk, 256, 0, st>>>(a);
    fund_final<<<N, 256, 0, st>>>(a);
    if (a.refit_rounds > 0) fund_refit<<<N, 256, 0, st>>>(a);
    gf_prof_end("fund_ransac", tok, st);
    if (lo && a.refit_rounds == 0 && hipMemsetAsync(rounds, 0, (size_t)N * sizeof(int32_t), st) != hipSuccess) {
        gf_set_error("%s: hipMemsetAsync failed", name);
        return GF_ERR_LAUNCH;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        gf_set_error("%s: launch failed: %s", name, hipGetErrorString(e));
        return GF_ERR_LAUNCH;
    }
    return GF_OK;
}

extern "C" int gf_fundamental_ransac(const float* matches, const float* scores, const int32_t* offsets, int N, int M, float sc_thres,
                                     float pixel_thr, int iters, uint32_t seed, double* F, int32_t* valid, int32_t* n_inliers,
                                     int32_t* best, uint8_t* inliers, void* workspace, size_t workspace_bytes, void* stream) {
    return fund_run("gf_fundamental_ransac", matches, scores, offsets, N, M, sc_thres, pixel_thr, iters, seed, F, valid, n_inliers, best, inliers,
                    -1, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int gf_fundamental_ransac_lo(const float* matches, const float* scores, const int32_t* offsets, int N, int M, float sc_thres,
                                        float pixel_thr, int iters, uint32_t seed, double* F, int32_t* valid, int32_t* n_inliers,
                                        int32_t* best, uint8_t* inliers, int refit_rounds, int32_t* rounds, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    GF_CHECK_ARG(refit_rounds >= 0 && refit_rounds <= FS_REFIT_MAX_ROUNDS, "refit_rounds must be 0 .. 8");
    return fund_run("gf_fundamental_ransac_lo", matches, scores, offsets, N, M, sc_thres, pixel_thr, iters, seed, F, valid, n_inliers, best, inliers,
                    refit_rounds, rounds, workspace, workspace_bytes, stream);
}
