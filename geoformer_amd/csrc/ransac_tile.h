// The RANSAC around the minimal solvers, stated once for k_ransac.hip (homography), k_pose.hip (essential matrix), k_fundamental.hip
// (fundamental matrix), k_abspose.hip (absolute pose) and k_relpose.hip (essential matrix for the pairs of a match list).  Device only: the
// host builds keep their own serial loops (host/pose_host.cpp, host/fund_host.cpp, host/abspose_host.cpp, host/relpose_host.cpp,
// oracle/ransac_oracle.c), the independent statements the kernels are tested against bit for bit.
//
// k_fundamental.hip, k_abspose.hip and k_relpose.hip are this file's stages - rt_prepare, rt_score, rt_final, rt_refit, and for
// k_relpose.hip rt_pose, launched by rt_run - over a Model each; k_ransac.hip, k_pose.hip and k_triangulate.hip use the helpers only.
//
//   rt_counts_range   a pair's slice of a match list addressed by a device-side counts array, clamped to the buffers' capacity.
//   rt_key            the selection rule "most inliers, then the smallest hypothesis" as one integer: count * 2^32 + (2^31 - 1 - hypothesis),
//                     -1 for "no solution".  Keys of different hypotheses are distinct, so a maximum over them does not depend on the order
//                     of reduction.  rt_key_count / rt_key_hyp take it apart; the packing is written nowhere else.
//   rt_best_key       the largest key of a 256-thread block and the payload that came with it, through LDS: rt_best_block's reduction.
//                     ransac_final and pose_final need no payload and keep their own maximum over rt_key, so that loop exists there too:
//                     ransac_final measured 2 - 3 % slower through this helper, and k_pose.hip's kernels are left as they compiled before.
//   RtBlocks          the per-block winners of rt_score in the workspace, 11 words per block: its size (rt_blocks_bytes), its carving
//                     (rt_blocks_take) and its reduction to the pair's winner (rt_best_block: rt_best_key, payload = the block).
//   rt_score<Model>   the scoring kernel: a flat grid of N * nblk blocks of 256 threads; block b works for pair b / nblk on hypotheses
//                     Model::HYP (b % nblk) ..
//                     - the first HYP lanes each draw a sample and run the minimal solver (Model::solve) with EVERYTHING it indexes at run
//                       time in an LDS tile of Model::WS doubles per hypothesis, interleaved across the solver lanes (element i of
//                       hypothesis h at ws[HYP i + h]: the lanes hit HYP consecutive doubles, conflict-free).  Nothing of the elimination
//                       lives in a lane's scratch memory (k_ransac.hip's header records what that cost the homography kernel);
//                     - all four waves score: wave w owns hypotheses (HYP / 4) w .. (HYP / 4)(w + 1) - 1, walks the pair's rows 64 at a time
//                       (Model::load) and counts the inliers (Model::inlier) of every root with one ballot + popcount - a wave-uniform
//                       integer, no shuffle reduction, no float atomics, no cross-wave traffic;
//                     - per hypothesis the best root (most inliers, then the smallest root), then the block's best hypothesis by rt_key,
//                       written with its solution to the block's slot of RtBlocks.
//                     k_pose.hip's pose_score is the same stage written out with per-hypothesis results: on this kernel's per-block
//                     winners it measured 1 - 3.5 % slower (profiles/ransac_tile.txt).  k_relpose.hip runs the same solver through this
//                     kernel at HYP = 32: 0.991 of pose_score + pose_final (0.976 .. 1.012, profiles/relative_pose.txt), inside the spread.
//
// The stages around rt_score, for problems addressed by an offsets array [N + 1] in device memory (gs_offsets_range of solver_common.h: a
// block reads its two entries, clamped before anything is indexed with them).  Grid N, 256 threads, one workgroup a problem:
//   rt_prepare<Model> stable compaction of the problem's surviving rows (Model::row_valid) into the workspace, 256 rows at a time: ballot per
//                     wave, prefix = popcount of the lower lanes + the counts of the lower waves, in row order.  Min / max of Model::BOX
//                     coordinates of the surviving rows through an LDS tree (order-free: min and max are exact), then thread 0 conditions
//                     (Model::condition) and writes use[n] - the surviving rows, 0 when the problem cannot be estimated - and norm.
//   rt_final<Model>   best block (rt_best_block), then the winner's inlier set over the problem's ORIGINAL rows (Model::original_inlier:
//                     the filter again, filtered rows 0), the count through ballot + popcount and an integer LDS atomic (order-free), the
//                     model's outputs, valid, n_inliers, best.  No solution: zero mask and outputs, valid 0, best -1.
//   rt_refit<Model>   launched only when refit_rounds > 0: the three launches above and their bits do not know of it.  One workgroup runs all
//                     rounds for its problem: stop below Model::MIN_INLIERS, Model::fit on the current set, the candidate scored by all
//                     threads as rt_final scores, "set unchanged" as a block-wide OR, a candidate with fewer inliers ends the rounds.  The
//                     current and the candidate set over the SURVIVING rows live in the workspace, one byte per row each, and change
//                     places when a candidate is accepted.  The last pass writes the model's outputs, n_inliers and the mask at the
//                     surviving rows (filtered rows stay 0 from rt_final) - nothing when no round was accepted - and rounds[n].
//   rt_pose<Model>    launched only for a model that declares the hook `pose`, between rt_final and rt_refit: what the model derives from the
//                     winner with the whole workgroup (k_relpose.hip: the pose of an essential matrix by the inliers' votes), and where
//                     that fails the withdrawal of valid, mask and outputs.  The other models launch exactly what they launched before.
//   rt_block_sums<NS> for Model::fit: the block sum of NS per-thread partials with the bits of fs_refit_tree.
//   rt_run<Model>     the entry point: the argument checks under the caller's name, the workspace carved, the launches between
//                     gf_prof_begin / gf_prof_end, rounds = 0 when nothing was refitted.
//
// A Model is a plain struct with the types Args (the kernels' argument; the members rt_run and the stages name: offsets, N, M, thr2, rows,
// use, norm, blk, valid, n_inliers, best, inliers, refit_rounds, set[2], rounds), Row and Cand (a refit's model), the constants HYP
// (hypotheses per workgroup, 64 or 32: iters is a multiple of 64 for every model), ROOTS (solutions per hypothesis at most), WS, OFF_SOL (where solve leaves
// solution r: 9 doubles at OFF_SOL + 9 r), BOX, NORM (doubles of norm per problem), MIN_INLIERS, MAX_ROUNDS, and the __forceinline__ hooks
//     void bind(const Args&, int n, int off)                 problem n's slices of the inputs, its first row being off; reads no workspace
//     int  init(const Args&, int n)                          bind, and what prepare left; returns the number of rows to score, 0 when the
//                                                            problem cannot be estimated (rt_score's block then writes nothing)
//     static void take(Args&, GfCarver&)                     host: what the model keeps in the workspace for itself, between norm and blk
//   rt_prepare
//     bool row_valid(int i) const                            does original row i take part
//     float coord(int i, int k) const                        its coordinate k < BOX
//     int  condition(int base, lo[BOX], hi[BOX], norm[NORM]) const     norm from the box of `base` surviving rows; 0: cannot be estimated
//   rt_score
//     int  solve(int t, const GsWs& w) const                 draw hypothesis t and solve it in w; returns the number of solutions
//     Row  load(int i, bool have) const                      surviving row i as inlier() wants it (have = 0: past the end, any value)
//     int  inlier(const double (&S)[9], const Row&) const
//   rt_final (write_*: thread 0)
//     int  original_inlier(const double (&S)[9], int i) const          row_valid and the predicate, on original row i
//     void write_invalid(const Args&, int n) const           the model's outputs for "no solution"
//     void write_solution(const Args&, int n, const double (&S)[9]) const
//   rt_pose (optional)
//     void pose(const Args&, int n, int len) const           block-cooperative: all 256 threads call it for problem n of len original rows
//                                                            behind rt_final's outputs; its own LDS, its own barriers
//   rt_refit
//     Cand load_winner(const Args&, int n) const             what rt_final wrote, as a Cand
//     int  fit(const uint8_t* cur, int cnt, Cand& c) const   block-cooperative: all 256 threads call it with c = the current model and
//                                                            leave with the same candidate; returns a uniform ok.  Its own LDS, its own
//                                                            barriers (it starts and ends behind one); every thread may read cur[i] at
//                                                            its own rows i = t, t + 256, .. only
//     int  cand_inlier(const Cand&, int i) const             the predicate on surviving row i
//     void write_refined(const Args&, int n, const Cand&) const        thread 0: the model's outputs
// Whatever only one model needs - intrinsics, a conditioning transform, the winner kept for the refit - lives in its struct.
// A stage is a KERNEL, not a device function called from one kernel per model: with that one more level of inlining the compiler unrolled
// the seven-point elimination completely (70 -> 106 SGPRs, 82 of them spilled, 36 B of scratch reserved per lane); as a kernel template
// FundModel compiles to what the hand-written fund_score did, and so do the three stages around it (profiles/ransac_stages.txt).
#pragma once
#include "gf_common.h"
#include "solver_common.h"

#pragma clang fp contract(off)

constexpr int RT_MAX_BLOCKS = 1 << 24;        // a flat grid x 256 threads must stay below 2^32 threads

// counts [1 + N]: total, then per pair (device memory, so nothing read from it is trusted: negative counts are 0, the slice ends at capacity)
__device__ __forceinline__ void rt_counts_range(const int32_t* counts, int n, int capacity, int& off, int& cnt) {
    off = 0;
    for (int b = 0; b < n; ++b) off += max(counts[1 + b], 0);
    cnt = max(counts[1 + n], 0);
    if (off > capacity) off = capacity;
    if (cnt > capacity - off) cnt = capacity - off;
}

__device__ __forceinline__ long long rt_key(int count, int t) { return ((long long)count << 32) | (long long)(0x7FFFFFFF - t); }
__device__ __forceinline__ int rt_key_count(long long key) { return key < 0 ? -1 : (int)(key >> 32); }
__device__ __forceinline__ int rt_key_hyp(long long key) { return key < 0 ? -1 : 0x7FFFFFFF - (int)(key & 0xFFFFFFFFll); }

// every thread of the block (256, all active) brings its best key and a payload; every thread gets the block's best key back, and its
// payload (unspecified when no thread has a key >= 0).  Once per kernel: the LDS is not fenced against a second call.
__device__ __forceinline__ long long rt_best_key(long long key, int& payload) {
    __shared__ long long sh_key[256];
    __shared__ int sh_pay[256];
    const int t = threadIdx.x;
    sh_key[t] = key;
    sh_pay[t] = payload;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (t < s && sh_key[t + s] > sh_key[t]) { sh_key[t] = sh_key[t + s]; sh_pay[t] = sh_pay[t + s]; }
        __syncthreads();
    }
    payload = sh_pay[0];
    return sh_key[0];
}

struct RtBlocks {
    int nblk;                // blocks per pair: hypotheses / Model::HYP
    double* sol;             // [N][nblk][9]  best solution of every block
    long long* key;          // [N][nblk]     rt_key of its inlier count and hypothesis; -1: no solution
    int32_t* root;           // [N][nblk]
};
static inline size_t rt_blocks_bytes(size_t nb) {
    return gf_align_up(nb * 9 * sizeof(double), 256) + gf_align_up(nb * sizeof(long long), 256) + gf_align_up(nb * sizeof(int32_t), 256);
}
static inline RtBlocks rt_blocks_take(GfCarver& cv, int N, int nblk) {
    const size_t nb = (size_t)N * nblk;
    RtBlocks b;
    b.nblk = nblk;
    b.sol = cv.take<double>(nb * 9);
    b.key = cv.take<long long>(nb);
    b.root = cv.take<int32_t>(nb);
    return b;
}

// the best block of pair n (any = 0: its blocks wrote nothing) -> its key, and its slot in b.sol / b.root (meaningless when the key is -1)
__device__ __forceinline__ long long rt_best_block(const RtBlocks& b, int n, bool any, size_t& slot) {
    const long long* keys = b.key + (size_t)n * b.nblk;
    long long key = -1;
    int blk = -1;
    if (any)
        for (int i = threadIdx.x; i < b.nblk; i += 256)
            if (keys[i] > key) { key = keys[i]; blk = i; }
    key = rt_best_key(key, blk);
    slot = (size_t)n * b.nblk + blk;
    return key;
}

template <class Model>
__global__ __launch_bounds__(256) void rt_score(typename Model::Args a) {
    constexpr int HYP = Model::HYP, ROOTS = Model::ROOTS, OFF_SOL = Model::OFF_SOL;
    __shared__ double ws[Model::WS * HYP];
    __shared__ int s_nroot[HYP];
    __shared__ int s_cnt[HYP * ROOTS];
    __shared__ long long s_key[HYP];
    __shared__ int s_root[HYP];
    const int n = (int)(blockIdx.x / (unsigned)a.blk.nblk), hb = (int)(blockIdx.x % (unsigned)a.blk.nblk);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    Model md;
    const int cnt = md.init(a, n);
    if (cnt == 0) return;                                              // (uniform per block; rt_best_block is told not to read the slots)
    for (int i = tid; i < HYP * ROOTS; i += 256) s_cnt[i] = 0;
    if (tid < HYP) s_nroot[tid] = md.solve(hb * HYP + tid, GsWs{ws + tid, HYP});
    __syncthreads();
    for (int i0 = 0; i0 < cnt; i0 += 64) {
        const bool have = i0 + lane < cnt;
        const typename Model::Row row = md.load(i0 + lane, have);
        for (int g = 0; g < HYP / 4; ++g) {
            const int h = wave * (HYP / 4) + g, nr = s_nroot[h];
            for (int r = 0; r < nr; ++r) {
                double S[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) S[k] = ws[(OFF_SOL + 9 * r + k) * HYP + h];
                const int in = have && md.inlier(S, row);
                const int pc = __popcll(__ballot(in));
                if (lane == 0) s_cnt[h * ROOTS + r] += pc;            // this wave alone touches its hypotheses' counters
            }
        }
    }
    __syncthreads();
    if (tid < HYP) {
        const int nr = s_nroot[tid];
        int bc = -1, br = -1;
        for (int r = 0; r < nr; ++r) {
            const int c = s_cnt[tid * ROOTS + r];
            if (c > bc) { bc = c; br = r; }
        }
        s_key[tid] = bc < 0 ? -1ll : rt_key(bc, hb * HYP + tid);
        s_root[tid] = br;
    }
    __syncthreads();
    if (tid == 0) {
        long long key = -1;
        int bh = -1;
        for (int h = 0; h < HYP; ++h)
            if (s_key[h] > key) { key = s_key[h]; bh = h; }
        const size_t o = (size_t)n * a.blk.nblk + hb;
        a.blk.key[o] = key;
        a.blk.root[o] = bh < 0 ? -1 : s_root[bh];
        if (bh >= 0)
            for (int k = 0; k < 9; ++k) a.blk.sol[o * 9 + k] = ws[(OFF_SOL + 9 * s_root[bh] + k) * HYP + bh];
    }
}

// ---- the stages around rt_score for problems addressed by an offsets array (gs_offsets_range): grid N, 256 threads, one workgroup a problem

template <class Model>
__global__ __launch_bounds__(256) void rt_prepare(typename Model::Args a) {
    constexpr int BOX = Model::BOX, NORM = Model::NORM;
    __shared__ int s_wave[4];
    __shared__ float s_red[2 * BOX][256];
    const int n = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int off, len;
    gs_offsets_range(a.offsets, n, a.M, off, len);
    Model md;
    md.bind(a, n, off);
    int32_t* rows = a.rows + off;
    float mn[BOX], mx[BOX];
#pragma unroll
    for (int k = 0; k < BOX; ++k) { mn[k] = INFINITY; mx[k] = -INFINITY; }
    int base = 0;
    for (int i0 = 0; i0 < len; i0 += 256) {
        const int i = i0 + tid;
        const bool v = i < len && md.row_valid(i);
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
            for (int k = 0; k < BOX; ++k) {
                const float c = md.coord(i, k);
                mn[k] = c < mn[k] ? c : mn[k];
                mx[k] = c > mx[k] ? c : mx[k];
            }
        }
        base += total;
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < BOX; ++k) { s_red[2 * k][tid] = mn[k]; s_red[2 * k + 1][tid] = mx[k]; }
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < BOX; ++k) {
                const float p = s_red[2 * k][tid + s], q = s_red[2 * k + 1][tid + s];
                if (p < s_red[2 * k][tid]) s_red[2 * k][tid] = p;
                if (q > s_red[2 * k + 1][tid]) s_red[2 * k + 1][tid] = q;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        float lo[BOX], hi[BOX];
        double nm[NORM];
#pragma unroll
        for (int k = 0; k < BOX; ++k) { lo[k] = s_red[2 * k][0]; hi[k] = s_red[2 * k + 1][0]; }
#pragma unroll
        for (int k = 0; k < NORM; ++k) nm[k] = 0.0;
        const int ok = md.condition(base, lo, hi, nm);
        a.use[n] = ok ? base : 0;
#pragma unroll
        for (int k = 0; k < NORM; ++k) a.norm[NORM * (size_t)n + k] = nm[k];
    }
}

template <class Model>
__global__ __launch_bounds__(256) void rt_final(typename Model::Args a) {
    __shared__ double sh_S[9];
    __shared__ int sh_nin;
    const int n = blockIdx.x, t = threadIdx.x, lane = t & 63;
    int off, len;
    gs_offsets_range(a.offsets, n, a.M, off, len);
    Model md;
    md.init(a, n);
    uint8_t* mask = a.inliers + off;
    if (t == 0) sh_nin = 0;
    // ---- best block: most inliers, then the smallest hypothesis
    size_t o;
    const long long key = rt_best_block(a.blk, n, a.use[n] > 0, o);
    if (key < 0) {                                                     // (uniform: every thread holds the same key)
        for (int i = t; i < len; i += 256) mask[i] = 0;
        if (t == 0) {
            md.write_invalid(a, n);
            a.valid[n] = 0; a.n_inliers[n] = 0; a.best[2 * n] = -1; a.best[2 * n + 1] = -1;
        }
        return;
    }
    if (t < 9) sh_S[t] = a.blk.sol[o * 9 + t];
    __syncthreads();
    double S[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) S[k] = sh_S[k];
    for (int i0 = 0; i0 < len; i0 += 256) {
        const int i = i0 + t;
        const int in = i < len && md.original_inlier(S, i);
        if (i < len) mask[i] = (uint8_t)in;
        const int pc = __popcll(__ballot(in));
        if (lane == 0 && pc) atomicAdd(&sh_nin, pc);
    }
    __syncthreads();
    if (t == 0) {
        md.write_solution(a, n, S);
        a.valid[n] = 1; a.n_inliers[n] = sh_nin;
        a.best[2 * n] = rt_key_hyp(key); a.best[2 * n + 1] = a.blk.root[o];
    }
}

// the block sum of the 256 threads' partials acc[e] -> dst[e], all threads calling: a wave's xor butterfly leaves the sum of its 64 partials
// in lane 0 with the bits of fs_refit_tree, the four waves meet in LDS as (b0 + b1) + (b2 + b3).  Ends on a barrier: dst may be read, and
// sh_part written again, right after.
template <int NS>
__device__ __forceinline__ void rt_block_sums(double (&acc)[NS], double (*sh_part)[NS], double* dst) {
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
#pragma unroll
    for (int e = 0; e < NS; ++e) {
#pragma unroll
        for (int stride = 32; stride >= 1; stride >>= 1) acc[e] = acc[e] + __shfl_xor(acc[e], stride, 64);
        if (lane == 0) sh_part[wave][e] = acc[e];
    }
    __syncthreads();
    if (t < NS) dst[t] = (sh_part[0][t] + sh_part[1][t]) + (sh_part[2][t] + sh_part[3][t]);
    __syncthreads();
}

template <class Model>
__global__ __launch_bounds__(256) void rt_refit(typename Model::Args a) {
    __shared__ int sh_nin, sh_diff;
    const int n = blockIdx.x, t = threadIdx.x, lane = t & 63;
    int off, len;
    gs_offsets_range(a.offsets, n, a.M, off, len);
    Model md;
    const int cnt = min(md.init(a, n), len);                           // (uniform; the compacted list has at most len entries)
    if (!a.valid[n] || cnt == 0) {
        if (t == 0) a.rounds[n] = 0;
        return;
    }
    const int32_t* rows = a.rows + off;
    uint8_t* mask = a.inliers + off;
    uint8_t* cur = a.set[0] + off;
    uint8_t* cand = a.set[1] + off;
    typename Model::Cand best = md.load_winner(a, n);
    int nin = a.n_inliers[n], rounds = 0;
    // every thread reads and writes the sets at its own rows only (i = t, t + 256, ..): no fence between the rounds
    for (int i = t; i < cnt; i += 256) cur[i] = mask[rows[i]];
    for (int r = 0; r < a.refit_rounds; ++r) {
        if (nin < Model::MIN_INLIERS) break;
        if (t == 0) { sh_nin = 0; sh_diff = 0; }
        __syncthreads();
        typename Model::Cand c = best;
        if (!md.fit(cur, cnt, c)) break;                               // (uniform)
        // ---- re-selection over all surviving rows
        int differ = 0;
        for (int i0 = 0; i0 < cnt; i0 += 256) {
            const int i = i0 + t;
            int in = 0;
            if (i < cnt) {
                in = md.cand_inlier(c, i);
                cand[i] = (uint8_t)in;
                differ |= in != (int)cur[i];
            }
            const int pc = __popcll(__ballot(in));
            if (lane == 0 && pc) atomicAdd(&sh_nin, pc);
        }
        if (__ballot(differ) != 0ull && lane == 0) atomicOr(&sh_diff, 1);
        __syncthreads();
        const int cn = sh_nin, changed = sh_diff;
        __syncthreads();                                               // (both are reset at the top of the next round)
        if (cn < nin) break;
        best = c;
        nin = cn;
        uint8_t* tmp = cur; cur = cand; cand = tmp;
        ++rounds;
        if (!changed) break;
    }
    if (rounds > 0) {
        for (int i = t; i < cnt; i += 256) mask[rows[i]] = cur[i];
        if (t == 0) {
            md.write_refined(a, n, best);
            a.n_inliers[n] = nin;
        }
    }
    if (t == 0) a.rounds[n] = rounds;
}

// a model with the hook `pose` gets one more launch between rt_final and rt_refit
template <class Model, class = void>
struct rt_has_pose { static constexpr bool value = false; };
template <class Model>
struct rt_has_pose<Model, decltype((void)&Model::pose)> { static constexpr bool value = true; };

template <class Model>
__global__ __launch_bounds__(256) void rt_pose(typename Model::Args a) {
    const int n = blockIdx.x;
    int off, len;
    gs_offsets_range(a.offsets, n, a.M, off, len);
    Model md;
    md.init(a, n);
    md.pose(a, n, len);
}

// ---- the entry point around the launches

#define RT_CHECK_ARG(cond, msg)                                   \
    do {                                                          \
        if (!(cond)) {                                            \
            gf_set_error("%s: %s", name, msg);                    \
            return GF_ERR_INVALID_ARGUMENT;                       \
        }                                                         \
    } while (0)

// `a` comes with the caller's inputs and outputs (N, M, rounds among them) and leaves with the workspace carved: rows, use, norm, what the
// model keeps for itself (Model::take), the blocks, and with `refit` the two inlier sets.  refit = false: an entry without the refit stage
// (no `rounds`, no sets, refit_rounds not looked at).  `pointers`: the caller's own null check; `need`: its workspace size.  `name` goes into
// the messages, `tag` to the profiler.
template <class Model>
static int rt_run(const char* name, const char* tag, typename Model::Args& a, bool pointers, float pixel_thr, int iters, bool refit,
                  int refit_rounds, void* workspace, size_t workspace_bytes, size_t need, void* stream) {
    static_assert((Model::HYP == 64 || Model::HYP == 32) && Model::MAX_ROUNDS == 8, "the messages below name these numbers");
    const int N = a.N, M = a.M;
    RT_CHECK_ARG(pointers, "null pointer");
    RT_CHECK_ARG(M >= 0, "need M >= 0");
    RT_CHECK_ARG(iters > 0 && iters % 64 == 0, Model::HYP == 64 ? "iters must be a positive multiple of 64 (the hypotheses of one workgroup)"
                                                                 : "iters must be a positive multiple of 64 (two workgroups of 32 hypotheses)");
    RT_CHECK_ARG(N > 0 && (long long)N * (iters / Model::HYP) <= RT_MAX_BLOCKS,
                 Model::HYP == 64 ? "N out of range: need N > 0 and N * (iters / 64) <= 16777216 workgroups in one launch"
                                  : "N out of range: need N > 0 and N * (iters / 32) <= 16777216 workgroups in one launch");
    RT_CHECK_ARG(pixel_thr > 0.f && pixel_thr < INFINITY, "pixel_thr must be positive and finite");
    RT_CHECK_ARG(!refit || (refit_rounds >= 0 && refit_rounds <= Model::MAX_ROUNDS), "refit_rounds must be 0 .. 8");
    if (workspace == nullptr || workspace_bytes < need) {
        gf_set_error("%s: workspace too small", name);
        return GF_ERR_WORKSPACE;
    }
    a.thr2 = (double)pixel_thr * (double)pixel_thr;
    a.refit_rounds = refit ? refit_rounds : 0;
    GfCarver cv(workspace);
    a.rows = cv.take<int32_t>((size_t)M);
    a.use = cv.take<int32_t>((size_t)N);
    a.norm = cv.take<double>((size_t)N * Model::NORM);
    Model::take(a, cv);
    a.blk = rt_blocks_take(cv, N, iters / Model::HYP);
    a.set[0] = refit ? cv.take<uint8_t>((size_t)M) : nullptr;
    a.set[1] = refit ? cv.take<uint8_t>((size_t)M) : nullptr;
    hipStream_t st = (hipStream_t)stream;
    void* tok = gf_prof_begin(tag, st, (double)N * iters);
    rt_prepare<Model><<<N, 256, 0, st>>>(a);
    rt_score<Model><<<(unsigned)N * a.blk.nblk, 256, 0, st>>>(a);
    rt_final<Model><<<N, 256, 0, st>>>(a);
    if constexpr (rt_has_pose<Model>::value) rt_pose<Model><<<N, 256, 0, st>>>(a);
    if (a.refit_rounds > 0) rt_refit<Model><<<N, 256, 0, st>>>(a);
    gf_prof_end(tag, tok, st);
    if (refit && a.refit_rounds == 0 && hipMemsetAsync(a.rounds, 0, (size_t)N * sizeof(int32_t), st) != hipSuccess) {
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
