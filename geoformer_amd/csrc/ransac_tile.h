// The RANSAC around the minimal solvers, stated once for k_ransac.hip (homography), k_pose.hip (essential matrix) and k_fundamental.hip
// (fundamental matrix).  Device only: the host builds keep their own serial loops (host/pose_host.cpp, host/fund_host.cpp,
// oracle/ransac_oracle.c), the independent statements the kernels are tested against bit for bit.
//
//   rt_counts_range   a pair's slice of a match list addressed by a device-side counts array, clamped to the buffers' capacity.
//   rt_key            the selection rule "most inliers, then the smallest hypothesis" as one integer: count * 2^32 + (2^31 - 1 - hypothesis),
//                     -1 for "no solution".  Keys of different hypotheses are distinct, so a maximum over them does not depend on the order
//                     of reduction.  rt_key_count / rt_key_hyp take it apart; the packing is written nowhere else.
//   rt_best_key       the largest key of a 256-thread block and the payload that came with it, through LDS: fund_final's reduction.
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
//                     A Model is a plain struct with the constants HYP (hypotheses per workgroup, a multiple of 4, at most 256), ROOTS
//                     (solutions per hypothesis at most), WS, OFF_SOL (where solve leaves solution r: 9 doubles at OFF_SOL + 9 r), the types
//                     Args (the kernel's argument, with a member `RtBlocks blk`) and Row, and
//                         int  init(const Args&, int n)             take what pair n needs from the arguments; returns the number of rows to
//                                                                   score, 0 when the pair cannot be estimated (the block then writes nothing)
//                         int  solve(int t, const GsWs& w) const    draw hypothesis t and solve it in w; returns the number of solutions
//                         Row  load(int i, bool have) const         row i of the pair as inlier() wants it (have = 0: past the end, any value)
//                         int  inlier(const double (&S)[9], const Row&) const
//                     Whatever only one model needs - intrinsics, a compacted row list, a conditioning transform - lives in its struct.
//                     The stage is the KERNEL, not a device function called from one kernel per model: with that one more level of inlining
//                     the compiler unrolled the seven-point elimination completely (70 -> 106 SGPRs, 82 of them spilled, 36 B
//                     of scratch reserved per lane); as a kernel template FundModel compiles to what the hand-written fund_score did.
//                     Instantiated by k_fundamental.hip and k_abspose.hip (AbsModel: P3P, a pose as two rows of R and t).  k_pose.hip's pose_score is the same stage written out with per-hypothesis
//                     results: on this kernel's per-block winners it measured 1 - 3.5 % slower (profiles/ransac_tile.txt).
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
