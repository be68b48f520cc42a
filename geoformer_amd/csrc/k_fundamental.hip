// On-device two-view verification without intrinsics: fundamental-matrix RANSAC for every pair of a match list in three launches.  The
// kernels run, operation for operation and in fp64 with contraction off, the algorithm stated in fund_solver.h, which host/fund_host.cpp
// compiles for the CPU: valid, the chosen hypothesis, the inlier mask and F can be checked bit for bit.  OpenCV parity is UNPINNED.
//
// Pairs are addressed by an offsets array [N + 1] in DEVICE memory (the layout consolidate_matches uploads): a block reads its two
// entries, no prefix loop.  Offsets are clamped to [0, M] and to ascending order before anything is indexed with them.
//
//   fund_prepare : grid N, 256 threads.  Stable compaction of the pair's surviving rows (fs_row_valid) into the workspace, 256 rows at a
//                  time: ballot per wave, prefix = popcount of the lower lanes + the counts of the lower waves, in row order.  Min / max
//                  of the surviving points per image through an LDS tree (order-free: min and max are exact), then fs_box_norm.
//   fund_score   : grid N * (iters / 64), 256 threads; block b works for pair b / (iters / 64).  The 64 lanes of wave 0 each draw the 7
//                  rows of one hypothesis and run the seven-point solver with EVERYTHING it indexes at run time - the 7x9 system, the
//                  null space, the cubic, its roots, the up to 3 solutions - in an LDS tile of FS_WS_DOUBLES doubles per hypothesis,
//                  interleaved across the 64 solver lanes (element i of hypothesis h at ws[64 i + h]: lanes hit 64 consecutive doubles,
//                  conflict-free).  Nothing of the elimination lives in a lane's scratch memory (k_ransac.hip's header records what that
//                  cost the homography kernel).  Then all four waves score: wave w owns hypotheses 16 w .. 16 w + 15, walks the pair's
//                  surviving rows 64 at a time and counts the Sampson inliers of every root with one ballot + popcount - a wave-uniform
//                  integer, no shuffle reduction, no float atomics.  The block's best (most inliers, smallest hypothesis, smallest root)
//                  goes to the workspace with its F: 11 words per block, not per hypothesis.
//                  FS_HYP_PER_WG = 64: the tile is 64 x 81 x 8 B = 41,472 B; 128 hypotheses (82,944 B) would pass the 64 KiB a kernel may
//                  declare statically - the static LDS limit bound the choice - and 64 is also exactly one wave of solver lanes.
//   fund_final   : grid N, 256 threads.  Best block (same order), then the winner's inlier set over the pair's ORIGINAL rows (filtered
//                  rows 0), the count through ballot + popcount and an integer LDS atomic (order-free), F, valid, best.
// No host synchronisation; every output is the same in every run.
#include "gf_common.h"
#include "fund_solver.h"

#pragma clang fp contract(off)

namespace {

constexpr int FUND_MAX_BLOCKS = 1 << 24;      // grid x 256 threads must stay below 2^32 threads

struct FundArgs {
    const float* m;          // [M][4] x0, y0, x1, y1 (px), sorted by pair
    const float* scores;     // [M] or null
    const int32_t* offsets;  // [N + 1]
    int N, M, iters, nblk;
    float sc_thres;
    double thr2;
    uint32_t seed;
    int32_t* rows;           // [M]        per pair: the surviving rows (relative to the pair's first), ascending
    int32_t* use;            // [N]        surviving rows where the pair can be estimated (>= 7, both boxes with an extent), else 0
    double* norm;            // [N][6]
    double* blk_F;           // [N][nblk][9]  best solution of every block
    long long* blk_key;      // [N][nblk]     its inlier count * 2^32 + (2^31 - 1 - hypothesis); -1: no solution
    int32_t* blk_root;       // [N][nblk]
    double* F;               // [N][9]
    int32_t* valid;          // [N]
    int32_t* n_inliers;      // [N]
    int32_t* best;           // [N][2] hypothesis, root (-1 when not valid)
    uint8_t* inliers;        // [M]
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

__global__ __launch_bounds__(256) void fund_score(FundArgs a) {
    __shared__ double ws[FS_WS_DOUBLES * FS_HYP_PER_WG];
    __shared__ int s_nroot[FS_HYP_PER_WG];
    __shared__ int s_cnt[FS_HYP_PER_WG * FS_MAX_ROOTS];
    __shared__ long long s_key[FS_HYP_PER_WG];
    __shared__ int s_root[FS_HYP_PER_WG];
    const int n = (int)(blockIdx.x / (unsigned)a.nblk), hb = (int)(blockIdx.x % (unsigned)a.nblk);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int cnt = a.use[n];
    if (cnt == 0) return;                                              // (uniform per block; fund_final does not read blk_* then)
    int off, len;
    fund_range(a, n, off, len);
    const float* m = a.m + 4 * (size_t)off;
    const int32_t* rows = a.rows + off;
    for (int i = tid; i < FS_HYP_PER_WG * FS_MAX_ROOTS; i += 256) s_cnt[i] = 0;
    if (tid < FS_HYP_PER_WG) {
        const int t = hb * FS_HYP_PER_WG + tid;                        // < iters: iters is a multiple of FS_HYP_PER_WG
        int idx[7], nr = 0;
        if (fs_draw7(a.seed, (uint32_t)n, (uint32_t)t, cnt, m, rows, idx)) {
            double x0[7][2], x1[7][2], nm[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) nm[k] = a.norm[6 * (size_t)n + k];
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const float* q = m + 4 * (size_t)rows[idx[k]];
                x0[k][0] = (double)q[0]; x0[k][1] = (double)q[1]; x1[k][0] = (double)q[2]; x1[k][1] = (double)q[3];
            }
            nr = fs_seven_point(x0, x1, nm, GsWs{ws + tid, FS_HYP_PER_WG});
        }
        s_nroot[tid] = nr;
    }
    __syncthreads();
    // ---- scoring: this wave's 16 hypotheses against every surviving row of the pair
    for (int i0 = 0; i0 < cnt; i0 += 64) {
        const int i = i0 + lane;
        const bool have = i < cnt;
        float q[4] = {0.f, 0.f, 0.f, 0.f};
        if (have) {
            const float* p = m + 4 * (size_t)rows[i];
            q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; q[3] = p[3];
        }
        for (int g = 0; g < FS_HYP_PER_WG / 4; ++g) {
            const int h = wave * (FS_HYP_PER_WG / 4) + g, nr = s_nroot[h];
            for (int r = 0; r < nr; ++r) {
                double F[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) F[k] = ws[(FS_OFF_F + 9 * r + k) * FS_HYP_PER_WG + h];
                const int in = have && fs_inlier(F, q, a.thr2);
                const int pc = __popcll(__ballot(in));
                if (lane == 0) s_cnt[h * FS_MAX_ROOTS + r] += pc;     // this wave alone touches its hypotheses' counters
            }
        }
    }
    __syncthreads();
    if (tid < FS_HYP_PER_WG) {
        const int t = hb * FS_HYP_PER_WG + tid, nr = s_nroot[tid];
        int bc = -1, br = -1;
        for (int r = 0; r < nr; ++r) {
            const int c = s_cnt[tid * FS_MAX_ROOTS + r];
            if (c > bc) { bc = c; br = r; }
        }
        s_key[tid] = bc < 0 ? -1ll : (((long long)bc << 32) | (long long)(0x7FFFFFFF - t));
        s_root[tid] = br;
    }
    __syncthreads();
    if (tid == 0) {
        long long key = -1;
        int bh = -1;
        for (int h = 0; h < FS_HYP_PER_WG; ++h)
            if (s_key[h] > key) { key = s_key[h]; bh = h; }
        const size_t o = (size_t)n * a.nblk + hb;
        a.blk_key[o] = key;
        a.blk_root[o] = bh < 0 ? -1 : s_root[bh];
        if (bh >= 0)
            for (int k = 0; k < 9; ++k) a.blk_F[o * 9 + k] = ws[(FS_OFF_F + 9 * s_root[bh] + k) * FS_HYP_PER_WG + bh];
    }
}

__global__ __launch_bounds__(256) void fund_final(FundArgs a) {
    __shared__ long long sh_key[256];
    __shared__ int sh_blk[256];
    __shared__ double sh_F[9];
    __shared__ int sh_nin;
    const int n = blockIdx.x, t = threadIdx.x, lane = t & 63;
    int off, len;
    fund_range(a, n, off, len);
    uint8_t* mask = a.inliers + off;
    const float* m = a.m + 4 * (size_t)off;
    const float* sc = a.scores ? a.scores + off : nullptr;
    // ---- best block: max count, ties -> smallest hypothesis (the key's low word)
    long long key = -1;
    int blk = -1;
    if (a.use[n] > 0)
        for (int i = t; i < a.nblk; i += 256) {
            const long long kk = a.blk_key[(size_t)n * a.nblk + i];
            if (kk > key) { key = kk; blk = i; }
        }
    sh_key[t] = key;
    sh_blk[t] = blk;
    if (t == 0) sh_nin = 0;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (t < s && sh_key[t + s] > sh_key[t]) { sh_key[t] = sh_key[t + s]; sh_blk[t] = sh_blk[t + s]; }      // keys are distinct unless -1
        __syncthreads();
    }
    key = sh_key[0];
    blk = sh_blk[0];
    if (key < 0) {                                                     // (uniform: every thread holds the same key)
        for (int i = t; i < len; i += 256) mask[i] = 0;
        if (t == 0) {
            for (int k = 0; k < 9; ++k) a.F[9 * (size_t)n + k] = 0.0;
            a.valid[n] = 0; a.n_inliers[n] = 0; a.best[2 * n] = -1; a.best[2 * n + 1] = -1;
        }
        return;
    }
    const size_t o = (size_t)n * a.nblk + blk;
    if (t < 9) sh_F[t] = a.blk_F[o * 9 + t];
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
        a.best[2 * n] = 0x7FFFFFFF - (int)(key & 0xFFFFFFFFll); a.best[2 * n + 1] = a.blk_root[o];
    }
}

}   // namespace

extern "C" size_t gf_fundamental_workspace_bytes(int N, int M, int iters) {
    if (N <= 0 || M < 0 || iters <= 0) return 0;
    const size_t nb = (size_t)N * ((size_t)(iters + FS_HYP_PER_WG - 1) / FS_HYP_PER_WG);
    return gf_align_up((size_t)M * sizeof(int32_t), 256) + gf_align_up((size_t)N * sizeof(int32_t), 256) +
           gf_align_up((size_t)N * 6 * sizeof(double), 256) + gf_align_up(nb * 9 * sizeof(double), 256) +
           gf_align_up(nb * sizeof(long long), 256) + gf_align_up(nb * sizeof(int32_t), 256);
}

extern "C" int gf_fundamental_ransac(const float* matches, const float* scores, const int32_t* offsets, int N, int M, float sc_thres,
                                     float pixel_thr, int iters, uint32_t seed, double* F, int32_t* valid, int32_t* n_inliers,
                                     int32_t* best, uint8_t* inliers, void* workspace, size_t workspace_bytes, void* stream) {
    GF_CHECK_ARG(matches && offsets && F && valid && n_inliers && best && inliers, "null pointer");
    GF_CHECK_ARG(M >= 0, "need M >= 0");
    GF_CHECK_ARG(iters > 0 && iters % FS_HYP_PER_WG == 0, "iters must be a positive multiple of 64 (the hypotheses of one workgroup)");
    GF_CHECK_ARG(N > 0 && (long long)N * (iters / FS_HYP_PER_WG) <= FUND_MAX_BLOCKS,
                 "N out of range: need N > 0 and N * (iters / 64) <= 16777216 workgroups in one launch");
    GF_CHECK_ARG(pixel_thr > 0.f && pixel_thr < INFINITY, "pixel_thr must be positive and finite");
    if (workspace == nullptr || workspace_bytes < gf_fundamental_workspace_bytes(N, M, iters)) {
        gf_set_error("gf_fundamental_ransac: workspace too small");
        return GF_ERR_WORKSPACE;
    }
    FundArgs a;
    a.m = matches; a.scores = scores; a.offsets = offsets; a.N = N; a.M = M; a.iters = iters; a.nblk = iters / FS_HYP_PER_WG;
    a.sc_thres = sc_thres; a.thr2 = (double)pixel_thr * (double)pixel_thr; a.seed = seed;
    const size_t nb = (size_t)N * a.nblk;
    GfCarver cv(workspace);
    a.rows = cv.take<int32_t>((size_t)M);
    a.use = cv.take<int32_t>((size_t)N);
    a.norm = cv.take<double>((size_t)N * 6);
    a.blk_F = cv.take<double>(nb * 9);
    a.blk_key = cv.take<long long>(nb);
    a.blk_root = cv.take<int32_t>(nb);
    a.F = F; a.valid = valid; a.n_inliers = n_inliers; a.best = best; a.inliers = inliers;
    hipStream_t st = (hipStream_t)stream;
    void* tok = gf_prof_begin("fund_ransac", st, (double)N * iters);
    fund_prepare<<<N, 256, 0, st>>>(a);
    fund_score<<<(unsigned)nb, 256, 0, st>>>(a);
    fund_final<<<N, 256, 0, st>>>(a);
    gf_prof_end("fund_ransac", tok, st);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
