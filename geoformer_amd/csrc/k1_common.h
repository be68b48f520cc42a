// K1 (dual-softmax correlation sweep), what its three objects share:
//   k1_dual_softmax.hip  inference: the tile kernels of both passes, the pipelined panel form of pass B, selection, compaction
//   k1_stats_panel.hip   the panel form of pass A, an object of its own because it is built without SLP vectorisation
//   k1_coarse_loss.hip   training: the sparse-supervision loss on the same statistics and its backward
#pragma once
#include <math.h>

#include <type_traits>

#include "gf_common.h"

struct K1Args {
    const void* f0;
    const void* f1;
    int N, L, S, C;
    const uint8_t* mask0;
    const uint8_t* mask1;
    float inv_c, temperature, mult;   // sim = acc*inv_c/temperature (exact) or acc*mult (fast)
    int tilesM, tilesN;
    int rowparts;      // number of row partials per row: tilesN (tile form) or the number of tile runs (panel form)
    float2* rowpart;   // [N][rowparts][L]  (max, sumexp)
    float2* colpart;   // [N][tilesM][S]
    float2* rstat;     // [N][L]  (max, sum)
    float2* cstat;     // [N][S]
    unsigned long long* rowbest;   // [N][L]  max over candidates of (conf bits << 32 | ~col); 0 = none
    unsigned* colmax;              // [N][S]  max conf bits over candidates; 0 = none
    float* conf;
    float thr;
    int dense;                     // thr so low that candidates are not rare: reduce in the tile first
    unsigned long long* stamp;     // [K1_STAMP_WORDS] or null: what the statistics in this workspace belong to (k1_stamp_words)
    int esize;                     // bytes per feature element (the stamp's content fingerprint samples whole 8-byte words)
};

// host functions that cross the objects (dtype: GF_F32 / GF_F16 / GF_BF16)
// pass A (k1_dual_softmax.hip): the panel form when `panel`, else one workgroup per tile; sets a.rowparts.  `panel` is the caller's
// to decide and is not checked here: k1_stats_panel needs 16-bit features, no masks, L % 128 == 0, S % 64 == 0 and C == 256.
// Then the reduction of the partials to a.rstat / a.cstat.
void k1_stats_launch(K1Args& a, int dtype, bool panel, hipStream_t st);
void k1_reduce_launch(const K1Args& a, int dtype, hipStream_t st);
void k1_stats_panel_launch(const K1Args& a, int dtype, int wgs, hipStream_t st);      // k1_stats_panel.hip (GF_F16 / GF_BF16)

namespace {

constexpr int BM = 128, BN = 64, NT = 256;      // workgroup tile; 4 waves stacked along M, each 32 rows x 64 cols
constexpr int ROWB = 128;                        // bytes per LDS operand row = one K step
constexpr int STAGE_BYTES = (BM + BN) * ROWB;    // 24 KiB, single stage (the next step's tile waits in registers)
constexpr float NEG_INF = -INFINITY;
constexpr float LOG2E = 1.4426950408889634f;
// the panel forms (k1_stats_panel, k1_conf_pipe, k1_grad_panel): a workgroup keeps 128 rows of one side as MFMA A fragments in
// registers and streams the other side's 64-row tiles [64][512 B] through LDS, 16-byte chunk c of row r at slot c ^ (r & 15)
constexpr int PANEL_TILES = 10;                   // column tiles per unit of the persistent walk (k1_walk)
constexpr int PANEL_LDS = BN * 512 + BM * 8;      // one tile + [128] float2
constexpr int STATS_LDS = 2 * BN * 512 + 2 * 4 * 64 * 8 + 4 * 32 * 4;         // k1_stats_panel: two tile buffers | column partials | row maxima

// ---------------------------------------------------------------------------------------------
// tile engine: acc[ni] = the wave's 32 x 64 block (two MFMA 32x32 tiles) of f0[m0:,:] . f1[n0:,:]^T.
// 24 KiB of LDS and < 128 VGPRs per lane keep 4 workgroups (16 waves) resident per CU: the epilogue of
// one overlaps the loads and MFMAs of the others.  Operand rows are clamped; validity is applied later.
// ---------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void sim_tile(const T* __restrict__ A, const T* __restrict__ B, int L, int S, int C,
                                         int m0, int n0, char* smem, v16f (&acc)[2]) {
    using M = Mma32<T>;
    using Frag = typename M::Frag;
    constexpr int EPC = 16 / sizeof(T);
    constexpr int BK = ROWB / sizeof(T);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, lr = lane & 31;
    const int srow = tid >> 3, schunk = tid & 7;
    v4u ra[4], rb[2];
    const T* ga[4];
    const T* gb[2];
#pragma unroll
    for (int p = 0; p < 4; ++p) ga[p] = A + (size_t)min(m0 + srow + 32 * p, L - 1) * C + schunk * EPC;
#pragma unroll
    for (int p = 0; p < 2; ++p) gb[p] = B + (size_t)min(n0 + srow + 32 * p, S - 1) * C + schunk * EPC;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ni][r] = 0.f;
    char* sa = smem;
    char* sb = smem + BM * ROWB;
    const int nk = C / BK;
#pragma unroll
    for (int p = 0; p < 4; ++p) ra[p] = *reinterpret_cast<const v4u*>(ga[p]);
#pragma unroll
    for (int p = 0; p < 2; ++p) rb[p] = *reinterpret_cast<const v4u*>(gb[p]);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 4; ++p) *reinterpret_cast<v4u*>(sa + gf_lds_off(srow + 32 * p, schunk)) = ra[p];
#pragma unroll
        for (int p = 0; p < 2; ++p) *reinterpret_cast<v4u*>(sb + gf_lds_off(srow + 32 * p, schunk)) = rb[p];
        __syncthreads();
        if (kt + 1 < nk) {
            const int k0 = (kt + 1) * BK;
#pragma unroll
            for (int p = 0; p < 4; ++p) ra[p] = *reinterpret_cast<const v4u*>(ga[p] + k0);
#pragma unroll
            for (int p = 0; p < 2; ++p) rb[p] = *reinterpret_cast<const v4u*>(gb[p] + k0);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int chunk = 2 * g + h;
            const Frag a0 = *reinterpret_cast<const Frag*>(sa + gf_lds_off(wave * 32 + lr, chunk));
            const Frag b0 = *reinterpret_cast<const Frag*>(sb + gf_lds_off(lr, chunk));
            const Frag b1 = *reinterpret_cast<const Frag*>(sb + gf_lds_off(32 + lr, chunk));
            M::mma(a0, b0, acc[0]);
            M::mma(a0, b1, acc[1]);
        }
    }
    __syncthreads();                 // the staging area is reused as scratch by the epilogues
}

// XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (each with its own L2), so
// id % 8 labels the XCD.  Giving every XCD a CONTIGUOUS run of tiles (row panel after row panel) keeps
// its f0 row panel and the f1 column tiles in that XCD's L2 instead of re-fetching them 8 times.
// Bijective for any tile count (speed only; correctness never depends on placement).
__device__ __forceinline__ void k1_tile(const K1Args& a, int& bm, int& bn) {
    const int nt = a.tilesM * a.tilesN, id = blockIdx.x;
    const int xcd = id & 7, slot = id >> 3, q = nt >> 3, r = nt & 7;
    const int t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
    bm = t / a.tilesN;
    bn = t % a.tilesN;
}

template <bool EXACT>
__device__ __forceinline__ float k1_exp(float x) {
    if constexpr (EXACT) return expf(x);
    else return __expf(x);
}

// Per-lane view of the wave's 32x64 block after the MFMAs: slot r (0..15) -> row m0 + wave*32 +
// acc_row(r, h); column ni -> n0 + ni*32 + (lane & 31).
struct LaneGeom {
    unsigned row_in, row_ok;   // bit r: row < L ; mask0 true (or no mask)
    unsigned col_in, col_ok;   // bit ni
};

// Branch-free; the packed words are made opaque so that the compiler keeps them as VGPRs instead of
// dozens of live lane masks in SGPRs (which spilled thousands of SGPRs).
__device__ __forceinline__ LaneGeom k1_geom(const K1Args& a, int n, int m0, int n0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, lr = lane & 31;
    LaneGeom g;
    const int row0 = m0 + wave * 32, col0 = n0 + lr;
    g.row_in = 0;
    g.row_ok = 0;
    const bool masked = a.mask0 != nullptr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row0 + gf_acc_row(r, h);
        const unsigned in = row < a.L ? 1u : 0u;
        g.row_in |= in << r;
        if (masked) g.row_ok |= (in & (a.mask0[(size_t)n * a.L + min(row, a.L - 1)] != 0 ? 1u : 0u)) << r;
    }
    if (!masked) g.row_ok = g.row_in;
    g.col_in = 0;
    g.col_ok = 0;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int col = col0 + ni * 32;
        const unsigned in = col < a.S ? 1u : 0u;
        g.col_in |= in << ni;
        if (masked) g.col_ok |= (in & (a.mask1[(size_t)n * a.S + min(col, a.S - 1)] != 0 ? 1u : 0u)) << ni;
    }
    if (!masked) g.col_ok = g.col_in;
    asm volatile("" : "+v"(g.row_in), "+v"(g.row_ok), "+v"(g.col_in), "+v"(g.col_ok));
    return g;
}

// sim values of this lane: sv[ni][r]; out-of-range -> -inf (ignored by every reduction),
// masked pair -> -1e9 exactly as masked_fill does (coarse_matching.py:123-124).
// GUARD=false is the interior, unmasked tile: no predicates at all.
template <bool EXACT, bool GUARD>
__device__ __forceinline__ void k1_sim_values(const K1Args& a, const LaneGeom& g, const v16f (&acc)[2], float (&sv)[2][16]) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float raw = acc[ni][r];
            float s;
            if constexpr (EXACT) s = (raw * a.inv_c) / a.temperature;
            else s = raw * a.mult;
            if constexpr (GUARD) {
                const bool in = ((g.row_in >> r) & (g.col_in >> ni) & 1u) != 0;
                const bool ok = ((g.row_ok >> r) & (g.col_ok >> ni) & 1u) != 0;
                s = in ? (ok ? s : -1e9f) : NEG_INF;
            }
            sv[ni][r] = s;
        }
}

__device__ __forceinline__ bool k1_interior(const K1Args& a, int m0, int n0) {
    return a.mask0 == nullptr && m0 + BM <= a.L && n0 + BN <= a.S;
}

// reduction over the 64 columns of the wave's block for each of its 16 row slots: the 32 (ni, r) values
// go through the 32-lane reduce-scatter (lane c ends with slot c = ni*16 + r), lanes c and c^16 then hold
// the two column halves of row slot r = c & 15
template <typename V, typename Op>
__device__ __forceinline__ V k1_row_reduce(V (&v)[32], Op op) {
    const V x = gf_reduce_scatter32(v, op);
    return op(x, gf_shfl_xor16(x));
}

// The row / column statistics a gf_dual_softmax_match call leaves in its workspace are stamped with what they were computed
// from (shape, scale, the two feature pointers); gf_dual_softmax_conf_at compares the stamp with its own arguments on the
// device and returns NaN for every entry when they differ (nothing else ties a later conf_at call to that call).
// Round 5: the caching allocator hands the address of a freed feature tensor to the next one of the same shape (the
// second CoarseMatching pass, the next batch), so pointers alone do not tell whose statistics the workspace holds: the LAST word is a
// fingerprint of the CONTENT - 32 eight-byte samples of each tensor, evenly spaced, one per lane of a wave, mixed and XOR-reduced.
// A SAMPLED check (512 bytes): it catches the workspace being reused for other tensors at the same addresses (the case that happens:
// the caching allocator hands the next batch the same blocks), not an in-place edit of a few rows between the two calls - a caller that
// edits f0 / f1 in place re-runs the statistics pass (ops.py says so).
constexpr int K1_STAMP_WORDS = 5;          // the words k1_stamp_word() makes; word K1_STAMP_WORDS is the fingerprint
__device__ __forceinline__ unsigned long long k1_fingerprint(const void* f0, const void* f1, size_t bytes0, size_t bytes1, int lane) {
    const bool second = lane >= 32;
    const unsigned short* p = (const unsigned short*)(second ? f1 : f0);      // two-byte pieces: a 16-bit tensor at an odd storage offset
    const size_t words = (second ? bytes1 : bytes0) / 8;                      // is only 2-byte aligned
    const int k = lane & 31;
    unsigned long long w = 0ull;
    if (words) {
        const unsigned short* q = p + 4 * ((words - 1) * (size_t)k / 31);
        w = (unsigned long long)q[0] | ((unsigned long long)q[1] << 16) | ((unsigned long long)q[2] << 32) | ((unsigned long long)q[3] << 48);
    }
    w = (w + 0x9e3779b97f4a7c15ull * (unsigned long long)(lane + 1)) * 0xff51afd7ed558ccdull;
    w ^= w >> 33;
    unsigned lo = (unsigned)w, hi = (unsigned)(w >> 32);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo ^= (unsigned)__shfl_xor((int)lo, d, 64);
        hi ^= (unsigned)__shfl_xor((int)hi, d, 64);
    }
    return ((unsigned long long)hi << 32) | lo;
}
__host__ __device__ __forceinline__ unsigned long long k1_stamp_word(int k, const void* f0, const void* f1, int N, int L, int S, int C, float mult) {
    union { float f; unsigned u; } m;
    m.f = mult;
    switch (k) {
        case 0: return 0x6b31737461747321ull;                                              // "k1stats!": a stamp has been written at all
        case 1: return ((unsigned long long)(unsigned)N << 32) | (unsigned)L;
        case 2: return ((unsigned long long)(unsigned)S << 32) | (unsigned)C;
        case 3: return (unsigned long long)(uintptr_t)f0 ^ ((unsigned long long)m.u << 40);
        default: return (unsigned long long)(uintptr_t)f1;
    }
}

// ---------------------------------------------------------------------------------------------
// panel forms: LDS offset of chunk `chunk` of tile row `row`, and the persistent walk of k1_stats_panel / k1_conf_pipe.
// A unit = (sample, row panel, run of up to PANEL_TILES column tiles).  Workgroups are dealt round-robin over the 8 XCDs, so
// blockIdx.x % 8 labels the XCD: each XCD gets a CONTIGUOUS range of units [ubeg, ubeg + ucnt) - its f0 panels and f1 tiles stay in
// its own L2 - and its workgroups stride through that range: for (ui = slot; ui < ucnt; ui += per_xcd) unit ubeg + ui.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int k1p_off(int row, int chunk) { return row * 512 + ((chunk ^ (row & 15)) << 4); }

__host__ __device__ __forceinline__ int k1_runs(const K1Args& a) { return (a.tilesN + PANEL_TILES - 1) / PANEL_TILES; }
inline int k1_panel_wgs(const K1Args& a) {                     // two resident workgroups per CU
    const int units = a.N * a.tilesM * k1_runs(a);
    return units < 512 ? units : 512;
}

struct K1Walk {
    int runs, ubeg, ucnt, slot, per_xcd;
};
// k1_walk(a, blockIdx.x, gridDim.x, w).  Filled through a reference, field by field: returned by value the compiler sinks slot and
// per_xcd behind the branch of ubeg and orders the kernels' scalar preambles differently.
__device__ __forceinline__ void k1_walk(const K1Args& a, unsigned block, unsigned blocks, K1Walk& w) {
    const int runs = k1_runs(a), units = a.N * a.tilesM * runs;
    w.runs = runs;
    const int nwg = blocks, xcd = block & 7;
    w.slot = block >> 3;
    w.per_xcd = (nwg + 7 - xcd) >> 3;
    const int q = units >> 3, rem = units & 7;
    w.ubeg = xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q;
    w.ucnt = q + (xcd < rem ? 1 : 0);
}
struct K1Unit {
    int n, bm, m0, run, t0, t1;      // sample, row panel and its first row, run and its column tiles [t0, t1)
};
__device__ __forceinline__ K1Unit k1_unit(const K1Args& a, const K1Walk& w, int ui) {
    const int u = w.ubeg + ui;
    const int run = u % w.runs, pm = u / w.runs, bm = pm % a.tilesM, n = pm / a.tilesM;
    const int m0 = bm * BM, t0 = run * PANEL_TILES, t1 = min(t0 + PANEL_TILES, a.tilesN);
    return K1Unit{n, bm, m0, run, t0, t1};
}

}   // namespace
