// K1: dual-softmax correlation sweep + mutual-nearest match extraction (CDNA4 / gfx950).
//
// Replaces CoarseMatching.forward / get_coarse_match of the reference
// (model/loftr_src/loftr/utils/coarse_matching.py:90-130, :132-212): there, ~10 full passes over
// the [N,L,S] fp32 matrix (einsum, 2 softmax, >, 2 max, 2 ==, 2 *, max, where).  Here:
//
//   pass A  k1_stats   : 128x128 MFMA tiles of sim = f0.f1^T/(C*tau); per tile the row and column
//                        (max, sum-exp) partials -> workspace.                       (no L*S traffic)
//   reduce  k1_reduce  : combine partials -> row/col softmax statistics.
//   pass B  k1_conf    : recompute the same tile (bit-identical), conf = softmax_col*softmax_row,
//                        ONE streaming write of conf [N,L,S] fp32 (the algorithmic 4*L*S bytes).
//                        Entries with conf > thr are rare (a row holds at most 1/thr of them), so the
//                        row-best (value, first column) key and the column maximum are kept with
//                        atomicMax on those candidates only - no cross-lane reduction in the hot loop
//                        (a dense in-tile reduction is used instead when thr < 0.05).
//   select  k1_select  : per row: best key, equality with the column maximum; exact
//                        first-True-column semantics incl. the tie case (re-reads that ONE row).
//   compact k1_compact : ordered compaction (torch.where order) + keypoint arithmetic.
//
// In the configuration the model runs (16-bit features, no masks, L % 128 == 0, S % 64 == 0, C == 256) both passes take their
// row-panel-persistent forms: k1_stats_panel (k1_stats_panel.hip) and k1_conf_pipe (below).  What the objects of K1 share is in
// k1_common.h; the training loss on the same statistics is k1_coarse_loss.hip.
//
// HBM roofline: pass B is bound by the conf write (L*S*4 B per sample); everything else is O(L*C).
// Measured (8 samples of 6400^2, fp16): the same two-128-B-segment store pattern alone reaches 5.6 TB/s
// (tools/probes/store_pattern.hip); pass B reaches ~3.2 TB/s: ablating the stores or 3 of its 4 K steps
// removes ~195 us each and the two do not overlap.  Non-temporal stores (conf is never re-read by this
// launch) bought 8 %.
#include "k1_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// pass A: row / column (max, sum-exp) partials of one tile
// ---------------------------------------------------------------------------------------------
template <typename T, bool GUARD>
__device__ __forceinline__ void k1_stats_epilogue(const K1Args& a, const v16f (&acc)[2], char* smem, int n, int bm, int bn) {
    constexpr bool EXACT = std::is_same<T, float>::value;
    const int m0 = bm * BM, n0 = bn * BN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, lr = lane & 31;
    LaneGeom g;
    if constexpr (GUARD) g = k1_geom(a, n, m0, n0);
    float sv[2][16];
    k1_sim_values<EXACT, GUARD>(a, g, acc, sv);
    float* rowbc = reinterpret_cast<float*>(smem) + wave * 32;             // [4][32] row maxima, per wave
    float2* colx = reinterpret_cast<float2*>(smem + 512);                   // [4 waves][64] column partials
    // ---- columns: lane-local over its 16 rows, then the other lane half
    float cm[2], cl[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        float m = NEG_INF;
#pragma unroll
        for (int r = 0; r < 16; ++r) m = fmaxf(m, sv[ni][r]);
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        const float ms = (GUARD && m == NEG_INF) ? 0.f : m;
        float l = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) l += k1_exp<EXACT>(sv[ni][r] - ms);
        l += __shfl_xor(l, 32, 64);
        cm[ni] = m;
        cl[ni] = l;
    }
    if (h == 0) {
        colx[wave * 64 + lr] = make_float2(cm[0], cl[0]);
        colx[wave * 64 + 32 + lr] = make_float2(cm[1], cl[1]);
    }
    // ---- rows
    float v[32];
#pragma unroll
    for (int q = 0; q < 32; ++q) v[q] = sv[q >> 4][q & 15];
    const float rmax = k1_row_reduce(v, GfMaxF());             // lanes c, c^16: row slot c & 15
    if (lr < 16) rowbc[h * 16 + lr] = rmax;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 32; ++q) {
        const float m = rowbc[h * 16 + (q & 15)];
        const float ms = (GUARD && m == NEG_INF) ? 0.f : m;
        v[q] = k1_exp<EXACT>(sv[q >> 4][q & 15] - ms);
    }
    const float rsum = k1_row_reduce(v, GfAddF());
    if (lr < 16) {
        const int row = m0 + wave * 32 + gf_acc_row(lr, h);
        if (row < a.L) a.rowpart[((size_t)n * a.tilesN + bn) * a.L + row] = make_float2(rmax, rsum);
    }
    // ---- combine the four waves' column partials
    const int t = threadIdx.x;
    if (t < 64) {
        float m = NEG_INF;
#pragma unroll
        for (int w = 0; w < 4; ++w) m = fmaxf(m, colx[w * 64 + t].x);
        const float ms = (m == NEG_INF) ? 0.f : m;
        float l = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) l += colx[w * 64 + t].y * k1_exp<EXACT>(colx[w * 64 + t].x - ms);
        const int col = n0 + t;
        if (col < a.S) a.colpart[((size_t)n * a.tilesM + bm) * a.S + col] = make_float2(m, l);
    }
}

template <typename T>
__global__ __launch_bounds__(NT, 4) void k1_stats(K1Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n = blockIdx.y;
    int bm, bn;
    k1_tile(a, bm, bn);
    v16f acc[2];
    sim_tile<T>((const T*)a.f0 + (size_t)n * a.L * a.C, (const T*)a.f1 + (size_t)n * a.S * a.C, a.L, a.S, a.C,
                bm * BM, bn * BN, smem, acc);
    if (k1_interior(a, bm * BM, bn * BN)) k1_stats_epilogue<T, false>(a, acc, smem, n, bm, bn);
    else k1_stats_epilogue<T, true>(a, acc, smem, n, bm, bn);
}

// combine per-tile (max, sumexp) partials: 32 rows (blockIdx.y==0) or columns (==1) per block,
// 8 threads per row each striding over the partials, merged through LDS
template <bool EXACT>
__global__ __launch_bounds__(256) void k1_reduce_stats(K1Args a) {
    __shared__ float2 sh[8][32];
    const int n = blockIdx.z;
    const bool rows = blockIdx.y == 0;
    if (a.stamp != nullptr && threadIdx.x < 64 && blockIdx.x == 0 && blockIdx.y == 0 && n == 0) {          // wave 0 of one block
        const unsigned long long fp = k1_fingerprint(a.f0, a.f1, (size_t)a.N * a.L * a.C * a.esize, (size_t)a.N * a.S * a.C * a.esize, threadIdx.x);
        if (threadIdx.x < K1_STAMP_WORDS) a.stamp[threadIdx.x] = k1_stamp_word(threadIdx.x, a.f0, a.f1, a.N, a.L, a.S, a.C, a.mult);
        if (threadIdx.x == K1_STAMP_WORDS) a.stamp[K1_STAMP_WORDS] = fp;
    }
    const int len = rows ? a.L : a.S, np = rows ? a.rowparts : a.tilesM;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + tx;
    if (blockIdx.x * 32 >= len) return;
    const float2* part = (rows ? a.rowpart : a.colpart) + (size_t)n * np * len + min(i, len - 1);
    float m = NEG_INF, l = 0.f;
    for (int p = ty; p < np; p += 8) {
        const float2 v = part[(size_t)p * len];
        const float mn = fmaxf(m, v.x);
        const float ms = (mn == NEG_INF) ? 0.f : mn;
        l = l * k1_exp<EXACT>(m - ms) + v.y * k1_exp<EXACT>(v.x - ms);
        m = mn;
    }
    sh[ty][tx] = make_float2(m, l);
    __syncthreads();
    if (ty == 0 && i < len) {
        float M = NEG_INF;
#pragma unroll
        for (int y = 0; y < 8; ++y) M = fmaxf(M, sh[y][tx].x);
        const float ms = (M == NEG_INF) ? 0.f : M;
        float lt = 0.f;
#pragma unroll
        for (int y = 0; y < 8; ++y) lt += sh[y][tx].y * k1_exp<EXACT>(sh[y][tx].x - ms);
        (rows ? a.rstat : a.cstat)[(size_t)n * len + i] = make_float2(M, lt);
    }
}

// ---------------------------------------------------------------------------------------------
// pass B: confidence tile -> HBM, row-best keys, column maxima
// ---------------------------------------------------------------------------------------------
template <typename T, bool GUARD, bool DENSE>
__device__ __forceinline__ void k1_conf_epilogue(const K1Args& a, const v16f (&acc)[2], char* smem, int n, int bm, int bn) {
    constexpr bool EXACT = std::is_same<T, float>::value;
    const int m0 = bm * BM, n0 = bn * BN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, lr = lane & 31;
    LaneGeom g;
    if constexpr (GUARD) g = k1_geom(a, n, m0, n0);
    // row statistics of the tile -> LDS once: EXACT keeps (max, sum); the fast path stores
    // (-max*log2e, 1/sum) so that conf = exp2(2*s*log2e + A_row + B_col) * (1/sum_row) * (1/sum_col),
    // ONE exponential per element (= softmax_col * softmax_row up to fp32 rounding)
    float2* rst = reinterpret_cast<float2*>(smem);
    if (threadIdx.x < BM) {
        const float2 st = a.rstat[(size_t)n * a.L + min(m0 + (int)threadIdx.x, a.L - 1)];
        rst[threadIdx.x] = EXACT ? st : make_float2(-st.x * LOG2E, __builtin_amdgcn_rcpf(st.y));
    }
    float ca[2], cb[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int col = GUARD ? min(n0 + ni * 32 + lr, a.S - 1) : n0 + ni * 32 + lr;
        const float2 st = a.cstat[(size_t)n * a.S + col];
        ca[ni] = EXACT ? st.x : -st.x * LOG2E;
        cb[ni] = EXACT ? st.y : __builtin_amdgcn_rcpf(st.y);
    }
    __syncthreads();
    const float k2 = 2.0f * a.mult * LOG2E;
    const int row_base = m0 + __builtin_amdgcn_readfirstlane(wave) * 32;
    float* cbase = a.conf + ((size_t)n * a.L + row_base) * a.S + n0;
    unsigned long long* rbest = a.rowbest + (size_t)n * a.L;
    unsigned* cmax = a.colmax + (size_t)n * a.S;
    const int lane_off = 4 * h * a.S + lr;               // 32-bit per-lane part of the store address
    unsigned long long key[DENSE ? 32 : 1];
    unsigned cbest[2] = {0u, 0u};
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float2 st = rst[wave * 32 + gf_acc_row(r, h)];
        float cf[2];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            if constexpr (EXACT) {
                float s = (acc[ni][r] * a.inv_c) / a.temperature;
                if constexpr (GUARD) {
                    const bool ok = ((g.row_ok >> r) & (g.col_ok >> ni) & 1u) != 0;
                    s = ok ? s : -1e9f;
                }
                cf[ni] = (expf(s - ca[ni]) / cb[ni]) * (expf(s - st.x) / st.y);
            } else {
                float e;
                if constexpr (GUARD) {
                    const bool ok = ((g.row_ok >> r) & (g.col_ok >> ni) & 1u) != 0;
                    const float s2 = ok ? acc[ni][r] * k2 : -2e9f * LOG2E;
                    e = __builtin_amdgcn_exp2f(s2 + (st.x + ca[ni]));
                } else {
                    e = __builtin_amdgcn_exp2f(fmaf(acc[ni][r], k2, st.x + ca[ni]));
                }
                cf[ni] = e * (st.y * cb[ni]);
            }
        }
        // the row of slot r: uniform base + compile-time multiple of S; lanes add their 32-bit offset
        float* rowp = cbase + (size_t)((r & 3) + 8 * (r >> 2)) * a.S;
        bool in0 = true, in1 = true;
        if constexpr (GUARD) {
            in0 = ((g.row_in >> r) & g.col_in & 1u) != 0;
            in1 = ((g.row_in >> r) & (g.col_in >> 1) & 1u) != 0;
        }
        if (in0) __builtin_nontemporal_store(cf[0], rowp + lane_off);
        if (in1) __builtin_nontemporal_store(cf[1], rowp + lane_off + 32);
        if constexpr (!DENSE) {
            // candidates above thr are rare (<= 1/thr per row or column): atomics on them only
            if (fmaxf(cf[0], cf[1]) > a.thr) {
                const int row = row_base + gf_acc_row(r, h);
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    if (cf[ni] > a.thr && (ni == 0 ? in0 : in1)) {
                        const int col = n0 + ni * 32 + lr;
                        const unsigned bits = __float_as_uint(cf[ni]);
                        atomicMax(rbest + row, ((unsigned long long)bits << 32) | (0xFFFFFFFFu - (unsigned)col));
                        atomicMax(cmax + col, bits);
                    }
                }
            }
        } else {
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const bool in = cf[ni] > a.thr && (ni == 0 ? in0 : in1);
                const unsigned bits = in ? __float_as_uint(cf[ni]) : 0u;
                cbest[ni] = max(cbest[ni], bits);
                key[ni * 16 + r] = in ? (((unsigned long long)bits << 32) | (0xFFFFFFFFu - (unsigned)(n0 + ni * 32 + lr))) : 0ull;
            }
        }
    }
    if constexpr (DENSE) {
        const unsigned long long kbest = k1_row_reduce(key, GfMaxU64());
        if (lr < 16 && kbest != 0ull) atomicMax(rbest + row_base + gf_acc_row(lr, h), kbest);
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const unsigned c = max(cbest[ni], (unsigned)__shfl_xor((int)cbest[ni], 32, 64));
            if (h == 0 && c != 0u) atomicMax(cmax + n0 + ni * 32 + lr, c);
        }
    }
}

template <typename T, bool DENSE>
__global__ __launch_bounds__(NT, 4) void k1_conf(K1Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n = blockIdx.y;
    int bm, bn;
    k1_tile(a, bm, bn);
    v16f acc[2];
    sim_tile<T>((const T*)a.f0 + (size_t)n * a.L * a.C, (const T*)a.f1 + (size_t)n * a.S * a.C, a.L, a.S, a.C,
                bm * BM, bn * BN, smem, acc);
    if (k1_interior(a, bm * BM, bn * BN)) k1_conf_epilogue<T, false, DENSE>(a, acc, smem, n, bm, bn);
    else k1_conf_epilogue<T, true, DENSE>(a, acc, smem, n, bm, bn);
}

// ---------------------------------------------------------------------------------------------
// pass B, row-panel-persistent pipelined form (16-bit, unmasked, L % 128 == 0, S % 64 == 0, C == 256): a workgroup keeps its 128
// f0 rows as MFMA A fragments in REGISTERS (16 k-groups x 4 VGPRs per wave) and walks a run of PANEL_TILES consecutive column
// tiles (k1_walk: each XCD a contiguous range of units); only the 64 x 512-B f1 tiles stream through LDS.
//   * the f1 tiles arrive by LDS-DMA (gf_lds_dma, swizzle applied on the source side) into TWO LDS buffers - no
//     staging registers, no ds_write pass, one barrier per tile;
//   * the run's column statistics sit in LDS (read once per unit);
//   * the 32 MFMAs of tile t+1 are interleaved with the exponentials / stores of tile t (two accumulator sets): the
//     store stream of a workgroup does not pause for its own K loop.
// The DMA of tile t+1 is waited for with a counted vmcnt: the 32 row-segment stores issued behind it stay in flight.
// Same k order as sim_tile: bit-identical sim values.  Both softmax normalisations are folded into the exponent.
// Measured at 8 pairs (tools/k1_time.py): 336 us sparse candidates, 385 us dense (bench: 334 us).
// What bounds it is NOT the store stream: with the conf stores compiled out the kernel still takes 308 us (sparse) /
// 341 us (dense), without the exponentials 323 / 353 us - it is paced by the instruction issue of its epilogue (add, fma,
// exp, lane swap, candidate bookkeeping per element) sharing the SIMDs with the 32 MFMAs per tile, at two waves per SIMD.
// ---------------------------------------------------------------------------------------------
constexpr int PIPE_LDS = 2 * BN * 512 + BM * 8 + PANEL_TILES * BN * 8;

template <typename H, bool DENSE, bool STORE>
__global__ __launch_bounds__(NT, 2) void k1_conf_pipe(K1Args a) {
    using V8 = gf_vec<H, 8>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* rst = reinterpret_cast<float*>(smem + 2 * BN * 512);              // per row:    -max log2(e) - log2(sum)
    float* cst = reinterpret_cast<float*>(smem + 2 * BN * 512 + BM * 8);     // per column of the run, likewise
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), h = lane >> 5, lr = lane & 31;
    K1Walk walk;
    k1_walk(a, blockIdx.x, gridDim.x, walk);
    const float k2 = 2.0f * a.mult * LOG2E;
    for (int ui = walk.slot; ui < walk.ucnt; ui += walk.per_xcd) {
        const K1Unit u = k1_unit(a, walk, ui);
        const int n = u.n, m0 = u.m0, t0 = u.t0, t1 = u.t1;
        const H* A = (const H*)a.f0 + ((size_t)n * a.L + m0 + wave * 32 + lr) * a.C + h * 8;
        const char* B = (const char*)((const H*)a.f1 + (size_t)n * a.S * a.C);
        V8 af[16];
#pragma unroll
        for (int kg = 0; kg < 16; ++kg) af[kg] = *reinterpret_cast<const V8*>(A + kg * 16);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (also drains the previous unit's stores: the counted waits below start clean)
        __syncthreads();                                      // previous unit's readers of rst / cst / the tile buffers are done
        // tile bn -> buffer `buf`: 32 pieces of 2 rows x 512 B, 8 per wave; LDS slot j of row r holds chunk j ^ (r & 15)
        const GfRsrc brs = gf_rsrc(B, (unsigned)a.S * a.C * (unsigned)sizeof(H));
        auto dma = [&](int bn, int buf) {
            int dl = lane;
            asm volatile("" : "+v"(dl));                     // per-piece source offsets recomputed here, not kept across the tile loop
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int p = wave * 8 + i, row = 2 * p + (dl >> 5), j = dl & 31;
                gf_lds_dma(brs, smem + buf * (BN * 512) + p * 1024, (row * a.C + ((j ^ (row & 15)) << 3)) * (int)sizeof(H), bn * BN * a.C * (int)sizeof(H));
            }
        };
        dma(t0, 0);
        if (tid < BM) {
            const float2 st = a.rstat[(size_t)n * a.L + m0 + tid];
            rst[tid] = -st.x * LOG2E - __builtin_amdgcn_logf(st.y);       // v_log_f32 = log2: exp2(.. + rst) = e^{-max} / sum
        }
        for (int i = tid; i < (t1 - t0) * BN; i += NT) {
            const float2 cs = a.cstat[(size_t)n * a.S + t0 * BN + i];
            cst[i] = -cs.x * LOG2E - __builtin_amdgcn_logf(cs.y);
        }
        const int row_base = m0 + wave * 32;
        unsigned long long* rbest = a.rowbest + (size_t)n * a.L;
        unsigned* cmax = a.colmax + (size_t)n * a.S;
        unsigned runv[DENSE ? 16 : 1], runc[DENSE ? 16 : 1];
        if constexpr (DENSE) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { runv[r] = 0u; runc[r] = 0u; }
        }
        // one row (register r of both column halves) of the epilogue of tile `bn`
        // conf = exp2(2 sim log2e + rst[row] + cst[col]): both softmax normalisations folded into the exponent (one add,
        // one fma and one exponential per element; the two products with 1/sum are gone)
        float ca[2];
        unsigned cbest[2];
#ifndef K1_CG
#define K1_CG 4
#endif
        constexpr int CG = K1_CG;                             // rows per candidate test
        [[maybe_unused]] float hold[CG][2], gmax = 0.f;
        const unsigned thr_bits = __float_as_uint(fmaxf(a.thr, 0.f));
        auto epi_begin = [&](int bn) {
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                ca[ni] = cst[(bn - t0) * BN + ni * 32 + lr];
                cbest[ni] = 0u;
            }
        };
        auto epi_row = [&](const v16f (&acc)[2], int bn, int r) {
            const int n0 = bn * BN;
            const float st = rst[wave * 32 + gf_acc_row(r, h)];
            float cf[2];
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) cf[ni] = __builtin_amdgcn_exp2f(fmaf(acc[ni][r], k2, st + ca[ni]));
            if constexpr (STORE) {                            // (match-only mode, conf == NULL: the matrix is never written)
                float* rowp = a.conf + ((size_t)n * a.L + row_base + (r & 3) + 8 * (r >> 2)) * a.S + n0;
                const gf_v2u sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(cf[0]), __float_as_uint(cf[1]), false, false);
                __builtin_nontemporal_store(__uint_as_float(sw.x), rowp + lane);
                __builtin_nontemporal_store(__uint_as_float(sw.y), rowp + 4 * a.S + lane);
            }
            if constexpr (!DENSE) {
                // candidates (conf > thr) are rare: the test runs once per CG rows on their maximum (one max3 per row; a
                // compare + branch per row cut the MFMA loop into 16 blocks), the rows are looked at one by one only on a hit
                hold[r % CG][0] = cf[0];
                hold[r % CG][1] = cf[1];
                gmax = r % CG == 0 ? fmaxf(cf[0], cf[1]) : fmaxf(gmax, fmaxf(cf[0], cf[1]));
                if (r % CG == CG - 1 && gmax > a.thr) {
#pragma unroll
                    for (int q = 0; q < CG; ++q) {
                        const int row = row_base + gf_acc_row(r - (CG - 1) + q, h);
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni)
                            if (hold[q][ni] > a.thr) {
                                const int col = n0 + ni * 32 + lr;
                                const unsigned bits = __float_as_uint(hold[q][ni]);
                                atomicMax(rbest + row, ((unsigned long long)bits << 32) | (0xFFFFFFFFu - (unsigned)col));
                                atomicMax(cmax + col, bits);
                            }
                    }
                }
            } else {
                // (conf >= 0: its bits order like its value; the threshold is applied once, to the maxima)
                const unsigned b0 = __float_as_uint(cf[0]), b1 = __float_as_uint(cf[1]);
                cbest[0] = max(cbest[0], b0);
                cbest[1] = max(cbest[1], b1);
                const bool second = b1 > b0;                          // ni = 1 is the later column: only a strict win
                const unsigned bv = second ? b1 : b0, bc = (unsigned)(n0 + lr) + (second ? 32u : 0u);
                const bool better = bv > runv[r];
                runv[r] = better ? bv : runv[r];
                runc[r] = better ? bc : runc[r];
            }
        };
        auto epi_end = [&](int bn) {
            if constexpr (DENSE) {
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    const unsigned c = max(cbest[ni], (unsigned)__shfl_xor((int)cbest[ni], 32, 64));
                    if (h == 0 && c > thr_bits) atomicMax(cmax + bn * BN + ni * 32 + lr, c);
                }
            }
        };
        v16f prev[2], cur[2];
        for (int bn = t0; bn <= t1; ++bn) {
            const bool mma = bn < t1, epi = bn > t0;
            if (mma) {
                // tile bn has landed: what was issued behind its DMA - the previous iteration's 32 row stores (and possibly
                // candidate atomics) - may stay in flight.  The unit's first two tiles have no stores behind their DMA (tile
                // t0 + 1 is requested in the iteration that only multiplies tile t0): they wait for everything.
                if (bn <= t0 + 1 || !STORE) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
            }
            __syncthreads();                                  // ... for every wave; and every wave is done with tile bn-1's buffer
            if (bn + 1 < t1) dma(bn + 1, (bn + 1 - t0) & 1);
            const char* tb = smem + ((bn - t0) & 1) * (BN * 512);
            if (epi) epi_begin(bn - 1);
            if (mma) {
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                    for (int r = 0; r < 16; ++r) cur[ni][r] = 0.f;
            }
            if (mma && epi) {
#pragma unroll
                for (int kg = 0; kg < 16; ++kg) {
                    const V8 b0 = *reinterpret_cast<const V8*>(tb + k1p_off(lr, 2 * kg + h));
                    const V8 b1 = *reinterpret_cast<const V8*>(tb + k1p_off(32 + lr, 2 * kg + h));
                    Mma32<H>::mma(af[kg], b0, cur[0]);
                    Mma32<H>::mma(af[kg], b1, cur[1]);
                    epi_row(prev, bn - 1, kg);
                }
            } else if (mma) {
#pragma unroll
                for (int kg = 0; kg < 16; ++kg) {
                    const V8 b0 = *reinterpret_cast<const V8*>(tb + k1p_off(lr, 2 * kg + h));
                    const V8 b1 = *reinterpret_cast<const V8*>(tb + k1p_off(32 + lr, 2 * kg + h));
                    Mma32<H>::mma(af[kg], b0, cur[0]);
                    Mma32<H>::mma(af[kg], b1, cur[1]);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) epi_row(prev, bn - 1, r);
            }
            if (epi) epi_end(bn - 1);
            if (mma) {
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) prev[ni] = cur[ni];
            }
        }
        if constexpr (DENSE) {
            unsigned long long key[32];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                key[r] = runv[r] > thr_bits ? (((unsigned long long)runv[r] << 32) | (0xFFFFFFFFu - runc[r])) : 0ull;
                key[16 + r] = 0ull;
            }
            const unsigned long long kbest = k1_row_reduce(key, GfMaxU64());
            if (lr < 16 && kbest != 0ull) atomicMax(rbest + row_base + gf_acc_row(lr, h), kbest);
        }
    }
}

struct SelArgs {
    const unsigned long long* stamp;   // the workspace stamp (k1_conf_at checks it)
    int N, L, S;
    const unsigned long long* rowbest;   // [N][L]
    const unsigned* colmax;              // [N][S]
    unsigned* colset;                    // [N][SET_WORDS] bitset over hash(colmax value)
    const float* conf;     // null in match-only mode: single entries are recomputed (k1_conf_entry)
    const void* f0;        // (match-only mode) the operands and statistics of the sweep
    const void* f1;
    const float2* rstat;
    const float2* cstat;
    int C;
    float mult;
    int* scanlist;         // [N*L] rows whose first-True column needs the tie rescan
    int* scancnt;          // [1]
    int* selj;             // [N][L]  matched column or -1
    int* samplecnt;        // [N][chunks]  matches per 1024-row chunk
    int chunks;
    int force_one;
    int w0c, w1c;
    float scale;
    const float* scale0;
    const float* scale1;
    int64_t* b_ids;
    int64_t* i_ids;
    int64_t* j_ids;
    float* mconf;
    float* mk0;
    float* mk1;
    int32_t* counts;
};

constexpr int SET_BITS = 1 << 20;                // per-sample bitset of column-maximum values
constexpr int SET_WORDS = SET_BITS / 32;
__device__ __forceinline__ unsigned set_hash(unsigned bits) {
    unsigned x = bits;
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x & (SET_BITS - 1);
}

// membership filter: which fp32 values occur as the maximum of SOME column
__global__ void k1_colset(SelArgs a) {
    const int n = blockIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.S) return;
    const unsigned v = a.colmax[(size_t)n * a.S + j];
    if (v == 0u) return;
    const unsigned h = set_hash(v);
    atomicOr(a.colset + (size_t)n * SET_WORDS + (h >> 5), 1u << (h & 31));
}

// one thread per (n, i): coarse_matching.py:161-185 on the candidate statistics instead of the matrix.
// rowbest holds the row maximum only if it exceeds thr (otherwise 0: no candidate, no match).
__global__ void k1_select(SelArgs a) {
    const int n = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.L) return;
    const unsigned long long k = a.rowbest[(size_t)n * a.L + i];
    int sel = -1;
    if (k != 0ull) {
        const unsigned bits = (unsigned)(k >> 32);
        const int j = (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull));
        const unsigned* cm = a.colmax + (size_t)n * a.S;
        if (cm[j] == bits) {
            sel = j;
        } else {
            // exact `mask.max(dim=2)` semantics: a LATER column may tie the row maximum AND be its own
            // column's maximum.  That needs some column whose maximum equals this row's maximum bit for
            // bit; the value filter rules that out for almost every row, the rest is queued for k1_rescan.
            const unsigned h = set_hash(bits);
            if ((a.colset[(size_t)n * SET_WORDS + (h >> 5)] >> (h & 31)) & 1u)
                a.scanlist[atomicAdd(a.scancnt, 1)] = n * a.L + i;
        }
    }
    a.selj[(size_t)n * a.L + i] = sel;
    // per-1024-row chunk counts (blockDim = 256: one ballot + one atomic per wave)
    const unsigned long long bal = __ballot(sel >= 0);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&a.samplecnt[n * a.chunks + (i >> 10)], __popcll(bal));
}

// One entry conf[n][i][j] exactly as k1_conf_pipe produces it (16-bit storage, the panel configuration), computed by one wave:
// the 32 x 32 similarity tile that holds (i, j) is multiplied with the same operands in the same k order - an MFMA result
// depends on nothing else - and pushed through the same epilogue arithmetic.  Match-only mode (conf == NULL) uses it where the
// contract mode reads the matrix: the tie rescan, the forced match, and gf_dual_softmax_conf_at.  Returned in every lane.
template <typename H>
__device__ __forceinline__ float k1_conf_entry(const SelArgs& a, int n, int i, int j) {
    using V8 = gf_vec<H, 8>;
    const int lane = threadIdx.x & 63, h = lane >> 5, lr = lane & 31;
    const int i0 = i & ~31, j0 = j & ~31;
    const H* A = (const H*)a.f0 + ((size_t)n * a.L + min(i0 + lr, a.L - 1)) * a.C + h * 8;
    const H* B = (const H*)a.f1 + ((size_t)n * a.S + min(j0 + lr, a.S - 1)) * a.C + h * 8;
    v16f acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int kg = 0; kg < a.C / 16; ++kg)
        Mma32<H>::mma(*reinterpret_cast<const V8*>(A + kg * 16), *reinterpret_cast<const V8*>(B + kg * 16), acc);
    // accumulator row ri = (r & 3) + 8 (r >> 2) + 4 h of column lane lr
    const int ri = i - i0, rsel = (ri & 3) + 4 * (ri >> 3), lsel = (j - j0) + 32 * ((ri >> 2) & 1);
    float v = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) v = r == rsel ? acc[r] : v;
    v = __shfl(v, lsel, 64);
    const float2 rs = a.rstat[(size_t)n * a.L + i], cs = a.cstat[(size_t)n * a.S + j];
    const float st = -rs.x * LOG2E - __builtin_amdgcn_logf(rs.y), ca = -cs.x * LOG2E - __builtin_amdgcn_logf(cs.y);
    return __builtin_amdgcn_exp2f(fmaf(v, 2.0f * a.mult * LOG2E, st + ca));
}

template <typename H>
__global__ __launch_bounds__(256) void k1_conf_at(SelArgs a, const int64_t* b, const int64_t* i, const int64_t* j, int P, float* out) {
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= P) return;
    // the statistics in the workspace must be those of THESE features at THIS shape, and the entry must exist: NaN otherwise
    bool ok = true;
#pragma unroll
    for (int k = 0; k < K1_STAMP_WORDS; ++k) ok = ok && a.stamp[k] == k1_stamp_word(k, a.f0, a.f1, a.N, a.L, a.S, a.C, a.mult);
    ok = ok && a.stamp[K1_STAMP_WORDS] == k1_fingerprint(a.f0, a.f1, (size_t)a.N * a.L * a.C * sizeof(H), (size_t)a.N * a.S * a.C * sizeof(H),
                                                         threadIdx.x & 63);
    const long long bb = b[e], ii = i[e], jj = j[e];
    ok = ok && bb >= 0 && bb < a.N && ii >= 0 && ii < a.L && jj >= 0 && jj < a.S;
    if (!ok) {                                                              // wave-uniform: e is per wave
        if ((threadIdx.x & 63) == 0) out[e] = __builtin_nanf("");
        return;
    }
    const float c = k1_conf_entry<H>(a, (int)bb, (int)ii, (int)jj);
    if ((threadIdx.x & 63) == 0) out[e] = c;
}

// rows queued by k1_select: one wave per row walks the (L2-resident) column maxima for later columns
// that hold the same value and confirms the tie on the confidence matrix itself
template <typename H, bool MATCH_ONLY>
__global__ __launch_bounds__(256) void k1_rescan(SelArgs a) {
    const int lane = threadIdx.x & 63;
    const int nwaves = gridDim.x * 4, total = *a.scancnt;
    for (int e = blockIdx.x * 4 + (threadIdx.x >> 6); e < total; e += nwaves) {
        const int row = a.scanlist[e], n = row / a.L, i = row % a.L;
        const unsigned long long k = a.rowbest[row];
        const unsigned bits = (unsigned)(k >> 32);
        const int j = (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull));
        const unsigned* cm = a.colmax + (size_t)n * a.S;
        int sel = -1;
        for (int j0 = ((j + 1) / 64) * 64; j0 < a.S && sel < 0; j0 += 64) {
            const int j2 = j0 + lane;
            if constexpr (!MATCH_ONLY) {
                const float* crow = a.conf + (size_t)row * a.S;
                const bool hit = j2 > j && j2 < a.S && cm[j2] == bits && __float_as_uint(crow[j2]) == bits;
                const unsigned long long bal = __ballot(hit);
                if (bal) sel = j0 + __ffsll((long long)bal) - 1;
            } else {
                // candidates by the column maxima alone, then (in column order) the entry itself, recomputed
                unsigned long long bal = __ballot(j2 > j && j2 < a.S && cm[j2] == bits);
                while (bal && sel < 0) {
                    const int jc = j0 + __ffsll((long long)bal) - 1;
                    bal &= bal - 1;
                    if (__float_as_uint(k1_conf_entry<H>(a, n, i, jc)) == bits) sel = jc;
                }
            }
        }
        if (lane == 0 && sel >= 0) {
            a.selj[row] = sel;
            atomicAdd(&a.samplecnt[n * a.chunks + (i >> 10)], 1);
        }
    }
}

// one workgroup per (1024-row chunk, sample): ordered compaction in (n, i) order + keypoints
// (coarse_matching.py:186-201).  Bases come from the chunk counts of everything in front.
template <typename H, bool MATCH_ONLY>
__global__ __launch_bounds__(1024) void k1_compact(SelArgs a) {
    __shared__ int wave_tot[16];
    __shared__ int sh_base, sh_forced;
    const int c = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) {
        int base = 0, forced = 0;
        for (int b = 0; b <= n; ++b) {
            int tot = 0, upto = 0;
            for (int k = 0; k < a.chunks; ++k) {
                const int v = a.samplecnt[b * a.chunks + k];
                tot += v;
                if (k < c) upto += v;
            }
            const bool f = (tot == 0 && a.force_one);
            if (b < n) base += f ? 1 : tot;
            else {
                base += upto;
                forced = f;
                if (c == 0) a.counts[1 + n] = f ? 1 : tot;
                if (c == 0 && n == a.N - 1) a.counts[0] = base + (f ? 1 : tot);
            }
        }
        sh_base = base;
        sh_forced = forced;
    }
    __syncthreads();
    const int base = sh_base;
    const float s0x = a.scale0 ? a.scale * a.scale0[2 * n] : a.scale, s0y = a.scale0 ? a.scale * a.scale0[2 * n + 1] : a.scale;
    const float s1x = a.scale1 ? a.scale * a.scale1[2 * n] : a.scale, s1y = a.scale1 ? a.scale * a.scale1[2 * n + 1] : a.scale;
    auto emit = [&](int pos, int i, int j) {
        a.b_ids[pos] = n;
        a.i_ids[pos] = i;
        a.j_ids[pos] = j;
        // match-only: a selected entry IS its row's best candidate value (k1_select / k1_rescan compared the bits)
        if constexpr (MATCH_ONLY) a.mconf[pos] = __uint_as_float((unsigned)(a.rowbest[(size_t)n * a.L + i] >> 32));
        else a.mconf[pos] = a.conf[((size_t)n * a.L + i) * a.S + j];
        a.mk0[2 * pos] = (float)(i % a.w0c) * s0x;
        a.mk0[2 * pos + 1] = (float)(i / a.w0c) * s0y;
        a.mk1[2 * pos] = (float)(j % a.w1c) * s1x;
        a.mk1[2 * pos + 1] = (float)(j / a.w1c) * s1y;
    };
    if (sh_forced) {
        if (tid == 0 && c == 0) emit(base, 0, 0);
        return;
    }
    const int i = c * 1024 + tid;
    const int j = (i < a.L) ? a.selj[(size_t)n * a.L + i] : -1;
    const bool f = j >= 0;
    const unsigned long long bal = __ballot(f);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[wave] = __popcll(bal);
    __syncthreads();
    int woff = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) woff += (w < wave) ? wave_tot[w] : 0;
    if (f) emit(base + woff + before, i, j);
}

template <typename T>
int k1_launch(K1Args a, SelArgs s, void* zero_begin, size_t zero_bytes, hipStream_t st) {
    constexpr bool EXACT = std::is_same<T, float>::value;
    const dim3 grid(a.tilesN * a.tilesM, a.N);
    (void)hipMemsetAsync(zero_begin, 0, zero_bytes, st);   // rowbest, colmax, samplecnt (contiguous)
    const bool panel = !EXACT && a.mask0 == nullptr && a.L % BM == 0 && a.S % BN == 0 && a.C == 256;
    const bool match_only = a.conf == nullptr;                 // (the entry point admits it in the panel configuration only)
    const int dtype = ElemTraits<T>::kDtype, wgs = k1_panel_wgs(a);
    // the whole call (statistics, reduction, confidence sweep, selection, compaction) against its algorithmic bytes
    void* pu = gf_prof_begin("k1_unit", st, (double)a.N * ((double)(a.L + a.S) * a.C * sizeof(T) + (match_only ? 0.0 : (double)a.L * a.S * 4.0)));
    void* p0 = gf_prof_begin("k1_stats", st, 2.0 * a.N * (double)a.L * a.S * a.C);
    k1_stats_launch(a, dtype, panel, st);
    gf_prof_end("k1_stats", p0, st);
    k1_reduce_launch(a, dtype, st);
    void* p1 = gf_prof_begin(match_only ? "k1_conf_matchonly" : "k1_conf", st,
                             (double)a.N * ((double)(a.L + a.S) * a.C * sizeof(T) + (match_only ? 0.0 : (double)a.L * a.S * 4.0)));
    bool done = false;
    if constexpr (!EXACT) {
        if (panel) {
            static std::atomic<uint64_t> attr{0};
            if (gf_first_use_on_device(attr)) {
                (void)hipFuncSetAttribute((const void*)k1_conf_pipe<T, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, PIPE_LDS);
                (void)hipFuncSetAttribute((const void*)k1_conf_pipe<T, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, PIPE_LDS);
                (void)hipFuncSetAttribute((const void*)k1_conf_pipe<T, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, PIPE_LDS);
                (void)hipFuncSetAttribute((const void*)k1_conf_pipe<T, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, PIPE_LDS);
            }
            if (match_only) {
                if (a.dense) k1_conf_pipe<T, true, false><<<wgs, NT, PIPE_LDS, st>>>(a);
                else k1_conf_pipe<T, false, false><<<wgs, NT, PIPE_LDS, st>>>(a);
            } else if (a.dense) k1_conf_pipe<T, true, true><<<wgs, NT, PIPE_LDS, st>>>(a);
            else k1_conf_pipe<T, false, true><<<wgs, NT, PIPE_LDS, st>>>(a);
            done = true;
        }
    }
    if (done) {
    } else if (a.dense) k1_conf<T, true><<<grid, NT, STAGE_BYTES, st>>>(a);
    else k1_conf<T, false><<<grid, NT, STAGE_BYTES, st>>>(a);
    gf_prof_end(match_only ? "k1_conf_matchonly" : "k1_conf", p1, st);
    k1_colset<<<dim3((a.S + 255) / 256, a.N), 256, 0, st>>>(s);
    k1_select<<<dim3((a.L + 255) / 256, a.N), 256, 0, st>>>(s);
    if constexpr (!EXACT) {
        if (match_only) {
            k1_rescan<T, true><<<256, 256, 0, st>>>(s);
            k1_compact<T, true><<<dim3(s.chunks, a.N), 1024, 0, st>>>(s);
        } else {
            k1_rescan<T, false><<<256, 256, 0, st>>>(s);
            k1_compact<T, false><<<dim3(s.chunks, a.N), 1024, 0, st>>>(s);
        }
    } else {
        k1_rescan<_Float16, false><<<256, 256, 0, st>>>(s);
        k1_compact<_Float16, false><<<dim3(s.chunks, a.N), 1024, 0, st>>>(s);
    }
    gf_prof_end("k1_unit", pu, st);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

struct K1Workspace {
    float2 *rowpart, *colpart, *rstat, *cstat;
    unsigned long long* rowbest;
    unsigned *colmax, *colset;
    int *samplecnt, *scancnt, *selj, *scanlist;
    unsigned long long* stamp;
    size_t zero_bytes, bytes;
};

K1Workspace k1_carve(void* ws, int N, int L, int S) {
    const int tilesM = (L + BM - 1) / BM, tilesN = (S + BN - 1) / BN;
    GfCarver c(ws);
    K1Workspace w;
    // zeroed every call (one memset): rowbest | colmax | colset | samplecnt | scancnt
    w.rowbest = c.take<unsigned long long>((size_t)N * L);
    w.colmax = c.take<unsigned>((size_t)N * S);
    w.colset = c.take<unsigned>((size_t)N * (1 << 15));
    w.samplecnt = c.take<int>((size_t)N * ((L + 1023) / 1024));
    w.scancnt = c.take<int>(1);
    w.zero_bytes = c.used();
    w.rowpart = c.take<float2>((size_t)N * tilesN * L);
    w.colpart = c.take<float2>((size_t)N * tilesM * S);
    w.rstat = c.take<float2>((size_t)N * L);
    w.cstat = c.take<float2>((size_t)N * S);
    w.selj = c.take<int>((size_t)N * L);
    w.scanlist = c.take<int>((size_t)N * L);
    w.stamp = c.take<unsigned long long>(K1_STAMP_WORDS + 1);
    w.bytes = c.used();
    return w;
}

}   // namespace

void k1_stats_launch(K1Args& a, int dtype, bool panel, hipStream_t st) {
    const dim3 grid(a.tilesN * a.tilesM, a.N);
    a.rowparts = panel ? k1_runs(a) : a.tilesN;
    if (panel) k1_stats_panel_launch(a, dtype, k1_panel_wgs(a), st);
    else if (dtype == GF_F32) k1_stats<float><<<grid, NT, STAGE_BYTES, st>>>(a);
    else if (dtype == GF_F16) k1_stats<_Float16><<<grid, NT, STAGE_BYTES, st>>>(a);
    else k1_stats<gf_bf16><<<grid, NT, STAGE_BYTES, st>>>(a);
}

void k1_reduce_launch(const K1Args& a, int dtype, hipStream_t st) {
    const int mx = a.L > a.S ? a.L : a.S;
    const dim3 grid((mx + 31) / 32, 2, a.N);
    if (dtype == GF_F32) k1_reduce_stats<true><<<grid, 256, 0, st>>>(a);
    else k1_reduce_stats<false><<<grid, 256, 0, st>>>(a);
}

extern "C" size_t gf_dual_softmax_workspace_bytes(int N, int L, int S) {
    if (N <= 0 || L <= 0 || S <= 0) return 0;
    return k1_carve(nullptr, N, L, S).bytes;
}

// match-only mode is built for the configuration the inference path runs (the row-panel form of the sweep)
extern "C" int gf_dual_softmax_match_only_supported(int dtype, int L, int S, int C, int masked, int force_one) {
    return (dtype == GF_F16 || dtype == GF_BF16) && C == 256 && L > 0 && S > 0 && L % BM == 0 && S % BN == 0 && !masked && !force_one;
}

// conf[b[e]][i[e]][j[e]] for e < P, recomputed bit-identically to what gf_dual_softmax_match wrote (or, in match-only mode, would
// have written) from the SAME features and the row / column statistics its last call left in `workspace`
extern "C" int gf_dual_softmax_conf_at(const void* f0, const void* f1, int dtype, int N, int L, int S, int C, float temperature,
                                       const int64_t* b, const int64_t* i, const int64_t* j, int P, float* out, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    GF_CHECK_ARG(f0 && f1 && b && i && j && out, "null pointer");
    GF_CHECK_ARG(gf_dual_softmax_match_only_supported(dtype, L, S, C, 0, 0) && N > 0 && P >= 0 && temperature > 0.f,
                 "built for 16-bit features, C = 256, L % 128 == 0, S % 64 == 0");
    if (workspace == nullptr || workspace_bytes < gf_dual_softmax_workspace_bytes(N, L, S)) {
        gf_set_error("gf_dual_softmax_conf_at: workspace too small");
        return GF_ERR_WORKSPACE;
    }
    if (P == 0) return GF_OK;
    const K1Workspace w = k1_carve(workspace, N, L, S);
    SelArgs s{};
    s.N = N; s.L = L; s.S = S; s.f0 = f0; s.f1 = f1; s.rstat = w.rstat; s.cstat = w.cstat; s.C = C; s.mult = (1.0f / (float)C) / temperature;
    s.stamp = w.stamp;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == GF_F16) k1_conf_at<_Float16><<<(P + 3) / 4, 256, 0, st>>>(s, b, i, j, P, out);
    else k1_conf_at<gf_bf16><<<(P + 3) / 4, 256, 0, st>>>(s, b, i, j, P, out);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_dual_softmax_match(const void* f0, const void* f1, int dtype, int N, int L, int S, int C,
                                     const uint8_t* mask0, const uint8_t* mask1, float temperature, float thr,
                                     int force_one, int w0c, int w1c, float scale, const float* scale0,
                                     const float* scale1, float* conf, int64_t* b_ids, int64_t* i_ids,
                                     int64_t* j_ids, float* mconf, float* mkpts0_c, float* mkpts1_c,
                                     int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    GF_CHECK_ARG(f0 && f1 && b_ids && i_ids && j_ids && mconf && mkpts0_c && mkpts1_c && counts, "null pointer");
    // conf == NULL: match-only mode (the matrix is not materialised; matches and mconf are bit-identical to the contract mode's)
    GF_CHECK_ARG(conf != nullptr || gf_dual_softmax_match_only_supported(dtype, L, S, C, mask0 != nullptr, force_one),
                 "match-only mode (conf == NULL) needs 16-bit features, C = 256, L % 128 == 0, S % 64 == 0, no masks, no forced match");
    GF_CHECK_ARG(N > 0 && L > 0 && S > 0, "empty problem");
    GF_CHECK_ARG(dtype >= GF_F32 && dtype <= GF_BF16, "bad dtype");
    GF_CHECK_ARG(C > 0 && C % (dtype == GF_F32 ? 32 : 64) == 0, "C must be a multiple of 32 (f32) / 64 (f16)");
    GF_CHECK_ARG((mask0 == nullptr) == (mask1 == nullptr), "mask0/mask1 must both be set or both be NULL");
    GF_CHECK_ARG(temperature > 0.f && w0c > 0 && w1c > 0, "bad temperature / grid width");
    GF_CHECK_ARG(thr >= 0.f, "thr must be >= 0 (confidences are probabilities)");
    if (workspace == nullptr || workspace_bytes < gf_dual_softmax_workspace_bytes(N, L, S)) {
        gf_set_error("gf_dual_softmax_match: workspace too small (%zu < %zu)", workspace_bytes,
                     gf_dual_softmax_workspace_bytes(N, L, S));
        return GF_ERR_WORKSPACE;
    }
    const K1Workspace w = k1_carve(workspace, N, L, S);
    K1Args a;
    a.f0 = f0; a.f1 = f1; a.N = N; a.L = L; a.S = S; a.C = C;
    a.mask0 = mask0; a.mask1 = mask1;
    a.inv_c = 1.0f / (float)C;                         // feat/sqrt(C) on both sides (coarse_matching.py:113)
    a.temperature = temperature;
    a.mult = (1.0f / (float)C) / temperature;
    a.tilesM = (L + BM - 1) / BM; a.tilesN = (S + BN - 1) / BN;
    a.rowpart = w.rowpart; a.colpart = w.colpart; a.rstat = w.rstat; a.cstat = w.cstat;
    a.rowbest = w.rowbest; a.colmax = w.colmax; a.conf = conf; a.thr = thr; a.dense = thr < 0.05f;
    a.stamp = w.stamp;
    a.esize = dtype == GF_F32 ? 4 : 2;
    SelArgs s;
    s.N = N; s.L = L; s.S = S;
    s.rowbest = w.rowbest; s.colmax = w.colmax; s.colset = w.colset; s.conf = conf; s.stamp = w.stamp;
    s.f0 = f0; s.f1 = f1; s.rstat = w.rstat; s.cstat = w.cstat; s.C = C; s.mult = a.mult;
    s.selj = w.selj; s.scanlist = w.scanlist; s.scancnt = w.scancnt; s.samplecnt = w.samplecnt; s.chunks = (L + 1023) / 1024; s.force_one = force_one; s.w0c = w0c; s.w1c = w1c;
    s.scale = scale; s.scale0 = scale0; s.scale1 = scale1;
    s.b_ids = b_ids; s.i_ids = i_ids; s.j_ids = j_ids; s.mconf = mconf; s.mk0 = mkpts0_c; s.mk1 = mkpts1_c;
    s.counts = counts;
    hipStream_t st = (hipStream_t)stream;
    return dtype == GF_F32 ? k1_launch<float>(a, s, w.rowbest, w.zero_bytes, st)
                           : dtype == GF_F16 ? k1_launch<_Float16>(a, s, w.rowbest, w.zero_bytes, st)
                                             : k1_launch<gf_bf16>(a, s, w.rowbest, w.zero_bytes, st);
}
