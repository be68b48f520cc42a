// hipcc-flags: -fno-slp-vectorize
// K1 pass A, panel form: k1_stats_panel and its launcher, nothing else.  An object of its own because of the flag above: packed into
// v_pk_*_f32 pairs the kernel's tile epilogue needs 256 registers + 76 bytes of scratch (a spill reload waits for vmcnt(0), i.e. for the
// LDS-DMA in flight), unpacked 229 and none: 328 -> 285 us per 8-pair call on the same box.  k1_conf_pipe (k1_dual_softmax.hip) is 3 %
// faster WITH the packing, hence an object and not a flag for all of K1.
#include "k1_common.h"

namespace {

// -DK1_TRACE=1: clock stamps of the phases of each workgroup's SECOND unit, per wave (tools/k1_trace.py)
#ifndef K1_TRACE
#define K1_TRACE 0
#endif
#if K1_TRACE
__device__ long long k1_trace[512 * 4 * 32];
#define K1_TS(s) do { if (lane == 0 && ui == walk.slot + walk.per_xcd && (s) < 32) k1_trace[(blockIdx.x * 4 + wave) * 32 + (s)] = clock64(); } while (0)
#else
#define K1_TS(s)
#endif

// ---------------------------------------------------------------------------------------------
// pass A in the row-panel-persistent form of k1_conf_pipe: the f0 panel lives in registers, f1 tiles stream through LDS one tile
// ahead, and - the point - the ROW statistics stay in the lane that owns the row slot for the whole run of tiles
// (online max / rescaled sum per slot, 3 exponentials per slot and tile) and cross the lanes once per run instead
// of two 32-lane reduce-scatters per tile.  Column statistics are lane-local per tile as before.
// ---------------------------------------------------------------------------------------------
template <typename H>
__global__ __launch_bounds__(NT, 2) void k1_stats_panel(K1Args a) {
    using V8 = gf_vec<H, 8>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // LDS: two f1 tile buffers (LDS-DMA, one tile ahead) | column partials of two tiles [2][4 waves][64] | row maxima of the run
    float2* colx = reinterpret_cast<float2*>(smem + 2 * BN * 512);
    float* rowbc = reinterpret_cast<float*>(smem + 2 * BN * 512 + 2 * 4 * 64 * 8);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), h = lane >> 5, lr = lane & 31;   // (wave as an SGPR:
    // the DMA pieces' LDS targets go through M0 - from a VGPR they were hoisted, spilled and reloaded with a vmcnt(0) between the requests)
    K1Walk walk;
    k1_walk(a, blockIdx.x, gridDim.x, walk);
    for (int ui = walk.slot; ui < walk.ucnt; ui += walk.per_xcd) {
        K1_TS(0);
        const K1Unit u = k1_unit(a, walk, ui);
        const int n = u.n, bm = u.bm, m0 = u.m0, t0 = u.t0, t1 = u.t1;
        const H* A = (const H*)a.f0 + ((size_t)n * a.L + m0 + wave * 32 + lr) * a.C + h * 8;
        const H* B = (const H*)a.f1 + (size_t)n * a.S * a.C;
        V8 af[16];
#pragma unroll
        for (int kg = 0; kg < 16; ++kg) af[kg] = *reinterpret_cast<const V8*>(A + kg * 16);
        // tile bn -> buffer `buf` by LDS-DMA (as k1_conf_pipe: 32 pieces of 2 rows x 512 B, 8 per wave; LDS slot j of row r holds
        // chunk j ^ (r & 15)): no staging registers, no ds_write pass
        const GfRsrc brs = gf_rsrc(B, (unsigned)a.S * a.C * (unsigned)sizeof(H));
        auto dma = [&](int bn, int buf) {
            int dl = lane;
            asm volatile("" : "+v"(dl));
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int p = wave * 8 + i, row = 2 * p + (dl >> 5), j = dl & 31;
                gf_lds_dma(brs, smem + buf * (BN * 512) + p * 1024, (row * a.C + ((j ^ (row & 15)) << 3)) * (int)sizeof(H), bn * BN * a.C * (int)sizeof(H));
            }
        };
        // the column partials of tile bn - 1 (parked in LDS by the four waves) are combined behind tile bn's barrier, by wave bn % 4:
        // no barrier of their own
        auto combine = [&](int bn, int par) {
            const float2* cx = colx + par * 256;
            float m = NEG_INF;
#pragma unroll
            for (int w = 0; w < 4; ++w) m = fmaxf(m, cx[w * 64 + lane].x);
            float l = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) l += cx[w * 64 + lane].y * __expf(cx[w * 64 + lane].x - m);
            a.colpart[((size_t)n * a.tilesM + bm) * a.S + bn * BN + lane] = make_float2(m, l);
        };
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                      // the previous unit's readers of the buffers / colx / rowbc are done
        dma(t0, 0);
        // Per-element work of this pass = 1 exponential, not 2.5: everything is referred to ONE lazily updated reference per
        // row slot (a register) of this lane,
        //     e = exp2(s2 - ref[r]),  s2 = acc * mult * log2(e),
        // which feeds the row sum directly (rs[r] += e) and the column sum through a cached per-slot factor
        //     csum += e * f[r],  f[r] = exp2(ref[r] - kappa)   (kappa = the lane's largest ref: csum = sum exp2(s2 - kappa)).
        // ref[r] is a former running maximum of the slot, so the element that set it contributes 1 and whatever flushes to zero is
        // below 2^-126 of the sum; it is moved up (rs rescaled, f recomputed: 'rescale') whenever a tile's maximum exceeds the
        // smallest reference of the lane by more than 2^LAZY, which also bounds e by 2^LAZY.  The column partial is reported
        // against the column's TRUE maximum (one exponential per column and tile); a tile in which some column lies more than
        // 2^LAZY below kappa takes the two-exponential path for its column sums instead ('deep' tiles).  Maxima are taken on the
        // raw accumulators and scaled once: bit-identical to the form this replaces; the sums are exact up to fp32 rounding.
        constexpr float LAZY = 64.f;
        const float mult2 = a.mult * LOG2E;
        float rmx[16], rs[16], ref[16], fcol[16];                         // raw running maximum | sum | reference (log2) | exp2(ref - kappa)
#pragma unroll
        for (int r = 0; r < 16; ++r) { rmx[r] = NEG_INF; rs[r] = 0.f; ref[r] = NEG_INF; fcol[r] = 0.f; }
        float minref = NEG_INF, kappa = NEG_INF;
        // the tile body, instantiated for both buffer parities (the loop below walks the tiles in pairs): with the parity a compile-time
        // constant the 32 fragment reads of a tile are the same 16 lane-constant addresses + an immediate offset - as a run-time
        // term it doubled them, and the spilled ones were reloaded from scratch between the DMA requests
        auto tile = [&](auto par_c, const int bn) {
            constexpr int PAR = decltype(par_c)::value;
            const char* tb = smem + PAR * (BN * 512);
            K1_TS(1 + 6 * (bn - t0));
            // ONE barrier per tile: tile bn has landed (every wave waits for its own pieces; the only other vector-memory operations
            // in flight are 64 column-partial stores of one wave), every wave is past tile bn - 1 (its buffer and colx slot are free)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            K1_TS(2 + 6 * (bn - t0));
            if (bn + 1 < t1) dma(bn + 1, PAR ^ 1);
            if (bn > t0 && wave == ((bn - t0) & 3)) combine(bn - 1, PAR ^ 1);
            v16f acc[2];
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[ni][r] = 0.f;
            // the f1 fragments of k-group kg + 1 are requested in front of the MFMAs of kg (two waves per SIMD do not hide an LDS
            // round trip in front of every MFMA pair: left alone the compiler reads each pair right where it is used)
            V8 b0 = *reinterpret_cast<const V8*>(tb + k1p_off(lr, h)), b1 = *reinterpret_cast<const V8*>(tb + k1p_off(32 + lr, h));
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);          // issue order: reads(0) | reads(1) MFMAs(0) | reads(2) MFMAs(1) | ...
#pragma unroll
            for (int kg = 0; kg < 16; ++kg) {
                V8 n0 = b0, n1 = b1;
                if (kg < 15) {
                    n0 = *reinterpret_cast<const V8*>(tb + k1p_off(lr, 2 * kg + 2 + h));
                    n1 = *reinterpret_cast<const V8*>(tb + k1p_off(32 + lr, 2 * kg + 2 + h));
                    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                }
                Mma32<H>::mma(af[kg], b0, acc[0]);
                Mma32<H>::mma(af[kg], b1, acc[1]);
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                b0 = n0;
                b1 = n1;
            }
            K1_TS(3 + 6 * (bn - t0));
            // ---- maxima on the raw accumulators: columns over the registers, row slots over the two column halves and the tiles
            float cmr0 = NEG_INF, cmr1 = NEG_INF;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                cmr0 = fmaxf(cmr0, acc[0][r]);
                cmr1 = fmaxf(cmr1, acc[1][r]);
                rmx[r] = fmaxf(rmx[r], fmaxf(acc[0][r], acc[1][r]));
            }
            const float lanemax2 = fmaxf(cmr0, cmr1) * mult2;
            if (__any(lanemax2 - minref > LAZY)) {                       // rescale (always taken by the run's first tile)
                float mn = INFINITY, mxr = NEG_INF;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float nr = rmx[r] * mult2;
                    rs[r] *= __builtin_amdgcn_exp2f(ref[r] - nr);        // 0 * exp2(-inf) = 0 on the first tile
                    ref[r] = nr;
                    mn = fminf(mn, nr);
                    mxr = fmaxf(mxr, nr);
                }
                minref = mn;
                kappa = mxr;
#pragma unroll
                for (int r = 0; r < 16; ++r) fcol[r] = __builtin_amdgcn_exp2f(ref[r] - kappa);
            }
            K1_TS(4 + 6 * (bn - t0));
            // column maxima over the wave's 32 rows (both lane halves), in log2 units
            const float cm0 = fmaxf(cmr0, __shfl_xor(cmr0, 32, 64)), cm1 = fmaxf(cmr1, __shfl_xor(cmr1, 32, 64));
            const float c20 = cm0 * mult2, c21 = cm1 * mult2;
            float cs0 = 0.f, cs1 = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e0 = __builtin_amdgcn_exp2f(fmaf(acc[0][r], mult2, -ref[r]));
                const float e1 = __builtin_amdgcn_exp2f(fmaf(acc[1][r], mult2, -ref[r]));
                rs[r] += e0 + e1;
                cs0 = fmaf(e0, fcol[r], cs0);
                cs1 = fmaf(e1, fcol[r], cs1);
            }
            // a 'deep' tile: column sums against their own maxima.  Also taken while the lane's references span more than 126: then some
            // fcol = exp2(ref - kappa) is below the normal range, v_exp_f32 flushes it to 0, and a column maximum up to 64 above such a
            // reference (no rescale) would drop out of the cached-factor sum
            if (__any(kappa - fminf(c20, c21) > LAZY || kappa - minref > 126.f)) {
                cs0 = 0.f; cs1 = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    cs0 += __builtin_amdgcn_exp2f(fmaf(acc[0][r], mult2, -c20));
                    cs1 += __builtin_amdgcn_exp2f(fmaf(acc[1][r], mult2, -c21));
                }
            } else {
                cs0 *= __builtin_amdgcn_exp2f(kappa - c20);              // from reference kappa to the column's own maximum
                cs1 *= __builtin_amdgcn_exp2f(kappa - c21);
            }
            cs0 += __shfl_xor(cs0, 32, 64);
            cs1 += __shfl_xor(cs1, 32, 64);
            if (h == 0) {
                float2* cx = colx + PAR * 256;
                cx[wave * 64 + lr] = make_float2(cm0 * a.mult, cs0);
                cx[wave * 64 + 32 + lr] = make_float2(cm1 * a.mult, cs1);
            }
            K1_TS(5 + 6 * (bn - t0));
        };
        for (int bn = t0; bn < t1; bn += 2) {
            tile(std::integral_constant<int, 0>{}, bn);
            if (bn + 1 < t1) tile(std::integral_constant<int, 1>{}, bn + 1);
        }
        __syncthreads();                                      // the last tile's column partials are parked
        if (wave == ((t1 - t0) & 3)) combine(t1 - 1, (t1 - 1 - t0) & 1);
        // ---- end of the run: row maxima across the lanes, sums moved from the lane's reference to them, sums across the lanes
        float v[32];
#pragma unroll
        for (int q = 0; q < 16; ++q) { v[q] = rmx[q]; v[16 + q] = NEG_INF; }
        const float rmax_raw = k1_row_reduce(v, GfMaxF());
        if (lr < 16) rowbc[wave * 32 + h * 16 + lr] = rmax_raw;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            v[q] = rs[q] * __builtin_amdgcn_exp2f(ref[q] - rowbc[wave * 32 + h * 16 + q] * mult2);
            v[16 + q] = 0.f;
        }
        const float rsum = k1_row_reduce(v, GfAddF());
        if (lr < 16) a.rowpart[((size_t)n * walk.runs + u.run) * a.L + m0 + wave * 32 + gf_acc_row(lr, h)] = make_float2(rmax_raw * a.mult, rsum);
    }
}

template <typename T>
void launch(const K1Args& a, int wgs, hipStream_t st) {
    static std::atomic<uint64_t> attr{0};                       // 68.5 KiB of dynamic LDS: opt in once per device
    if (gf_first_use_on_device(attr))
        (void)hipFuncSetAttribute((const void*)k1_stats_panel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, STATS_LDS);
    k1_stats_panel<T><<<wgs, NT, STATS_LDS, st>>>(a);
}

}   // namespace

void k1_stats_panel_launch(const K1Args& a, int dtype, int wgs, hipStream_t st) {
    if (dtype == GF_F16) launch<_Float16>(a, wgs, st);
    else launch<gf_bf16>(a, wgs, st);
}

#if K1_TRACE
extern "C" int gf_debug_k1_trace(long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(k1_trace), sizeof(long long) * 512 * 4 * 32);
}
#endif
