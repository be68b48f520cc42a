// Fine level (CDNA4 / gfx950).
//
//   gf_fine_gather  K7 (a13): FinePreprocess.forward's F.unfold(5x5, stride 4, pad 2) + gather by
//                   (b_ids, i_ids / j_ids) (model/loftr_src/loftr/loftr_module/fine_preprocess.py:41-56),
//                   without materialising the [N, 25*C, L] unfold: each match reads only its own 5x5
//                   window; plus the gather of the two coarse feature rows that feed down_proj (:61).
//                   The same kernels behind gf_fine_gather_ptrs (the N maps of a side in separate allocations) and
//                   gf_fine_gather_ragged (of unequal extents too): the entries differ in the map source they hand over (gf_maps.h).
//   gf_fine_match   K8 (a14/a15): FineMatching2.forward + get_fine_match (model/fine_matching2.py:21-126):
//                   25x25 dual-softmax per match, global arg-max, threshold, ordered compaction and the
//                   fine keypoint arithmetic.
#include <math.h>

#include <type_traits>

#include "gf_maps.h"

namespace {

template <typename Src>
struct FgArgs {
    Src f0, f1;              // the fine maps of the two sides (gf_maps.h), viewed as [C, H, W] per sample
    int C;
    const void* c0;          // coarse (geo) features [N, L, CC], [N, S, CC]
    const void* c1;
    int L, S, CC;
    const int64_t* b_ids;
    const int64_t* i_ids;
    const int64_t* j_ids;
    int M, w0c, w1c, stride, W;   // w0c / w1c: the width in coarse cells (ragged source: of the CANVAS)
    void* win;               // [2M][W*W][C]  (image0 windows first, then image1: torch.cat(..., 0))
    void* ccat;              // [2M][CC]
};

// one workgroup per (match, side): thread c < C copies channel c of the 25 window positions.  A tap outside the sample's OWN extent is
// zero like F.unfold's padding - also where memory continues behind the map: nothing outside [0, h) x [0, w) is loaded.
template <typename TF, typename T, typename Src>
__global__ __launch_bounds__(256) void fine_gather(FgArgs<Src> a) {
    const int m = blockIdx.x, side = blockIdx.y, t = threadIdx.x;
    const int b = (int)a.b_ids[m];
    const int cell = (int)(side ? a.j_ids[m] : a.i_ids[m]);
    const int wc = side ? a.w1c : a.w0c;
    const GfMapView<TF> f = (side ? a.f1 : a.f0).template view<TF>(b);      // b = b_ids[blockIdx.x]: uniform
    const int cy = (cell / wc) * a.stride - a.W / 2, cx = (cell % wc) * a.stride - a.W / 2;
    T* out = (T*)a.win + ((size_t)side * a.M + m) * a.W * a.W * a.C;
    if (t < a.C) {
        for (int k = 0; k < a.W * a.W; ++k) {
            const int y = cy + k / a.W, x = cx + k % a.W;
            float v = 0.f;                                        // F.unfold's padding, and the canvas beyond the sample's extent
            if (y >= 0 && y < f.h && x >= 0 && x < f.w) v = gf_to_float(f.base[t * f.sc + y * f.sh + x * f.sw]);
            out[(size_t)k * a.C + t] = gf_from_float<T>(v);
        }
    }
    const T* cf = (const T*)(side ? a.c1 : a.c0) + ((size_t)b * (side ? a.S : a.L) + cell) * a.CC;
    T* co = (T*)a.ccat + ((size_t)side * a.M + m) * a.CC;
    for (int c = t; c < a.CC; c += blockDim.x) co[c] = cf[c];
}

// One 16-byte piece of 8 elements TF -> T in registers (TF == T: the piece itself); see fine_gather_rows below.
template <typename TF, typename T>
__device__ __forceinline__ v4u fg_convert8(v4u v) {
    if constexpr (std::is_same<TF, T>::value) {
        return v;
    } else {
        const gf_vec<TF, 8> x = __builtin_bit_cast(gf_vec<TF, 8>, v);
        gf_vec<T, 8> o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = gf_from_float<T>(gf_to_float(x[k]));
        return __builtin_bit_cast(v4u, o);
    }
}

// The 16-bit inference form (channels-last 16-bit fine maps, 16-bit window tensor): ONE WAVE per (match, side) moves the
// 25 x C window as 16-byte pieces - C / 8 lanes per window position, 64 / (C / 8) positions per instruction - and the coarse
// feature row behind it; out-of-image positions are zeros (F.unfold's padding).  The general kernel above moves 2 bytes per
// lane and instruction with half its threads idle (226 us per 8-pair call at the nominal load against ~100 us of HBM time).
// TF == T: a plain copy.  TF != T (bf16 maps -> fp16 windows: the bf16-backbone / fp16-matching mode; or the reverse): the 8
// elements of a piece are converted in registers between the load and the store - widened to fp32 (exact for both types), then
// rounded ONCE to nearest even into T, the bits of torch's x.float().to(T) for every input pattern.  No clamp and no flush: a finite
// bf16 value above 65504 becomes +-inf in fp16, one below fp16's subnormal spacing rounds to nearest even (to a subnormal or to
// a signed zero).  The fp16 mode has the same range through its own backbone.  Same bytes per match as the copy: 16-byte loads
// and stores either way.  The coarse row is in T already and stays a copy.
// Whether a map can be read in pieces (channels-last, row and pixel strides multiples of 8 elements) the host has checked - except
// for the ragged source, where it is known from the sample's record only: a wave whose sample cannot takes the element loop
// instead - same values, a uniform branch.
template <typename TF, typename T, typename Src>
__global__ __launch_bounds__(256) void fine_gather_rows(FgArgs<Src> a) {
    static_assert(sizeof(TF) == 2 && sizeof(T) == 2, "16-byte pieces of 8 elements on both sides");
    // the wave's unit is the same in all 64 lanes but the compiler cannot know (it comes from threadIdx): it goes through
    // v_readfirstlane, so that side, match and sample index are scalars and the sample's view is a few scalar loads per wave in front
    // of the loop - not 64 lanes fetching one address
    const int lane = threadIdx.x & 63, u = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (u >= 2 * a.M) return;
    const int side = u >= a.M, m = side ? u - a.M : u;
    const int b = (int)a.b_ids[m];
    const int cell = (int)(side ? a.j_ids[m] : a.i_ids[m]);
    const int wc = side ? a.w1c : a.w0c;
    const GfMapView<TF> f = (side ? a.f1 : a.f0).template view<TF>(b);
    const int cy = (cell / wc) * a.stride - a.W / 2, cx = (cell % wc) * a.stride - a.W / 2;
    T* out = (T*)a.win + (size_t)u * a.W * a.W * a.C;
    bool in_pieces = true;
    if constexpr (Src::per_sample) in_pieces = f.sc == 1 && f.sh % 8 == 0 && f.sw % 8 == 0;
    if (in_pieces) {
        const int ppp = a.C / 8, pieces = a.W * a.W * ppp;              // 16-byte pieces per position / per window
        const v4u zero{0u, 0u, 0u, 0u};
        for (int e = lane; e < pieces; e += 64) {
            const int k = e / ppp, c8 = (e - k * ppp) * 8, y = cy + k / a.W, x = cx + k % a.W;
            v4u v = zero;
            if (y >= 0 && y < f.h && x >= 0 && x < f.w) v = fg_convert8<TF, T>(*reinterpret_cast<const v4u*>(f.base + y * f.sh + x * f.sw + c8));
            *reinterpret_cast<v4u*>(out + (size_t)k * a.C + c8) = v;
        }
    } else if constexpr (Src::per_sample) {
        for (int e = lane; e < a.W * a.W * a.C; e += 64) {
            const int k = e / a.C, c = e - k * a.C, y = cy + k / a.W, x = cx + k % a.W;
            float v = 0.f;
            if (y >= 0 && y < f.h && x >= 0 && x < f.w) v = gf_to_float(f.base[c * f.sc + y * f.sh + x * f.sw]);
            out[e] = gf_from_float<T>(v);
        }
    }
    const T* cf = (const T*)(side ? a.c1 : a.c0) + ((size_t)b * (side ? a.S : a.L) + cell) * a.CC;
    T* co = (T*)a.ccat + (size_t)u * a.CC;
    for (int c8 = lane * 8; c8 < a.CC; c8 += 512) *reinterpret_cast<v4u*>(co + c8) = *reinterpret_cast<const v4u*>(cf + c8);
}

// The 16-bit entry without the copy (maps already of the compute type, channels-last): the window rows are NAMED, not moved.  One wave per
// (match, side) writes the addresses of its W x W taps' channel rows - 0 where fine_gather_rows writes zeros: a tap outside the sample's own
// extent - and of its coarse feature row; gf_linear_rows (k3_linear.hip) then reads the rows where they lie.  Element size 2 for every type.
template <typename Src>
struct FrArgs {
    Src f0, f1;
    const void* c0;          // coarse (geo) features [N, L, CC], [N, S, CC]
    const void* c1;
    int L, S, CC;
    const int64_t* b_ids;
    const int64_t* i_ids;
    const int64_t* j_ids;
    int M, w0c, w1c, stride, W;
    unsigned long long* win_rows;   // [2M][W*W]  (image0 windows first, then image1)
    unsigned long long* c_rows;     // [2M]
};

template <typename Src>
__global__ __launch_bounds__(256) void fine_row_table(FrArgs<Src> a) {
    using E = unsigned short;
    const int lane = threadIdx.x & 63, u = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (u >= 2 * a.M) return;
    const int side = u >= a.M, m = side ? u - a.M : u;
    const int b = (int)a.b_ids[m];
    const int cell = (int)(side ? a.j_ids[m] : a.i_ids[m]);
    const int wc = side ? a.w1c : a.w0c;
    const GfMapView<E> f = (side ? a.f1 : a.f0).template view<E>(b);
    const int cy = (cell / wc) * a.stride - a.W / 2, cx = (cell % wc) * a.stride - a.W / 2;
    for (int k = lane; k < a.W * a.W; k += 64) {
        const int y = cy + k / a.W, x = cx + k % a.W;
        unsigned long long p = 0ull;
        if (y >= 0 && y < f.h && x >= 0 && x < f.w) p = (unsigned long long)(uintptr_t)(f.base + y * f.sh + x * f.sw);
        a.win_rows[(size_t)u * a.W * a.W + k] = p;
    }
    if (lane == 0) a.c_rows[u] = (unsigned long long)(uintptr_t)((const E*)(side ? a.c1 : a.c0) + ((size_t)b * (side ? a.S : a.L) + cell) * a.CC);
}

template <typename Src>
int fr_launch(const FrArgs<Src>& a, void* stream) {
    fine_row_table<Src><<<(2 * a.M + 3) / 4, 256, 0, (hipStream_t)stream>>>(a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

// ------------------------------------------------------------------------------------------------
struct FmArgs {
    const void* f0;          // [M][WW][C]
    const void* f1;
    int M, C;
    float temperature, thr;
    const int64_t* b_ids;    // coarse match -> sample
    const float* mk0c;       // [M][2]
    const float* mk1c;
    float coarse_scale, c2f, fine_scale;   // hw0_i/hw0_c, hw0_f/hw0_c, hw0_i/hw0_f
    const float* scale0;     // [N][2] or null
    const float* scale1;
    float* fine_matrix;      // [M][WW][WW]
    int32_t* sel;            // [M] flat arg-max index i*WW+j, or -1 when below thr
    int32_t* chunk_cnt;      // [chunks]
    int chunks;
    float* mk0f;             // [M][2] compacted
    float* mk1f;
    float* mconf;
    int64_t* m_bids;
    int32_t* count;          // [1]
};

constexpr int WW = 25;

template <typename T>
__global__ __launch_bounds__(256) void fine_match(FmArgs a) {
    __shared__ float s0[WW][129], s1[WW][129];
    __shared__ float sim[WW][WW + 1];
    __shared__ float rmax[WW], rsum[WW], cmax[WW], csum[WW];
    __shared__ unsigned long long best[256];
    const int m = blockIdx.x, t = threadIdx.x, C = a.C;
    const float rs = sqrtf((float)C);
    const T* p0 = (const T*)a.f0 + (size_t)m * WW * C;
    const T* p1 = (const T*)a.f1 + (size_t)m * WW * C;
    for (int i = t; i < WW * C; i += 256) {
        s0[i / C][i % C] = gf_to_float(p0[i]) / rs;      // feat / C**.5 on both sides (fine_matching2.py:52)
        s1[i / C][i % C] = gf_to_float(p1[i]) / rs;
    }
    __syncthreads();
    for (int o = t; o < WW * WW; o += 256) {
        const int i = o / WW, j = o % WW;
        float acc = 0.f;
        for (int c = 0; c < C; ++c) acc += s0[i][c] * s1[j][c];
        sim[i][j] = acc / a.temperature;
    }
    __syncthreads();
    if (t < WW) {                       // softmax over dim 2 (row statistics)
        float mx = -INFINITY;
        for (int j = 0; j < WW; ++j) mx = fmaxf(mx, sim[t][j]);
        float s = 0.f;
        for (int j = 0; j < WW; ++j) s += expf(sim[t][j] - mx);
        rmax[t] = mx; rsum[t] = s;
    } else if (t >= 64 && t < 64 + WW) {   // softmax over dim 1 (column statistics)
        const int j = t - 64;
        float mx = -INFINITY;
        for (int i = 0; i < WW; ++i) mx = fmaxf(mx, sim[i][j]);
        float s = 0.f;
        for (int i = 0; i < WW; ++i) s += expf(sim[i][j] - mx);
        cmax[j] = mx; csum[j] = s;
    }
    __syncthreads();
    unsigned long long key = 0ull;
    for (int o = t; o < WW * WW; o += 256) {
        const int i = o / WW, j = o % WW;
        const float s = sim[i][j];
        const float cf = (expf(s - cmax[j]) / csum[j]) * (expf(s - rmax[i]) / rsum[i]);
        a.fine_matrix[(size_t)m * WW * WW + o] = cf;
        const unsigned long long k = ((unsigned long long)__float_as_uint(cf) << 32) | (0xFFFFFFFFu - (unsigned)o);
        key = k > key ? k : key;        // arg-max with first-index tie-break (fine_matching2.py:79)
    }
    best[t] = key;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (t < s) best[t] = best[t] > best[t + s] ? best[t] : best[t + s];
        __syncthreads();
    }
    if (t == 0) {
        const float v = __uint_as_float((unsigned)(best[0] >> 32));
        const int o = (int)(0xFFFFFFFFu - (unsigned)(best[0] & 0xFFFFFFFFull));
        // the one-hot arg-max is automatically its row's and column's maximum, so the mask of
        // fine_matching2.py:73-82 reduces to the threshold test
        const bool ok = v > a.thr;
        a.sel[m] = ok ? o : -1;
    }
}

// 16-bit storage modes: ONE WAVE per match, the 25 x 25 x C correlation on the matrix cores (32 x 32 tile, rows / columns
// 25..31 re-read window position 24 and are masked out of the statistics), operands straight from global memory (a lane's
// 16 bytes of its window row per k-step).  The tile is computed TWICE, as f0.f1^T and as f1.f0^T (C / 16 MFMAs each, the same
// bits: a product's two factors commute and the k order is the same): a softmax statistic over a tile's ROW index is a
// reduction over the registers of one lane (+ one exchange between the lane halves), so the column statistics come from the
// first tile and the row statistics from the second - no 32-lane butterflies (those were 160 cross-lane operations per
// match); the row statistics reach the first tile's layout by v_readlane.  Hardware exp2 (the arguments are <= 0) and
// reciprocals of the two sums instead of libm's expf and 1250 divisions.  Same arithmetic as fine_match above up to fp32
// rounding (the dot products sum in the matrix cores' order and are scaled once by 1 / (C * temperature) instead of dividing every
// operand by sqrt(C)): 249 us -> HBM time per 8-pair call at the nominal load.
template <typename T>
__global__ __launch_bounds__(256) void fine_match_mfma(FmArgs a) {
    // No contraction in this kernel: the maxima below are taken over the ROUNDED products acc * scale2, and with contraction the compiler
    // forms the exponents as fma(acc, scale2, -max) from the unrounded ones - at the maximum itself that is the product's rounding residual
    // instead of 0, up to half an ulp of the logit (3e-5 at 500 log2 units): probabilities above 1 (confidences up to 1.00002 were seen in
    // saturated windows) and saturated cells that are no longer equal, so that the first-index rule picked by residual.
#pragma clang fp contract(off)
    using Mm = Mma32<T>;
    using Frag = typename Mm::Frag;
    const int lane = threadIdx.x & 63, h = lane >> 5, lr = lane & 31, m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= a.M) return;
    const int C = a.C, row = lr < WW ? lr : WW - 1;
    const T* p0 = (const T*)a.f0 + ((size_t)m * WW + row) * C + h * 8;
    const T* p1 = (const T*)a.f1 + ((size_t)m * WW + row) * C + h * 8;
    v16f acc, acct;                     // acc[r]: row i = (r & 3) + 8 (r >> 2) + 4 h of column j = lr;  acct: the transpose
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[r] = 0.f; acct[r] = 0.f; }
    for (int ks = 0; ks < C / 16; ++ks) {
        const Frag x0 = *reinterpret_cast<const Frag*>(p0 + ks * 16), x1 = *reinterpret_cast<const Frag*>(p1 + ks * 16);
        Mm::mma(x0, x1, acc);
        Mm::mma(x1, x0, acct);
    }
    const float scale2 = 1.4426950408889634f / ((float)C * a.temperature);     // logits in log2 units
    const bool lok = lr < WW;           // this lane's column (first tile) / row (second tile) exists
    // statistics over the register index: first tile -> column lr, second tile -> row lr
    float cmx = -INFINITY, rmx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const bool ok = gf_acc_row(r, h) < WW;
        acc[r] *= scale2;
        acct[r] *= scale2;
        cmx = fmaxf(cmx, ok ? acc[r] : -INFINITY);
        rmx = fmaxf(rmx, ok ? acct[r] : -INFINITY);
    }
    cmx = fmaxf(cmx, __shfl_xor(cmx, 32, 64));
    rmx = fmaxf(rmx, __shfl_xor(rmx, 32, 64));
    float csm = 0.f, rsm = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const bool ok = gf_acc_row(r, h) < WW;
        csm += ok ? __builtin_amdgcn_exp2f(acc[r] - cmx) : 0.f;
        rsm += ok ? __builtin_amdgcn_exp2f(acct[r] - rmx) : 0.f;
    }
    csm += __shfl_xor(csm, 32, 64);
    rsm += __shfl_xor(rsm, 32, 64);
    const float icsm = 1.0f / csm, irsm = 1.0f / rsm;
    unsigned long long key = 0ull;
    float* fm = a.fine_matrix + (size_t)m * WW * WW;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        // row i of this register differs between the lane halves: both candidates by v_readlane (wave-uniform lane index)
        const int i0 = gf_acc_row(r, 0), i1 = gf_acc_row(r, 1), i = h ? i1 : i0;
        const int m0 = __builtin_amdgcn_readlane(__float_as_int(rmx), i0), m1 = __builtin_amdgcn_readlane(__float_as_int(rmx), i1);
        const int q0 = __builtin_amdgcn_readlane(__float_as_int(irsm), i0), q1 = __builtin_amdgcn_readlane(__float_as_int(irsm), i1);
        const float rm = __int_as_float(h ? m1 : m0), rq = __int_as_float(h ? q1 : q0);
        if (i < WW && lok) {
            const float cf = (__builtin_amdgcn_exp2f(acc[r] - cmx) * icsm) * (__builtin_amdgcn_exp2f(acc[r] - rm) * rq);
            const int o = i * WW + lr;
            fm[o] = cf;
            const unsigned long long k = ((unsigned long long)__float_as_uint(cf) << 32) | (0xFFFFFFFFu - (unsigned)o);
            key = k > key ? k : key;            // arg-max with first-index tie-break (fine_matching2.py:79)
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)key, d, 64), hi = __shfl_xor((unsigned)(key >> 32), d, 64);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        key = other > key ? other : key;
    }
    if (lane == 0) {
        const float v = __uint_as_float((unsigned)(key >> 32));
        const int o = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
        const bool ok = v > a.thr;
        a.sel[m] = ok ? o : -1;
    }
}

// matches that passed the threshold, per 1024-match chunk (one ballot per wave; the per-match atomicAdd this replaces put ~1000
// same-address atomics on each of ~18 counters: 140 of fine_match's 214 us at the nominal load)
__global__ __launch_bounds__(1024) void fine_count(FmArgs a) {
    __shared__ int wave_tot[16];
    const int c = blockIdx.x, tid = threadIdx.x, m = c * 1024 + tid;
    const unsigned long long bal = __ballot(m < a.M && a.sel[m] >= 0);
    if ((tid & 63) == 0) wave_tot[tid >> 6] = __popcll(bal);
    __syncthreads();
    if (tid == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) t += wave_tot[w];
        a.chunk_cnt[c] = t;
    }
}

__global__ __launch_bounds__(1024) void fine_compact(FmArgs a) {
    __shared__ int wave_tot[16];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0, total = 0;
    for (int k = 0; k < a.chunks; ++k) {
        const int v = a.chunk_cnt[k];
        if (k < c) base += v;
        total += v;
    }
    if (c == 0 && tid == 0) a.count[0] = total;
    const int m = c * 1024 + tid;
    const int o = m < a.M ? a.sel[m] : -1;
    const bool f = o >= 0;
    const unsigned long long bal = __ballot(f);
    if (lane == 0) wave_tot[wave] = __popcll(bal);
    __syncthreads();
    int woff = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) woff += (w < wave) ? wave_tot[w] : 0;
    if (!f) return;
    const int pos = base + woff + __popcll(bal & ((1ull << lane) - 1ull));
    const int i = o / WW, j = o % WW, b = (int)a.b_ids[m];
    const int W = 5;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const float cs0 = a.scale0 ? a.coarse_scale * a.scale0[2 * b + d] : a.coarse_scale;
        const float cs1 = a.scale1 ? a.coarse_scale * a.scale1[2 * b + d] : a.coarse_scale;
        const float fs0 = a.scale0 ? a.fine_scale * a.scale0[2 * b + d] : a.fine_scale;
        const float fs1 = a.scale1 ? a.fine_scale * a.scale1[2 * b + d] : a.fine_scale;
        const float c0 = a.mk0c[2 * m + d] / cs0 * a.c2f;             // fine_matching2.py:101-102
        const float c1 = a.mk1c[2 * m + d] / cs1 * a.c2f;
        const int oi = d == 0 ? (i % W - W / 2) : (i / W - W / 2);
        const int oj = d == 0 ? (j % W - W / 2) : (j / W - W / 2);
        a.mk0f[2 * pos + d] = ((float)oi + c0) * fs0;                 // :104-116
        a.mk1f[2 * pos + d] = ((float)oj + c1) * fs1;
    }
    a.mconf[pos] = a.fine_matrix[(size_t)m * WW * WW + o];
    a.m_bids[pos] = b;
}

// feat_align (table sources): the largest power of two, in bytes, that divides EVERY entry of both tables - the caller built them and knows
template <typename TF, typename T, typename Src>
int fg_launch(const FgArgs<Src>& a, hipStream_t st, unsigned feat_align) {
    if constexpr (sizeof(TF) == 2 && sizeof(T) == 2) {
        bool rows16 = a.C % 8 == 0 && a.CC % 8 == 0 && a.f0.bases_aligned(16, 2, feat_align) && a.f1.bases_aligned(16, 2, feat_align) &&
                      (uintptr_t)a.c0 % 16 == 0 && (uintptr_t)a.c1 % 16 == 0 && (uintptr_t)a.win % 16 == 0 && (uintptr_t)a.ccat % 16 == 0;
        if constexpr (!Src::per_sample)          // per-sample strides: each wave looks at its own record
            rows16 = rows16 && a.f0.sc == 1 && a.f1.sc == 1 && a.f0.sh % 8 == 0 && a.f0.sw % 8 == 0 && a.f1.sh % 8 == 0 && a.f1.sw % 8 == 0;
        if (rows16) {
            fine_gather_rows<TF, T, Src><<<(2 * a.M + 3) / 4, 256, 0, st>>>(a);
            GF_CHECK_LAUNCH();
            return GF_OK;
        }
    }
    fine_gather<TF, T, Src><<<dim3(a.M, 2), 256, 0, st>>>(a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

template <typename TF, typename Src>
int fg_launch_to(int dtype, const FgArgs<Src>& a, hipStream_t st, unsigned feat_align) {
    return dtype == GF_F32 ? fg_launch<TF, float>(a, st, feat_align)
                           : dtype == GF_F16 ? fg_launch<TF, _Float16>(a, st, feat_align) : fg_launch<TF, gf_bf16>(a, st, feat_align);
}

template <typename Src>
int fg_dispatch(int feat_dtype, int dtype, const FgArgs<Src>& a, void* stream, int feat_align) {
    hipStream_t st = (hipStream_t)stream;
    if (feat_dtype == GF_F32) return fg_launch_to<float>(dtype, a, st, (unsigned)feat_align);
    if (feat_dtype == GF_F16) return fg_launch_to<_Float16>(dtype, a, st, (unsigned)feat_align);
    return fg_launch_to<gf_bf16>(dtype, a, st, (unsigned)feat_align);
}

}   // namespace

// The checks of the three gf_fine_gather entries, in one order; a macro, so that GF_CHECK_ARG's message names the entry that was called.
// maps_ok: the entry's own map arguments are non-null;  n_ok / n_max_ok / feat_align: the table entries' (true / true / 1 otherwise).
#define FG_CHECK_ARGS(maps_ok, n_ok, n_max_ok, feat_align)                                                                                 \
    GF_CHECK_ARG((maps_ok) && feat_c0 && feat_c1 && b_ids && i_ids && j_ids && win_out && ccat_out, "null pointer");                       \
    GF_CHECK_ARG(n_ok, "empty table");                                                                                                     \
    GF_CHECK_ARG(n_max_ok, "at most 65535 table entries");                                                                                 \
    GF_CHECK_ARG(M > 0, "M must be > 0 (the M == 0 early return of fine_preprocess.py:35-38 is the caller's)");                            \
    GF_CHECK_ARG(C > 0 && C <= 256 && window > 0 && stride > 0 && w0c > 0 && w1c > 0, "bad sizes");                                        \
    GF_CHECK_ARG((feat_align) > 0 && ((feat_align) & ((feat_align) - 1)) == 0, "feat_align must be a power of two");                       \
    GF_CHECK_ARG(feat_dtype >= GF_F32 && feat_dtype <= GF_BF16 && dtype >= GF_F32 && dtype <= GF_BF16, "bad dtype")
// the arguments behind the two map sources, under the names all three entries give them
#define FG_COMMON_ARGS C, feat_c0, feat_c1, L, S, CC, b_ids, i_ids, j_ids, M, w0c, w1c, stride, window, win_out, ccat_out

extern "C" int gf_fine_gather(const void* feat_f0, const void* feat_f1, int feat_dtype, const long* strides0,
                              const long* strides1, int H0, int W0, int H1, int W1, int C, const void* feat_c0,
                              const void* feat_c1, int dtype, int L, int S, int CC, const int64_t* b_ids,
                              const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c, int stride,
                              int window, void* win_out, void* ccat_out, void* stream) {
    FG_CHECK_ARGS(feat_f0 && feat_f1 && strides0 && strides1, true, true, 1);
    FgArgs<GfTensorMaps> a{{feat_f0, strides0[0], strides0[1], strides0[2], strides0[3], H0, W0},
                           {feat_f1, strides1[0], strides1[1], strides1[2], strides1[3], H1, W1}, FG_COMMON_ARGS};
    return fg_dispatch(feat_dtype, dtype, a, stream, 0);
}

extern "C" int gf_fine_gather_ptrs(const void* const* f0_table, const void* const* f1_table, int N, int feat_dtype, int feat_align,
                                   const long* strides0, const long* strides1, int H0, int W0, int H1, int W1, int C,
                                   const void* feat_c0, const void* feat_c1, int dtype, int L, int S, int CC, const int64_t* b_ids,
                                   const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c, int stride, int window,
                                   void* win_out, void* ccat_out, void* stream) {
    FG_CHECK_ARGS(f0_table && f1_table && strides0 && strides1, N > 0, true, feat_align);
    FgArgs<GfTableMaps> a{{f0_table, strides0[0], strides0[1], strides0[2], H0, W0},
                          {f1_table, strides1[0], strides1[1], strides1[2], H1, W1}, FG_COMMON_ARGS};
    return fg_dispatch(feat_dtype, dtype, a, stream, feat_align);
}

extern "C" int gf_fine_gather_ragged(const gf_map_record* f0_table, const gf_map_record* f1_table, int N, int feat_dtype, int feat_align, int C,
                                     const void* feat_c0, const void* feat_c1, int dtype, int L, int S, int CC, const int64_t* b_ids,
                                     const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c, int stride, int window,
                                     void* win_out, void* ccat_out, void* stream) {
    FG_CHECK_ARGS(f0_table && f1_table, N > 0, N <= 65535, feat_align);
    FgArgs<GfRaggedMaps> a{{f0_table}, {f1_table}, FG_COMMON_ARGS};
    return fg_dispatch(feat_dtype, dtype, a, stream, feat_align);
}

// The three gf_fine_rows entries: the checks in one order, as above.  rows_ok: what the entry knows about its maps' channel rows (contiguous,
// 16-byte aligned); a ragged table's records are the caller's promise.
#define FR_CHECK_ARGS(maps_ok, n_ok, rows_ok)                                                                                              \
    GF_CHECK_ARG((maps_ok) && feat_c0 && feat_c1 && b_ids && i_ids && j_ids && win_rows && coarse_rows, "null pointer");                   \
    GF_CHECK_ARG(n_ok, "empty table");                                                                                                     \
    GF_CHECK_ARG(M > 0 && (long)M * window * window < (1l << 30), "M must be > 0 and 2 M window^2 < 2^31");                                \
    GF_CHECK_ARG(window > 0 && stride > 0 && w0c > 0 && w1c > 0 && CC > 0, "bad sizes");                                                   \
    GF_CHECK_ARG(rows_ok, "channel rows must be contiguous and 16-byte aligned (channels-last maps, strides multiples of 8 elements)");    \
    GF_CHECK_ARG((uintptr_t)feat_c0 % 16 == 0 && (uintptr_t)feat_c1 % 16 == 0 && CC % 8 == 0, "coarse rows must be 16-byte aligned")
#define FR_COMMON_ARGS feat_c0, feat_c1, L, S, CC, b_ids, i_ids, j_ids, M, w0c, w1c, stride, window, (unsigned long long*)win_rows, (unsigned long long*)coarse_rows
#define FR_STRIDES_OK(s) ((s)[0] == 1 && (s)[1] % 8 == 0 && (s)[2] % 8 == 0)

extern "C" int gf_fine_rows(const void* feat_f0, const void* feat_f1, const long* strides0, const long* strides1, int H0, int W0, int H1,
                            int W1, const void* feat_c0, const void* feat_c1, int L, int S, int CC, const int64_t* b_ids,
                            const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c, int stride, int window,
                            uint64_t* win_rows, uint64_t* coarse_rows, void* stream) {
    FR_CHECK_ARGS(feat_f0 && feat_f1 && strides0 && strides1, true,
                  strides0[0] % 8 == 0 && strides1[0] % 8 == 0 && FR_STRIDES_OK(strides0 + 1) &&
                      FR_STRIDES_OK(strides1 + 1) && (uintptr_t)feat_f0 % 16 == 0 && (uintptr_t)feat_f1 % 16 == 0);
    FrArgs<GfTensorMaps> a{{feat_f0, strides0[0], strides0[1], strides0[2], strides0[3], H0, W0},
                           {feat_f1, strides1[0], strides1[1], strides1[2], strides1[3], H1, W1}, FR_COMMON_ARGS};
    return fr_launch(a, stream);
}

extern "C" int gf_fine_rows_ptrs(const void* const* f0_table, const void* const* f1_table, int N, int feat_align, const long* strides0,
                                 const long* strides1, int H0, int W0, int H1, int W1, const void* feat_c0, const void* feat_c1, int L,
                                 int S, int CC, const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c,
                                 int stride, int window, uint64_t* win_rows, uint64_t* coarse_rows, void* stream) {
    FR_CHECK_ARGS(f0_table && f1_table && strides0 && strides1, N > 0,
                  FR_STRIDES_OK(strides0) && FR_STRIDES_OK(strides1) && feat_align > 0 && feat_align % 16 == 0);
    FrArgs<GfTableMaps> a{{f0_table, strides0[0], strides0[1], strides0[2], H0, W0},
                          {f1_table, strides1[0], strides1[1], strides1[2], H1, W1}, FR_COMMON_ARGS};
    return fr_launch(a, stream);
}

extern "C" int gf_fine_rows_ragged(const gf_map_record* f0_table, const gf_map_record* f1_table, int N, int feat_align, const void* feat_c0,
                                   const void* feat_c1, int L, int S, int CC, const int64_t* b_ids, const int64_t* i_ids,
                                   const int64_t* j_ids, int M, int w0c, int w1c, int stride, int window, uint64_t* win_rows,
                                   uint64_t* coarse_rows, void* stream) {
    FR_CHECK_ARGS(f0_table && f1_table, N > 0, feat_align > 0 && feat_align % 16 == 0);
    FrArgs<GfRaggedMaps> a{{f0_table}, {f1_table}, FR_COMMON_ARGS};
    return fr_launch(a, stream);
}

extern "C" size_t gf_fine_match_workspace_bytes(int M) {
    if (M <= 0) return 0;
    return gf_align_up((size_t)((M + 1023) / 1024) * sizeof(int32_t), 256) + gf_align_up((size_t)M * sizeof(int32_t), 256);
}

extern "C" int gf_fine_match(const void* f0, const void* f1, int dtype, int M, int WWin, int C, float temperature,
                             float thr, const int64_t* b_ids, const float* mkpts0_c, const float* mkpts1_c,
                             float coarse_scale, float c2f_scale, float fine_scale, const float* scale0,
                             const float* scale1, float* fine_matrix, float* mkpts0_f, float* mkpts1_f, float* mconf,
                             int64_t* m_bids, int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
    GF_CHECK_ARG(f0 && f1 && b_ids && mkpts0_c && mkpts1_c && fine_matrix && mkpts0_f && mkpts1_f && mconf && m_bids && count, "null pointer");
    GF_CHECK_ARG(M > 0, "M must be > 0 (the M == 0 early return of fine_matching2.py:34-42 is the caller's)");
    GF_CHECK_ARG(WWin == WW && C > 0 && C <= 128, "built for 5x5 windows and C <= 128");
    GF_CHECK_ARG(dtype >= GF_F32 && dtype <= GF_BF16, "bad dtype");
    if (workspace == nullptr || workspace_bytes < gf_fine_match_workspace_bytes(M)) {
        gf_set_error("gf_fine_match: workspace too small");
        return GF_ERR_WORKSPACE;
    }
    FmArgs a;
    a.f0 = f0; a.f1 = f1; a.M = M; a.C = C; a.temperature = temperature; a.thr = thr; a.b_ids = b_ids;
    a.mk0c = mkpts0_c; a.mk1c = mkpts1_c; a.coarse_scale = coarse_scale; a.c2f = c2f_scale; a.fine_scale = fine_scale;
    a.scale0 = scale0; a.scale1 = scale1; a.fine_matrix = fine_matrix;
    a.chunks = (M + 1023) / 1024;
    a.chunk_cnt = (int32_t*)workspace;
    a.sel = (int32_t*)((char*)workspace + gf_align_up((size_t)a.chunks * sizeof(int32_t), 256));
    a.mk0f = mkpts0_f; a.mk1f = mkpts1_f; a.mconf = mconf; a.m_bids = m_bids; a.count = count;
    hipStream_t st = (hipStream_t)stream;
    const bool mfma = dtype != GF_F32 && C % 16 == 0 && (uintptr_t)f0 % 16 == 0 && (uintptr_t)f1 % 16 == 0;
    if (dtype == GF_F32) fine_match<float><<<M, 256, 0, st>>>(a);
    else if (dtype == GF_F16) {
        if (mfma) fine_match_mfma<_Float16><<<(M + 3) / 4, 256, 0, st>>>(a);
        else fine_match<_Float16><<<M, 256, 0, st>>>(a);
    } else {
        if (mfma) fine_match_mfma<gf_bf16><<<(M + 3) / 4, 256, 0, st>>>(a);
        else fine_match<gf_bf16><<<M, 256, 0, st>>>(a);
    }
    fine_count<<<a.chunks, 1024, 0, st>>>(a);
    fine_compact<<<a.chunks, 1024, 0, st>>>(a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
