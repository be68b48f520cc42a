// a1: position encoding add + flatten to [N, H*W, C]  (PositionEncodingSine.forward,
// model/loftr_src/loftr/utils/position_encoding.py:37-42, followed by the permute/reshape of
// model/full_model.py:69-77).  The sin/cos table is built on the host exactly as the reference builds
// its buffer (:22-35) and passed in as fp32 [H, W, C]; the kernel is a strided read + add + cast.
//
// Every input / output type pair is built, bf16 -> fp16 and fp16 -> bf16 included (the bf16-backbone / fp16-matching mode reads the
// backbone's bf16 maps and writes fp16 tokens: no cast pass over the maps in between).  The arithmetic is the same for all nine:
// input widened to fp32 (exact), + the fp32 table, ONE rounding to nearest even into the output type - the bits of torch's
// (x.float() + pe).to(out).  No clamp and no flush: a sum above 65504 becomes +-inf in fp16, one below fp16's subnormal spacing rounds
// to nearest even like every other.  The fp16 mode has the same range through its own backbone.
//
// Three entries over the same arithmetic: gf_pos_encode (one batch tensor), gf_pos_encode_ptrs (N maps of one shape in separate allocations)
// and gf_pos_encode_ragged (N maps of unequal extents on a common canvas, zeros outside each map's own extent, optional padding mask).
#include "gf_common.h"

namespace {

struct PeArgs {
    const void* x;         // TBL forms: the device table of N per-sample base addresses (const void* const*), sn unused
    long sn, sc, sh, sw;   // element strides of x viewed as [N, C, H, W]
    const float* pe;       // [H][W][C]
    void* out;             // [N][H*W][C]
    int N, C, H, W;
};

// The one difference between the batch-tensor forms (TBL = false: gf_pos_encode) and the address-table forms (TBL = true:
// gf_pos_encode_ptrs) is where sample n starts: x + n * sn, or entry n of a table in device memory.  n is uniform over the
// workgroup in every TBL form (a grid dimension), so the entry is ONE scalar 8-byte load per workgroup in front of the loop.
template <typename TI, bool TBL>
__device__ __forceinline__ const TI* pe_sample(const void* x, int n) {
    if constexpr (TBL) return (const TI*)((const void* const*)x)[n];
    else return (const TI*)x;       // + n * a.sn: added where the element offset is formed, as before the table forms existed
}

// the arithmetic of all forms: input widened to fp32 (exact), + the fp32 table entry, one rounding into TO
template <typename TO, typename TI>
__device__ __forceinline__ TO pe_add(TI x, float pe) { return gf_from_float<TO>(gf_to_float(x) + pe); }

// channels-last input (sc == 1): plain elementwise over [N*H*W, C]  (TBL: over the [H*W, C] of sample blockIdx.y)
template <typename TI, typename TO, bool TBL>
__global__ void pe_nhwc(PeArgs a) {
    const long total = (long)(TBL ? 1 : a.N) * a.H * a.W * a.C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % a.C);
        const long p = i / a.C;
        const int w = (int)(p % a.W);
        const long q = p / a.W;
        const int h = (int)(q % a.H), n = (int)(q / a.H);      // TBL: q < H, n == 0
        const float v = gf_to_float(pe_sample<TI, TBL>(a.x, blockIdx.y)[(TBL ? 0 : n * a.sn) + c * a.sc + h * a.sh + w * a.sw]);   // TBL: the entry is loop-invariant
        ((TO*)a.out)[(TBL ? blockIdx.y * total : 0) + i] = pe_add<TO>(v, a.pe[((long)h * a.W + w) * a.C + c]);
    }
}

// dense channels-last input, C % 8 == 0: 8 channels per lane, 32-bit index arithmetic
template <typename TI, typename TO, bool TBL>
__global__ __launch_bounds__(256) void pe_nhwc_vec(PeArgs a) {
    typedef TI VI __attribute__((ext_vector_type(8)));
    typedef TO VO __attribute__((ext_vector_type(8)));
    typedef float VF __attribute__((ext_vector_type(8)));
    const unsigned cv = a.C / 8, hw = (unsigned)a.H * a.W, total = (TBL ? 1u : (unsigned)a.N) * hw * cv;
    const VI* xs = reinterpret_cast<const VI*>(pe_sample<TI, TBL>(a.x, blockIdx.y));
    VO* out = reinterpret_cast<VO*>(a.out) + (TBL ? (size_t)blockIdx.y * hw * cv : 0);
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const unsigned p = i / cv, c = i - p * cv, q = p % hw;
        const VI x = xs[i];
        const VF pe = reinterpret_cast<const VF*>(a.pe)[q * cv + c];
        VO o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = pe_add<TO>(x[k], pe[k]);
        out[i] = o;
    }
}

// NCHW input (sw == 1): 32 x 32 (position x channel) tile transposed through LDS
template <typename TI, typename TO, bool TBL>
__global__ __launch_bounds__(256) void pe_nchw(PeArgs a) {
    __shared__ float tile[32][33];
    const int n = blockIdx.z, HW = a.H * a.W;
    const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const TI* xs = pe_sample<TI, TBL>(a.x, n);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = c0 + ty + 8 * k, p = p0 + tx;
        float v = 0.f;
        if (c < a.C && p < HW) {
            const int h = p / a.W, w = p % a.W;
            v = gf_to_float(xs[(TBL ? 0 : n * a.sn) + c * a.sc + h * a.sh + w * a.sw]);
        }
        tile[ty + 8 * k][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = p0 + ty + 8 * k, c = c0 + tx;
        if (c < a.C && p < HW)
            ((TO*)a.out)[((long)n * HW + p) * a.C + c] = pe_add<TO>(tile[tx][ty + 8 * k], a.pe[(long)p * a.C + c]);
    }
}

constexpr int PE_MAX_BLOCKS = 4096;

// x_align (TBL): the largest power of two, in bytes, that divides EVERY table entry - the caller built the table and knows
template <typename TI, typename TO, bool TBL>
int pe_launch(const PeArgs& a, hipStream_t st, unsigned x_align) {
    const long per = (long)a.H * a.W * a.C, elems = (long)a.N * per;
    const bool dense = a.sc == 1 && a.C % 8 == 0 && a.sw == a.C && a.sh == (long)a.W * a.C && (TBL || a.sn == per) && elems < (1l << 34);
    const bool x_ok = TBL ? x_align % 32 == 0 : (uintptr_t)a.x % 32 == 0;
    const long work = TBL ? per : elems;                        // per grid row: TBL forms put the sample on a grid dimension
    if (dense && x_ok && (uintptr_t)a.out % 32 == 0 && (uintptr_t)a.pe % 32 == 0) {
        const long nv = work / 8;
        const int blocks = (int)((nv + 255) / 256 < PE_MAX_BLOCKS ? (nv + 255) / 256 : PE_MAX_BLOCKS);
        pe_nhwc_vec<TI, TO, TBL><<<dim3(blocks, TBL ? a.N : 1), 256, 0, st>>>(a);
    } else if (a.sc == 1) {
        const int blocks = (int)((work + 255) / 256 < PE_MAX_BLOCKS ? (work + 255) / 256 : PE_MAX_BLOCKS);
        pe_nhwc<TI, TO, TBL><<<dim3(blocks, TBL ? a.N : 1), 256, 0, st>>>(a);
    } else {
        pe_nchw<TI, TO, TBL><<<dim3((a.H * a.W + 31) / 32, (a.C + 31) / 32, a.N), 256, 0, st>>>(a);
    }
    GF_CHECK_LAUNCH();
    return GF_OK;
}

template <typename TI, bool TBL>
int pe_launch_to(int out_dtype, const PeArgs& a, hipStream_t st, unsigned x_align) {
    return out_dtype == GF_F32 ? pe_launch<TI, float, TBL>(a, st, x_align)
                               : out_dtype == GF_F16 ? pe_launch<TI, _Float16, TBL>(a, st, x_align) : pe_launch<TI, gf_bf16, TBL>(a, st, x_align);
}

template <bool TBL>
int pe_dispatch(int x_dtype, int out_dtype, const PeArgs& a, hipStream_t st, unsigned x_align) {
    if (x_dtype == GF_F32) return pe_launch_to<float, TBL>(out_dtype, a, st, x_align);
    if (x_dtype == GF_F16) return pe_launch_to<_Float16, TBL>(out_dtype, a, st, x_align);
    return pe_launch_to<gf_bf16, TBL>(out_dtype, a, st, x_align);
}

// ------------------------------------------------------------------------------------------------
// Ragged form (gf_pos_encode_ragged): the N maps differ in extent and are laid at the top left of one H x W canvas; a canvas position
// outside sample n's own h x w takes the value 0 (+ the table entry): the bits of the forms above on the maps zero-padded and stacked.
// The sample is blockIdx.y, so its record (base, strides, extent: five 8-byte words) is a few scalar loads at the head, and the choice
// among the three forms - made from the record, since strides are per sample now - is a uniform branch.  Nothing outside
// [0, h) x [0, w) of a map is loaded.  The same launch writes the padding mask when asked to.
struct PeRagArgs {
    const gf_map_record* tab;   // [N], device memory
    const float* pe;            // [H][W][C]
    void* out;                  // [N][H*W][C]
    unsigned char* mask;        // null, or [N][H][W]
    int N, C, H, W;             // the canvas
};

// VEC: the host's half of the vector form's conditions holds (C % 8 == 0, every base / pe / out 32-byte aligned)
template <typename TI, typename TO, bool VEC>
__global__ __launch_bounds__(256) void pe_ragged(PeRagArgs a) {
    __shared__ float tile[32][33];
    const int n = blockIdx.y, HW = a.H * a.W, t = threadIdx.x;
    const gf_map_record r = a.tab[n];
    const TI* xs = (const TI*)r.base;
    if (a.mask)
        for (int p = blockIdx.x * 256 + t; p < HW; p += gridDim.x * 256) a.mask[(size_t)n * HW + p] = (p / a.W < r.h && p % a.W < r.w) ? 1 : 0;
    if (r.sc == 1 && VEC && r.sh % 8 == 0 && r.sw % 8 == 0) {
        // channels-last, 8 channels per lane
        typedef TI VI __attribute__((ext_vector_type(8)));
        typedef TO VO __attribute__((ext_vector_type(8)));
        typedef float VF __attribute__((ext_vector_type(8)));
        const unsigned cv = a.C / 8, total = (unsigned)HW * cv;
        VO* out = reinterpret_cast<VO*>(a.out) + (size_t)n * total;
        for (unsigned i = blockIdx.x * 256 + t; i < total; i += gridDim.x * 256) {
            const unsigned p = i / cv, c = i - p * cv;
            const int y = (int)(p / a.W), x = (int)(p % a.W);
            VI v;
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = (TI)0.f;
            if (y < r.h && x < r.w) v = *reinterpret_cast<const VI*>(xs + y * r.sh + x * r.sw + c * 8);
            const VF pe = reinterpret_cast<const VF*>(a.pe)[i];
            VO o;
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = pe_add<TO>(v[k], pe[k]);
            out[i] = o;
        }
    } else if (r.sc == 1) {
        // channels-last, one element per lane
        const long total = (long)HW * a.C;
        TO* out = (TO*)a.out + (size_t)n * total;
        for (long i = (long)blockIdx.x * 256 + t; i < total; i += (long)gridDim.x * 256) {
            const int c = (int)(i % a.C), p = (int)(i / a.C);
            const int y = p / a.W, x = p % a.W;
            float v = 0.f;
            if (y < r.h && x < r.w) v = gf_to_float(xs[c + y * r.sh + x * r.sw]);
            out[i] = pe_add<TO>(v, a.pe[i]);
        }
    } else {
        // [C, h, w] maps: 32 x 32 (position x channel) tiles of the canvas transposed through LDS
        const int tx = t & 31, ty = t >> 5;      // 32 x 8
        const int ptiles = (HW + 31) / 32, tiles = ptiles * ((a.C + 31) / 32);
        TO* out = (TO*)a.out + (size_t)n * HW * a.C;
        for (int tl = blockIdx.x; tl < tiles; tl += gridDim.x) {     // uniform trip count: the barriers below are met by all
            const int p0 = (tl % ptiles) * 32, c0 = (tl / ptiles) * 32;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c0 + ty + 8 * k, p = p0 + tx;
                float v = 0.f;
                if (c < a.C && p < HW) {
                    const int y = p / a.W, x = p % a.W;
                    if (y < r.h && x < r.w) v = gf_to_float(xs[c * r.sc + y * r.sh + x * r.sw]);
                }
                tile[ty + 8 * k][tx] = v;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int p = p0 + ty + 8 * k, c = c0 + tx;
                if (c < a.C && p < HW) out[(long)p * a.C + c] = pe_add<TO>(tile[tx][ty + 8 * k], a.pe[(long)p * a.C + c]);
            }
            __syncthreads();
        }
    }
}

template <typename TI, typename TO>
int pe_ragged_launch(const PeRagArgs& a, hipStream_t st, unsigned x_align) {
    const long per = (long)a.H * a.W * a.C;
    const bool vec = a.C % 8 == 0 && x_align % 32 == 0 && (uintptr_t)a.out % 32 == 0 && (uintptr_t)a.pe % 32 == 0 && per < (1l << 34);
    const long work = vec ? per / 8 : per;
    const int blocks = (int)((work + 255) / 256 < PE_MAX_BLOCKS ? (work + 255) / 256 : PE_MAX_BLOCKS);
    if (vec) pe_ragged<TI, TO, true><<<dim3(blocks, a.N), 256, 0, st>>>(a);
    else pe_ragged<TI, TO, false><<<dim3(blocks, a.N), 256, 0, st>>>(a);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

template <typename TI>
int pe_ragged_to(int out_dtype, const PeRagArgs& a, hipStream_t st, unsigned x_align) {
    return out_dtype == GF_F32 ? pe_ragged_launch<TI, float>(a, st, x_align)
                               : out_dtype == GF_F16 ? pe_ragged_launch<TI, _Float16>(a, st, x_align) : pe_ragged_launch<TI, gf_bf16>(a, st, x_align);
}

}   // namespace

extern "C" int gf_pos_encode(const void* x, int x_dtype, long sn, long sc, long sh, long sw, const float* pe,
                             void* out, int out_dtype, int N, int C, int H, int W, void* stream) {
    GF_CHECK_ARG(x && pe && out, "null pointer");
    GF_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0, "empty problem");
    GF_CHECK_ARG(x_dtype >= GF_F32 && x_dtype <= GF_BF16 && out_dtype >= GF_F32 && out_dtype <= GF_BF16, "bad dtype");
    PeArgs a{x, sn, sc, sh, sw, pe, out, N, C, H, W};
    return pe_dispatch<false>(x_dtype, out_dtype, a, (hipStream_t)stream, 0);
}

extern "C" int gf_pos_encode_ptrs(const void* const* x_table, int x_dtype, long sc, long sh, long sw, int x_align, const float* pe,
                                  void* out, int out_dtype, int N, int C, int H, int W, void* stream) {
    GF_CHECK_ARG(x_table && pe && out, "null pointer");
    GF_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0, "empty problem");
    GF_CHECK_ARG(N <= 65535, "at most 65535 table entries (the sample is a grid dimension)");
    GF_CHECK_ARG(x_align > 0 && (x_align & (x_align - 1)) == 0, "x_align must be a power of two");
    GF_CHECK_ARG(x_dtype >= GF_F32 && x_dtype <= GF_BF16 && out_dtype >= GF_F32 && out_dtype <= GF_BF16, "bad dtype");
    PeArgs a{x_table, 0, sc, sh, sw, pe, out, N, C, H, W};
    return pe_dispatch<true>(x_dtype, out_dtype, a, (hipStream_t)stream, (unsigned)x_align);
}

extern "C" int gf_pos_encode_ragged(const gf_map_record* x_table, int x_dtype, int x_align, const float* pe, void* out, int out_dtype,
                                    int N, int C, int H, int W, unsigned char* mask_out, void* stream) {
    GF_CHECK_ARG(x_table && pe && out, "null pointer");
    GF_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0, "empty problem");
    GF_CHECK_ARG(N <= 65535, "at most 65535 table entries (the sample is a grid dimension)");
    GF_CHECK_ARG((long)H * W < (1l << 24), "canvas too large");
    GF_CHECK_ARG(x_align > 0 && (x_align & (x_align - 1)) == 0, "x_align must be a power of two");
    GF_CHECK_ARG(x_dtype >= GF_F32 && x_dtype <= GF_BF16 && out_dtype >= GF_F32 && out_dtype <= GF_BF16, "bad dtype");
    PeRagArgs a{x_table, pe, out, mask_out, N, C, H, W};
    hipStream_t st = (hipStream_t)stream;
    if (x_dtype == GF_F32) return pe_ragged_to<float>(out_dtype, a, st, (unsigned)x_align);
    if (x_dtype == GF_F16) return pe_ragged_to<_Float16>(out_dtype, a, st, (unsigned)x_align);
    return pe_ragged_to<gf_bf16>(out_dtype, a, st, (unsigned)x_align);
}
