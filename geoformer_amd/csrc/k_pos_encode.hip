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
// ONE kernel behind three entries, which differ only in the map source they hand it (gf_maps.h): gf_pos_encode (one batch tensor),
// gf_pos_encode_ptrs (N maps of one shape in separate allocations) and gf_pos_encode_ragged (N maps of unequal extents on a common
// canvas, zeros outside each map's own extent, optional padding mask).
#include "gf_maps.h"

namespace {

template <typename Src>
struct PeArgs {
    Src src;               // the N maps
    const float* pe;       // [H][W][C]
    void* out;             // [N][H*W][C]
    unsigned char* mask;   // null, or [N][H][W]
    int n0, N, C, H, W;    // n0: the first sample of this launch;  H, W: the canvas (every map's own extent, except for the ragged source)
};

// the arithmetic of all forms: input widened to fp32 (exact), + the fp32 table entry, one rounding into TO
template <typename TO, typename TI>
__device__ __forceinline__ TO pe_add(TI x, float pe) { return gf_from_float<TO>(gf_to_float(x) + pe); }

// The sample is a grid dimension, so its view (for a table source: one or five 8-byte words) is a few scalar loads at the head, and the
// choice among the three forms - made from the view's strides, which the ragged source has per sample - is a uniform branch.  A canvas
// position outside the sample's own h x w takes the value 0 (+ the table entry): the bits of the maps zero-padded and stacked.  Nothing
// outside [0, h) x [0, w) of a map is loaded.  The same launch writes the padding mask when asked to.
// VEC: the host's half of the vector form's conditions holds (C % 8 == 0, every base / pe / out 32-byte aligned)
template <typename TI, typename TO, typename Src, bool VEC>
__global__ __launch_bounds__(256) void pos_encode(PeArgs<Src> a) {
    __shared__ float tile[32][33];
    const int n = a.n0 + blockIdx.y, t = threadIdx.x;
    const long HW = (long)a.H * a.W;
    const GfMapView<TI> m = a.src.template view<TI>(n);
    if (a.mask)
        for (int p = blockIdx.x * 256 + t; p < HW; p += gridDim.x * 256) a.mask[(size_t)n * HW + p] = (p / a.W < m.h && p % a.W < m.w) ? 1 : 0;
    if (m.sc == 1 && VEC && m.sh % 8 == 0 && m.sw % 8 == 0) {
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
            if (y < m.h && x < m.w) v = *reinterpret_cast<const VI*>(m.base + y * m.sh + x * m.sw + c * 8);
            const VF pe = reinterpret_cast<const VF*>(a.pe)[i];
            VO o;
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = pe_add<TO>(v[k], pe[k]);
            out[i] = o;
        }
    } else if (m.sc == 1) {
        // channels-last, one element per lane
        const long total = HW * a.C;
        TO* out = (TO*)a.out + (size_t)n * total;
        for (long i = (long)blockIdx.x * 256 + t; i < total; i += (long)gridDim.x * 256) {
            const long p = i / a.C, y = p / a.W;
            const int c = (int)(i - p * a.C), x = (int)(p - y * a.W);
            float v = 0.f;
            if (y < m.h && x < m.w) v = gf_to_float(m.base[c + y * m.sh + x * m.sw]);
            out[i] = pe_add<TO>(v, a.pe[i]);
        }
    } else {
        // [C, h, w] maps: 32 x 32 (position x channel) tiles of the canvas transposed through LDS
        const int tx = t & 31, ty = t >> 5;      // 32 x 8
        const int hw = (int)HW, ptiles = (hw + 31) / 32, tiles = ptiles * ((a.C + 31) / 32);
        TO* out = (TO*)a.out + (size_t)n * HW * a.C;
        for (int tl = blockIdx.x; tl < tiles; tl += gridDim.x) {     // uniform trip count: the barriers below are met by all
            const int p0 = (tl % ptiles) * 32, c0 = (tl / ptiles) * 32;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c0 + ty + 8 * k, p = p0 + tx;
                float v = 0.f;
                if (c < a.C && p < hw) {
                    const int y = p / a.W, x = p % a.W;
                    if (y < m.h && x < m.w) v = gf_to_float(m.base[c * m.sc + y * m.sh + x * m.sw]);
                }
                tile[ty + 8 * k][tx] = v;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int p = p0 + ty + 8 * k, c = c0 + tx;
                if (c < a.C && p < hw) out[(long)p * a.C + c] = pe_add<TO>(tile[tx][ty + 8 * k], a.pe[(long)p * a.C + c]);
            }
            __syncthreads();
        }
    }
}

constexpr int PE_MAX_BLOCKS = 4096, PE_MAX_SAMPLES = 65535;      // the latter: what a grid's y dimension holds

// x_align (table sources): the largest power of two, in bytes, that divides EVERY table entry - the caller built the table and knows
template <typename TI, typename TO, typename Src>
int pe_launch(PeArgs<Src> a, hipStream_t st, unsigned x_align) {
    const long per = (long)a.H * a.W * a.C;
    const bool vec = a.C % 8 == 0 && a.src.bases_aligned(32, sizeof(TI), x_align) && (uintptr_t)a.out % 32 == 0 && (uintptr_t)a.pe % 32 == 0 &&
                     per < (1l << 34);
    const long work = vec ? per / 8 : per;
    const int blocks = (int)((work + 255) / 256 < PE_MAX_BLOCKS ? (work + 255) / 256 : PE_MAX_BLOCKS);
    // slices of PE_MAX_SAMPLES samples: one, except for a batch tensor of more (the table entries refuse more)
    for (a.n0 = 0; a.n0 < a.N; a.n0 += PE_MAX_SAMPLES) {
        const dim3 grid(blocks, a.N - a.n0 < PE_MAX_SAMPLES ? a.N - a.n0 : PE_MAX_SAMPLES);
        if (vec) pos_encode<TI, TO, Src, true><<<grid, 256, 0, st>>>(a);
        else pos_encode<TI, TO, Src, false><<<grid, 256, 0, st>>>(a);
    }
    GF_CHECK_LAUNCH();
    return GF_OK;
}

template <typename TI, typename Src>
int pe_launch_to(int out_dtype, const PeArgs<Src>& a, hipStream_t st, unsigned x_align) {
    return out_dtype == GF_F32 ? pe_launch<TI, float>(a, st, x_align)
                               : out_dtype == GF_F16 ? pe_launch<TI, _Float16>(a, st, x_align) : pe_launch<TI, gf_bf16>(a, st, x_align);
}

template <typename Src>
int pe_dispatch(int x_dtype, int out_dtype, const PeArgs<Src>& a, void* stream, int x_align) {
    hipStream_t st = (hipStream_t)stream;
    if (x_dtype == GF_F32) return pe_launch_to<float>(out_dtype, a, st, (unsigned)x_align);
    if (x_dtype == GF_F16) return pe_launch_to<_Float16>(out_dtype, a, st, (unsigned)x_align);
    return pe_launch_to<gf_bf16>(out_dtype, a, st, (unsigned)x_align);
}

}   // namespace

// The checks of the three entries, in one order; a macro, so that GF_CHECK_ARG's message names the entry that was called.
// table: the entry takes a device table - its sample count is bounded by a grid dimension and x_align is the caller's word.
#define PE_CHECK_ARGS(x, table, x_align, canvas_ok)                                                                                        \
    GF_CHECK_ARG((x) && pe && out, "null pointer");                                                                                        \
    GF_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0, "empty problem");                                                                       \
    GF_CHECK_ARG(!(table) || N <= PE_MAX_SAMPLES, "at most 65535 table entries (the sample is a grid dimension)");                        \
    GF_CHECK_ARG(canvas_ok, "canvas too large");                                                                                           \
    GF_CHECK_ARG(!(table) || ((x_align) > 0 && ((x_align) & ((x_align) - 1)) == 0), "x_align must be a power of two");                   \
    GF_CHECK_ARG(x_dtype >= GF_F32 && x_dtype <= GF_BF16 && out_dtype >= GF_F32 && out_dtype <= GF_BF16, "bad dtype")

extern "C" int gf_pos_encode(const void* x, int x_dtype, long sn, long sc, long sh, long sw, const float* pe,
                             void* out, int out_dtype, int N, int C, int H, int W, void* stream) {
    PE_CHECK_ARGS(x, false, 0, true);
    PeArgs<GfTensorMaps> a{{x, sn, sc, sh, sw, H, W}, pe, out, nullptr, 0, N, C, H, W};
    return pe_dispatch(x_dtype, out_dtype, a, stream, 0);
}

extern "C" int gf_pos_encode_ptrs(const void* const* x_table, int x_dtype, long sc, long sh, long sw, int x_align, const float* pe,
                                  void* out, int out_dtype, int N, int C, int H, int W, void* stream) {
    PE_CHECK_ARGS(x_table, true, x_align, true);
    PeArgs<GfTableMaps> a{{x_table, sc, sh, sw, H, W}, pe, out, nullptr, 0, N, C, H, W};
    return pe_dispatch(x_dtype, out_dtype, a, stream, x_align);
}

extern "C" int gf_pos_encode_ragged(const gf_map_record* x_table, int x_dtype, int x_align, const float* pe, void* out, int out_dtype,
                                    int N, int C, int H, int W, unsigned char* mask_out, void* stream) {
    PE_CHECK_ARGS(x_table, true, x_align, (long)H * W < (1l << 24));
    PeArgs<GfRaggedMaps> a{{x_table}, pe, out, mask_out, 0, N, C, H, W};
    return pe_dispatch(x_dtype, out_dtype, a, stream, x_align);
}
