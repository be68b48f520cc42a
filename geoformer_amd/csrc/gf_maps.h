// Where the N feature maps of a batch lie: the one difference between the three entries of a1 (k_pos_encode.hip) and of K7 (k_fine.hip).
// A source is passed by value in the kernel arguments and turns a sample index into a GfMapView; everything after that is one kernel.
// The index given to view() must be wave-uniform (a grid dimension, or through v_readfirstlane): the table entry or record is then a
// few scalar loads at the head of the kernel, not 64 lanes fetching one address.
#pragma once
#include "gf_common.h"

template <typename T>
struct GfMapView {
    const T* base;      // element [0][0][0] of the sample's map
    long sc, sh, sw;    // element strides of the map viewed as [C, h, w]
    int h, w;           // the map's own extent: nothing outside [0, h) x [0, w) is loaded
};

// per_sample: strides and extent differ between samples, so a choice that depends on them is made in the kernel (a uniform branch) and
// not by the host.   bases_aligned (host): is every sample's base a multiple of `bytes`?  A table's caller built it and says so (`align`,
// the largest power of two dividing every entry).

// one batch tensor [N, C, h, w] with element strides (gf_pos_encode, gf_fine_gather)
struct GfTensorMaps {
    static constexpr bool per_sample = false;
    const void* x;
    long sn, sc, sh, sw;
    int h, w;
    template <typename T>
    __device__ __forceinline__ GfMapView<T> view(int n) const { return {(const T*)x + n * sn, sc, sh, sw, h, w}; }
    bool bases_aligned(unsigned bytes, unsigned elem, unsigned) const { return (uintptr_t)x % bytes == 0 && sn * elem % bytes == 0; }
};

// a device table of N base addresses, strides and extent common to all (gf_pos_encode_ptrs, gf_fine_gather_ptrs)
struct GfTableMaps {
    static constexpr bool per_sample = false;
    const void* const* table;
    long sc, sh, sw;
    int h, w;
    template <typename T>
    __device__ __forceinline__ GfMapView<T> view(int n) const { return {(const T*)table[n], sc, sh, sw, h, w}; }
    bool bases_aligned(unsigned bytes, unsigned, unsigned align) const { return align % bytes == 0; }
};

// a device table of N gf_map_record: base, strides and extent per sample (gf_pos_encode_ragged, gf_fine_gather_ragged)
struct GfRaggedMaps {
    static constexpr bool per_sample = true;
    const gf_map_record* table;
    template <typename T>
    __device__ __forceinline__ GfMapView<T> view(int n) const {
        const gf_map_record r = table[n];
        return {(const T*)r.base, r.sc, r.sh, r.sw, r.h, r.w};
    }
    bool bases_aligned(unsigned bytes, unsigned, unsigned align) const { return align % bytes == 0; }
};
