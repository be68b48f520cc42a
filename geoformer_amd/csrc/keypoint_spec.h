// Keypoint consolidation for SfM (eval_tool/immatch/utils/localize_sfm_helper.py: quantize_keypoints, compute_keypoints,
// get_unique_matches_ids, matches_to_keypoint_ids): the arithmetic and the orderings, stated once for the device (k_keypoints.hip)
// and the serial host build (host/keypoint_host.cpp).  All arithmetic is fp32 with contraction off.
//
// POINT STREAM.  Row r of pair q (rows pair_offsets[q] .. pair_offsets[q + 1]) survives when kp_row_valid says so.  Every row, surviving or
// not, owns two ARRIVAL INDICES: side 0 -> 2 * off_q + (r - off_q), side 1 -> 2 * off_q + n_q + (r - off_q).  Ascending arrival index is
// the reference's processing order: lexicographic in (pair, side, row).  A point belongs to image pair_images[q][side].
//
// CELL.  kp_cell(x, psize) = floor(x / psize) of the EXACT quotient (numpy.floor_divide on float32).  Rounding is monotone, so floorf of
// the rounded quotient is either that floor or, where the quotient was rounded UP onto an integer, one above it; the second case is
// q * psize > x, read off the sign of fmaf(-q, psize, x) (one rounding, which keeps the sign: the exact value is a multiple of 2^-149
// and cannot round to zero).  Cells of coordinates inside +-KP_MAX_COORD with psize > KP_MIN_PSIZE lie inside +-KP_CELL_LIMIT.
//
// WALK.  The points of one (image, cell) group are taken in arrival order against the group's centres in creation order:
// d = sqrtf(dx * dx + dy * dy) (two products, one sum, a correctly rounded root), the candidate is the FIRST minimum of d, and
// d < dthres merges: centre = (centre + point) / 2.  Otherwise the point creates a centre.  kp_distance and kp_merge are the two steps;
// the first-minimum search is a loop on the host and a wave reduction on the device, over the same (d, index) order: kp_closer.
//
// FILTER.  Within a pair a row stays iff it is the winner among the rows sharing its id0 and among the rows sharing its id1; the
// winner is the largest kp_winner_key: the higher score, and between equal scores (-0.0 == 0.0) the LOWER row.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define KP_HD __host__ __device__ inline
#else
#define KP_HD static inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define KP_MAX_COORD 4194304.0f      /* 2^22: the largest |coordinate| of the quantised mode (a larger one is reported, never wrapped) */
#define KP_MIN_PSIZE 2.0f            /* psize must be LARGER than this: then |cell| <= KP_MAX_COORD / psize < KP_CELL_LIMIT */
#define KP_CELL_BITS 22
#define KP_CELL_LIMIT (1 << (KP_CELL_BITS - 1))      /* cells -2^21 .. 2^21 - 1 */
#define KP_IMAGE_BITS 19
#define KP_MAX_IMAGES (1 << KP_IMAGE_BITS)           /* image indices 0 .. 524287 */
#define KP_INVALID_KEY 0x7fffffffffffffffll          /* sorts behind every valid key */

/* bits of the per-call status word (device: OR-ed by the key kernel; host build: returned in stats) */
#define KP_FLAG_COORD_RANGE 1        /* a surviving row had a |coordinate| > KP_MAX_COORD in the quantised mode (the row was dropped) */
#define KP_FLAG_IMAGE_RANGE 2        /* pair_images held an index outside [0, n_images) (the pair's rows were dropped) */

KP_HD uint32_t kp_bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

KP_HD bool kp_finite(float v) { return (kp_bits(v) & 0x7f800000u) != 0x7f800000u; }

// the score filter of process_matches_and_keypoints_exporth5 (scores >= sc_thres; a NaN score fails it) plus: all four coordinates finite
KP_HD bool kp_row_valid(const float* m4, float score, float sc_thres) {
    return score >= sc_thres && kp_finite(m4[0]) && kp_finite(m4[1]) && kp_finite(m4[2]) && kp_finite(m4[3]);
}

KP_HD bool kp_coord_in_range(float v) { return fabsf(v) <= KP_MAX_COORD; }

// floor of the exact x / psize, psize > 0, both finite
KP_HD float kp_cell(float x, float psize) {
    float q = floorf(x / psize);
    if (fmaf(-q, psize, x) < 0.f) q -= 1.f;      // x - q * psize, rounded once: q * psize > x, the quotient had been rounded up
    return q;
}

// group key of the quantised mode; the caller has checked image < KP_MAX_IMAGES and the coordinate range
KP_HD int64_t kp_cell_key(int image, float x, float y, float psize) {
    const int64_t cx = (int64_t)kp_cell(x, psize) + KP_CELL_LIMIT, cy = (int64_t)kp_cell(y, psize) + KP_CELL_LIMIT;
    return ((int64_t)image << (2 * KP_CELL_BITS)) | (cy << KP_CELL_BITS) | cx;
}

// exact mode: points with equal (x, y) share a key; -0.0 == 0.0
KP_HD int64_t kp_exact_key(float x, float y) {
    const uint32_t bx = x == 0.f ? 0u : kp_bits(x), by = y == 0.f ? 0u : kp_bits(y);
    return (int64_t)(((uint64_t)by << 32) | bx);
}

KP_HD float kp_distance(float px, float py, float cx, float cy) {
    const float dx = px - cx, dy = py - cy;
    const float a = dx * dx, b = dy * dy;
    return sqrtf(a + b);
}

// (d, j) precedes (best_d, best_j): the order whose minimum is numpy.argmin's first minimum.  d is never NaN (finite operands)
KP_HD bool kp_closer(float d, int j, float best_d, int best_j) { return d < best_d || (d == best_d && j < best_j); }

KP_HD void kp_merge(float& cx, float& cy, float px, float py) {
    cx = (cx + px) / 2.f;
    cy = (cy + py) / 2.f;
}

// the winner of a group of rows is the one with the largest key: score first (ordered bits, -0.0 as 0.0), then the lower row
KP_HD uint64_t kp_winner_key(float score, uint32_t row) {
    uint32_t b = score == 0.f ? 0u : kp_bits(score);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)b << 32) | (uint32_t)(0xffffffffu - row);
}
