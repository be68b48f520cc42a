// The counter-based hash behind every RANSAC draw (k_ransac.hip, k_pose.hip, host/pose_host.cpp): one text for the device and the
// host, so a sample of hypothesis t is the same set of matches wherever it is drawn.  The bits are pinned by the homography tests
// against oracle/ransac_oracle.c.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GF_HASH_FN __host__ __device__ __forceinline__
#else
#define GF_HASH_FN static inline
#endif

GF_HASH_FN uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}
GF_HASH_FN uint32_t draw(uint32_t seed, uint32_t sample, uint32_t t, uint32_t k, uint32_t attempt) {
    uint32_t x = seed * 0x9E3779B1u;
    x = mix32(x ^ (sample + 0x7F4A7C15u));
    x = mix32(x ^ (t * 0x85EBCA6Bu + 0x165667B1u));
    x = mix32(x ^ (k * 0xC2B2AE35u + 0x27D4EB2Fu));
    x = mix32(x ^ (attempt * 0x9E3779B1u + 0x61C88647u));
    return x;
}
