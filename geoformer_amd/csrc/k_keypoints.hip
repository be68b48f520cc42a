// Keypoint consolidation for SfM on the device: pair matches -> one keypoint list per image + every match as two keypoint indices
// (the reference's quantize_keypoints / compute_keypoints / get_unique_matches_ids, eval_tool/immatch/utils/localize_sfm_helper.py).
// The arithmetic and the orderings are keypoint_spec.h, shared with the serial host build (host/keypoint_host.cpp); this file is the
// parallel decomposition.  N = 2 M points, indexed by ARRIVAL INDEX (keypoint_spec.h): ascending index = the reference's order.
//
//   keys    one thread per point: validity + the 63-bit group key (image | cell y | cell x; exact mode: image, and the coordinate
//           bits as a second key; there the walk is trivial and has a kernel of its own, one thread per point).  Dropped points get KP_INVALID_KEY and sort behind everything.
//   [the caller sorts the keys STABLY: equal keys keep arrival order]
//   heads   one thread per sorted position: 1 where a group starts.  [the caller scans the flags: group index per position]
//   walk    the hot path, sequential per group and parallel across groups.  One wave64 per (image, cell) group, several waves per
//           workgroup, no workgroup barrier and no LDS: groups are dealt to up to 4096 waves, so a long group delays nobody.  The group's
//           centres are spread over the lanes - centre j lives in lane j % 64; centres 0 .. 63 in registers, further ones in chunks of
//           64 in a global scratch area at the group's own offset (a group has no more centres than points, so the scratch is linear
//           in N and groups never overlap).  Lane l is the only lane that ever reads or writes centre j = l (mod 64): same-lane program
//           order is all the memory ordering the scratch needs; whatever crosses lanes does so in registers.
//           Per point: every lane takes the distance to its centre of the chunk, the wave takes the minimum of the distance bits with
//           DPP / permute steps (non-negative floats order like their bits), a ballot picks the LOWEST lane that holds it, and chunks
//           are compared in order with kp_closer - the (distance, index) order of numpy's first minimum.  Any number of centres works.
//           Besides the centre, the walk keeps per centre the first point of the CURRENT (pair, side) segment that reached it: the
//           points of a segment are contiguous in a group (arrival order), so this names a slot that is unique per (pair, side,
//           keypoint) - what the filter needs - in memory linear in N.
//   [the caller scans the creator flags in arrival order and turns per-segment counts into per-image ranks: tiny tensors]
//   filter  per surviving row a 64-bit atomicMax of kp_winner_key into the two slots, then: a row stays iff it holds both.  Integer
//           max is order-independent, so the result is the same bits in every run.
//   emit    keypoint coordinates gathered into per-image lists, kept rows compacted in row order with their two ids, pair offsets.
// Nothing here synchronises or allocates; data-dependent sizes (K keypoints, M' rows, the status flags) land in `counts`.
#include "gf_common.h"
#include "keypoint_spec.h"

namespace {

enum { KP_C_FLAGS = 0, KP_C_GROUPS = 1, KP_C_K = 4, KP_C_ROWS = 5, KP_C_WORDS = 8 };

constexpr int kWalkThreads = 256;          // 4 waves per workgroup, each on its own group
constexpr int kWalkMaxBlocks = 1024;       // 4 per CU: enough waves to hide each other's cross-lane and scratch latency

// largest q in [0, P) with off[q] <= r (pairs without rows share an offset with their successor: the successor is found)
__device__ __forceinline__ int kp_find_pair(const int* __restrict__ off, int P, int r) {
    int lo = 0, hi = P;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= r) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void kp_keys_kernel(const float* __restrict__ matches, const float* __restrict__ scores, const int* __restrict__ off,
                               const int* __restrict__ pair_images, int P, int M, int n_images, float sc_thres, float psize, int quant,
                               long long* __restrict__ keys, long long* __restrict__ keys2, float* __restrict__ pts, int* __restrict__ pseg,
                               int* __restrict__ seg_begin, int* __restrict__ counts) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= 2 * M) return;
    // arrival index -> (pair, side, row): pair q owns arrival indices 2 off[q] .. 2 off[q + 1]
    const int q = kp_find_pair(off, P, a >> 1);
    const int o = off[q], n = off[q + 1] - o, t = a - 2 * o;
    const int side = t >= n ? 1 : 0, r = o + t - side * n;
    long long key = KP_INVALID_KEY, key2 = 0;
    float px = 0.f, py = 0.f;
    int flags = 0;
    if (n > 0 && t >= 0 && t < 2 * n && r >= 0 && r < M) {             // (offsets that are not ascending: the point is dropped, nothing is read outside)
        const float* m = matches + 4 * (size_t)r;
        const float m4[4] = {m[0], m[1], m[2], m[3]};
        px = m4[2 * side], py = m4[2 * side + 1];
        if (kp_row_valid(m4, scores[r], sc_thres)) {
            const int i0 = pair_images[2 * q], i1 = pair_images[2 * q + 1];
            const int image = side ? i1 : i0;
            if (i0 < 0 || i0 >= n_images || i1 < 0 || i1 >= n_images) flags = KP_FLAG_IMAGE_RANGE;
            else if (!quant) key = image, key2 = kp_exact_key(px, py);
            else if (!(kp_coord_in_range(m4[0]) && kp_coord_in_range(m4[1]) && kp_coord_in_range(m4[2]) && kp_coord_in_range(m4[3]))) flags = KP_FLAG_COORD_RANGE;
            else key = kp_cell_key(image, px, py, psize);
        }
    }
    keys[a] = key;
    if (keys2) keys2[a] = key2;
    pts[2 * (size_t)a] = px, pts[2 * (size_t)a + 1] = py;
    pseg[a] = 2 * q + side;
    seg_begin[a] = 2 * o + side * n;
    if (flags) atomicOr(&counts[KP_C_FLAGS], flags);
}

__global__ void kp_heads_kernel(const long long* __restrict__ keys, const long long* __restrict__ keys2, const long long* __restrict__ order, int N,
                                int* __restrict__ head) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const unsigned long long a = (unsigned long long)order[i];
    int h = 0;
    if (a < (unsigned long long)N && keys[a] != KP_INVALID_KEY) {
        h = 1;
        if (i > 0) {
            const unsigned long long b = (unsigned long long)order[i - 1];
            if (b < (unsigned long long)N && keys[b] == keys[a] && (!keys2 || keys2[b] == keys2[a])) h = 0;
        }
    }
    head[i] = h;
}

// gstart[g] = sorted position of group g's first point, gstart[n_groups] = number of surviving points (they precede every dropped point:
// KP_INVALID_KEY is the largest key); the dropped points get their outputs here
__global__ void kp_group_starts_kernel(const long long* __restrict__ keys, const long long* __restrict__ order, const int* __restrict__ head,
                                       const int* __restrict__ gid, int N, int* __restrict__ gstart, int* __restrict__ owner,
                                       int* __restrict__ slot, int* __restrict__ creator, int* __restrict__ counts) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const unsigned long long a = (unsigned long long)order[i];
    if (a >= (unsigned long long)N) return;
    if (keys[a] == KP_INVALID_KEY) {
        owner[a] = -1, slot[a] = -1, creator[a] = 0;
        return;
    }
    if (head[i]) gstart[gid[i] - 1] = i;
    bool last = i == N - 1;
    if (!last) {
        const unsigned long long b = (unsigned long long)order[i + 1];
        last = b >= (unsigned long long)N || keys[b] == KP_INVALID_KEY;
    }
    if (last) {
        gstart[gid[i]] = i + 1;
        counts[KP_C_GROUPS] = gid[i];
    }
}

// minimum over the wave, in every lane: xor butterflies, 1 .. 8 as DPP moves, 16 and 32 as permutes
__device__ __forceinline__ unsigned kp_wave_min(unsigned v) {
    v = min(v, gf_fetch_xor<1>(v));
    v = min(v, gf_fetch_xor<2>(v));
    v = min(v, gf_fetch_xor<4>(v));
    v = min(v, gf_fetch_xor<8>(v));
    v = min(v, (unsigned)__shfl_xor((int)v, 16, 64));
    v = min(v, (unsigned)__shfl_xor((int)v, 32, 64));
    return v;
}

// exact mode: every point of a group is the same point; the first arrival creates the keypoint and the others refer to it - one thread
// per sorted position, nothing sequential
__global__ void kp_exact_kernel(const long long* __restrict__ keys, const long long* __restrict__ order, const int* __restrict__ head,
                                const int* __restrict__ gid, const float* __restrict__ pts, const int* __restrict__ gstart, int N,
                                int* __restrict__ owner, int* __restrict__ slot, int* __restrict__ creator, float* __restrict__ cxy) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const unsigned long long a = (unsigned long long)order[i];
    if (a >= (unsigned long long)N || keys[a] == KP_INVALID_KEY) return;
    const int first = gstart[gid[i] - 1];                   // a surviving position lies in a group: gid >= 1
    if (first < 0 || first > i) return;
    const int a0 = (int)order[first];
    owner[a] = a0, slot[a] = (int)a, creator[a] = head[i];
    if (head[i]) cxy[2 * a] = pts[2 * a], cxy[2 * a + 1] = pts[2 * a + 1];
}

// Everything that steers the walk - the group, its range, the point, the number of centres - is wave-uniform, and the loop over groups is
// a static deal (group g to wave g mod waves) on a scalar: no lane ever takes another path through the loops than its wave, so the
// cross-lane steps always run with all 64 lanes.  This must hold: with groups drawn from a counter under `if (lane == 0)` and skipped
// with `continue`, the compiler is free to send the other 63 lanes back to the broadcast without lane 0, and they spin on group 0.
__global__ __launch_bounds__(kWalkThreads) void kp_walk_kernel(const long long* __restrict__ order, const float* __restrict__ pts,
                                                               const int* __restrict__ seg_begin, const int* __restrict__ gstart, int N,
                                                               float dthres, int* __restrict__ owner, int* __restrict__ slot,
                                                               int* __restrict__ creator, float* __restrict__ cxy, float* sc_x, float* sc_y,
                                                               int* sc_cr, int* sc_rep, const int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kWalkThreads / 64) + (threadIdx.x >> 6)));
    const int n_waves = (int)gridDim.x * (kWalkThreads / 64);
    const int n_groups = __builtin_amdgcn_readfirstlane(counts[KP_C_GROUPS]);
    for (int g = wave; g < n_groups; g += n_waves) {
        const int s = __builtin_amdgcn_readfirstlane(gstart[g]), e = __builtin_amdgcn_readfirstlane(gstart[g + 1]);
        if (s >= 0 && e <= N && s < e) {
            float cx = 0.f, cy = 0.f;        // this lane's centre of chunk 0 (centre index = lane)
            int ccr = -1, crep = -1;         // its creating point; the first point of the latest segment that reached it
            int ncent = 0;
            for (int i = s; i < e; ++i) {
                const int a = __builtin_amdgcn_readfirstlane((int)order[i]);
                const float px = pts[2 * (size_t)a], py = pts[2 * (size_t)a + 1];
                const int sb = seg_begin[a];
                float best_d = 0.f;
                int best_j = -1, best_cr = -1;
                const int nch = (ncent + 63) >> 6;
                for (int c = 0; c < nch; ++c) {
                    const int j = 64 * c + lane;
                    const bool act = j < ncent;
                    float x = cx, y = cy;
                    int cr = ccr;
                    if (c > 0 && act) x = sc_x[s + j], y = sc_y[s + j], cr = sc_cr[s + j];
                    const unsigned db = act ? kp_bits(kp_distance(px, py, x, y)) : 0x7f800000u;      // idle lanes: +inf
                    const unsigned mb = kp_wave_min(db);
                    const unsigned long long holders = __ballot(act && db == mb);
                    const int l = __ffsll((long long)holders) - 1;                                    // the lowest centre index at the minimum
                    const int cr_l = __shfl(cr, l, 64);
                    const float dm = __uint_as_float(mb);
                    if (best_j < 0 || kp_closer(dm, 64 * c + l, best_d, best_j)) best_d = dm, best_j = 64 * c + l, best_cr = cr_l;
                }
                // (the search's results are equal in every lane; through readfirstlane the compiler knows it too)
                const bool merge = __builtin_amdgcn_readfirstlane((int)(best_j >= 0 && best_d < dthres)) != 0;
                const int k = merge ? __builtin_amdgcn_readfirstlane(best_j) : ncent;      // the centre this point goes to
                int rep = a;
                if ((k & 63) == lane) {
                    if (k < 64) {
                        if (merge) kp_merge(cx, cy, px, py);
                        else cx = px, cy = py, ccr = a, crep = -1;
                        rep = crep >= sb ? crep : a;
                        crep = rep;
                    } else if (merge) {
                        float x = sc_x[s + k], y = sc_y[s + k];
                        kp_merge(x, y, px, py);
                        sc_x[s + k] = x, sc_y[s + k] = y;
                        const int old = sc_rep[s + k];
                        rep = old >= sb ? old : a;
                        sc_rep[s + k] = rep;
                    } else {
                        sc_x[s + k] = px, sc_y[s + k] = py, sc_cr[s + k] = a, sc_rep[s + k] = a;
                    }
                }
                rep = __shfl(rep, k & 63, 64);
                if (lane == 0) owner[a] = merge ? best_cr : a, slot[a] = rep, creator[a] = merge ? 0 : 1;
                ncent += merge ? 0 : 1;
            }
            // the centres' final coordinates, stored under their creating points
            if (lane < ncent) cxy[2 * (size_t)ccr] = cx, cxy[2 * (size_t)ccr + 1] = cy;
            for (int j = 64 + lane; j < ncent; j += 64) {
                const int cr = sc_cr[s + j];
                cxy[2 * (size_t)cr] = sc_x[s + j], cxy[2 * (size_t)cr + 1] = sc_y[s + j];
            }
        }
    }
}

// global keypoint slot (image-major, then rank among the image's creators in arrival order) of creating point o
__device__ __forceinline__ int kp_slot_of(const int* __restrict__ cscan, const int* __restrict__ pseg, const int* __restrict__ seg_adj, int o) {
    return seg_adj[pseg[o]] + cscan[o] - 1;
}

__global__ void kp_winners_kernel(const float* __restrict__ scores, const int* __restrict__ off, int P, int M, const int* __restrict__ owner,
                                  const int* __restrict__ slot, unsigned long long* __restrict__ winners) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;
    const int q = kp_find_pair(off, P, r);
    const int a0 = off[q] + r, a1 = a0 + (off[q + 1] - off[q]);
    if (a0 < 0 || a1 >= 2 * M || owner[a0] < 0) return;
    const unsigned long long key = kp_winner_key(scores[r], (uint32_t)r);
    atomicMax(&winners[slot[a0]], key);
    atomicMax(&winners[slot[a1]], key);
}

__global__ void kp_keep_kernel(const float* __restrict__ scores, const int* __restrict__ off, int P, int M, const int* __restrict__ owner,
                               const int* __restrict__ slot, const unsigned long long* __restrict__ winners, int unique, int* __restrict__ keep) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;
    const int q = kp_find_pair(off, P, r);
    const int a0 = off[q] + r, a1 = a0 + (off[q + 1] - off[q]);
    int k = 0;
    if (a0 >= 0 && a1 < 2 * M && owner[a0] >= 0) {
        k = 1;
        if (unique) {
            const unsigned long long key = kp_winner_key(scores[r], (uint32_t)r);
            k = winners[slot[a0]] == key && winners[slot[a1]] == key;
        }
    }
    keep[r] = k;
}

__global__ void kp_gather_kernel(const int* __restrict__ creator, const int* __restrict__ cscan, const int* __restrict__ pseg,
                                 const int* __restrict__ seg_adj, const float* __restrict__ cxy, int N, float* __restrict__ keypoints,
                                 int* __restrict__ counts) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= N) return;
    if (a == N - 1) counts[KP_C_K] = cscan[a];
    if (!creator[a]) return;
    const int ks = kp_slot_of(cscan, pseg, seg_adj, a);
    if (ks < 0 || ks >= N) return;
    keypoints[2 * (size_t)ks] = cxy[2 * (size_t)a], keypoints[2 * (size_t)ks + 1] = cxy[2 * (size_t)a + 1];
}

__global__ void kp_rows_kernel(const int* __restrict__ keep, const int* __restrict__ kscan, const int* __restrict__ off,
                               const int* __restrict__ pair_images, int P, int M, const int* __restrict__ owner, const int* __restrict__ cscan,
                               const int* __restrict__ pseg, const int* __restrict__ seg_adj, const int* __restrict__ kp_offsets,
                               int* __restrict__ ids, int* __restrict__ pair_offsets_out, int* __restrict__ counts) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r <= P) {                                              // the first P + 1 threads also write the pair offsets
        const int o = off[r];
        pair_offsets_out[r] = o > 0 ? kscan[min(o, M) - 1] : 0;
    }
    if (r >= M) return;
    if (r == M - 1) counts[KP_C_ROWS] = kscan[r];
    if (!keep[r]) return;
    const int q = kp_find_pair(off, P, r);
    const int a0 = off[q] + r, a1 = a0 + (off[q + 1] - off[q]);
    const int pos = kscan[r] - 1;
    ids[2 * (size_t)pos] = kp_slot_of(cscan, pseg, seg_adj, owner[a0]) - kp_offsets[pair_images[2 * q]];
    ids[2 * (size_t)pos + 1] = kp_slot_of(cscan, pseg, seg_adj, owner[a1]) - kp_offsets[pair_images[2 * q + 1]];
}

struct KpWorkspace {
    int* gstart;
    float *sc_x, *sc_y;
    int *sc_cr, *sc_rep;
    unsigned long long* winners;
    size_t bytes;
};

KpWorkspace kp_carve(void* ws, int M) {
    const size_t N = 2 * (size_t)M;
    GfCarver c(ws);
    KpWorkspace w;
    w.winners = c.take<unsigned long long>(N);
    w.gstart = c.take<int>(N + 1);
    w.sc_x = c.take<float>(N);
    w.sc_y = c.take<float>(N);
    w.sc_cr = c.take<int>(N);
    w.sc_rep = c.take<int>(N);
    w.bytes = c.used();
    return w;
}

inline int kp_blocks(long long n) { return (int)((n + 255) / 256); }

}   // namespace

#define KP_MAX_ROWS ((1 << 30) - 1)

extern "C" size_t gf_keypoint_workspace_bytes(int M) {
    if (M <= 0 || M > KP_MAX_ROWS) return 0;
    return kp_carve(nullptr, M).bytes;
}

extern "C" int gf_keypoint_keys(const float* matches, const float* scores, const int* pair_offsets, const int* pair_images, int P, int M,
                                int n_images, float sc_thres, float psize, float dthres, long long* keys, long long* keys2, float* pts,
                                int* pseg, int* seg_begin, int* counts, void* stream) {
    GF_CHECK_ARG(P >= 0 && M >= 0 && M <= KP_MAX_ROWS, "P and M must be >= 0 and M < 2^30");
    GF_CHECK_ARG(n_images >= 0 && n_images <= KP_MAX_IMAGES, "image index range: n_images must be within 0 .. 524288 (19 key bits)");
    const bool quant = psize > 0.f && dthres > 0.f;
    GF_CHECK_ARG(!quant || (kp_finite(psize) && psize > KP_MIN_PSIZE),
                 "cell index range: psize must be finite and larger than 2, so that coordinates up to 2^22 stay inside 22-bit cell indices");
    GF_CHECK_ARG(counts, "counts is a null pointer");
    GF_CHECK_ARG(pair_offsets, "pair_offsets is a null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (M > 0) {
        GF_CHECK_ARG(P > 0, "rows without pairs");
        GF_CHECK_ARG(matches && scores && pair_images && keys && pts && pseg && seg_begin, "null pointer");
        GF_CHECK_ARG(quant || keys2, "the exact mode needs keys2");
    }
    (void)hipMemsetAsync(counts, 0, KP_C_WORDS * sizeof(int), st);
    if (M > 0) {
        kp_keys_kernel<<<kp_blocks(2 * (long long)M), 256, 0, st>>>(matches, scores, pair_offsets, pair_images, P, M, n_images, sc_thres, psize,
                                                                   quant ? 1 : 0, keys, quant ? nullptr : keys2, pts, pseg, seg_begin, counts);
    }
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_keypoint_heads(const long long* keys, const long long* keys2, const long long* order, int M, int* head, void* stream) {
    GF_CHECK_ARG(M >= 0 && M <= KP_MAX_ROWS, "M must be within 0 .. 2^30 - 1");
    if (M == 0) return GF_OK;
    GF_CHECK_ARG(keys && order && head, "null pointer");
    kp_heads_kernel<<<kp_blocks(2 * (long long)M), 256, 0, (hipStream_t)stream>>>(keys, keys2, order, 2 * M, head);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_keypoint_walk(const long long* keys, const long long* order, const int* head, const int* group_scan, const float* pts,
                                const int* seg_begin, int M, float psize, float dthres, int* owner, int* slot, int* creator, float* cxy,
                                int* counts, void* workspace, size_t workspace_bytes, void* stream) {
    GF_CHECK_ARG(M >= 0 && M <= KP_MAX_ROWS, "M must be within 0 .. 2^30 - 1");
    if (M == 0) return GF_OK;
    GF_CHECK_ARG(keys && order && head && group_scan && pts && seg_begin && owner && slot && creator && cxy && counts && workspace, "null pointer");
    const KpWorkspace w = kp_carve(workspace, M);
    if (workspace_bytes < w.bytes) {
        gf_set_error("%s: workspace too small (%zu < %zu)", __func__, workspace_bytes, w.bytes);
        return GF_ERR_WORKSPACE;
    }
    const bool quant = psize > 0.f && dthres > 0.f;
    const int N = 2 * M;
    hipStream_t st = (hipStream_t)stream;
    kp_group_starts_kernel<<<kp_blocks(N), 256, 0, st>>>(keys, order, head, group_scan, N, w.gstart, owner, slot, creator, counts);
    const int blocks = min(kWalkMaxBlocks, (N + kWalkThreads - 1) / kWalkThreads);
    void* tok = gf_prof_begin("kp_walk", st, (double)N);
    if (quant) {
        kp_walk_kernel<<<blocks, kWalkThreads, 0, st>>>(order, pts, seg_begin, w.gstart, N, dthres, owner, slot, creator, cxy, w.sc_x, w.sc_y,
                                                       w.sc_cr, w.sc_rep, counts);
    } else {
        kp_exact_kernel<<<kp_blocks(N), 256, 0, st>>>(keys, order, head, group_scan, pts, w.gstart, N, owner, slot, creator, cxy);
    }
    gf_prof_end("kp_walk", tok, st);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_keypoint_filter(const float* scores, const int* pair_offsets, int P, int M, const int* owner, const int* slot, int unique,
                                  int* keep, void* workspace, size_t workspace_bytes, void* stream) {
    GF_CHECK_ARG(P >= 0 && M >= 0 && M <= KP_MAX_ROWS, "P and M must be >= 0 and M < 2^30");
    if (M == 0) return GF_OK;
    GF_CHECK_ARG(P > 0 && scores && pair_offsets && owner && slot && keep && workspace, "null pointer");
    const KpWorkspace w = kp_carve(workspace, M);
    if (workspace_bytes < w.bytes) {
        gf_set_error("%s: workspace too small (%zu < %zu)", __func__, workspace_bytes, w.bytes);
        return GF_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    if (unique) {
        (void)hipMemsetAsync(w.winners, 0, 2 * (size_t)M * sizeof(unsigned long long), st);
        kp_winners_kernel<<<kp_blocks(M), 256, 0, st>>>(scores, pair_offsets, P, M, owner, slot, w.winners);
    }
    kp_keep_kernel<<<kp_blocks(M), 256, 0, st>>>(scores, pair_offsets, P, M, owner, slot, w.winners, unique ? 1 : 0, keep);
    GF_CHECK_LAUNCH();
    return GF_OK;
}

extern "C" int gf_keypoint_emit(const int* creator, const int* creator_scan, const int* pseg, const int* seg_adj, const float* cxy, const int* keep,
                                const int* keep_scan, const int* pair_offsets, const int* pair_images, int P, int M, const int* owner,
                                const int* kp_offsets, float* keypoints, int* ids, int* pair_offsets_out, int* counts, void* stream) {
    GF_CHECK_ARG(P >= 0 && M >= 0 && M <= KP_MAX_ROWS, "P and M must be >= 0 and M < 2^30");
    GF_CHECK_ARG(pair_offsets && pair_offsets_out && counts, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (M > 0) {
        GF_CHECK_ARG(creator && creator_scan && pseg && seg_adj && cxy && keep && keep_scan && pair_images && owner && kp_offsets && keypoints && ids,
                     "null pointer");
        kp_gather_kernel<<<kp_blocks(2 * (long long)M), 256, 0, st>>>(creator, creator_scan, pseg, seg_adj, cxy, 2 * M, keypoints, counts);
    }
    kp_rows_kernel<<<kp_blocks((long long)(M > P + 1 ? M : P + 1)), 256, 0, st>>>(keep, keep_scan, pair_offsets, pair_images, P, M, owner,
                                                                                  creator_scan, pseg, seg_adj, kp_offsets, ids, pair_offsets_out, counts);
    GF_CHECK_LAUNCH();
    return GF_OK;
}
