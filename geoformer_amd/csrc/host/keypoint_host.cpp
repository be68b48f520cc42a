// TEST INFRASTRUCTURE and CPU reference: the whole keypoint consolidation, serially, over keypoint_spec.h (the text k_keypoints.hip
// compiles for the device), built by the host C++ compiler (geoformer_amd/build.py: -O2 -ffp-contract=off, no offload) into
// csrc/_obj/libkeypoint_host.so.  The tests compare the device path against it bit for bit; nothing in the package loads it.
// It keeps the reference's own structure (per image a dictionary cell -> centres, points taken in arrival order), not the device's
// sort-and-walk decomposition, so agreement between the two checks the decomposition as well as the arithmetic.
#include <stdint.h>

#include <map>
#include <unordered_map>
#include <vector>

#include "../keypoint_spec.h"

namespace {

struct Centre {
    float x, y;
    int kid;
};
struct Image {
    std::vector<float> kps;                                  // x, y per keypoint, in id order
    std::map<int64_t, std::vector<Centre>> cells;            // quantised mode
    std::map<int64_t, int> exact;                            // exact mode: coordinate bits -> id
};

void filter_pass(const int* ids, const float* scores, const int* rows, int n, unsigned char* keep) {
    std::unordered_map<int, uint64_t> best[2];
    for (int k = 0; k < n; ++k) {
        const uint64_t key = kp_winner_key(scores[k], (uint32_t)rows[k]);
        for (int s = 0; s < 2; ++s) {
            auto it = best[s].find(ids[2 * k + s]);
            if (it == best[s].end()) best[s].emplace(ids[2 * k + s], key);
            else if (key > it->second) it->second = key;
        }
    }
    for (int k = 0; k < n; ++k) {
        const uint64_t key = kp_winner_key(scores[k], (uint32_t)rows[k]);
        keep[k] = best[0][ids[2 * k]] == key && best[1][ids[2 * k + 1]] == key;
    }
}

}   // namespace

extern "C" {

float gf_keypoint_host_cell(float x, float psize) { return kp_cell(x, psize); }

// one pass of the uniqueness filter over n id rows of one pair (row k counts as row index k): keep[k] = 1 for the rows that stay
int gf_keypoint_host_filter(const int* ids, const float* scores, int n, unsigned char* keep) {
    if (n < 0 || (n > 0 && (!ids || !scores || !keep))) return -1;
    std::vector<int> rows(n);
    for (int k = 0; k < n; ++k) rows[k] = k;
    filter_pass(ids, scores, rows.data(), n, keep);
    return 0;
}

// matches [M][4] (x0, y0, x1, y1), scores [M], pair_offsets [P + 1] (rows of pair q: pair_offsets[q] .. pair_offsets[q + 1], M = the last
// entry), pair_images [P][2].  Outputs, caller-owned: keypoints [2 M][2] (image-major, K rows used), kp_offsets [n_images + 1], ids [M][2]
// (per-image keypoint indices, M' rows used, in row order), pair_offsets_out [P + 1].  stats: NULL or 8 words - status flags
// (KP_FLAG_*), surviving points, groups, longest group, most centres in a group, rows dropped by the filter, K, M'.
// psize <= 0 or dthres <= 0 is the exact mode (compute_keypoints; `unique` is ignored there, as in the reference).
// Returns 0, or -1 for an argument outside the supported range (keypoint_spec.h).
int gf_keypoint_host_consolidate(const float* matches, const float* scores, const int* pair_offsets, const int* pair_images, int P, int n_images,
                                 float sc_thres, float psize, float dthres, int unique, float* keypoints, int* kp_offsets, int* ids,
                                 int* pair_offsets_out, long long* stats) {
    if (P < 0 || n_images < 0 || n_images > KP_MAX_IMAGES || !pair_offsets || !kp_offsets || !pair_offsets_out) return -1;
    const bool quant = psize > 0.f && dthres > 0.f;
    if (quant && !(kp_finite(psize) && psize > KP_MIN_PSIZE)) return -1;
    if (pair_offsets[0] != 0) return -1;
    for (int q = 0; q < P; ++q)
        if (pair_offsets[q + 1] < pair_offsets[q]) return -1;
    const int M = pair_offsets[P];
    if (M > 0 && (!matches || !scores || !keypoints || !ids)) return -1;
    if (P > 0 && !pair_images) return -1;
    std::vector<Image> images(n_images);
    long long flags = 0, points = 0, longest = 0, most = 0, dropped = 0;
    std::map<std::pair<int, int64_t>, long long> group_len;
    int out = 0;
    std::vector<int> pid, rows;
    std::vector<float> psc;
    std::vector<unsigned char> keep;
    for (int q = 0; q < P; ++q) {
        pair_offsets_out[q] = out;
        const int b = pair_offsets[q], e = pair_offsets[q + 1];
        const int im[2] = {pair_images[2 * q], pair_images[2 * q + 1]};
        if (im[0] < 0 || im[0] >= n_images || im[1] < 0 || im[1] >= n_images) {
            if (e > b) flags |= KP_FLAG_IMAGE_RANGE;
            continue;
        }
        rows.clear();
        for (int r = b; r < e; ++r) {
            const float* m = matches + 4 * (size_t)r;
            if (!kp_row_valid(m, scores[r], sc_thres)) continue;
            if (quant && !(kp_coord_in_range(m[0]) && kp_coord_in_range(m[1]) && kp_coord_in_range(m[2]) && kp_coord_in_range(m[3]))) {
                flags |= KP_FLAG_COORD_RANGE;
                continue;
            }
            rows.push_back(r);
        }
        const int n = (int)rows.size();
        pid.assign(2 * (size_t)n, 0);
        psc.resize(n);
        for (int s = 0; s < 2; ++s) {
            Image& I = images[im[s]];
            for (int k = 0; k < n; ++k) {
                const float px = matches[4 * (size_t)rows[k] + 2 * s], py = matches[4 * (size_t)rows[k] + 2 * s + 1];
                ++points;
                int kid;
                if (!quant) {
                    const int64_t key = kp_exact_key(px, py);
                    ++group_len[{im[s], key}];
                    auto it = I.exact.find(key);
                    if (it == I.exact.end()) {
                        kid = (int)(I.kps.size() / 2);
                        I.kps.push_back(px), I.kps.push_back(py);
                        I.exact.emplace(key, kid);
                    } else {
                        kid = it->second;
                    }
                } else {
                    const int64_t key = kp_cell_key(im[s], px, py, psize);
                    ++group_len[{im[s], key}];
                    std::vector<Centre>& cs = I.cells[key];
                    int best = -1;
                    float best_d = 0.f;
                    for (int j = 0; j < (int)cs.size(); ++j) {
                        const float d = kp_distance(px, py, cs[j].x, cs[j].y);
                        if (best < 0 || kp_closer(d, j, best_d, best)) best = j, best_d = d;
                    }
                    if (best >= 0 && best_d < dthres) {
                        kp_merge(cs[best].x, cs[best].y, px, py);
                        kid = cs[best].kid;
                        I.kps[2 * (size_t)kid] = cs[best].x, I.kps[2 * (size_t)kid + 1] = cs[best].y;
                    } else {
                        kid = (int)(I.kps.size() / 2);
                        I.kps.push_back(px), I.kps.push_back(py);
                        cs.push_back(Centre{px, py, kid});
                        if ((long long)cs.size() > most) most = (long long)cs.size();
                    }
                }
                pid[2 * (size_t)k + s] = kid;
            }
        }
        keep.assign(n, 1);
        if (quant && unique && n > 0) {
            for (int k = 0; k < n; ++k) psc[k] = scores[rows[k]];
            filter_pass(pid.data(), psc.data(), rows.data(), n, keep.data());
        }
        for (int k = 0; k < n; ++k) {
            if (!keep[k]) {
                ++dropped;
                continue;
            }
            ids[2 * (size_t)out] = pid[2 * (size_t)k], ids[2 * (size_t)out + 1] = pid[2 * (size_t)k + 1];
            ++out;
        }
    }
    pair_offsets_out[P] = out;
    int K = 0;
    for (int i = 0; i < n_images; ++i) {
        kp_offsets[i] = K;
        for (size_t k = 0; k < images[i].kps.size(); ++k) keypoints[2 * (size_t)K + k] = images[i].kps[k];
        K += (int)(images[i].kps.size() / 2);
    }
    kp_offsets[n_images] = K;
    if (!quant) most = group_len.empty() ? 0 : 1;
    for (auto& g : group_len)
        if (g.second > longest) longest = g.second;
    if (stats) {
        stats[0] = flags, stats[1] = points, stats[2] = (long long)group_len.size(), stats[3] = longest, stats[4] = most, stats[5] = dropped;
        stats[6] = K, stats[7] = out;
    }
    return 0;
}

}   // extern "C"
