// Covisibility clustering and unique 2-D - 3-D rows for sparse localisation: THE RULE, compiled by k_covis.hip for the device and by
// host/covis_host.cpp for the CPU.  Integer work only, so the two builds agree bit for bit whatever the order of execution.  hloc /
// pycolmap parity is UNPINNED (hloc's do_covisibility_clustering is not on hand); the rule is stated here.
//
// Inputs: kp_off [n + 1] (node of keypoint k of image i = kp_off[i] + k), the flat point_of_keypoint [n_nodes] (-1: none), obs_offsets
// [T + 1] and obs_image [N] of the points, the contributing pairs in pair order, the match rows ids [E, 2].
// A contributing pair is 8 int32 words: CV_Q the query's index, CV_QIMG its image, CV_DIMG the database image, CV_RB / CV_RE its rows of
// ids, CV_QCOL the column of ids that holds the query's keypoint, CV_POS the position of the database image in the query's list, one spare.
//
//  1. The database list of query q holds the images that share a pair with q (the query on either side).  An image in the list is not
//     itself a query and has at least one point.  The list is in order of first appearance in the pair list; an image's POSITION is its
//     index in this list.  More than CV_MAX_LIST images in one list is an error, never a wrapped index.  (Pair-level bookkeeping, on
//     the host in both builds: gf_covis_host_lists of host/covis_host.cpp, matcher._covis_tables in the package.)
//  2. Positions a and b of a list are linked iff some point has an observation in both images (obs_image over obs_offsets).
//     point_of_keypoint and the observation lists agree: a keypoint with point p is one of p's observations.
//  3. A cluster is a connected component of that graph on the list alone; a path through an image outside the list links nothing.  Its
//     label is its smallest position; the clusters of a query are numbered 0 .. C_q - 1 in ascending label order.  With clustering off
//     every position has cluster 0.  For a point it is enough to unite each listed observer with the FIRST listed observer of that point
//     (cv_point_star, run from the position that is that first observer: every point is walked once).
//  4. A row is (query keypoint, point id) of a contributing pair; a row whose database keypoint has no point is dropped.  A row's problem
//     is (query, cluster of its database image); problems are numbered query-major, then by cluster number: prob_base[q] + cluster.
//     Inside a problem rows keep pair order, then row order (cv_row).
//  5. With dedup a row whose (query keypoint, point id) occurred earlier in its problem is dropped and first_of[row] names that earlier
//     row; without, first_of[row] = row.  (first_of of a row dropped in step 4 is -1.)
//  6. p2d is the query keypoint, p3d the point rounded once to fp32.
//  7. One absolute-pose RANSAC per problem (gf_abspose_ransac, unchanged): N = the number of problems, K of the problem's query, the
//     draws keyed by the problem index.
//  8. The winner of a query is its valid problem with the most inliers, then the lowest cluster number (cv_select).  localized = a winner
//     exists and it has at least min_inliers inliers.
//  9. The mask byte of a row of the winning problem is the RANSAC inlier byte of first_of[row]; every other row's is 0 (cv_mask).
#ifndef GEOFORMER_COVIS_SPEC_H_
#define GEOFORMER_COVIS_SPEC_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define CV_HD __host__ __device__ inline
#else
#define CV_HD inline
#endif

#define CV_MAX_LIST 1024          /* positions of one query: its labels and sorted ids fit one workgroup's LDS */
#define CV_PAIR_WORDS 8
#define CV_Q 0
#define CV_QIMG 1
#define CV_DIMG 2
#define CV_RB 3
#define CV_RE 4
#define CV_QCOL 5
#define CV_POS 6
#define CV_FLAG_IMAGE_RANGE 1     /* status bits: a list or a pair names an image outside [0, n_images) */
#define CV_FLAG_KEYPOINT_RANGE 2  /* a match row names a keypoint its image does not have, or lies outside ids */
#define CV_FLAG_POINT_RANGE 4     /* point_of_keypoint names a point outside [0, T) */
#define CV_FLAG_LIST_RANGE 8      /* a list longer than CV_MAX_LIST, or a pair whose position lies outside its query's list */

struct CvView {
    const int32_t* kp_off;        // [n_images + 1]
    const int32_t* pok;           // [n_nodes]
    const int32_t* obs_offsets;   // [T + 1]
    const int32_t* obs_image;     // [n_obs]
    int n_images, n_nodes, T, n_obs;
};

CV_HD int cv_clamp(long v, long lo, long hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }

// the position of `image` among the L sorted ids of a list, -1 when it is not listed
CV_HD int cv_find_pos(const int32_t* sorted_img, const int32_t* sorted_pos, int L, int image) {
    int lo = 0, hi = L;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (sorted_img[mid] < image) lo = mid + 1; else hi = mid;
    }
    return lo < L && sorted_img[lo] == image ? sorted_pos[lo] : -1;
}

// Step 3 for keypoint `node` of the image at position a: when a is the first listed observer of the node's point, unite(a, b) for every
// other listed observer b.  Returns status bits.  Every index read from memory is clamped or checked before it is used.
template <class Unite>
CV_HD int cv_point_star(const CvView& v, const int32_t* sorted_img, const int32_t* sorted_pos, int L, int a, int node, Unite&& unite) {
    const int pt = v.pok[node];
    if (pt < 0) return 0;
    if (pt >= v.T) return CV_FLAG_POINT_RANGE;
    const int b = cv_clamp(v.obs_offsets[pt], 0, v.n_obs), e = cv_clamp(v.obs_offsets[pt + 1], b, v.n_obs);
    bool mine = false;
    for (int o = b; o < e; ++o) {
        const int pos = cv_find_pos(sorted_img, sorted_pos, L, v.obs_image[o]);
        if (pos < 0) continue;
        if (!mine) {
            if (pos != a) return 0;                                    // another position walks this point
            mine = true;
        } else if (pos != a) {
            unite(a, pos);
        }
    }
    return 0;
}

// Step 4 for row r of the contributing pairs (pair_row_off [C + 1]: the rows of pair c among all M0).  -> qnode (the query keypoint's
// node), pt, prob; returns keep (1: the row has a point).  Status bits through `flags`.
CV_HD int cv_row(const int32_t* pairs, const int32_t* pair_row_off, int C, const int32_t* ids, int E, const CvView& v, const int32_t* list_off,
                 const int32_t* cluster, int L_total, const int32_t* prob_base, int Q, int r, int& qnode, int& pt, int& prob, int& flags) {
    qnode = pt = prob = -1;
    int lo = 0, hi = C;                                                // the last pair whose first row is <= r
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (pair_row_off[mid] <= r) lo = mid; else hi = mid;
    }
    const int32_t* p = pairs + (long)CV_PAIR_WORDS * lo;
    const int q = p[CV_Q], qi = p[CV_QIMG], di = p[CV_DIMG], col = p[CV_QCOL];
    const long e = (long)p[CV_RB] + (r - pair_row_off[lo]);
    if (q < 0 || q >= Q || qi < 0 || qi >= v.n_images || di < 0 || di >= v.n_images) { flags |= CV_FLAG_IMAGE_RANGE; return 0; }
    if (e < 0 || e >= E || e >= p[CV_RE] || (col != 0 && col != 1)) { flags |= CV_FLAG_KEYPOINT_RANGE; return 0; }
    const int kq = ids[2 * e + col], kd = ids[2 * e + 1 - col];
    const long nq = (long)v.kp_off[qi] + kq, nd = (long)v.kp_off[di] + kd;
    if (kq < 0 || kd < 0 || nq >= v.kp_off[qi + 1] || nd >= v.kp_off[di + 1] || nq >= v.n_nodes || nd >= v.n_nodes || v.kp_off[qi] < 0 ||
        v.kp_off[di] < 0) {
        flags |= CV_FLAG_KEYPOINT_RANGE;
        return 0;
    }
    const long slot = (long)list_off[q] + p[CV_POS];
    if (p[CV_POS] < 0 || slot >= list_off[q + 1] || slot >= L_total || slot < 0) { flags |= CV_FLAG_LIST_RANGE; return 0; }
    const int x = v.pok[nd];
    if (x >= v.T) { flags |= CV_FLAG_POINT_RANGE; return 0; }
    qnode = (int)nq;
    prob = prob_base[q] + cluster[slot];
    if (x < 0) return 0;
    pt = x;
    return 1;
}

// Step 8 for the problems [b, e) of one query: the index of the winner, -1 when no problem is valid
CV_HD int cv_select(const int32_t* valid, const int32_t* n_inliers, int b, int e) {
    int win = -1;
    for (int k = b; k < e; ++k)
        if (valid[k] == 1 && (win < 0 || n_inliers[k] > n_inliers[win])) win = k;
    return win;
}

// Step 9: slot = the RANSAC row of first_of[row] (-1: the row was dropped in step 4)
CV_HD uint8_t cv_mask(const uint8_t* is_win, const uint8_t* inliers, int N, int M, int prob, int slot) {
    return (prob >= 0 && prob < N && slot >= 0 && slot < M && is_win[prob]) ? (uint8_t)(inliers[slot] != 0) : (uint8_t)0;
}

#endif /* GEOFORMER_COVIS_SPEC_H_ */
