"""The structure-from-motion library behind the matcher: what happens to the pair matches of `GeoFormerMatcher.match_many` after matching.

  * `consolidate_matches`                                  keypoints and match ids per image (process_matches_and_keypoints_exporth5)
  * `verify_matches`, `relative_poses`                     two-view verification without and with intrinsics
  * `undistort_results`, `undistort_points`                lens distortion removed before any geometry
  * `localize_queries`, `localize_queries_sparse`          camera poses of queries against 3-D maps / triangulated points
  * `triangulate`, `refine`                                points from known poses, bundle adjustment
  * the result types and the file formats that belong to them: intrinsics, cameras, poses, the consolidated directory, triangulated points

Every stage runs on the device with one upload and one read back.  Both go through the two helpers at the top of this file: `_upload`
packs numpy arrays into one block of 32-bit words and returns one device view per array, `_download` concatenates device tensors into one
block of bytes and returns one numpy view per tensor.  No stage computes an offset into either block.  The module imports `ops`, numpy and
torch only; `matcher` imports its names back, so `geoformer_amd.matcher.<name>` resolves as before and the command line stays there.
"""
import math
import os
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import ops


# ---------------------------------------------------------------------------------------------
# the one packed transfer of every stage
# ---------------------------------------------------------------------------------------------
_DEVICE_DTYPE = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32, np.dtype(np.float64): torch.float64,
                 np.dtype(np.int64): torch.int64}
_HOST_DTYPE = {torch.float32: (np.float32, 4), torch.int32: (np.int32, 4), torch.float64: (np.float64, 8), torch.int64: (np.int64, 8),
               torch.uint8: (np.uint8, 1), torch.bool: (np.bool_, 1)}                    # and the bytes of an element


def _upload(device, *items):
    """numpy arrays -> one device view per item, with the item's dtype and shape, after ONE host-to-device copy: the items are laid out
    in the order given as one block of 32-bit words.  An item is an array (float32, int32, float64 or int64; anything else is a
    TypeError - a caller widens flags to int32 itself) or a non-empty list of arrays of one dtype that agree in all but their first axis:
    the list is one item, its arrays joined along the first axis, without a concatenated copy on the host.  The alignment rule lives here:
    an 8-byte item starts on an even word, one padding word is inserted where it would not (none with the 8-byte items first, the order
    every stage uses).  Every array is copied once, straight into its place in the block, contiguous or not; a zero-size item gives a
    zero-size view.  `torch.from_numpy` is looked up when called and no device context is entered: device='cpu' works."""
    spans, pads, o = [], [], 0
    for item in items:
        joined = isinstance(item, list)
        first = item[0] if joined else item
        dtype = first.dtype
        device_dtype = _DEVICE_DTYPE.get(dtype)
        if device_dtype is None or (joined and any(p.dtype is not dtype and p.dtype != dtype for p in item)):
            raise TypeError(f'_upload: float32, int32, float64 or int64 arrays, one dtype per item; got '
                            f'{sorted({str(p.dtype) for p in (item if joined else [item])})}')
        shape = (sum(map(len, item)),) + first.shape[1:] if joined else first.shape
        n = math.prod(shape)
        if dtype.itemsize == 8:
            n *= 2
            if o % 2:
                pads.append(o)
                o += 1
        spans.append((o, o + n, dtype, device_dtype, shape))
        o += n
    block = np.empty(o, np.int32)
    if pads:
        block[pads] = 0
    for item, (b, e, dtype, _, shape) in zip(items, spans):
        if e > b:
            dst = block[b:e].view(dtype).reshape(shape)
            if isinstance(item, list):
                np.concatenate(item, out=dst)
            else:
                dst[...] = item
    d = torch.from_numpy(block).to(device)
    return tuple(d[b:e].view(dtype).view(shape) if e > b else d.new_empty(shape, dtype=dtype) for b, e, _, dtype, shape in spans)


def _download(*tensors):
    """Device tensors (float32, int32, float64, int64, uint8 or bool) -> one numpy array per tensor, with the tensor's dtype and shape, after
    ONE device-to-host copy of their concatenated bytes.  The arrays are views of that one block: a stage copies what leaves it in its
    result (`.copy()`, or a conversion such as `.astype(bool)`), so that no result keeps the block alive."""
    block = torch.cat([x.reshape(-1).view(torch.uint8) for x in tensors]).cpu().numpy()
    out, o = [], 0
    for x in tensors:
        dtype, size = _HOST_DTYPE[x.dtype]
        shape = tuple(x.shape)
        n = math.prod(shape) * size
        out.append(block[o:o + n].view(dtype).reshape(shape))
        o += n
    return tuple(out)


def _row_offsets(rows):
    """int32 [len(rows) + 1]: where each array of the list starts in their concatenation."""
    return np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)


def _pair_rows(what, pairs, results):
    """The rows of the pair stages: per pair the [n, 4] float32 matches (element 0 of a match_many tuple) and the [n] float32 scores
    (element 3), and the int32 [P + 1] offsets of the pairs in their concatenation.  `what` names the stage in the errors."""
    if len(pairs) != len(results):
        raise ValueError(f'{what}: {len(pairs)} pairs but {len(results)} results')
    ms = [np.asarray(r[0], dtype=np.float32).reshape(-1, 4) for r in results]
    ss = [np.asarray(r[3], dtype=np.float32).reshape(-1) for r in results]
    if any(len(m) != len(s) for m, s in zip(ms, ss)):
        raise ValueError(f'{what}: a result whose matches and scores differ in length')
    return ms, ss, _row_offsets(ms)


def _verified_masks(valid, n_inliers, min_inliers, inliers, offsets, owner=None):
    """(verified, masks) of a RANSAC over problems: verified[k] = a model was found and it has at least min_inliers inliers; masks[g] =
    the inlier flags of row group g (offsets[g] : offsets[g + 1]) where the problem of the group, owner[g] (default: g), is verified, all
    False otherwise."""
    verified = (valid == 1) & (n_inliers >= min_inliers)
    off, ok = np.asarray(offsets).tolist(), verified.tolist()
    owner = range(len(off) - 1) if owner is None else owner
    return verified, [inliers[b:e].copy() if ok[k] else np.zeros(e - b, bool) for b, e, k in zip(off, off[1:], owner)]


def _absolute_poses(rs):
    """The dict of ops.ransac_absolute_pose, read back once -> (R [N,3,3], t [N,3], valid, n_inliers, rounds [N], inliers bool [M])."""
    R, t, valid, nin, rounds, inl = _download(*(rs[k] for k in ('R', 't', 'valid', 'n_inliers', 'rounds', 'inliers')))
    return R.copy(), t.copy(), valid, nin.copy(), rounds.copy(), inl.astype(bool)


# ---------------------------------------------------------------------------------------------
# keypoints and match ids for SfM from pair matches (process_matches_and_keypoints_exporth5 of localize_sfm_helper.py, on the device)
# ---------------------------------------------------------------------------------------------
class ConsolidatedMatches(NamedTuple):
    names: list              # image paths in order of first appearance in the pair list
    keypoints: list          # per image: [K_i, 2] float32
    pair_images: np.ndarray  # [P, 2] int32: indices into names
    matches: list            # per pair: [n_p, 2] int32 keypoint indices (into keypoints[pair_images[p, 0]], keypoints[pair_images[p, 1]])


def consolidate_matches(pairs, results, sc_thres=0.25, qt_psize=48, qt_dthres=4, qt_unique=True, device='cuda', keep=None):
    """[(path0, path1), ...] and the tuples match_many returned for them (either return convention: element 0 is the [n, 4] matches,
    element 3 the scores) -> ConsolidatedMatches: what COLMAP-style triangulation and localisation consume - one keypoint list per image
    and every match as two keypoint indices.  The reference's process_matches_and_keypoints_exporth5 with its defaults: matches scoring
    below sc_thres are dropped, keypoints of an image closer than qt_dthres inside one qt_psize cell are merged into their running midpoint
    (a detector-free matcher never returns the same sub-pixel point twice: without merging every track has length two), and with qt_unique
    a keypoint keeps only its best match per pair.  qt_psize <= 0 or qt_dthres <= 0: keypoints are merged only where coordinates are equal.
    Matches are taken as float32 (match_many's upscaled float64 is cast first; the reference stores float32 keypoints anyway).  One upload,
    ops.consolidate_keypoints on the device, bit-identical to the serial rule (csrc/keypoint_spec.h).  A pair without surviving rows gives
    [0, 2]; a pair listed twice contributes twice, as in the reference.
    keep: one boolean mask per pair (verify_matches(...).masks): only the rows it marks enter - the result is that of the same call on lists
    with the other rows removed beforehand."""
    pairs = [tuple(p) for p in pairs]
    ms, ss, offsets = _pair_rows('consolidate_matches', pairs, results)
    if keep is not None and len(keep) != len(pairs):
        raise ValueError(f'consolidate_matches: {len(pairs)} pairs but {len(keep)} masks')
    index = {}
    pair_images = np.array([[index.setdefault(path, len(index)) for path in p] for p in pairs], np.int32).reshape(-1, 2)
    if keep is not None:
        ks = [np.asarray(k, dtype=bool).reshape(-1) for k in keep]
        if any(len(k) != len(m) for k, m in zip(ks, ms)):
            raise ValueError('consolidate_matches: a mask whose length is not its pair\'s number of matches')
        ms, ss = [m[k] for m, k in zip(ms, ks)], [x[k] for x, k in zip(ss, ks)]
        offsets = _row_offsets(ms)
    with torch.cuda.device(device):
        matches, scores, off, pim = _upload(device, ms or [np.zeros((0, 4), np.float32)], ss or [np.zeros(0, np.float32)], offsets, pair_images)
        kp, kpo, ids, ido = _download(*ops.consolidate_keypoints(matches, scores, off, pim, len(index), sc_thres, qt_psize, qt_dthres, qt_unique))
    return ConsolidatedMatches(list(index), [kp[kpo[i]:kpo[i + 1]].copy() for i in range(len(index))], pair_images,
                               [ids[ido[q]:ido[q + 1]].copy() for q in range(len(pairs))])


# ---------------------------------------------------------------------------------------------
# two-view geometric verification without intrinsics: a fundamental-matrix RANSAC per pair, all pairs in one call on the device
# ---------------------------------------------------------------------------------------------
class VerifiedMatches(NamedTuple):
    F: np.ndarray            # [P, 3, 3] float64, x1^T F x0 = 0 in pixels, Frobenius norm 1 (zeros where RANSAC found no model)
    n_inliers: np.ndarray    # [P] int32
    verified: np.ndarray     # [P] bool: a model was found and it has at least min_inliers inliers
    masks: list              # per pair: [n_p] bool, the inliers of a verified pair; all False otherwise
    rounds: np.ndarray       # [P] int32: refits on the inliers accepted per pair (zeros without refit)


def verify_matches(pairs, results, thr=1.0, min_inliers=15, sc_thres=0.25, iters=None, device='cuda', refit=0):
    """Geometric verification of the matches of every pair, for image sets without poses or intrinsics: a detector-free matcher returns
    confident-looking matches for pairs that show different scenes, and a track should only see matches that one epipolar geometry
    explains.  Per pair a fundamental-matrix RANSAC (ops.ransac_fundamental: rows scoring below sc_thres or not finite take no part,
    seven-point hypotheses, squared Sampson distance below thr^2 pixels; the rule is csrc/fund_solver.h) - one upload, three launches for
    all pairs, one read back.  verified[p] = a model was found and n_inliers[p] >= min_inliers.  refit = R in 1 .. 8: one more launch
    refits every winner on its inliers up to R times (normalised eight-point fit, rank 2, inliers selected again; never fewer inliers
    than before); F, n_inliers, verified and masks are then the refined model's and rounds counts the accepted refits.  No
    planar-degeneracy test: the F of a planar scene is valid but arbitrary, its inlier set is still the plane's.  pairs / results as
    consolidate_matches takes them."""
    ms, ss, offsets = _pair_rows('verify_matches', pairs, results)
    P = len(results)
    if P == 0:
        return VerifiedMatches(np.zeros((0, 3, 3)), np.zeros(0, np.int32), np.zeros(0, bool), [], np.zeros(0, np.int32))
    with torch.cuda.device(device):
        matches, scores, off = _upload(device, ms, ss, offsets)
        rs = ops.ransac_fundamental(matches, scores, off, P, pixel_thr=thr, sc_thres=sc_thres,
                                    iters=ops.FUND_RANSAC_ITERS if iters is None else iters, refit=refit)
        if not refit:
            rs['rounds'] = torch.zeros(P, dtype=torch.int32, device=rs['valid'].device)
        F, valid, nin, rounds, inl = _download(*(rs[k] for k in ('F', 'valid', 'n_inliers', 'rounds', 'inliers')))
    verified, masks = _verified_masks(valid, nin, min_inliers, inl.astype(bool), offsets)
    return VerifiedMatches(F.copy(), nin.copy(), verified, masks, rounds.copy())


# ---------------------------------------------------------------------------------------------
# calibrated two-view verification: an essential-matrix RANSAC with pose recovery per pair, all pairs in one call on the device
# ---------------------------------------------------------------------------------------------
class RelativePoses(NamedTuple):
    E: np.ndarray            # [P, 3, 3] float64, x1^T E x0 = 0 in normalised coordinates, Frobenius norm 1 (zeros where no pose was found)
    R: np.ndarray            # [P, 3, 3] float64, x1 ~ R x0 + t
    t: np.ndarray            # [P, 3] float64, unit length (the scale of a relative pose is not observable)
    n_inliers: np.ndarray    # [P] int32
    verified: np.ndarray     # [P] bool: a pose was found and it has at least min_inliers inliers
    masks: list              # per pair: [n_p] bool, the inliers of a verified pair; all False otherwise
    rounds: np.ndarray       # [P] int32: refits on the inliers accepted per pair (zeros without refit)


def relative_poses(pairs, results, intrinsics, thr=1.0, min_inliers=15, sc_thres=0.25, iters=None, device='cuda', refit=0):
    """The relative pose of every pair from its matches, for image sets with known intrinsics: where K is known a fundamental matrix is
    the wrong model - two degrees of freedom too many, and no R, t.  Per pair an essential-matrix RANSAC with pose recovery
    (ops.ransac_relative_pose: rows scoring below sc_thres or not finite take no part, five-point hypotheses on normalised coordinates,
    squared Sampson distance below (thr / mean focal length)^2, the pose by the inliers' cheirality votes; the rule is
    csrc/rel_solver.h) - one upload, four launches for all pairs, one read back.  intrinsics[path]: 3 x 3 K of the image, in the pixels of
    the matches (what localize_queries takes and undistort_results returns); a pair whose image has no entry is a ValueError.
    verified[p] = a pose was found and n_inliers[p] >= min_inliers; verified and masks mean what they mean in VerifiedMatches, so
    consolidate_matches(..., keep=rp.masks) works unchanged.  refit = R in 1 .. 8: one more launch refits every pose on its inliers up to
    R times (Gauss-Newton on the Sampson residual over R and unit t, inliers selected again; never fewer inliers than before); E, R, t,
    n_inliers, verified and masks are then the refined model's and rounds counts the accepted refits.  On a purely planar scene the
    essential matrix has a twin solution and either may be returned; there is no homography model test.  pairs / results as
    consolidate_matches takes them."""
    pairs = [tuple(p) for p in pairs]
    ms, ss, offsets = _pair_rows('relative_poses', pairs, results)
    for p in pairs:
        for path in p:
            if path not in intrinsics:
                raise ValueError(f'relative_poses: no intrinsics for {path!r}')
    P = len(results)
    if P == 0:
        return RelativePoses(np.zeros((0, 3, 3)), np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros(0, bool), [],
                             np.zeros(0, np.int32))
    Ks = np.stack([np.stack([np.asarray(intrinsics[path], dtype=np.float32).reshape(3, 3) for path in p]) for p in pairs])      # [P, 2, 3, 3]
    with torch.cuda.device(device):
        matches, scores, off, K0, K1 = _upload(device, ms, ss, offsets, Ks[:, 0], Ks[:, 1])
        rs = ops.ransac_relative_pose(matches, scores, off, P, K0, K1, pixel_thr=thr, sc_thres=sc_thres,
                                      iters=ops.REL_RANSAC_ITERS if iters is None else iters, refit=refit)
        if not refit:
            rs['rounds'] = torch.zeros(P, dtype=torch.int32, device=rs['valid'].device)
        E, R, t, valid, nin, rounds, inl = _download(*(rs[q] for q in ('E', 'R', 't', 'valid', 'n_inliers', 'rounds', 'inliers')))
    verified, masks = _verified_masks(valid, nin, min_inliers, inl.astype(bool), offsets)
    return RelativePoses(E.copy(), R.copy(), t.copy(), nin.copy(), verified, masks, rounds.copy())


# ---------------------------------------------------------------------------------------------
# localisation: a camera pose per query from its matches against database images with known 3-D points, all queries in one call
# ---------------------------------------------------------------------------------------------
class LocalizedQueries(NamedTuple):
    names: list              # the queries, in order of first appearance in the pair list
    R: np.ndarray            # [Q, 3, 3] float64, x_cam = R X + t in world units (zeros where RANSAC found no model)
    t: np.ndarray            # [Q, 3] float64
    n_inliers: np.ndarray    # [Q] int32
    localized: np.ndarray    # [Q] bool: a model was found and it has at least min_inliers inliers
    masks: list              # per PAIR: [n_p] bool, the inliers of a localised query's pair; all False otherwise
    rounds: np.ndarray       # [Q] int32: refits on the inliers accepted per query (zeros without refit)
    # localize_queries_sparse with covis_cluster or dedup (None otherwise):
    n_clusters: Optional[np.ndarray] = None   # [Q] int32: covisibility clusters of the query's database images (1 with clustering off, 0: no image)
    cluster: Optional[np.ndarray] = None      # [Q] int32: the number of the winning cluster, -1 if there is none
    db_names: Optional[list] = None           # per query: its database images, in order of first appearance in the pair list
    db_cluster: Optional[list] = None         # per query: int32 array, the cluster of each entry of db_names
    cluster_inliers: Optional[list] = None    # per query: int32 [C_q], the inliers of each cluster's pose (0: RANSAC found no model)


def localize_queries(pairs, results, intrinsics, xyz_maps, thr=12.0, min_inliers=12, sc_thres=0.25, iters=None, device='cuda', refit=0):
    """Camera poses of query images from their matches against database images whose pixels have known 3-D points - the step the
    reference's eval_aachen / eval_robotcar / eval_inloc leave to hloc and pycolmap.  pairs: (query, database) paths, results: what
    match_many returned for them (matches [n, 4] = query x, y, database x, y; scores).  intrinsics[query]: 3 x 3 K of the query in the
    coordinates of its matches.  xyz_maps[database]: float32 [H, W, 3] array (NaN: no 3-D point) or the path of a .npy holding one, in
    the coordinates of the database keypoints; each map is uploaded once.  Every database keypoint gets its 3-D point by bilinear lookup
    (ops.xyz_lookup), all pairs of a query form one problem in pair order, and one absolute-pose RANSAC per query follows
    (ops.ransac_absolute_pose: P3P hypotheses, reprojection error below thr pixels; the rule is csrc/abs_solver.h) - one upload, the
    lookup, three launches (four with refit) for all queries, one read back.  localized[q] = a model was found and n_inliers[q] >=
    min_inliers.  No covisibility clustering; no distortion parameters here: undistort_results removes lens distortion from the matches
    beforehand."""
    ms, ss, _ = _pair_rows('localize_queries', pairs, results)
    P = len(results)
    names, qidx = [], {}
    for q, _ in pairs:
        if q not in qidx:
            qidx[q] = len(names)
            names.append(q)
    Q = len(names)
    if P == 0:
        return LocalizedQueries([], np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros(0, bool), [], np.zeros(0, np.int32))
    missing = [q for q in names if q not in intrinsics] + [d for _, d in pairs if d not in xyz_maps]
    if missing:
        raise ValueError(f'localize_queries: no intrinsics / 3-D map for {missing[0]!r}')
    order = sorted(range(P), key=lambda p: qidx[pairs[p][0]])          # stable: a query's pairs stay in pair order
    owner = [qidx[pairs[p][0]] for p in order]
    pair_off = _row_offsets([ms[p] for p in order])
    query_off = np.concatenate([[0], np.cumsum(np.bincount(owner, weights=np.diff(pair_off), minlength=Q))]).astype(np.int32)
    Ks = np.stack([np.asarray(intrinsics[q], dtype=np.float32).reshape(9) for q in names])
    with torch.cuda.device(device):
        dmaps = {}
        for _, dname in pairs:
            if dname not in dmaps:
                m = xyz_maps[dname]
                m = np.load(m) if isinstance(m, (str, os.PathLike)) else np.asarray(m)
                if m.ndim != 3 or m.shape[2] != 3:
                    raise ValueError(f'localize_queries: the 3-D map of {dname!r} has shape {m.shape}, expected [H, W, 3]')
                dmaps[dname] = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).to(device)
        table = np.array([[dmaps[pairs[p][1]].data_ptr(), dmaps[pairs[p][1]].shape[0] | (dmaps[pairs[p][1]].shape[1] << 32)] for p in order],
                         dtype=np.int64)
        # one upload: the query side and the database side of the rows, in the order of the problems
        tab, p2d, pdb, sc, poff, qoff, Kd = _upload(device, table, [ms[p][:, :2] for p in order], [ms[p][:, 2:] for p in order],
                                                    [ss[p] for p in order], pair_off, query_off, Ks)
        p3d = ops.xyz_lookup(tab, poff, pdb)
        rs = ops.ransac_absolute_pose(p2d, p3d, sc, qoff, Q, Kd, pixel_thr=thr, sc_thres=sc_thres,
                                      iters=ops.ABS_RANSAC_ITERS if iters is None else iters, refit=refit)
        R, t, valid, nin, rounds, inl = _absolute_poses(rs)
        del dmaps
    localized, sorted_masks = _verified_masks(valid, nin, min_inliers, inl, pair_off, owner)
    masks = [None] * P
    for k, p in enumerate(order):
        masks[p] = sorted_masks[k]
    return LocalizedQueries(names, R, t, nin, localized, masks, rounds)


def rotation_to_quaternion(R):
    """(qw, qx, qy, qz) of a rotation matrix, qw >= 0 - the convention of the localisation benchmarks' submission files."""
    R = np.asarray(R, dtype=np.float64)
    k = np.array([[R[0, 0] - R[1, 1] - R[2, 2], 0, 0, 0],
                  [R[0, 1] + R[1, 0], R[1, 1] - R[0, 0] - R[2, 2], 0, 0],
                  [R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], R[2, 2] - R[0, 0] - R[1, 1], 0],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    w, v = np.linalg.eigh(k)                                          # the eigenvector of the largest eigenvalue: (x, y, z, w)
    q = v[[3, 0, 1, 2], np.argmax(w)]
    return q if q[0] >= 0 else -q


def read_intrinsics(path):
    """One line per query: `path fx fy cx cy` (blank lines and '#' lines are skipped; a relative path is relative to the file) ->
    {path: 3 x 3 K}."""
    base = os.path.dirname(os.path.abspath(path))
    out = {}
    with open(path) as f:
        for no, line in enumerate(f, 1):
            parts = line.split()
            if not parts or parts[0].startswith('#'):
                continue
            if len(parts) != 5:
                raise ValueError(f'{path}:{no}: expected `path fx fy cx cy`, got {len(parts)} fields')
            fx, fy, cx, cy = (float(v) for v in parts[1:])
            name = parts[0] if os.path.isabs(parts[0]) else os.path.normpath(os.path.join(base, parts[0]))
            out[name] = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    return out


def write_intrinsics(path, intrinsics, names=None):
    """The inverse of read_intrinsics: one line `name fx fy cx cy` per entry of `names` (default: every key), names as they are."""
    with open(path, 'w') as f:
        for name in (intrinsics if names is None else names):
            K = np.asarray(intrinsics[name], dtype=np.float64)
            f.write(' '.join([name] + [repr(float(v)) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2])]) + '\n')


# ---------------------------------------------------------------------------------------------
# lens distortion: the match coordinates of real cameras are undistorted once, on the device, before any geometry runs
# ---------------------------------------------------------------------------------------------
CAMERA_MODELS = {'SIMPLE_PINHOLE': 3, 'PINHOLE': 4, 'SIMPLE_RADIAL': 4, 'RADIAL': 5, 'OPENCV': 8}     # COLMAP's names -> number of parameters


class Camera(NamedTuple):
    model: str               # a key of CAMERA_MODELS
    width: int
    height: int
    params: tuple            # COLMAP's order: f | fx fy, then cx cy, then the model's distortion terms


def canonical_camera(camera):
    """The canonical record (fx, fy, cx, cy, k1, k2, p1, p2) of csrc/camera_spec.h for a Camera of any supported model."""
    model, p = camera.model, tuple(float(v) for v in camera.params)
    if model not in CAMERA_MODELS:
        raise ValueError(f'camera model {model!r} is not supported (supported: {", ".join(CAMERA_MODELS)})')
    if len(p) != CAMERA_MODELS[model]:
        raise ValueError(f'{model} takes {CAMERA_MODELS[model]} parameters, got {len(p)}')
    if model in ('PINHOLE', 'OPENCV'):
        return p + (0.0,) * (8 - len(p))
    return (p[0], p[0], p[1], p[2]) + p[3:] + (0.0,) * (7 - len(p))


def read_cameras(path):
    """hloc's query-list lines: `path MODEL W H params...` with COLMAP's model names and parameter order (SIMPLE_PINHOLE f cx cy; PINHOLE
    fx fy cx cy; SIMPLE_RADIAL f cx cy k; RADIAL f cx cy k1 k2; OPENCV fx fy cx cy k1 k2 p1 p2).  Blank lines and '#' lines are skipped; a
    relative path is relative to the file -> {path: Camera}.  An unknown model, a wrong number of parameters, a value that is not finite
    or a focal length that is not positive is a ValueError naming file and line."""
    base = os.path.dirname(os.path.abspath(path))
    out = {}
    with open(path) as f:
        for no, line in enumerate(f, 1):
            parts = line.split()
            if not parts or parts[0].startswith('#'):
                continue
            if len(parts) < 4:
                raise ValueError(f'{path}:{no}: expected `path MODEL W H params...`, got {len(parts)} fields')
            model = parts[1]
            if model not in CAMERA_MODELS:
                raise ValueError(f'{path}:{no}: unknown camera model {model!r} (supported: {", ".join(CAMERA_MODELS)})')
            if len(parts) - 4 != CAMERA_MODELS[model]:
                raise ValueError(f'{path}:{no}: {model} takes {CAMERA_MODELS[model]} parameters, got {len(parts) - 4}')
            try:
                w, h = int(parts[2]), int(parts[3])
                params = tuple(float(v) for v in parts[4:])
            except ValueError:
                raise ValueError(f'{path}:{no}: W and H must be integers and the parameters numbers') from None
            if not all(math.isfinite(v) for v in params):
                raise ValueError(f'{path}:{no}: a parameter that is not finite')
            if not all(v > 0 for v in params[:2 if model in ('PINHOLE', 'OPENCV') else 1]):
                raise ValueError(f'{path}:{no}: a focal length that is not positive')
            name = parts[0] if os.path.isabs(parts[0]) else os.path.normpath(os.path.join(base, parts[0]))
            out[name] = Camera(model, w, h, params)
    return out


def write_cameras(path, cameras):
    """The inverse of read_cameras: one line per camera; a name under the file's directory is written relative to it."""
    base = os.path.dirname(os.path.abspath(path))
    with open(path, 'w') as f:
        for name, cam in cameras.items():
            canonical_camera(cam)                                          # (the model and its parameter count)
            full = os.path.abspath(name)
            shown = os.path.relpath(full, base) if full.startswith(base + os.sep) else full
            f.write(' '.join([shown, cam.model, str(int(cam.width)), str(int(cam.height))] + [repr(float(v)) for v in cam.params]) + '\n')


def pinhole_of(cameras):
    """{name: Camera} -> {name: 3 x 3 K}: the intrinsics that hold for undistorted coordinates (what read_intrinsics returns)."""
    out = {}
    for name, cam in cameras.items():
        fx, fy, cx, cy = canonical_camera(cam)[:4]
        out[name] = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    return out


class UndistortedResults(list):
    """The list undistort_results returns, with n_failed int32 [P] (rows of a pair with a side that has no pre-image) and status (per
    pair: uint8 [n_p, 2], the status byte of each side of each row: 0 fine, 1 non-finite input, 2 no pre-image)."""
    n_failed = None
    status = None


def _original_pixel_rows(results):
    """[n, 4] float32 matches in the pixels of the original images for either return convention of match_many: the four-element tuple
    holds them, the five-element one (no_match_upscale) holds resized coordinates and, as element 4, the factors that scale them back."""
    return [np.ascontiguousarray((np.asarray(r[0], dtype=np.float64).reshape(-1, 4) * np.asarray(r[4], dtype=np.float64).reshape(1, 4)
                                  if len(r) > 4 else np.asarray(r[0])).astype(np.float32).reshape(-1, 4)) for r in results]


def undistort_results(pairs, results, cameras, device='cuda'):
    """[(path0, path1), ...], the tuples match_many returned for them (either return convention) and {path: Camera} -> (results',
    intrinsics): the same tuples with every coordinate replaced by the pixel of an ideal pinhole camera with the same fx, fy, cx, cy, and
    {path: 3 x 3 K} of those cameras (pinhole_of) - what verify_matches, consolidate_matches, localize_queries, triangulate, refine and
    localize_queries_sparse take, unchanged.  The rule is csrc/camera_spec.h (COLMAP's SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL,
    OPENCV; a guarded Newton iteration in fp64): one upload of all rows, one launch per side (ops.undistort_points reads the two sides of
    the [M, 4] block in place), one read back.  Scores are untouched; matches, kpts1 and kpts2 come back as float32.  A row with a side
    that has no pre-image (the pixel lies beyond the model's range) or a non-finite coordinate is NaN on that side: the stages downstream
    drop such rows.  results'.n_failed counts them per pair, results'.status holds the status bytes.
    Camera parameters refer to the original image, so the coordinates of a no_match_upscale tuple are first scaled back by its element 4;
    the tuple returned for it holds original-image coordinates and ones as element 4.
    Every image of `pairs` needs an entry in `cameras`, else ValueError.  Thresholds downstream are then in ideal-pinhole pixels, which
    are stretched towards the corners under barrel distortion."""
    pairs = [tuple(p) for p in pairs]
    if len(pairs) != len(results):
        raise ValueError(f'undistort_results: {len(pairs)} pairs but {len(results)} results')
    index = {}
    pim = np.array([[index.setdefault(path, len(index)) for path in p] for p in pairs], np.int32).reshape(-1, 2)
    missing = [n for n in index if n not in cameras]
    if missing:
        raise ValueError(f'undistort_results: no camera for {missing[0]!r}')
    names = list(index)
    intrinsics = pinhole_of({n: cameras[n] for n in names})
    ms = _original_pixel_rows(results)
    offsets = _row_offsets(ms)
    M = int(offsets[-1])
    out = UndistortedResults()
    if M:
        table = np.array([canonical_camera(cameras[n]) for n in names], dtype=np.float64)
        with torch.cuda.device(device):
            tab, rows, off, cam = _upload(device, table, ms, offsets, pim.T)            # cam[s]: the camera of side s of every pair
            res = torch.empty(2, M, 2, dtype=torch.float32, device=rows.device)
            flags = torch.zeros(2, dtype=torch.int32, device=rows.device)
            st = [ops.undistort_points(rows[:, 2 * s:2 * s + 2], off, cam[s], tab, out=res[s], flags=flags)[1] for s in (0, 1)]
            xy, flags, *status = _download(res, flags, *st)
        ops.raise_camera_flags('undistort_results', flags)
    else:
        xy, status = np.zeros((2, 0, 2), np.float32), np.zeros((2, 0), np.uint8)
    out.status, failed = [], []
    for p, r in enumerate(results):
        b, e = int(offsets[p]), int(offsets[p + 1])
        k0, k1 = xy[0, b:e].copy(), xy[1, b:e].copy()
        m = np.concatenate([k0, k1], axis=1)
        out.append((m, k0, k1, r[3], np.ones(4)) if len(r) > 4 else (m, k0, k1, r[3]))
        s = np.stack([status[0][b:e], status[1][b:e]], axis=1)
        out.status.append(s)
        failed.append(int((s == ops.CM_ST_NO_PREIMAGE).any(axis=1).sum()))
    out.n_failed = np.array(failed, np.int32)
    return out, intrinsics


def undistort_points(points, camera, device='cuda'):
    """[n, 2] pixels of one Camera -> (float32 [n, 2] pixels of the ideal pinhole camera with its fx, fy, cx, cy, uint8 [n] status as in
    undistort_results) - for the point lists of estimate_relative_pose and estimate_absolute_pose, with K = pinhole_of's."""
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float32).reshape(-1, 2))
    n = len(pts)
    if n == 0:
        canonical_camera(camera)
        return np.zeros((0, 2), np.float32), np.zeros(0, np.uint8)
    with torch.cuda.device(device):
        tab = ops.camera_table([canonical_camera(camera)], device)
        seg = torch.tensor([0, n, 0], dtype=torch.int32).to(device)
        out, st = ops.undistort_points(torch.from_numpy(pts).to(device), seg[:2], seg[2:], tab)
        return out.cpu().numpy(), st.cpu().numpy()


def write_consolidated(out_dir, cm: ConsolidatedMatches):
    """names.txt (one image path per line, line i = image i), keypoints.npz (k00000, ...: [K_i, 2] float32 per image) and matches.npz
    (pairs [P, 2] int32 image indices; m00000, ...: [n_p, 2] int32 keypoint indices per pair)."""
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, 'names.txt'), 'w') as f:
        f.writelines(n + '\n' for n in cm.names)
    np.savez(os.path.join(out_dir, 'keypoints.npz'), **{f'k{i:05d}': k for i, k in enumerate(cm.keypoints)})
    np.savez(os.path.join(out_dir, 'matches.npz'), pairs=cm.pair_images, **{f'm{q:05d}': m for q, m in enumerate(cm.matches)})


def read_consolidated(in_dir) -> ConsolidatedMatches:
    """The inverse of write_consolidated: names.txt, keypoints.npz and matches.npz under in_dir -> ConsolidatedMatches."""
    with open(os.path.join(in_dir, 'names.txt')) as f:
        names = [line.rstrip('\n') for line in f if line.rstrip('\n')]
    with np.load(os.path.join(in_dir, 'keypoints.npz')) as kz:
        keypoints = [np.asarray(kz[f'k{i:05d}'], dtype=np.float32).reshape(-1, 2) for i in range(len(names))]
    with np.load(os.path.join(in_dir, 'matches.npz')) as mz:
        pair_images = np.asarray(mz['pairs'], dtype=np.int32).reshape(-1, 2)
        matches = [np.asarray(mz[f'm{q:05d}'], dtype=np.int32).reshape(-1, 2) for q in range(len(pair_images))]
    return ConsolidatedMatches(names, keypoints, pair_images, matches)


def quaternion_to_rotation(q):
    """The rotation matrix of (qw, qx, qy, qz), normalised first: the inverse of rotation_to_quaternion."""
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def read_poses(path):
    """One line per image: `path qw qx qy qz tx ty tz` with x_cam = R X + t, the format `localize --out` writes (blank lines and '#' lines
    are skipped; a relative path is relative to the file) -> {path: (R 3 x 3, t [3])}."""
    base = os.path.dirname(os.path.abspath(path))
    out = {}
    with open(path) as f:
        for no, line in enumerate(f, 1):
            parts = line.split()
            if not parts or parts[0].startswith('#'):
                continue
            if len(parts) != 8:
                raise ValueError(f'{path}:{no}: expected `path qw qx qy qz tx ty tz`, got {len(parts)} fields')
            v = np.array([float(x) for x in parts[1:]])
            if not np.all(np.isfinite(v)) or not np.linalg.norm(v[:4]) > 0:
                raise ValueError(f'{path}:{no}: the pose is not finite or its quaternion is zero')
            name = parts[0] if os.path.isabs(parts[0]) else os.path.normpath(os.path.join(base, parts[0]))
            out[name] = (quaternion_to_rotation(v[:4]), v[4:].copy())
    return out


# ---------------------------------------------------------------------------------------------
# triangulation of the database images from their known poses (hloc's triangulation / COLMAP's point_triangulator in
# localize_sfm_helper.py:reconstruct_database_pairs), and localisation against the triangulated points
# ---------------------------------------------------------------------------------------------
class TriangulatedTracks(NamedTuple):
    points: np.ndarray       # [T_valid, 3] float64: the triangulated 3-D points, in world units
    errors: np.ndarray       # [T_valid] float64: root of the mean squared reprojection error of a point's inliers, in pixels
    obs_offsets: np.ndarray  # [T_valid + 1] int32: the inlier observations of point k are obs_offsets[k] : obs_offsets[k + 1]
    obs_image: np.ndarray    # [N] int32: index into the ConsolidatedMatches' names
    obs_keypoint: np.ndarray  # [N] int32: index into that image's keypoints
    point_of_keypoint: list  # per image: [K_i] int32, the point a keypoint is an inlier observation of; -1: none
    n_tracks: int            # connected components of the match graph with at least two keypoints
    n_conflict: int          # of them: tracks in which an image occurs twice (not triangulated)
    n_rejected: int          # of them: tracks without a conflict that ended without a point (no solution, or fewer than min_obs inliers)


def triangulate(cm: ConsolidatedMatches, intrinsics, poses, thr=4.0, min_angle=1.5, min_obs=2, refit=2, device='cuda') -> TriangulatedTracks:
    """3-D points for the tracks of a ConsolidatedMatches from known camera poses, on the device.  intrinsics[name]: 3 x 3 K in the
    coordinates of the keypoints; poses[name] = (R, t) with x_cam = R X + t (what localize_queries returns and read_poses reads).  Images
    without an entry in poses take no part.  A track is a connected component of the graph whose nodes are keypoints and whose edges are
    matches (ops.build_tracks); a track with the same image twice is a conflict and is left out; every other track gets the best two-view
    midpoint among its observation pairs (rays meeting at min_angle degrees or more; inliers: reprojection error below thr pixels), refitted
    on its inliers up to `refit` times (ops.triangulate_tracks; the rule is csrc/tri_solver.h), and is kept with at least min_obs
    inliers.  refit defaults to 2 here (0 in ops): a two-ray midpoint alone is a poor point for a long track.  Before the upload the world
    origin is moved to the centre of the bounding box of the camera centres (fp64), and the points are moved back afterwards.  One upload,
    one read back.  No bundle adjustment, no re-triangulation or merging of tracks, no splitting of conflict tracks; no distortion
    here: undistort_results removes it from the matches before they are consolidated."""
    n, kp_off, K, R, t, origin, ids, id_off, kps, pim = _triangulation_inputs(cm, intrinsics, poses)
    n_nodes = int(kp_off[-1])
    empty = _assemble_tracks(n, kp_off, 0, *([np.zeros(0)] * 4), np.zeros(1, np.int32), *([np.zeros(0, np.int32)] * 2), np.zeros(0, bool), origin)
    if n_nodes == 0 or len(ids) == 0:
        return empty
    with torch.cuda.device(device):
        Rd, td, Kd, kpd, idd, iod, pimd, kpod = _upload(device, R, t, K, kps, ids, id_off, pim, kp_off)
        track_off, obs_image, obs_kp, obs_node = ops.build_tracks(idd, iod, pimd, kpod, n_nodes=n_nodes)
        T = int(track_off.numel()) - 1
        if T == 0:
            return empty
        rs = ops.triangulate_tracks(track_off, obs_image, kpd[obs_node.long()], Kd, Rd, td, pixel_thr=thr, min_angle_deg=min_angle, min_obs=min_obs,
                                    refit=refit)
        out = _download(rs['X'], rs['err2'], rs['valid'], rs['conflict'], track_off, obs_image, obs_kp, rs['inliers'])
    return _assemble_tracks(n, kp_off, T, *out, origin)


def _triangulation_inputs(cm, intrinsics, poses):
    """What triangulate uploads: (n images, kp_off int32 [n+1], K fp32 [n,9], R fp64 [n,9] and t fp64 [n,3] with NaN for an image without
    a pose and t moved to the new origin, origin [3], ids int32 [E,2], id_off int32 [P+1], keypoints fp32 [n_nodes,2], pair_images)."""
    n = len(cm.names)
    counts = np.array([len(k) for k in cm.keypoints], np.int64)
    kp_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    K, R, t = np.zeros((n, 9), np.float32), np.full((n, 9), np.nan), np.full((n, 3), np.nan)
    K[:, [0, 4, 8]] = 1.0
    for i, name in enumerate(cm.names):
        if name not in poses:
            continue
        if name not in intrinsics:
            raise ValueError(f'triangulate: no intrinsics for {name!r}')
        K[i] = np.asarray(intrinsics[name], dtype=np.float32).reshape(9)
        R[i] = np.asarray(poses[name][0], dtype=np.float64).reshape(9)
        t[i] = np.asarray(poses[name][1], dtype=np.float64).reshape(3)
    posed = np.isfinite(R).all(1) & np.isfinite(t).all(1)
    origin = np.zeros(3)
    if posed.any():
        centres = -np.einsum('nji,nj->ni', R[posed].reshape(-1, 3, 3), t[posed])
        origin = 0.5 * (centres.min(0) + centres.max(0))
        t[posed] = t[posed] + np.einsum('nij,j->ni', R[posed].reshape(-1, 3, 3), origin)        # x_cam = R (X' + origin) + t
    ids = np.concatenate([np.asarray(m, np.int32).reshape(-1, 2) for m in cm.matches]) if len(cm.matches) else np.zeros((0, 2), np.int32)
    id_off = np.concatenate([[0], np.cumsum([len(m) for m in cm.matches])]).astype(np.int32)
    kps = np.concatenate([np.asarray(k, np.float32).reshape(-1, 2) for k in cm.keypoints]) if n else np.zeros((0, 2), np.float32)
    return n, kp_off, K, R, t, origin, ids, id_off, kps, np.asarray(cm.pair_images, np.int32).reshape(-1, 2)


def _assemble_tracks(n, kp_off, T, X, err2, valid, conflict, toff, oimg, okp, inl, origin) -> TriangulatedTracks:
    """The per-track and per-observation outputs of ops.triangulate_tracks -> TriangulatedTracks (points moved back by origin)."""
    valid, conflict, inl = np.asarray(valid) == 1, np.asarray(conflict) == 1, np.asarray(inl).astype(bool)
    nv = int(valid.sum())
    track_of_obs = np.repeat(np.arange(T), np.diff(toff))
    point_of_track = np.full(T, -1, np.int64)
    point_of_track[valid] = np.arange(nv)
    keep = inl & valid[track_of_obs]
    per_point = np.bincount(point_of_track[track_of_obs[keep]], minlength=nv)
    pok = np.full(int(kp_off[-1]), -1, np.int32)
    pok[kp_off[oimg[keep]] + okp[keep]] = point_of_track[track_of_obs[keep]]
    return TriangulatedTracks(np.asarray(X, np.float64).reshape(T, 3)[valid] + origin, np.sqrt(np.asarray(err2, np.float64)[valid]),
                              np.concatenate([[0], np.cumsum(per_point)]).astype(np.int32), oimg[keep].astype(np.int32), okp[keep].astype(np.int32),
                              [pok[kp_off[i]:kp_off[i + 1]].copy() for i in range(n)], int(T), int(conflict.sum()),
                              int(T - conflict.sum() - nv))


# ---------------------------------------------------------------------------------------------
# bundle adjustment: the database poses and the triangulated points refined jointly (ops.bundle_adjust; the rule is csrc/ba_spec.h)
# ---------------------------------------------------------------------------------------------
class RefinedStructure(NamedTuple):
    poses: dict              # name -> (R 3 x 3, t [3]) with x_cam = R X + t: every entry of the input, the free ones refined
    tracks: TriangulatedTracks  # the points refined; only observations that are inliers at the final state, points with at least min_obs
    cost: np.ndarray         # [stages * iters + stages] float64: the truncated cost before the first and after every iteration, per stage
    accepted: np.ndarray     # [stages * iters] int32: 1 where the iteration's step was taken
    n_free: int              # cameras that were free to move
    cg_used: Optional[np.ndarray] = None  # solver='pcg': [stages * iters] int32, the CG iterations of every iteration; None for 'dense'


def _refine_inputs(cm, tt, intrinsics, poses, fixed):
    """What refine uploads: dict(K fp32 [n,9], R / t fp64 with NaN for an image without a pose and t moved to the new origin, origin [3], X
    fp64 [T,3] moved likewise, obs_off, obs_image int32, uv fp32 [N,2], free bool [n]).  Free: a pose, not named in fixed, and at least one
    observation."""
    n, kp_off, K, R, t, origin = _triangulation_inputs(cm, intrinsics, poses)[:6]
    unknown = [f for f in fixed if f not in cm.names]
    if unknown:
        raise ValueError(f'refine: fixed names {unknown[0]!r}, which is not an image of the keypoints')
    obs_image = np.ascontiguousarray(tt.obs_image, np.int32)
    obs_kp = np.asarray(tt.obs_keypoint, np.int64)
    if len(obs_image) and (obs_image.min() < 0 or obs_image.max() >= n):
        raise ValueError('refine: the tracks name an image the keypoints do not have')
    kps = np.concatenate([np.asarray(k, np.float32).reshape(-1, 2) for k in cm.keypoints]) if n else np.zeros((0, 2), np.float32)
    counts = np.diff(kp_off)
    if len(obs_image) and (obs_kp.min() < 0 or (obs_kp >= counts[obs_image]).any()):
        raise ValueError('refine: the tracks name a keypoint its image does not have')
    posed = np.isfinite(R).all(1) & np.isfinite(t).all(1)
    fixed = set(fixed)
    free = posed & np.array([name not in fixed for name in cm.names], bool) & (np.bincount(obs_image, minlength=n) > 0)
    return dict(n=n, kp_off=kp_off, K=K, R=R, t=t, origin=origin, X=np.asarray(tt.points, np.float64).reshape(-1, 3) - origin,
                obs_off=np.ascontiguousarray(tt.obs_offsets, np.int32), obs_image=obs_image, obs_kp=obs_kp.astype(np.int32),
                uv=np.ascontiguousarray(kps[kp_off[obs_image].astype(np.int64) + obs_kp]), free=free, posed=posed)


def _refine_device(a, thrs, iters, device, solver='dense', cg_iters=64, cg_tol=1e-6):
    """One upload, one ops.bundle_adjust per threshold (each from the state the one before left, all on the device, all with the same
    solver), one read back -> dict(R [n,9], t [n,3], X [T,3], inliers uint8 [N], cost, accepted; with solver='pcg' also cg_used) in numpy."""
    n, T = a['n'], len(a['X'])
    with torch.cuda.device(device):
        R, t, X, K, uv, ooff, oimg, free = _upload(device, a['R'], a['t'], a['X'], a['K'], a['uv'], a['obs_off'], a['obs_image'],
                                                   a['free'].astype(np.int32))
        host = {'obs_off': a['obs_off'], 'obs_image': a['obs_image'], 'free': a['free']}
        costs, accs, used = [], [], []
        pcg = solver == 'pcg'
        kw = dict(solver=solver, cg_iters=cg_iters, cg_tol=cg_tol) if pcg else {}
        for thr in thrs:
            rs = ops.bundle_adjust(ooff, oimg, uv, K, R, t, X, free, thr=thr, iters=iters, host=host, **kw)
            R, t, X = rs['R'], rs['t'], rs['X']
            costs.append(rs['cost'])
            accs.append(rs['accepted'])
            used.append(rs['cg_used'] if pcg else rs['accepted'][:0])
        R, t, X, cost, accepted, cg_used, inliers = _download(R, t, X, torch.cat(costs), torch.cat(accs), torch.cat(used), rs['inliers'])
    r = dict(R=R.reshape(n, 9), t=t.reshape(n, 3), X=X.reshape(T, 3), cost=cost.copy(), accepted=accepted.copy(), inliers=inliers.copy())
    if pcg:
        r['cg_used'] = cg_used.copy()
    return r


def _assemble_refined(cm, tt, poses, a, r, min_obs) -> RefinedStructure:
    """The outputs of the device (or of the host build: the CPU tests) -> RefinedStructure, in world coordinates."""
    n, T, origin = a['n'], len(a['X']), a['origin']
    inl = np.asarray(r['inliers']).astype(bool)
    point_of_obs = np.repeat(np.arange(T), np.diff(a['obs_off']))
    valid = np.bincount(point_of_obs[inl], minlength=T) >= min_obs
    keep = inl & valid[point_of_obs]
    nv = int(valid.sum())
    new_id = np.full(T, -1, np.int64)
    new_id[valid] = np.arange(nv)
    oimg, okp, pt = a['obs_image'][keep], a['obs_kp'][keep], new_id[point_of_obs[keep]]
    R, t, X = r['R'].reshape(n, 3, 3), r['t'], r['X']
    Y = np.einsum('nij,nj->ni', R[oimg], X[point_of_obs[keep]]) + t[oimg]
    K = a['K'].astype(np.float64)[oimg]
    e2 = (K[:, 0] * Y[:, 0] / Y[:, 2] + K[:, 2] - a['uv'][keep, 0]) ** 2 + (K[:, 4] * Y[:, 1] / Y[:, 2] + K[:, 5] - a['uv'][keep, 1]) ** 2
    per_point = np.bincount(pt, minlength=nv)
    err = np.sqrt(np.bincount(pt, weights=e2, minlength=nv) / np.maximum(per_point, 1))
    pok = np.full(int(a['kp_off'][-1]), -1, np.int32)
    pok[a['kp_off'][oimg] + okp] = pt
    tracks = TriangulatedTracks(X[valid] + origin, err, np.concatenate([[0], np.cumsum(per_point)]).astype(np.int32), oimg.astype(np.int32),
                                okp.astype(np.int32), [pok[a['kp_off'][i]:a['kp_off'][i + 1]].copy() for i in range(n)], tt.n_tracks,
                                tt.n_conflict, tt.n_rejected + int(T - nv))
    out = dict(poses)
    for i, name in enumerate(cm.names):
        if a['free'][i]:
            out[name] = (R[i].copy(), t[i] - R[i] @ origin)             # t' = t + R origin
    return RefinedStructure(out, tracks, np.asarray(r['cost']), np.asarray(r['accepted']), int(a['free'].sum()),
                            np.asarray(r['cg_used']) if 'cg_used' in r else None)


def refine(cm: ConsolidatedMatches, tt: TriangulatedTracks, intrinsics, poses, fixed=(), iters=16, thr=4.0, min_obs=2,
           device='cuda', solver='dense', cg_iters=64, cg_tol=1e-6) -> RefinedStructure:
    """Bundle adjustment on the device: the poses of the images of cm and the points of tt refined jointly, minimising the squared
    reprojection error of tt's observations truncated at thr pixels (ops.bundle_adjust; the rule is csrc/ba_spec.h: Levenberg-Marquardt,
    points eliminated by the Schur complement, dense Cholesky of the reduced camera system, `iters` iterations enqueued at once).  poses[name]
    = (R, t) as triangulate takes them; fixed: names of images whose poses are trusted and stay as they are.  An image is free when it has
    a pose, is not fixed and has an observation; more than 128 free images is a ValueError (ops.BA_MAX_FREE).  With fewer than two fixed
    images nothing but the damping holds the frame, and the result may drift by a small similarity: fix the images whose poses are
    trusted.  An observation takes part only while its error is below thr, so thr must exceed the reprojection error of the start or the
    observations never join: thr may be a sequence, e.g. (20, 8, 4) - one run per threshold, each from the state the one before left.
    Returns RefinedStructure: poses (a dict like the input), tracks (the layout of tt: only observations that are inliers at the final
    state, points with fewer than min_obs of them dropped, errors recomputed, point_of_keypoint rebuilt), cost, accepted, n_free.  The world
    origin is moved to the centre of the camera centres' bounding box before the upload and back afterwards, as in triangulate.  One upload,
    one read back.  solver='pcg' (csrc/ba_pcg_spec.h) solves the reduced camera system by matrix-free preconditioned conjugate gradients
    instead of the dense Cholesky: up to 65536 free images (ops.BA_PCG_MAX_FREE), at most cg_iters (1 .. 256) CG iterations per iteration,
    stopped at the relative tolerance cg_tol (in [0, 1)); every stage of a thr schedule uses the same solver, and the result's cg_used is
    the log of CG iterations (None for 'dense').  The preconditioner is block Jacobi and the tolerance is fixed.  No intrinsics or
    distortion refinement, no robust loss other than the truncation, no re-triangulation inside the loop: call triangulate again with the
    refined poses to win observations back."""
    if solver not in ('dense', 'pcg'):
        raise ValueError(f"refine: solver must be 'dense' or 'pcg', not {solver!r}")
    pcg = solver == 'pcg'
    if pcg and not 1 <= int(cg_iters) <= ops.BA_PCG_MAX_ITERS:
        raise ValueError(f'refine: cg_iters must be 1 .. {ops.BA_PCG_MAX_ITERS}')
    if pcg and not 0.0 <= float(cg_tol) < 1.0:
        raise ValueError('refine: cg_tol must be in [0, 1)')
    thrs = tuple(float(x) for x in (thr if isinstance(thr, (tuple, list, np.ndarray)) else (thr,)))
    if not thrs or not all(x > 0 and np.isfinite(x) for x in thrs):
        raise ValueError('refine: thr must be positive')
    if not 1 <= int(iters) <= ops.BA_MAX_ITERS:
        raise ValueError(f'refine: iters must be 1 .. {ops.BA_MAX_ITERS}')
    if min_obs < 2:
        raise ValueError('refine: min_obs must be at least 2')
    a = _refine_inputs(cm, tt, intrinsics, poses, fixed)
    if pcg and int(a['free'].sum()) > ops.BA_PCG_MAX_FREE:
        raise ValueError(f"refine: {int(a['free'].sum())} free images, the limit is {ops.BA_PCG_MAX_FREE} with solver='pcg': name more "
                         'images in fixed')
    if not pcg and int(a['free'].sum()) > ops.BA_MAX_FREE:
        raise ValueError(f"refine: {int(a['free'].sum())} free images, the limit is {ops.BA_MAX_FREE} (the reduced camera system is solved "
                         "densely): name more images in fixed, or pass solver='pcg'")
    if len(a['X']) == 0 or len(a['obs_image']) == 0:
        return RefinedStructure(dict(poses), tt, np.zeros(0), np.zeros(0, np.int32), int(a['free'].sum()), np.zeros(0, np.int32) if pcg else None)
    if pcg:
        return _assemble_refined(cm, tt, poses, a, _refine_device(a, thrs, int(iters), device, solver='pcg', cg_iters=int(cg_iters),
                                                                  cg_tol=float(cg_tol)), min_obs)
    return _assemble_refined(cm, tt, poses, a, _refine_device(a, thrs, int(iters), device), min_obs)


def write_poses(path, poses):
    """One line per image: `path qw qx qy qz tx ty tz` with x_cam = R X + t - what read_poses reads."""
    with open(path, 'w') as f:
        for name, (R, t) in poses.items():
            f.write(' '.join([name] + [repr(float(v)) for v in (*rotation_to_quaternion(R), *np.asarray(t, np.float64).reshape(3))]) + '\n')


def localize_queries_sparse(cm: ConsolidatedMatches, tt: TriangulatedTracks, queries, intrinsics, thr=12.0, min_inliers=12, iters=None, refit=0,
                            device='cuda', covis_cluster=False, dedup=False) -> LocalizedQueries:
    """Camera poses of query images against triangulated points: the sparse counterpart of localize_queries for datasets with database
    poses and no depth.  queries: image names of cm.  For every pair of cm that joins a query and an image with points (the query on either
    side), the rows are p2d = the query's keypoints, p3d = the point of the other image's keypoint (tt.point_of_keypoint; NaN where it has
    none, such a row takes no part).  All pairs of a query form one problem in pair order, then ops.ransac_absolute_pose as in
    localize_queries.  intrinsics[query]: 3 x 3 K.  masks: one per pair of cm ([n_p] bool; all False for a pair that joins no query to
    points).  With both flags off: indexing on the host and an existing op.
    covis_cluster (hloc's covisibility_clustering): the database images of a query are split into the connected components of the
    covisibility graph restricted to them (two images are linked iff they share a point of tt), one pose per component, and the component
    with the most inliers wins (then the lowest cluster number) - retrieval that returns two places that look alike no longer pools them.
    dedup: every (query keypoint, point) counts once per problem, however many database images show it; the mask of a repeated row is
    its first occurrence's.  With either flag the rows are built on the device (ops.covis_clusters, ops.sparse_rows, ops.select_cluster;
    the rule is csrc/covis_spec.h; one upload, pair-level bookkeeping on the host) and the result carries n_clusters, cluster, db_names,
    db_cluster and cluster_inliers.  At most 1024 database images per query."""
    names = list(dict.fromkeys(queries))
    Q = len(names)
    missing = [q for q in names if q not in intrinsics or q not in cm.names]
    if missing:
        raise ValueError(f'localize_queries_sparse: no intrinsics for, or no image named {missing[0]!r}')
    if covis_cluster or dedup:
        return _localize_sparse_device(cm, tt, names, intrinsics, thr, min_inliers, iters, refit, device, bool(covis_cluster), bool(dedup))
    p2d, p3d, query_off, pair_off, used, owner = _sparse_rows(cm, tt, names)
    masks = [np.zeros(len(m), bool) for m in cm.matches]
    M = len(p2d)
    if Q == 0 or M == 0:
        return LocalizedQueries(names, np.zeros((Q, 3, 3)), np.zeros((Q, 3)), np.zeros(Q, np.int32), np.zeros(Q, bool), masks, np.zeros(Q, np.int32))
    Ks = np.stack([np.asarray(intrinsics[q], dtype=np.float32).reshape(9) for q in names])
    with torch.cuda.device(device):
        p2d, p3d, query_off, Ks = _upload(device, p2d, p3d, query_off, Ks)
        rs = ops.ransac_absolute_pose(p2d, p3d, None, query_off, Q, Ks, pixel_thr=thr, iters=ops.ABS_RANSAC_ITERS if iters is None else iters,
                                      refit=refit)
        R, t, valid, nin, rounds, inl = _absolute_poses(rs)
    localized, used_masks = _verified_masks(valid, nin, min_inliers, inl, pair_off, owner)
    for p, mask in zip(used, used_masks):
        masks[p] = mask
    return LocalizedQueries(names, R, t, nin, localized, masks, rounds)


def _sparse_rows(cm, tt, names):
    """The 2-D - 3-D rows of localize_queries_sparse, sorted by query (a query's pairs in pair order): p2d fp32 [M,2], p3d fp32 [M,3] (NaN:
    the keypoint has no point), query_off int32 [Q+1], pair_off [n+1] (the rows of the n contributing pairs), and per contributing pair
    its index in cm and its query."""
    qidx = {q: k for k, q in enumerate(names)}
    image_q = np.array([qidx.get(nm, -1) for nm in cm.names], np.int64)
    has_pts = np.array([bool((p >= 0).any()) for p in tt.point_of_keypoint])
    rows2, rows3, owner, used = [], [], [], []
    for p in range(len(cm.matches)):
        i, j = (int(v) for v in cm.pair_images[p])
        m = np.asarray(cm.matches[p]).reshape(-1, 2)
        for qs, ds, a, b in ((i, j, 0, 1), (j, i, 1, 0)):
            if image_q[qs] >= 0 and image_q[ds] < 0 and has_pts[ds]:
                pt = tt.point_of_keypoint[ds][m[:, b]]
                x = np.full((len(m), 3), np.nan, np.float32)
                x[pt >= 0] = tt.points[pt[pt >= 0]]
                rows2.append(np.asarray(cm.keypoints[qs], np.float32).reshape(-1, 2)[m[:, a]]), rows3.append(x)
                owner.append(int(image_q[qs])), used.append(p)
                break
    order = sorted(range(len(used)), key=lambda k: owner[k])            # stable: a query's pairs stay in pair order
    lens = [len(rows2[k]) for k in order]
    pair_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    query_off = np.concatenate([[0], np.cumsum(np.bincount([owner[k] for k in order], weights=lens, minlength=len(names)))]).astype(np.int32)
    p2d = np.concatenate([rows2[k] for k in order]) if order else np.zeros((0, 2), np.float32)
    p3d = np.concatenate([rows3[k] for k in order]) if order else np.zeros((0, 3), np.float32)
    return p2d, p3d, query_off, pair_off, [used[k] for k in order], [owner[k] for k in order]


def _covis_tables(cm, tt, names):
    """The pair-level bookkeeping of the device path (csrc/covis_spec.h, step 1; O(pairs), after one count of tt.obs_image per image for
    "has a point"): which pairs contribute (the rule of _sparse_rows), every query's database list in order of first appearance, and each
    list sorted by image id.  -> dict(pairs int32 [C,8], pair_row_off
    int32 [C+1], used: the index in cm of each contributing pair, list_off int32 [Q+1], list_img, sorted_img, sorted_pos int32 [L])."""
    qidx = {q: k for k, q in enumerate(names)}
    image_q = [qidx.get(nm, -1) for nm in cm.names]
    has_pts = np.bincount(np.asarray(tt.obs_image, np.int64), minlength=len(cm.names)) > 0       # an image with a point has an observation
    id_off = np.concatenate([[0], np.cumsum([len(m) for m in cm.matches])]).astype(np.int64)
    if id_off[-1] >= 2 ** 31:
        raise ValueError('localize_queries_sparse: 2^31 match rows or more')
    lists, where, pairs, used = [[] for _ in names], [{} for _ in names], [], []
    for p in range(len(cm.matches)):
        i, j = (int(v) for v in cm.pair_images[p])
        for qs, ds, col in ((i, j, 0), (j, i, 1)):
            if image_q[qs] >= 0 and image_q[ds] < 0 and has_pts[ds]:
                q = image_q[qs]
                pos = where[q].setdefault(ds, len(lists[q]))
                if pos == len(lists[q]):
                    lists[q].append(ds)
                pairs.append((q, qs, ds, id_off[p], id_off[p + 1], col, pos, 0)), used.append(p)
                break
    longest = max([len(x) for x in lists], default=0)
    if longest > ops.CV_MAX_LIST:
        raise ValueError(f'localize_queries_sparse: a query with {longest} database images; at most {ops.CV_MAX_LIST}')
    pairs = np.array(pairs, np.int32).reshape(-1, ops.CV_PAIR_WORDS)
    flat = lambda xs: np.array([v for x in xs for v in x], np.int32)              # noqa: E731
    by_id = [sorted(range(len(x)), key=x.__getitem__) for x in lists]
    return {'pairs': pairs, 'pair_row_off': np.concatenate([[0], np.cumsum(pairs[:, 4].astype(np.int64) - pairs[:, 3])]).astype(np.int32),
            'used': used, 'list_off': np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32), 'list_img': flat(lists),
            'sorted_img': flat([[x[a] for a in o] for x, o in zip(lists, by_id)]), 'sorted_pos': flat(by_id)}


def _device_rows(cm, tt, names, intrinsics, tb, device, covis_cluster, dedup):
    """The device row path of localize_queries_sparse for the tables tb of _covis_tables: one upload, ops.covis_clusters, ops.sparse_rows
    (one read of the sizes) -> (K fp32 [Q,9], cluster, n_clusters, the dict of ops.sparse_rows with p2d and p3d), all on the device."""
    T = len(tt.points)
    Ks = np.stack([np.asarray(intrinsics[q], dtype=np.float32).reshape(9) for q in names])
    kpo, pok, ooff, oimg, prs, pro, idd, loff, limg, simg, spos, Kd, kpd, ptd = _upload(
        device, _row_offsets(cm.keypoints), np.concatenate(tt.point_of_keypoint).astype(np.int32), np.asarray(tt.obs_offsets, np.int32),
        np.asarray(tt.obs_image, np.int32), tb['pairs'], tb['pair_row_off'], [np.asarray(m, np.int32).reshape(-1, 2) for m in cm.matches],
        tb['list_off'], tb['list_img'], tb['sorted_img'], tb['sorted_pos'], Ks, [np.asarray(k, np.float32).reshape(-1, 2) for k in cm.keypoints],
        np.asarray(tt.points).astype(np.float32).reshape(T, 3))        # the points rounded once to fp32, as _sparse_rows does
    cluster, ncl, status = ops.covis_clusters(kpo, pok, ooff, oimg, loff, limg, simg, spos, tb, enable=covis_cluster)
    rows = ops.sparse_rows(prs, pro, idd, kpo, pok, T, loff, cluster, ncl, tb, dedup=dedup, status=status, keypoints=kpd, points=ptd)
    return Kd, cluster, ncl, rows


def _localize_sparse_device(cm, tt, names, intrinsics, thr, min_inliers, iters, refit, device, covis_cluster, dedup):
    """localize_queries_sparse with covis_cluster or dedup: one upload, the cluster kernel, the row kernel with torch's sorts behind it, one
    read of the sizes, ops.ransac_absolute_pose over the problems, the selection kernel, one read back."""
    Q = len(names)
    tb = _covis_tables(cm, tt, names)
    Lt, used = len(tb['list_img']), tb['used']
    masks = [np.zeros(len(m), bool) for m in cm.matches]
    db_names = [[cm.names[i] for i in tb['list_img'][tb['list_off'][q]:tb['list_off'][q + 1]]] for q in range(Q)]
    zero = np.zeros(Q, np.int32)

    def result(R, t, nin, localized, rounds, ncl, win, cluster, cin):
        base = np.concatenate([[0], np.cumsum(ncl)])
        return LocalizedQueries(names, R, t, nin, localized, masks, rounds, ncl, win,
                                db_names, [cluster[tb['list_off'][q]:tb['list_off'][q + 1]].copy() for q in range(Q)],
                                [cin[base[q]:base[q + 1]].copy() for q in range(Q)])
    if Q == 0 or Lt == 0:                                              # no contributing pair: every list is empty, C_q = 0
        return result(np.zeros((Q, 3, 3)), np.zeros((Q, 3)), zero, np.zeros(Q, bool), zero.copy(), zero.copy(), np.full(Q, -1, np.int32),
                      np.zeros(0, np.int32), np.zeros(0, np.int32))
    with torch.cuda.device(device):
        Kd, cluster, ncl, rows = _device_rows(cm, tt, names, intrinsics, tb, device, covis_cluster, dedup)
        N, M = rows['N'], rows['M']
        if M == 0:
            ncl_h, cl_h = _download(ncl, cluster)
            return result(np.zeros((Q, 3, 3)), np.zeros((Q, 3)), zero, np.zeros(Q, bool), zero.copy(), ncl_h.copy(), np.full(Q, -1, np.int32), cl_h,
                          np.zeros(N, np.int32))
        query_of_prob = torch.repeat_interleave(torch.arange(Q, device=ncl.device), ncl.long(), output_size=N)
        rs = ops.ransac_absolute_pose(rows['p2d'], rows['p3d'], None, rows['prob_off'], N, Kd[query_of_prob], pixel_thr=thr,
                                      iters=ops.ABS_RANSAC_ITERS if iters is None else iters, refit=refit)
        sel = ops.select_cluster(rows['prob_base'], rs, rows['row_prob'], rows['slot'], min_inliers)
        R, t, win, localized, nin, rounds, ncl_h, cl_h, cin, mask = _download(
            sel['R'], sel['t'], sel['winner'], sel['localized'], sel['n_inliers'], sel['rounds'], ncl, cluster, sel['cluster_inliers'], sel['mask'])
    localized, mask = localized.astype(bool), mask.astype(bool)
    for c, p in enumerate(used):                                       # (a pair listed with a query contributes once; the masks of a query
        if localized[tb['pairs'][c, 0]]:                               #  that is not localised stay False, as with the flags off)
            masks[p] = mask[tb['pair_row_off'][c]:tb['pair_row_off'][c + 1]].copy()
    return result(R.reshape(Q, 3, 3).copy(), t.reshape(Q, 3).copy(), nin.copy(), localized, rounds.copy(), ncl_h.copy(), win.copy(), cl_h, cin)


def read_triangulated(path) -> TriangulatedTracks:
    """What `triangulate --out FILE.npz` wrote -> TriangulatedTracks.  A file from before n_tracks, n_conflict and n_rejected were saved
    reads with -1 for the three counts."""
    with np.load(path) as z:
        kp_off = np.asarray(z['kp_offsets'], np.int64)
        pok = np.asarray(z['point_of_keypoint'], np.int32)
        counts = [int(z[k]) if k in z.files else -1 for k in ('n_tracks', 'n_conflict', 'n_rejected')]
        return TriangulatedTracks(np.asarray(z['points'], np.float64).reshape(-1, 3), np.asarray(z['errors'], np.float64),
                                  np.asarray(z['obs_offsets'], np.int32), np.asarray(z['obs_image'], np.int32), np.asarray(z['obs_keypoint'], np.int32),
                                  [pok[kp_off[i]:kp_off[i + 1]].copy() for i in range(len(kp_off) - 1)], *counts)


def write_triangulated(path, tt: TriangulatedTracks):
    """What `triangulate --out` writes and read_triangulated reads: points, errors, obs_offsets, obs_image, obs_keypoint, point_of_keypoint
    (all images, concatenated in the order of names.txt), kp_offsets, and the counts n_tracks, n_conflict, n_rejected."""
    np.savez(path, points=tt.points, errors=tt.errors, obs_offsets=tt.obs_offsets, obs_image=tt.obs_image, obs_keypoint=tt.obs_keypoint,
             point_of_keypoint=np.concatenate(tt.point_of_keypoint) if tt.point_of_keypoint else np.zeros(0, np.int32),
             kp_offsets=np.concatenate([[0], np.cumsum([len(p) for p in tt.point_of_keypoint])]).astype(np.int32),
             n_tracks=np.int32(tt.n_tracks), n_conflict=np.int32(tt.n_conflict), n_rejected=np.int32(tt.n_rejected))
