"""Shared by the triangulation tests: ctypes wrappers of the serial host build (csrc/host/tri_host.cpp over csrc/tri_solver.h), planted
cameras and tracks, and the match graphs of the track tests."""
import ctypes
import math

import numpy as np

SEED = 0x5EED
TR_MAX_HYP, TR_LEX_MAX = 64, 11
OUT_KEYS = ('X', 'valid', 'conflict', 'n_inliers', 'hypothesis', 'rounds', 'err2', 'inliers')

_host = None


def host_lib():
    global _host
    if _host is None:
        import os
        from geoformer_amd import build
        if not os.path.exists(build.TRI_HOST_LIB):
            build.build_tri_host(verbose=False)
        h = ctypes.CDLL(build.TRI_HOST_LIB)
        vp, ci, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
        h.gf_tri_host_hyp_count.restype, h.gf_tri_host_hyp_count.argtypes = ci, [ci]
        h.gf_tri_host_pair.restype, h.gf_tri_host_pair.argtypes = ci, [u32, u32, ci, ci, vp]
        h.gf_tri_host_midpoint.restype, h.gf_tri_host_midpoint.argtypes = ci, [vp] * 8 + [ctypes.c_double, vp]
        h.gf_tri_host_label.restype, h.gf_tri_host_label.argtypes = ci, [vp, vp, vp, ci, ci, vp, ci, ci, vp]
        h.gf_tri_host_tracks.restype, h.gf_tri_host_tracks.argtypes = None, [vp, ci, vp, ci, vp, vp, vp, vp, vp]
        h.gf_tri_host_triangulate.restype = ci
        h.gf_tri_host_triangulate.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, ci, ctypes.c_float, ctypes.c_double, ci, ci, u32] + [vp] * 8
        _host = h
    return _host


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def cos_of(deg):
    return math.cos(math.radians(float(deg)))


def host_pair(track, t, L, seed=SEED):
    out = np.zeros(2, np.int32)
    ok = host_lib().gf_tri_host_pair(seed, track, t, L, _p(out))
    return ok, (int(out[0]), int(out[1]))


def host_midpoint(Ka, Ra, ta, uva, Kb, Rb, tb, uvb, min_angle_deg=1.5, cos_min=None):
    a = [np.ascontiguousarray(Ka, np.float32).reshape(9), np.ascontiguousarray(Ra, np.float64).reshape(9), np.ascontiguousarray(ta, np.float64),
         np.ascontiguousarray(uva, np.float32), np.ascontiguousarray(Kb, np.float32).reshape(9), np.ascontiguousarray(Rb, np.float64).reshape(9),
         np.ascontiguousarray(tb, np.float64), np.ascontiguousarray(uvb, np.float32)]
    X = np.zeros(3)
    ok = host_lib().gf_tri_host_midpoint(*[_p(x) for x in a], cos_of(min_angle_deg) if cos_min is None else cos_min, _p(X))
    return ok, X


def host_label(g):
    parent = np.zeros(max(g['n_nodes'], 1), np.int32)
    st = host_lib().gf_tri_host_label(_p(g['ids']), _p(g['id_off']), _p(g['pair_images']), len(g['pair_images']), len(g['ids']), _p(g['kp_off']),
                                      len(g['kp_off']) - 1, g['n_nodes'], _p(parent))
    return st, parent[:g['n_nodes']]


def host_tracks(g):
    """-> (status, parent, track_off, obs_image, obs_kp, obs_node) of the serial build."""
    st, parent = host_label(g)
    n = g['n_nodes']
    toff, node, img, kp = (np.zeros(n + 2, np.int32) for _ in range(4))
    sizes = np.zeros(2, np.int32)
    par = np.ascontiguousarray(parent) if n else np.zeros(1, np.int32)
    host_lib().gf_tri_host_tracks(_p(par), n, _p(g['kp_off']), len(g['kp_off']) - 1, _p(toff), _p(node), _p(img), _p(kp), _p(sizes))
    T, m = int(sizes[0]), int(sizes[1])
    return st, parent, toff[:T + 1].copy(), img[:m].copy(), kp[:m].copy(), node[:m].copy()


def host_triangulate(track_off, obs_image, obs_uv, K, R, t, pixel_thr=4.0, min_angle_deg=1.5, min_obs=2, refit=0, seed=SEED, cos_min=None):
    """The serial build on numpy arrays -> (rc, dict as ops.triangulate_tracks returns it)."""
    track_off = np.ascontiguousarray(track_off, np.int32)
    obs_image = np.ascontiguousarray(obs_image, np.int32)
    obs_uv = np.ascontiguousarray(obs_uv, np.float32).reshape(-1, 2)
    K = np.ascontiguousarray(K, np.float32).reshape(-1, 9)
    R = np.ascontiguousarray(R, np.float64).reshape(-1, 9)
    t = np.ascontiguousarray(t, np.float64).reshape(-1, 3)
    T, n = len(track_off) - 1, len(obs_image)
    X, err2 = np.zeros((max(T, 1), 3)), np.zeros(max(T, 1))
    valid, conflict, nin, hyp, rounds = (np.zeros(max(T, 1), np.int32) for _ in range(5))
    inl = np.zeros(max(n, 1), np.uint8)
    rc = host_lib().gf_tri_host_triangulate(_p(track_off), T, n, _p(obs_image), _p(obs_uv), _p(K), _p(R), _p(t), len(K), pixel_thr,
                                            cos_of(min_angle_deg) if cos_min is None else cos_min, min_obs, refit, seed, _p(X), _p(valid),
                                            _p(conflict), _p(nin), _p(hyp), _p(rounds), _p(err2), _p(inl))
    return rc, {'X': X[:T], 'valid': valid[:T], 'conflict': conflict[:T], 'n_inliers': nin[:T], 'hypothesis': hyp[:T], 'rounds': rounds[:T],
                'err2': err2[:T], 'inliers': inl[:n]}


# --------------------------------------------------------------------------------------------- planted cameras and tracks
def look_at(centre, target, roll):
    z = target - centre
    z = z / np.linalg.norm(z)
    x = np.cross(np.array([math.sin(roll), math.cos(roll), 0.0]), z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z])            # rows: the camera axes in world coordinates, x_cam = R (X - c)


def make_cameras(n, seed, fx=800.0, cx=800.0, cy=600.0):
    """n cameras on an arc of 8 units looking at a scene 5 to 9 units away -> K fp32 [n,9], R fp64 [n,3,3], t fp64 [n,3] (x_cam = R X + t)."""
    rng = np.random.default_rng(seed)
    K = np.tile(np.array([fx, 0, cx, 0, fx * 1.01, cy, 0, 0, 1], np.float32), (n, 1))
    R, t = np.zeros((n, 3, 3)), np.zeros((n, 3))
    for i in range(n):
        c = np.array([-4.0 + 8.0 * i / max(n - 1, 1), rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5)])
        R[i] = look_at(c, np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 7.0]), rng.uniform(-0.1, 0.1))
        t[i] = -R[i] @ c
    return K, R, t


def project(K, R, t, X):
    Y = R @ X + t
    k = np.asarray(K, np.float64).reshape(9)
    return np.array([k[0] * Y[0] / Y[2] + k[2], k[4] * Y[1] / Y[2] + k[5]])


def planted_tracks(K, R, t, lengths, seed, noise=0.5, outlier_frac=0.0, outlier_from=5):
    """One planted point per entry of lengths, seen by that many distinct cameras (ascending: image-major; an entry that is a list names
    the cameras), pixels with Gaussian noise;
    from length outlier_from up, outlier_frac of a track's observations (rounded down) are replaced by a pixel anywhere in the image.
    -> dict(track_off, obs_image, obs_uv fp32, X [T,3], planted [N] bool: the observation is no outlier)."""
    rng = np.random.default_rng(seed)
    n_cam = len(K)
    toff, img, uv, pts, planted = [0], [], [], [], []
    for L in lengths:
        X = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(5, 9)])
        if not isinstance(L, (int, np.integer)):                             # the cameras themselves instead of their number
            cams, L = np.asarray(L), len(L)
        else:
            cams = np.sort(rng.choice(n_cam, L, replace=False))
        bad = set(rng.choice(L, int(outlier_frac * L), replace=False).tolist()) if L >= outlier_from else set()
        for j, c in enumerate(cams):
            p = project(K[c], R[c], t[c], X) + rng.normal(0, noise, 2) if noise else project(K[c], R[c], t[c], X)
            if j in bad:
                p = np.array([rng.uniform(0, 1600), rng.uniform(0, 1200)])
            img.append(c), uv.append(p), planted.append(j not in bad)
        toff.append(len(img))
        pts.append(X)
    return {'track_off': np.array(toff, np.int32), 'obs_image': np.array(img, np.int32), 'obs_uv': np.array(uv, np.float32).reshape(-1, 2),
            'X': np.array(pts).reshape(-1, 3), 'planted': np.array(planted, bool)}


# --------------------------------------------------------------------------------------------- match graphs
def graph(kp_counts, edges):
    """edges: (image, keypoint, image, keypoint) rows in order; rows of one image pair that follow each other form one pair of the list."""
    kp_off = np.concatenate([[0], np.cumsum(kp_counts)]).astype(np.int32)
    pairs, id_off, ids = [], [0], []
    for (i, k, j, l) in edges:
        if not pairs or pairs[-1] != (i, j):
            if pairs:
                id_off.append(len(ids))
            pairs.append((i, j))
        ids.append((k, l))
    id_off.append(len(ids))
    if not pairs:
        id_off = [0]
    return {'ids': np.array(ids, np.int32).reshape(-1, 2), 'id_off': np.array(id_off, np.int32), 'pair_images': np.array(pairs, np.int32).reshape(-1, 2),
            'kp_off': kp_off, 'n_nodes': int(kp_off[-1])}


def graph_cases():
    rng = np.random.default_rng(7)
    cases = {
        'no_edges': graph([3, 2, 4], []),
        'one_edge': graph([3, 2, 4], [(0, 1, 2, 3)]),
        'self_loop': graph([3, 2], [(0, 1, 0, 1), (0, 2, 1, 0)]),
        'duplicate_edges': graph([3, 3], [(0, 1, 1, 2), (0, 1, 1, 2), (0, 0, 1, 0), (0, 1, 1, 2)]),
        # one keypoint per image, 199 pairs of one row each, the chain's far end first: long parent chains for the compare-and-swap loop
        'path_200_reversed': graph([1] * 200, [(i, 0, i + 1, 0) for i in range(198, -1, -1)]),
        'star': graph([1] * 70, [(0, 0, i, 0) for i in range(1, 70)]),
        'joined_by_last_edge': graph([4, 4, 4, 4], [(0, 0, 1, 0), (1, 0, 2, 1), (0, 3, 3, 3), (3, 3, 2, 2), (2, 1, 3, 3)]),
        'empty_image': graph([2, 0, 2], [(0, 1, 2, 0), (0, 0, 2, 1)]),
    }
    counts = [100] * 50
    e = []
    for _ in range(60):                      # 60 image pairs of 50 rows: 3000 edges over 5000 nodes
        i, j = sorted(rng.choice(50, 2, replace=False).tolist())
        e += [(i, int(a), j, int(b)) for a, b in zip(rng.integers(0, 100, 50), rng.integers(0, 100, 50))]
    cases['random_5000'] = graph(counts, e)
    return cases


# --------------------------------------------------------------------------------------------- the chain pairs -> keypoints -> points -> poses
DB, QUERIES = (0, 1, 3, 4, 6, 7), (2, 5)            # of the eight cameras of matcher_scene


def matcher_scene(seed=51, n_points=300, noise=0.5, share=0.7):
    """Six database cameras and two queries between them on the arc of make_cameras, n_points planted points, every image's observation
    of a point fixed once (projection + Gaussian noise, fp32) so that equal coordinates make one keypoint; 15 database pairs and 12
    (query, database) pairs, each holding a random `share` of the points, as the tuples match_many returns (matches [n,4], kpts1, kpts2,
    scores).  The model is not run."""
    rng = np.random.default_rng(seed)
    K, R, t = make_cameras(8, seed)
    X = np.c_[rng.uniform(-2, 2, n_points), rng.uniform(-1.5, 1.5, n_points), rng.uniform(5, 9, n_points)]
    uv = np.array([[project(K[i], R[i], t[i], x) + rng.normal(0, noise, 2) for x in X] for i in range(8)]).astype(np.float32)
    names = [f'/scene/{"query" if i in QUERIES else "db"}/{i}.png' for i in range(8)]
    idx = [(DB[a], DB[b]) for a in range(6) for b in range(a + 1, 6)] + [(q, d) for q in QUERIES for d in DB]
    pairs, results = [], []
    for i, j in idx:
        sel = np.sort(rng.choice(n_points, int(share * n_points), replace=False))
        m = np.concatenate([uv[i, sel], uv[j, sel]], 1)
        pairs.append((names[i], names[j]))
        results.append((m, m[:, :2].copy(), m[:, 2:].copy(), np.ones(len(sel), np.float32)))
    intr = {names[i]: K[i].reshape(3, 3).astype(np.float64) for i in range(8)}
    poses = {names[i]: (R[i], t[i]) for i in range(8)}
    return {'names': names, 'queries': [names[q] for q in QUERIES], 'intrinsics': intr, 'poses': poses,
            'db_poses': {names[i]: poses[names[i]] for i in DB}, 'pairs': pairs, 'results': results, 'X': X, 'uv': uv}


def planted_of_keypoints(scene, cm):
    """per image of cm: the planted point behind each keypoint (the keypoints are the scene's observations, matched by their bits)"""
    out = []
    for name, kp in zip(cm.names, cm.keypoints):
        i = scene['names'].index(name)
        table = {p.tobytes(): k for k, p in enumerate(scene['uv'][i])}
        out.append(np.array([table[np.asarray(p, np.float32).tobytes()] for p in kp], np.int64))
    return out


def host_consolidated(scene):
    """consolidate_matches(pairs, results, qt_psize=0) through the serial host build of the keypoint consolidation"""
    import keypoint_cases as KC
    from geoformer_amd import matcher
    index = {}
    pim = np.array([[index.setdefault(p, len(index)) for p in pr] for pr in scene['pairs']], np.int32)
    ms = [r[0] for r in scene['results']]
    off = np.concatenate([[0], np.cumsum([len(m) for m in ms])]).astype(np.int32)
    kp, kpo, ids, ido, _ = KC.host_consolidate(np.concatenate(ms), np.concatenate([r[3] for r in scene['results']]), off, pim, len(index), psize=0.0,
                                               dthres=0.0)
    return matcher.ConsolidatedMatches(list(index), [kp[kpo[i]:kpo[i + 1]].copy() for i in range(len(index))], pim,
                                       [ids[ido[q]:ido[q + 1]].copy() for q in range(len(ms))])


def host_triangulated(cm, intrinsics, poses, thr=4.0, min_angle=1.5, min_obs=2, refit=2):
    """matcher.triangulate with the serial host build in the place of the device"""
    from geoformer_amd import matcher
    n, kp_off, K, R, t, origin, ids, id_off, kps, pim = matcher._triangulation_inputs(cm, intrinsics, poses)
    g = {'ids': ids, 'id_off': id_off, 'pair_images': pim, 'kp_off': kp_off, 'n_nodes': int(kp_off[-1])}
    st, _, toff, oimg, okp, onode = host_tracks(g)
    assert st == 0
    rc, o = host_triangulate(toff, oimg, kps[onode], K, R, t, pixel_thr=thr, min_angle_deg=min_angle, min_obs=min_obs, refit=refit)
    assert rc == 0
    return matcher._assemble_tracks(n, kp_off, len(toff) - 1, o['X'], o['err2'], o['valid'], o['conflict'], toff, oimg, okp, o['inliers'], origin)


def centre_of(R, t):
    return -np.asarray(R).T @ np.asarray(t)
