"""Pairs for the calibrated two-view tests, and the ctypes front end of the host build of the rule
(geoformer_amd/csrc/host/relpose_host.cpp over csrc/rel_solver.h, TEST INFRASTRUCTURE built by geoformer_amd/build.py).

Scenes are pose_cases.scene's (planted pose, 30 % outliers that are never true inliers, image-1 noise); this file adds
  * rows(sc): the [n, 4] fp32 match rows of a scene;
  * reproject(sc, K0, K1): the same scene seen through other intrinsics (pixels moved by K' K^-1, rounded to fp32 again);
  * noisy_scene(seed): the scenes of the refit gate - scene(seed, 300, 0.3, 0.5) plus 0.5 px noise on image 0 of the planted inliers;
  * with_filtered(m): a copy with rows that the filter must drop - low and NaN scores, NaN / +-inf coordinates, some in the middle of a
    64-row group - and the scores that go with it;
  * planar_scene(seed): near-planar and planar scenes for the record of the rule's limits;
  * batch(): eight pairs of sizes SIZES with per-pair different, anisotropic K0, K1, packed for one call.
"""
import ctypes

import numpy as np

import pose_cases as P

SIZES = (0, 4, 5, 63, 64, 65, 129, 300)
K = P.K
SC_THRES = 0.25


def rows(sc):
    return np.ascontiguousarray(np.concatenate([sc['mk0'], sc['mk1']], 1), np.float32)


def intrinsics(k):
    """anisotropic intrinsics number k (fp32-exact values)"""
    return np.array([[460.0 + 8 * k, 0, 300.0 + 3 * k], [0, 540.0 - 6 * k, 250.0 - 2 * k], [0, 0, 1]])


def reproject(m, K0, K1):
    """rows made with pose_cases.K -> the rows of the same rays under K0, K1"""
    m = np.asarray(m, np.float64).reshape(-1, 4)
    out = np.empty_like(m)
    for s, Kn in ((0, K0), (2, K1)):
        out[:, s] = (m[:, s] - K[0, 2]) / K[0, 0] * Kn[0, 0] + Kn[0, 2]
        out[:, s + 1] = (m[:, s + 1] - K[1, 2]) / K[1, 1] * Kn[1, 1] + Kn[1, 2]
    return out.astype(np.float32)


def noisy_scene(seed):
    sc = P.scene(seed, 300, 0.3, 0.5)
    keep = ~sc['outlier']
    mk0 = sc['mk0'].astype(np.float64)
    mk0[keep] += np.random.default_rng(seed + 5000).standard_normal((int(keep.sum()), 2)) * 0.5
    sc['mk0'] = mk0.astype(np.float32)
    return sc


def planar_scene(seed, n=300, plane_frac=0.9, outlier_frac=0.2, noise_px=0.3):
    """-> (rows [n,4] fp32, R, t, outlier [n], off_plane [n]): the first plane_frac of the world points lie on the plane
    z = 7 + 0.3 x - 0.2 y, image-1 noise, uniform outliers (not re-drawn: an outlier may fall near its epipolar line)"""
    rng = np.random.default_rng(seed)
    R, t = P.random_pose(rng)
    X = P.world_points(rng, n)
    npl = int(round(plane_frac * n))
    X[:npl, 2] = 7 + 0.3 * X[:npl, 0] - 0.2 * X[:npl, 1]
    X1 = X @ R.T + t
    p0, p1 = ((X / X[:, 2:]) @ K.T)[:, :2], ((X1 / X1[:, 2:]) @ K.T)[:, :2]
    out = np.zeros(n, bool)
    out[rng.permutation(n)[:int(round(outlier_frac * n))]] = True
    p1 = p1 + rng.standard_normal((n, 2)) * noise_px
    p1[out] = np.c_[rng.uniform(0, 640, int(out.sum())), rng.uniform(0, 480, int(out.sum()))]
    return np.c_[p0, p1].astype(np.float32), R, t, out, np.arange(n) >= npl


def with_filtered(m, seed=0):
    """-> (rows, scores, gone): `gone` marks the rows the filter drops.  Needs no particular length; short lists lose fewer rows."""
    m = np.array(m, np.float32).reshape(-1, 4)
    n = len(m)
    sc = np.full(n, 0.9, np.float32)
    gone = np.zeros(n, bool)
    plan = [(0, 'low'), (2, 'nan_score'), (31, 'nan'), (32, 'inf'), (33, 'ninf'), (63, 'low'), (64, 'nan'), (100, 'low'), (n - 1, 'inf')]
    for i, what in plan:
        if not 0 <= i < n or gone[i]:
            continue
        gone[i] = True
        if what == 'low':
            sc[i] = 0.2
        elif what == 'nan_score':
            sc[i] = np.nan
        else:
            m[i, (i + seed) % 4] = {'nan': np.nan, 'inf': np.inf, 'ninf': -np.inf}[what]
    return m, sc, gone


def batch(filtered=False, seed0=900):
    """-> dict(m [M,4], scores [M] or None, offsets [9], K0, K1 [8,3,3] fp32, gone [M])"""
    ms, ss, gs, K0s, K1s = [], [], [], [], []
    for k, n in enumerate(SIZES):
        K0, K1 = intrinsics(k), intrinsics(k + 3)
        sc = P.scene(seed0 + k, n, 0.3, 0.3)
        m = reproject(rows(sc), K0, K1)
        if filtered:
            m, s, g = with_filtered(m, k)
            if k == 3:                                # 63 rows, all filtered
                s[:] = 0.1
                g[:] = True
            if k == 4:                                # 64 rows, four left
                drop = np.flatnonzero(~g)[4:]
                s[drop] = 0.1
                g[drop] = True
        else:
            s, g = np.ones(n, np.float32), np.zeros(n, bool)
        ms.append(m.reshape(-1, 4)); ss.append(s); gs.append(g); K0s.append(K0); K1s.append(K1)
    off = np.concatenate([[0], np.cumsum([len(m) for m in ms])]).astype(np.int32)
    return {'m': np.concatenate(ms).astype(np.float32), 'scores': np.concatenate(ss).astype(np.float32) if filtered else None, 'offsets': off,
            'K0': np.stack(K0s).astype(np.float32), 'K1': np.stack(K1s).astype(np.float32), 'gone': np.concatenate(gs)}


# ---------------------------------------------------------------------------------------------------------------- host build
_host = None
_P = ctypes.c_void_p


def host_lib():
    global _host
    if _host is None:
        from geoformer_amd import build
        so = build.build_relpose_host(verbose=False)
        h = ctypes.CDLL(so)
        h.gf_rel_host_ransac.restype = ctypes.c_int
        h.gf_rel_host_ransac.argtypes = [_P, _P, ctypes.c_int, _P, _P, ctypes.c_float, ctypes.c_double, ctypes.c_int, ctypes.c_uint32,
                                         ctypes.c_uint32, ctypes.c_int] + [_P] * 8
        h.gf_rel_host_gn_row.restype = ctypes.c_int
        h.gf_rel_host_gn_row.argtypes = [_P] * 5
        h.gf_rel_host_gn_update.restype = ctypes.c_int
        h.gf_rel_host_gn_update.argtypes = [_P] * 3
        h.gf_rel_host_refit_once.restype = ctypes.c_int
        h.gf_rel_host_refit_once.argtypes = [_P, ctypes.c_int, _P, _P, _P]
        _host = h
    return _host


def host_ransac(m, scores=None, K0=K, K1=K, pixel_thr=1.0, sc_thres=SC_THRES, iters=128, seed=0x5EED, sample=0, refit=0):
    m = np.ascontiguousarray(m, np.float32).reshape(-1, 4)
    n = len(m)
    s = None if scores is None else np.ascontiguousarray(scores, np.float32)
    k0, k1 = np.ascontiguousarray(K0, np.float32), np.ascontiguousarray(K1, np.float32)
    E, R, t = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros(3)
    hyp, nin, nch, rounds = np.zeros(2, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    mask = np.zeros(max(n, 1), np.uint8)
    rc = host_lib().gf_rel_host_ransac(m.ctypes.data, None if s is None else s.ctypes.data, n, k0.ctypes.data, k1.ctypes.data, float(sc_thres),
                                       float(pixel_thr), int(iters), int(seed), int(sample), int(refit), E.ctypes.data, R.ctypes.data,
                                       t.ctypes.data, hyp.ctypes.data, nin.ctypes.data, nch.ctypes.data, mask.ctypes.data, rounds.ctypes.data)
    return {'status': rc, 'valid': int(rc == 1), 'E': E, 'R': R, 't': t, 'hyp': hyp, 'n_inliers': int(nin[0]), 'n_cheiral': int(nch[0]),
            'inliers': mask[:n].astype(bool), 'rounds': int(rounds[0])}


def host_batch(b, pixel_thr=1.0, iters=128, seed=0x5EED, refit=0):
    """the host rule on every pair of batch(): pair n as sample n"""
    off = b['offsets']
    return [host_ransac(b['m'][off[n]:off[n + 1]], None if b['scores'] is None else b['scores'][off[n]:off[n + 1]], b['K0'][n], b['K1'][n],
                        pixel_thr=pixel_thr, iters=iters, seed=seed, sample=n, refit=refit) for n in range(len(off) - 1)]


def normalise(m, K0=K, K1=K):
    """rows [n, 4] fp32 pixels -> fp64 normalised coordinates with ps_normalise's expressions"""
    m = np.asarray(m, np.float32).astype(np.float64).reshape(-1, 4)
    k0, k1 = np.asarray(K0, np.float32).astype(np.float64), np.asarray(K1, np.float32).astype(np.float64)
    return np.stack([(m[:, 0] - k0[0, 2]) / k0[0, 0], (m[:, 1] - k0[1, 2]) / k0[1, 1], (m[:, 2] - k1[0, 2]) / k1[0, 0],
                     (m[:, 3] - k1[1, 2]) / k1[1, 1]], 1)


def host_gn_row(R, t, row4):
    R, t, row4 = (np.ascontiguousarray(a, np.float64) for a in (R, t, row4))
    J, res = np.zeros(5), np.zeros(1)
    ok = host_lib().gf_rel_host_gn_row(R.ctypes.data, t.ctypes.data, row4.ctypes.data, J.ctypes.data, res.ctypes.data)
    return ok, J, float(res[0])


def host_gn_update(d, R, t):
    d = np.ascontiguousarray(d, np.float64)
    R, t = np.array(R, np.float64), np.array(t, np.float64)
    ok = host_lib().gf_rel_host_gn_update(d.ctypes.data, R.ctypes.data, t.ctypes.data)
    return ok, R, t


def host_refit_once(rows4, mask, R, t):
    rows4 = np.ascontiguousarray(rows4, np.float64).reshape(-1, 4)
    mask = np.ascontiguousarray(mask, np.uint8)
    R, t = np.array(R, np.float64), np.array(t, np.float64)
    ok = host_lib().gf_rel_host_refit_once(rows4.ctypes.data, len(rows4), mask.ctypes.data, R.ctypes.data, t.ctypes.data)
    return ok, R, t


def sampson_signed(R, t, x):
    """r = e / sqrt(s) of rows x [n, 4] normalised under E = [t]x R, in numpy"""
    E = P.cross_matrix(t) @ R
    x0 = np.c_[x[:, :2], np.ones(len(x))]
    x1 = np.c_[x[:, 2:], np.ones(len(x))]
    a, b = x0 @ E.T, x1 @ E
    return np.sum(x1 * a, 1) / np.sqrt(a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2)
