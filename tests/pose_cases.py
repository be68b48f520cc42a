"""Planted two-view scenes for the relative-pose tests, and the ctypes front end of the host build of the solver
(geoformer_amd/csrc/host/pose_host.cpp, TEST INFRASTRUCTURE built by geoformer_amd/build.py).

Scene generator (every pose test uses it):
  * R = Rodrigues(v), v ~ N(0, I) * 12 degrees;  t ~ N(0, I), normalised to unit length;
  * world points uniform in [-2.5, 2.5] x [-2, 2] x [4, 10] (camera 0 frame), projected by K = [[500, 0, 320], [0, 500, 240], [0, 0, 1]]
    into both images; keypoints are stored as fp32;
  * an outlier keeps its image-0 keypoint and gets a uniform point of the 640 x 480 second image, re-drawn until its TRUE Sampson
    distance exceeds 10 px (20 x the 0.5 px threshold) - checked here from the ground truth, so an outlier is never a true inlier;
    a match that finds no such point in MAX_REDRAWS draws (its image-0 keypoint sits on the epipole) stays an inlier.
"""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]])
HYP_PER_WG = 32
MAX_REDRAWS = 200


def rodrigues(v):
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def cross_matrix(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def random_pose(rng):
    R = rodrigues(rng.standard_normal(3) * np.deg2rad(12.0))
    t = rng.standard_normal(3)
    return R, t / np.linalg.norm(t)


def world_points(rng, n):
    return np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-2, 2, n), rng.uniform(4, 10, n)], 1)


def sampson_px(E, p0, p1):
    """Sampson distance in pixels (square root of OpenCV's residual, scaled by the focal length) of pixel matches under E."""
    Ki = np.linalg.inv(K)
    x0 = np.c_[p0, np.ones(len(p0))] @ Ki.T
    x1 = np.c_[p1, np.ones(len(p1))] @ Ki.T
    Ex0 = x0 @ E.T
    Etx1 = x1 @ E
    num = np.sum(x1 * Ex0, 1)
    return np.sqrt(num ** 2 / (Ex0[:, 0] ** 2 + Ex0[:, 1] ** 2 + Etx1[:, 0] ** 2 + Etx1[:, 1] ** 2)) * K[0, 0]


def minimal_scene(seed):
    """Five exact matches in normalised fp64 coordinates and the planted E (Frobenius norm 1)."""
    rng = np.random.default_rng(seed)
    R, t = random_pose(rng)
    X = world_points(rng, 5)
    X1 = X @ R.T + t
    E = cross_matrix(t) @ R
    return X[:, :2] / X[:, 2:], X1[:, :2] / X1[:, 2:], E / np.linalg.norm(E)


def scene(seed, n, outlier_frac=0.3, noise_px=0.0):
    """-> dict(mk0, mk1 fp32 [n,2], R, t, T_0to1 [4,4], E, outlier bool [n])"""
    rng = np.random.default_rng(seed)
    R, t = random_pose(rng)
    E = cross_matrix(t) @ R
    X = world_points(rng, n)
    X1 = X @ R.T + t
    p0 = (X / X[:, 2:]) @ K.T
    p1 = (X1 / X1[:, 2:]) @ K.T
    p0, p1 = p0[:, :2].copy(), p1[:, :2].copy()
    n_out = int(round(outlier_frac * n)) if n >= 10 else 0
    outlier = np.zeros(n, bool)
    outlier[rng.permutation(n)[:n_out]] = True
    if noise_px > 0:
        p1[~outlier] += rng.standard_normal((int((~outlier).sum()), 2)) * noise_px
    for i in np.flatnonzero(outlier):
        # (a keypoint next to the epipole of image 0 has E x0 ~ 0: NO second-image point is 10 px from its epipolar "line", so the
        # re-draw is bounded and such a match stays the exact inlier it was)
        outlier[i] = False
        q0 = p0[i:i + 1].astype(np.float32).astype(np.float64)
        for _ in range(MAX_REDRAWS):
            q = np.array([rng.uniform(0, 640), rng.uniform(0, 480)])
            if sampson_px(E, q0, q.astype(np.float32).astype(np.float64)[None])[0] > 10.0:
                p1[i] = q
                outlier[i] = True
                break
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return {'mk0': p0.astype(np.float32), 'mk1': p1.astype(np.float32), 'R': R, 't': t, 'T_0to1': T, 'E': E / np.linalg.norm(E),
            'outlier': outlier}


def pose_errors(R, t, R_gt, t_gt):
    """(R error, t error) in degrees, the t error folded over the sign ambiguity - metrics.py:12-27 in plain numpy."""
    c = np.clip(np.dot(t, t_gt) / (np.linalg.norm(t) * np.linalg.norm(t_gt)), -1, 1)
    te = np.rad2deg(np.arccos(c))
    te = min(te, 180 - te)
    cr = np.clip((np.trace(R.T @ R_gt) - 1) / 2, -1, 1)
    return np.rad2deg(abs(np.arccos(cr))), te


# ---------------------------------------------------------------------------------------------------------------- host build
_host = None


def host_lib():
    global _host
    if _host is None:
        from geoformer_amd import build
        so = build.POSE_HOST_LIB
        if not os.path.exists(so):
            build.build_pose_host(verbose=False)
        h = ctypes.CDLL(so)
        h.gf_pose_host_five_point.restype = ctypes.c_int
        h.gf_pose_host_five_point.argtypes = [ctypes.c_void_p] * 3
        h.gf_pose_host_ransac.restype = ctypes.c_int
        h.gf_pose_host_ransac.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double,
                                          ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 6
        _host = h
    return _host


def host_five_point(x0, x1):
    x0 = np.ascontiguousarray(x0, np.float64)
    x1 = np.ascontiguousarray(x1, np.float64)
    E = np.zeros((10, 3, 3))
    n = host_lib().gf_pose_host_five_point(x0.ctypes.data, x1.ctypes.data, E.ctypes.data)
    return E[:n]


def host_ransac(mk0, mk1, K0=K, K1=K, pixel_thr=0.5, iters=256, seed=0x5EED, sample=0):
    mk0 = np.ascontiguousarray(mk0, np.float32).reshape(-1, 2)
    mk1 = np.ascontiguousarray(mk1, np.float32).reshape(-1, 2)
    k0 = np.ascontiguousarray(K0, np.float32)
    k1 = np.ascontiguousarray(K1, np.float32)
    n = len(mk0)
    E, R, t = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros(3)
    hyp, nin, mask = np.zeros(2, np.int32), np.zeros(1, np.int32), np.zeros(max(n, 1), np.uint8)
    rc = host_lib().gf_pose_host_ransac(mk0.ctypes.data, mk1.ctypes.data, n, k0.ctypes.data, k1.ctypes.data, float(pixel_thr), int(iters),
                                        int(seed), int(sample), E.ctypes.data, R.ctypes.data, t.ctypes.data, hyp.ctypes.data,
                                        nin.ctypes.data, mask.ctypes.data)
    return {'status': rc, 'valid': int(rc == 1), 'E': E, 'R': R, 't': t, 'hyp': hyp, 'n_inliers': int(nin[0]), 'inliers': mask[:n].astype(bool)}
