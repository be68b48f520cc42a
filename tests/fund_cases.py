"""Planted two-view scenes for the fundamental-matrix tests, an independent numpy seven-point solver and RANSAC, and the ctypes front
end of the host build of the solver (geoformer_amd/csrc/host/fund_host.cpp, TEST INFRASTRUCTURE built by geoformer_amd/build.py).

Scene generator (every fundamental-matrix test uses it), seeded:
  * camera 0 at the origin, camera 1 at R = Rodrigues(angle * axis), axis uniform on the sphere, angle uniform in [0.05, 0.4] rad;
    t = baseline * direction, direction uniform on the sphere, baseline uniform in [0.3, 1];
  * K = [[500, 0, 320], [0, 500, 240], [0, 0, 1]] for both 640 x 480 images;
  * a point is a uniform pixel of image 0 at a depth uniform in [3, 8]; it is kept when it lies in front of camera 1 (depth > 0.1) and
    projects inside image 1;
  * scene(): keypoints are rounded to fp32; an outlier keeps its image-0 keypoint and gets a uniform point of image 1.
"""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]])
W, H = 640, 480
HYP_PER_WG = 64
MIN_MATCHES = 7
DRAW_ATTEMPTS = 16
SEED = 0x5EED


def rodrigues(v):
    th = np.linalg.norm(v)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def cross_matrix(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def _unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def geometry(rng):
    """-> R, t, F (pixels, x1^T F x0 = 0, Frobenius norm 1)"""
    R = rodrigues(_unit(rng) * rng.uniform(0.05, 0.4))
    t = _unit(rng) * rng.uniform(0.3, 1.0)
    Ki = np.linalg.inv(K)
    F = Ki.T @ cross_matrix(t) @ R @ Ki
    return R, t, F / np.linalg.norm(F)


def visible_points(rng, R, t, n):
    """n exact fp64 correspondences [n, 2], [n, 2] visible in both images"""
    p0, p1 = np.zeros((n, 2)), np.zeros((n, 2))
    k = 0
    while k < n:
        px = np.array([rng.uniform(0, W), rng.uniform(0, H)])
        X = np.linalg.solve(K, np.array([px[0], px[1], 1.0])) * rng.uniform(3.0, 8.0)
        Y = R @ X + t
        if Y[2] <= 0.1:
            continue
        q = (K @ (Y / Y[2]))[:2]
        if not (0 <= q[0] < W and 0 <= q[1] < H):
            continue
        p0[k], p1[k] = (K @ (X / X[2]))[:2], q
        k += 1
    return p0, p1


def box_norm(p0, p1):
    """(cx, cy, s) per image: centre of the bounding box, half its longer side - the conditioning rule of fund_solver.h, in numpy"""
    out = []
    for p in (p0, p1):
        lo, hi = p.min(0).astype(np.float64), p.max(0).astype(np.float64)
        out += [0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), max(0.5 * (hi[0] - lo[0]), 0.5 * (hi[1] - lo[1]))]
    return np.array(out)


def minimal_scene(seed):
    """57 exact fp64 correspondences: the first seven are the minimal problem, 50 are held out; the box over all 57; the planted F."""
    rng = np.random.default_rng(seed)
    R, t, F = geometry(rng)
    p0, p1 = visible_points(rng, R, t, 57)
    return p0, p1, box_norm(p0, p1), F


def scene(seed, n, outlier_frac=0.3):
    """-> dict(m fp32 [n,4], F, outlier bool [n])"""
    rng = np.random.default_rng(seed)
    R, t, F = geometry(rng)
    p0, p1 = visible_points(rng, R, t, n)
    outlier = np.zeros(n, bool)
    outlier[rng.permutation(n)[:int(round(outlier_frac * n))]] = True
    for i in np.flatnonzero(outlier):
        p1[i] = [rng.uniform(0, W), rng.uniform(0, H)]
    return {'m': np.c_[p0, p1].astype(np.float32), 'F': F, 'outlier': outlier}


def sampson_px(F, p0, p1):
    """Sampson distance in pixels (the square root of gs_sampson) of pixel matches under F"""
    x0, x1 = np.c_[p0, np.ones(len(p0))], np.c_[p1, np.ones(len(p1))]
    Fx0, Ftx1 = x0 @ F.T, x1 @ F
    num = np.sum(x1 * Fx0, 1)
    return np.abs(num) / np.sqrt(Fx0[:, 0] ** 2 + Fx0[:, 1] ** 2 + Ftx1[:, 0] ** 2 + Ftx1[:, 1] ** 2)


def line_distance_px(F, p0, p1):
    """distance of p1 from the epipolar line F x0 in image 1"""
    l = np.c_[p0, np.ones(len(p0))] @ F.T
    return np.abs(np.sum(np.c_[p1, np.ones(len(p1))] * l, 1)) / np.hypot(l[:, 0], l[:, 1])


# ---------------------------------------------------------------------------------------------------------------- independent numpy solver
def numpy_seven_point(p0, p1, norm):
    """SVD null space, the cubic through four sampled determinants, numpy.roots; solutions in pixels, Frobenius norm 1."""
    T0 = np.array([[1 / norm[2], 0, -norm[0] / norm[2]], [0, 1 / norm[2], -norm[1] / norm[2]], [0, 0, 1]])
    T1 = np.array([[1 / norm[5], 0, -norm[3] / norm[5]], [0, 1 / norm[5], -norm[4] / norm[5]], [0, 0, 1]])
    x0 = np.c_[p0, np.ones(7)] @ T0.T
    x1 = np.c_[p1, np.ones(7)] @ T1.T
    A = np.einsum('ni,nj->nij', x1, x0).reshape(7, 9)
    if not np.isfinite(A).all():
        return np.zeros((0, 3, 3))
    _, _, vt = np.linalg.svd(A)
    F1, F2 = vt[7].reshape(3, 3), vt[8].reshape(3, 3)
    xs = np.array([-1.0, 0.0, 1.0, 2.0])
    dets = np.array([np.linalg.det(x * F1 + (1 - x) * F2) for x in xs])
    coef = np.linalg.solve(np.vander(xs, 4), dets)                  # descending powers
    out = []
    for z in np.roots(coef):
        if abs(z.imag) < 1e-9 * max(1.0, abs(z.real)):
            F = T1.T @ (z.real * F1 + (1 - z.real) * F2) @ T0
            out.append(F / np.linalg.norm(F))
    return np.array(out).reshape(-1, 3, 3)


def mix32(x):
    x ^= x >> 16; x = (x * 0x85EBCA6B) & 0xFFFFFFFF; x ^= x >> 13; x = (x * 0xC2B2AE35) & 0xFFFFFFFF; x ^= x >> 16
    return x


def draw(seed, sample, t, k, attempt):
    """csrc/gf_hash.h restated"""
    x = (seed * 0x9E3779B1) & 0xFFFFFFFF
    x = mix32(x ^ ((sample + 0x7F4A7C15) & 0xFFFFFFFF))
    x = mix32(x ^ ((t * 0x85EBCA6B + 0x165667B1) & 0xFFFFFFFF))
    x = mix32(x ^ ((k * 0xC2B2AE35 + 0x27D4EB2F) & 0xFFFFFFFF))
    x = mix32(x ^ ((attempt * 0x9E3779B1 + 0x61C88647) & 0xFFFFFFFF))
    return x


def draw7(seed, sample, t, m):
    """fs_draw7 restated over the surviving rows m [cnt, 4]: seven positions, or None"""
    idx = []
    for k in range(7):
        for attempt in range(DRAW_ATTEMPTS):
            c = draw(seed, sample, t, k, attempt) % len(m)
            if all(j != c and not (m[j, 0] == m[c, 0] and m[j, 1] == m[c, 1]) and not (m[j, 2] == m[c, 2] and m[j, 3] == m[c, 3]) for j in idx):
                idx.append(c)
                break
        else:
            return None
    return idx


def numpy_ransac(m, thr=1.0, iters=256, seed=SEED, sample=0):
    """The selection rule of fund_solver.h over the SAME samples (the draw is part of the rule), with the numpy solver; -> mask or None"""
    m = np.asarray(m, np.float32)
    md = m.astype(np.float64)
    norm = box_norm(m[:, :2], m[:, 2:])
    best, mask = -1, None
    for t in range(iters):
        idx = draw7(seed, sample, t, m)
        if idx is None:
            continue
        for F in numpy_seven_point(md[idx, :2], md[idx, 2:], norm):
            inl = sampson_px(F, md[:, :2], md[:, 2:]) ** 2 < thr * thr
            if inl.sum() > best:
                best, mask = int(inl.sum()), inl
    return mask


# ---------------------------------------------------------------------------------------------------------------- host build
_host = None


def host_lib():
    global _host
    if _host is None:
        from geoformer_amd import build
        so = build.build_fund_host(verbose=False)
        h = ctypes.CDLL(so)
        h.gf_fund_host_seven_point.restype = ctypes.c_int
        h.gf_fund_host_seven_point.argtypes = [ctypes.c_void_p] * 4
        h.gf_fund_host_pencil.restype = ctypes.c_int
        h.gf_fund_host_pencil.argtypes = [ctypes.c_void_p] * 3
        h.gf_fund_host_ransac.restype = ctypes.c_int
        h.gf_fund_host_ransac.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_int,
                                          ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 4
        _host = h
    return _host


def host_seven_point(p0, p1, norm):
    p0, p1, norm = (np.ascontiguousarray(a, np.float64) for a in (p0, p1, norm))
    F = np.zeros((3, 3, 3))
    n = host_lib().gf_fund_host_seven_point(p0.ctypes.data, p1.ctypes.data, norm.ctypes.data, F.ctypes.data)
    return F[:n]


def host_pencil(F1, F2):
    F1, F2 = np.ascontiguousarray(F1, np.float64), np.ascontiguousarray(F2, np.float64)
    F = np.full((3, 3, 3), 0.0)
    n = host_lib().gf_fund_host_pencil(F1.ctypes.data, F2.ctypes.data, F.ctypes.data)
    return F[:n]


def host_ransac(m, scores=None, sc_thres=0.25, thr=1.0, iters=256, seed=SEED, sample=0):
    m = np.ascontiguousarray(m, np.float32).reshape(-1, 4)
    n = len(m)
    mm = m if n else np.zeros((1, 4), np.float32)
    sc = None if scores is None else np.ascontiguousarray(scores, np.float32)
    F, hyp, nin, mask = np.zeros((3, 3)), np.zeros(2, np.int32), np.zeros(1, np.int32), np.zeros(max(n, 1), np.uint8)
    rc = host_lib().gf_fund_host_ransac(mm.ctypes.data, None if sc is None or n == 0 else sc.ctypes.data, n, float(sc_thres), float(np.float32(thr)),
                                        int(iters), int(seed), int(sample), F.ctypes.data, hyp.ctypes.data, nin.ctypes.data, mask.ctypes.data)
    return {'status': rc, 'valid': int(rc == 1), 'F': F, 'hyp': hyp, 'n_inliers': int(nin[0]), 'inliers': mask[:n].astype(bool)}
