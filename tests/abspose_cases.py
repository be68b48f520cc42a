"""Planted localisation scenes for the absolute-pose tests, an independent numpy P3P solver and RANSAC, and the ctypes front end of the
host build of the solver (geoformer_amd/csrc/host/abspose_host.cpp, TEST INFRASTRUCTURE built by geoformer_amd/build.py).

Scene generator (every absolute-pose test uses it), seeded:
  * K = [[500, 0, 320], [0, 500, 240], [0, 0, 1]], image 640 x 480;
  * R = Rodrigues(angle * axis), axis uniform on the sphere, angle uniform in [0.05, 1.2] rad; the camera centre is (120, -45, 30) plus
    uniform +-2 per axis - far from the origin, so the conditioning matters; x_cam = R X + t, t = -R C;
  * a point is a uniform pixel at a depth uniform in [3, 8], taken to the world frame;
  * scene(): pixels (after optional Gaussian noise) and 3-D points are rounded to fp32; an outlier keeps its 3-D point and gets a uniform
    pixel.
"""
import ctypes
import os

import numpy as np

from fund_cases import draw, rodrigues

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]])
K9 = K.astype(np.float32).reshape(9)
W, H = 640, 480
HYP_PER_WG = 64
MIN_ROWS = 4
DRAW_ATTEMPTS = 16
SEED = 0x5EED
CENTRE = np.array([120.0, -45.0, 30.0])


def _unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def geometry(rng):
    """-> R, t with x_cam = R X + t"""
    R = rodrigues(_unit(rng) * rng.uniform(0.05, 1.2))
    C = CENTRE + rng.uniform(-2.0, 2.0, 3)
    return R, -R @ C


def points(rng, R, t, n):
    """n exact fp64 correspondences: pixels [n, 2], world points [n, 3]"""
    px = np.c_[rng.uniform(0, W, n), rng.uniform(0, H, n)]
    depth = rng.uniform(3.0, 8.0, n)
    Xc = (np.linalg.inv(K) @ np.c_[px, np.ones(n)].T).T * depth[:, None]
    return px, (Xc - t) @ R                                       # R^T (Xc - t), row-wise


def box_norm(X):
    """(cx, cy, cz, s): centre of the bounding box of the 3-D points, half its longest side - as_box_norm in numpy"""
    lo, hi = X.min(0).astype(np.float64), X.max(0).astype(np.float64)
    return np.r_[0.5 * (lo + hi), (0.5 * (hi - lo)).max()]


def minimal_scene(seed):
    """three exact fp64 correspondences, the box over 40 points of the same scene, the planted pose"""
    rng = np.random.default_rng(seed)
    R, t = geometry(rng)
    px, X = points(rng, R, t, 40)
    return px[:3], X[:3], box_norm(X), R, t


def scene(seed, n, outlier_frac=0.3, noise=0.0):
    """-> dict(p2d fp32 [n,2], p3d fp32 [n,3], R, t, outlier bool [n])"""
    rng = np.random.default_rng(seed)
    R, t = geometry(rng)
    px, X = points(rng, R, t, n)
    if noise:
        px = px + rng.standard_normal((n, 2)) * noise
    outlier = np.zeros(n, bool)
    outlier[rng.permutation(n)[:int(round(outlier_frac * n))]] = True
    for i in np.flatnonzero(outlier):
        px[i] = [rng.uniform(0, W), rng.uniform(0, H)]
    return {'p2d': px.astype(np.float32), 'p3d': X.astype(np.float32), 'R': R, 't': t, 'outlier': outlier}


def reproj_px(R, t, p2d, p3d, Kmat=K):
    """reprojection error in pixels; inf behind the camera"""
    Y = np.asarray(p3d, np.float64) @ R.T + t
    with np.errstate(all='ignore'):
        q = (Y[:, :2] / Y[:, 2:3]) * np.array([Kmat[0, 0], Kmat[1, 1]]) + np.array([Kmat[0, 2], Kmat[1, 2]])
        e = np.linalg.norm(q - np.asarray(p2d, np.float64), axis=1)
    return np.where(Y[:, 2] > 0, e, np.inf)


def rotation_error_deg(R0, R1):
    return np.degrees(np.arccos(np.clip((np.trace(R0.T @ R1) - 1) / 2, -1, 1)))


def centre(R, t):
    return -R.T @ t


# ---------------------------------------------------------------------------------------------------------------- independent numpy solver
def kabsch(P, Q):
    """R, t with Q ~ R P + t (rows are points), by SVD"""
    pc, qc = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((Q - qc).T @ (P - pc))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return R, qc - R @ pc


def numpy_p3p(px, X, Kmat=K):
    """Grunert's three-point pose: the quartic in v = s3 / s1 built by polynomial arithmetic from the two law-of-cosines relations (not from
    the closed-form coefficients the C++ uses), numpy.roots, Kabsch alignment of the two triangles.  -> list of (R, t), world units."""
    px, X = np.asarray(px, np.float64), np.asarray(X, np.float64)
    if not (np.isfinite(px).all() and np.isfinite(X).all()):
        return []
    j = np.c_[(px[:, 0] - Kmat[0, 2]) / Kmat[0, 0], (px[:, 1] - Kmat[1, 2]) / Kmat[1, 1], np.ones(3)]
    j /= np.linalg.norm(j, axis=1)[:, None]
    a2, b2, c2 = np.sum((X[1] - X[2]) ** 2), np.sum((X[0] - X[2]) ** 2), np.sum((X[0] - X[1]) ** 2)
    ca, cb, cg = j[1] @ j[2], j[0] @ j[2], j[0] @ j[1]
    if min(a2, b2, c2) <= 0:
        return []
    q = (a2 - c2) / b2
    num = np.array([q - 1, -2 * q * cb, 1 + q])                  # u = num(v) / den(v), descending powers
    den = np.array([-2 * ca, 2 * cg])
    law = np.array([1.0, -2 * cb, 1.0])                          # 1 + v^2 - 2 v cos(beta)
    # 1 + u^2 - 2 u cos(gamma) = (c^2 / b^2) (1 + v^2 - 2 v cos(beta)), times den^2
    d2 = np.polymul(den, den)
    poly = np.polysub(np.polyadd(np.polyadd(d2, np.polymul(num, num)), -2 * cg * np.polymul(num, den)), (c2 / b2) * np.polymul(law, d2))
    if not np.isfinite(poly).all() or abs(poly[0]) < 1e-14 * np.abs(poly).max():
        return []
    out = []
    for z in np.roots(poly):
        if abs(z.imag) > 1e-7 * max(1.0, abs(z.real)):
            continue
        v = z.real
        dn = np.polyval(den, v)
        if abs(dn) < 1e-12:
            continue
        u = np.polyval(num, v) / dn
        s1 = np.sqrt(b2 / np.polyval(law, v))
        s = np.array([s1, u * s1, v * s1])
        if not (np.isfinite(s).all() and (s > 0).all()):
            continue
        out.append(kabsch(X, j * s[:, None]))
    return out


def draw3(seed, sample, t, p2d, p3d):
    """as_draw3 restated over the surviving rows: three positions, or None"""
    idx = []
    n = len(p2d)
    for k in range(3):
        for attempt in range(DRAW_ATTEMPTS):
            c = draw(seed, sample, t, k, attempt) % n
            if all(j != c and not (p2d[j] == p2d[c]).all() and not (p3d[j] == p3d[c]).all() for j in idx):
                idx.append(c)
                break
        else:
            return None
    return idx


def numpy_ransac(p2d, p3d, thr=2.0, iters=256, seed=SEED, sample=0):
    """The selection rule of abs_solver.h over the SAME samples (the draw is part of the rule), with the numpy solver.
    -> (mask, R, t, smallest distance of a squared error from thr^2) or None"""
    p2d, p3d = np.asarray(p2d, np.float32), np.asarray(p3d, np.float32)
    best, res = -1, None
    for t in range(iters):
        idx = draw3(seed, sample, t, p2d, p3d)
        if idx is None:
            continue
        sols = numpy_p3p(p2d[idx].astype(np.float64), p3d[idx].astype(np.float64))
        sols.sort(key=lambda s: _root_order(s, p2d[idx], p3d[idx]))
        for R, tt in sols:
            e2 = reproj_px(R, tt, p2d, p3d) ** 2
            inl = e2 < thr * thr
            if inl.sum() > best:
                best, res = int(inl.sum()), (inl, R, tt, float(np.abs(e2 - thr * thr).min()))
    return res


def _root_order(sol, px, X):
    """the quartic's root v = s3 / s1 of a solution: depth of point 3 over depth of point 1 along their bearings"""
    R, t = sol
    Y = np.asarray(X, np.float64) @ R.T + t
    return np.linalg.norm(Y[2]) / np.linalg.norm(Y[0])


# ---------------------------------------------------------------------------------------------------------------- 3-D map lookup
def numpy_lookup(m, x, y):
    """as_xyz_sample in numpy fp64, the same expression order, rounded once to fp32"""
    Hm, Wm = m.shape[:2]
    x, y = np.float64(np.float32(x)), np.float64(np.float32(y))
    nan3 = np.full(3, np.nan, np.float32)
    if not (x >= 0.0 and x <= Wm - 1 and y >= 0.0 and y <= Hm - 1):
        return nan3
    x0, y0 = int(x), int(y)
    x1, y1 = min(x0 + 1, Wm - 1), min(y0 + 1, Hm - 1)
    fx, fy = x - np.float64(x0), y - np.float64(y0)
    p00, p01, p10, p11 = (m[a, b].astype(np.float64) for a, b in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
    if not all(np.isfinite(p).all() for p in (p00, p01, p10, p11)):
        return nan3
    top = p00 * (1.0 - fx) + p01 * fx
    bot = p10 * (1.0 - fx) + p11 * fx
    return (top * (1.0 - fy) + bot * fy).astype(np.float32)


def lookup_maps():
    """two maps of different sizes, 5 x 7 and 33 x 65 (H x W), with NaN holes"""
    rng = np.random.default_rng(77)
    a = rng.uniform(-50, 50, (5, 7, 3)).astype(np.float32)
    b = rng.uniform(-50, 50, (33, 65, 3)).astype(np.float32)
    a[2, 3] = np.nan
    b[10:13, 20:24] = np.nan
    b[32, 64, 1] = np.inf
    b[0, 5, 2] = np.nan
    return a, b


def lookup_points(Hm, Wm, seed):
    """integer coordinates, the last row and column, just outside, negative and non-finite points, and uniform points"""
    rng = np.random.default_rng(seed)
    eps = 1e-3
    pts = [(0, 0), (1, 1), (Wm - 1, Hm - 1), (Wm - 1, 0), (0, Hm - 1), (Wm - 1, 1.5), (2.25, Hm - 1), (Wm - 2, Hm - 2),
           (Wm - 1 + eps, 1), (1, Hm - 1 + eps), (-eps, 1), (1, -eps), (-3, -4), (Wm, Hm), (np.nan, 1), (1, np.inf), (-np.inf, 2),
           (Wm - 1 - eps, Hm - 1 - eps), (0.5, 0.5), (3, 2), (2.5, 1.5)]
    pts += [(rng.uniform(0, Wm - 1), rng.uniform(0, Hm - 1)) for _ in range(60)]
    return np.array(pts, np.float32)


# ---------------------------------------------------------------------------------------------------------------- host build
_host = None
_vp = ctypes.c_void_p


def host_lib():
    global _host
    if _host is None:
        from geoformer_amd import build
        h = ctypes.CDLL(build.build_abspose_host(verbose=False))
        h.gf_abs_host_p3p.restype = ctypes.c_int
        h.gf_abs_host_p3p.argtypes = [_vp] * 5
        h.gf_abs_host_refit_once.restype = ctypes.c_int
        h.gf_abs_host_refit_once.argtypes = [_vp, _vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]
        h.gf_abs_host_xyz_lookup.restype = None
        h.gf_abs_host_xyz_lookup.argtypes = [_vp, _vp, _vp, ctypes.c_int, _vp, _vp, ctypes.c_long, ctypes.c_int, _vp]
        h.gf_abs_host_ransac.restype = ctypes.c_int
        h.gf_abs_host_ransac.argtypes = [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_float, ctypes.c_double, ctypes.c_int, ctypes.c_uint32,
                                         ctypes.c_uint32, ctypes.c_int] + [_vp] * 6
        _host = h
    return _host


def host_p3p(px, X, norm, K9_=K9):
    """-> list of (R, t) in world units, in the order of the quartic's roots"""
    px, X, norm = (np.ascontiguousarray(a, np.float64) for a in (px, X, norm))
    k = np.ascontiguousarray(K9_, np.float32)
    out = np.full((4, 12), np.nan)
    n = host_lib().gf_abs_host_p3p(px.ctypes.data, X.ctypes.data, k.ctypes.data, norm.ctypes.data, out.ctypes.data)
    return [(out[r, :9].reshape(3, 3).copy(), out[r, 9:].copy()) for r in range(n)]


def host_refit_once(p2d, p3d, mask, norm, R, t, K9_=K9):
    """one round's Gauss-Newton fit from the CONDITIONED pose (R, t') -> (ok, R, t')"""
    p2d, p3d = np.ascontiguousarray(p2d, np.float32), np.ascontiguousarray(p3d, np.float32)
    mask = np.ascontiguousarray(mask, np.uint8)
    norm, R, t = np.ascontiguousarray(norm, np.float64), np.array(R, np.float64).copy(), np.array(t, np.float64).copy()
    k = np.ascontiguousarray(K9_, np.float32)
    ok = host_lib().gf_abs_host_refit_once(p2d.ctypes.data, p3d.ctypes.data, len(p2d), mask.ctypes.data, k.ctypes.data, norm.ctypes.data,
                                           R.ctypes.data, t.ctypes.data)
    return ok, R, t


def host_xyz_lookup(maps, pair_offsets, pts):
    """maps: list of fp32 [H, W, 3]; pair_offsets [P + 1]; pts fp32 [M, 2] -> fp32 [M, 3]"""
    maps = [np.ascontiguousarray(m, np.float32) for m in maps]
    P, M = len(maps), len(pts)
    ptrs = (ctypes.c_void_p * max(P, 1))(*[m.ctypes.data for m in maps])
    Hs = np.array([m.shape[0] for m in maps] or [0], np.int32)
    Ws = np.array([m.shape[1] for m in maps] or [0], np.int32)
    off = np.ascontiguousarray(pair_offsets, np.int32)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    out = np.zeros((max(M, 1), 3), np.float32)
    host_lib().gf_abs_host_xyz_lookup(ctypes.cast(ptrs, _vp), Hs.ctypes.data, Ws.ctypes.data, P, off.ctypes.data,
                                      pts.ctypes.data if M else None, 2, M, out.ctypes.data)
    return out[:M]


def host_ransac(p2d, p3d, scores=None, sc_thres=0.25, thr=2.0, iters=256, seed=SEED, sample=0, refit=0, K9_=K9):
    p2d = np.ascontiguousarray(p2d, np.float32).reshape(-1, 2)
    p3d = np.ascontiguousarray(p3d, np.float32).reshape(-1, 3)
    n = len(p2d)
    a = p2d if n else np.zeros((1, 2), np.float32)
    b = p3d if n else np.zeros((1, 3), np.float32)
    sc = None if scores is None else np.ascontiguousarray(scores, np.float32)
    k = np.ascontiguousarray(K9_, np.float32)
    R, t, hyp, nin = np.zeros((3, 3)), np.zeros(3), np.zeros(2, np.int32), np.zeros(1, np.int32)
    mask, rounds = np.zeros(max(n, 1), np.uint8), np.zeros(1, np.int32)
    rc = host_lib().gf_abs_host_ransac(a.ctypes.data, b.ctypes.data, None if sc is None or n == 0 else sc.ctypes.data, n, k.ctypes.data,
                                       float(sc_thres), float(np.float32(thr)), int(iters), int(seed), int(sample), int(refit), R.ctypes.data,
                                       t.ctypes.data, hyp.ctypes.data, nin.ctypes.data, mask.ctypes.data, rounds.ctypes.data)
    return {'status': rc, 'valid': int(rc == 1), 'R': R, 't': t, 'hyp': hyp, 'n_inliers': int(nin[0]), 'inliers': mask[:n].astype(bool),
            'rounds': int(rounds[0])}
