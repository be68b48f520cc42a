"""Shared by the lens-distortion tests: ctypes wrappers of the serial host build (csrc/host/camera_host.cpp over csrc/camera_spec.h), the
planted cameras, a numpy longdouble gold that does not read the header, and the distorted matcher_scene of the chain tests."""
import ctypes

import numpy as np

LD = np.longdouble

# the five models with the parameter sets of the prototype (COLMAP's parameter order)
CAMERAS = {
    'simple_pinhole': ('SIMPLE_PINHOLE', (1000.0, 640.0, 480.0)),
    'pinhole': ('PINHOLE', (1000.0, 1010.0, 640.0, 480.0)),
    'simple_radial_p0.1': ('SIMPLE_RADIAL', (1000.0, 640.0, 480.0, 0.1)),
    'simple_radial_m0.1': ('SIMPLE_RADIAL', (1000.0, 640.0, 480.0, -0.1)),
    'simple_radial_m0.3': ('SIMPLE_RADIAL', (1000.0, 640.0, 480.0, -0.3)),
    'radial': ('RADIAL', (1000.0, 640.0, 480.0, -0.2, 0.05)),
    'opencv': ('OPENCV', (900.0, 950.0, 700.0, 500.0, -0.25, 0.08, 1e-3, -2e-3)),
}

_host = None


def host_lib():
    global _host
    if _host is None:
        import os
        from geoformer_amd import build
        if not os.path.exists(build.CAMERA_HOST_LIB):
            build.build_camera_host(verbose=False)
        h = ctypes.CDLL(build.CAMERA_HOST_LIB)
        vp, ci, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        h.gf_camera_host_points.restype = ci
        h.gf_camera_host_points.argtypes = [vp, ctypes.c_long, ci, vp, vp, ci, vp, ci, ci, vp, vp, vp]
        h.gf_camera_host_undistort.restype, h.gf_camera_host_undistort.argtypes = ci, [vp, dbl, dbl, vp, vp]
        h.gf_camera_host_distort.restype, h.gf_camera_host_distort.argtypes = ci, [vp, dbl, dbl, vp, vp]
        _host = h
    return _host


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def camera(key):
    from geoformer_amd import matcher
    model, params = CAMERAS[key]
    return matcher.Camera(model, 1280, 960, params)


def record(cam):
    from geoformer_amd import matcher
    return np.array(matcher.canonical_camera(cam), np.float64)


def host_points(block, col, seg_off, seg_cam, table, inverse=1, P=None):
    """The serial build on rows of a float32 [P, W] block, (x, y) at columns col, col + 1, read in place with stride W ->
    (rc, out [P, 2], status [P], flags [2])."""
    block = np.ascontiguousarray(block, np.float32)
    P = len(block) if P is None else P
    W = block.shape[1] if block.ndim == 2 and block.size else 2
    seg_off, seg_cam = np.ascontiguousarray(seg_off, np.int32), np.ascontiguousarray(seg_cam, np.int32)
    table = np.ascontiguousarray(table, np.float64).reshape(-1, 8)
    out = np.zeros((max(P, 1), 2), np.float32)
    status, flags = np.zeros(max(P, 1), np.uint8), np.zeros(2, np.int32)
    base = block.ctypes.data + 4 * col if block.size else None
    rc = host_lib().gf_camera_host_points(base, W, P, _p(seg_off), _p(seg_cam), len(seg_cam), _p(table) if table.size else None, len(table), inverse,
                                          _p(out), _p(status), _p(flags))
    return rc, out[:max(P, 0)], status[:max(P, 0)], flags


def host_one(cam, pts, inverse=1):
    """one list of one camera through the serial build -> (out, status)"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    rc, out, st, flags = host_points(pts, 0, [0, len(pts)], [0], record(cam), inverse)
    assert rc == 0 and not flags.any()
    return out, st


# --------------------------------------------------------------------------------------------- the gold: numpy longdouble, not the header
def np_distort(rec, x, y):
    """the closed form on arrays; rec, x and y in one float type, which carries through"""
    k1, k2, p1, p2 = rec[4:]
    r2 = x * x + y * y
    rad = 1 + k1 * r2 + k2 * r2 * r2
    return x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y


def np_jacobian(rec, x, y):
    k1, k2, p1, p2 = rec[4:]
    r2 = x * x + y * y
    rad = 1 + k1 * r2 + k2 * r2 * r2
    g = 2 * (k1 + 2 * k2 * r2)
    j00 = rad + g * x * x + 2 * p1 * y + 6 * p2 * x
    j01 = g * x * y + 2 * p1 * x + 2 * p2 * y
    j11 = rad + g * y * y + 6 * p1 * y + 2 * p2 * x
    return j00, j01, j01, j11


def in_domain_points(rec, n, seed, radius=1.0):
    """n ideal points (normalised, float64) in the disc of `radius` whose whole ray from the centre has a Jacobian determinant > 0: inside
    the first fold of the model."""
    rng = np.random.default_rng(seed)
    xs, ys = [], []
    while len(xs) < n:
        r, a = radius * np.sqrt(rng.uniform(0, 1, 2 * n)), rng.uniform(0, 2 * np.pi, 2 * n)
        x, y = r * np.cos(a), r * np.sin(a)
        ok = np.ones(2 * n, bool)
        for s in np.linspace(1 / 32, 1.0, 32):
            j00, j01, j10, j11 = np_jacobian(rec, s * x, s * y)
            ok &= j00 * j11 - j01 * j10 > 0
        xs += x[ok].tolist()
        ys += y[ok].tolist()
    return np.array(xs[:n]), np.array(ys[:n])


def distorted_pixels(rec, x, y):
    """ideal normalised points -> their real-image pixels, formed in longdouble and rounded once to fp32: [n, 2]"""
    r = rec.astype(LD)
    xd, yd = np_distort(r, x.astype(LD), y.astype(LD))
    return np.stack([(r[0] * xd + r[2]).astype(np.float32), (r[1] * yd + r[3]).astype(np.float32)], 1)


def gold_undistort(rec, px, steps=60):
    """fp32 pixels [n, 2] -> (ideal pixels fp32 [n, 2]: 60 plain Newton steps in longdouble from the target, the pixel formed in longdouble
    and rounded once to fp32; the largest residual left, in normalised units)"""
    r = rec.astype(LD)
    tx, ty = (px[:, 0].astype(LD) - r[2]) / r[0], (px[:, 1].astype(LD) - r[3]) / r[1]
    x, y = tx.copy(), ty.copy()
    for _ in range(steps):
        dx, dy = np_distort(r, x, y)
        f0, f1 = dx - tx, dy - ty
        j00, j01, j10, j11 = np_jacobian(r, x, y)
        det = j00 * j11 - j01 * j10
        x, y = x - (j11 * f0 - j01 * f1) / det, y - (j00 * f1 - j10 * f0) / det
    dx, dy = np_distort(r, x, y)
    res = float(max(np.abs(dx - tx).max(), np.abs(dy - ty).max())) if len(px) else 0.0
    return np.stack([(r[0] * x + r[2]).astype(np.float32), (r[1] * y + r[3]).astype(np.float32)], 1), res


def ulps_apart(a, b):
    """|a - b| in units of the fp32 spacing at the larger magnitude, per element"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


# --------------------------------------------------------------------------------------------- the distorted scene of the chain tests
def scene_cameras(scene, k):
    """The cameras of triangulate_cases.matcher_scene with the radial term k.  The scene's cameras have fy = 1.01 fx, which SIMPLE_RADIAL
    cannot say, so the term is planted as k1 of an OPENCV camera with k2 = p1 = p2 = 0: the same radial polynomial."""
    from geoformer_amd import matcher
    out = {}
    for name in scene['names']:
        K = scene['intrinsics'][name]
        out[name] = matcher.Camera('OPENCV', 1600, 1200, (K[0, 0], K[1, 1], K[0, 2], K[1, 2], float(k), 0.0, 0.0, 0.0))
    return out


def distorted_scene(scene, cams):
    """matcher_scene with every observation pushed through its camera's model (longdouble, rounded once to fp32): uv and the results'
    coordinates.  Equal observations stay equal."""
    uvd = np.zeros_like(scene['uv'])
    for i, name in enumerate(scene['names']):
        rec = record(cams[name])
        uv = scene['uv'][i].astype(np.float64)
        uvd[i] = distorted_pixels(rec, (uv[:, 0] - rec[2]) / rec[0], (uv[:, 1] - rec[3]) / rec[1])
    results = []
    for (a, b), r in zip(scene['pairs'], scene['results']):
        cols = []
        for side, name in enumerate((a, b)):
            i = scene['names'].index(name)
            table = {p.tobytes(): k for k, p in enumerate(scene['uv'][i])}
            sel = np.array([table[np.ascontiguousarray(p, np.float32).tobytes()] for p in r[0][:, 2 * side:2 * side + 2]])
            cols.append(uvd[i][sel])
        m = np.concatenate(cols, 1)
        results.append((m, m[:, :2].copy(), m[:, 2:].copy(), r[3]))
    return dict(scene, uv=uvd, results=results)


def host_undistorted_results(pairs, results, cams):
    """matcher.undistort_results with the serial host build in the place of the device -> (results', status per pair)"""
    from geoformer_amd import matcher
    index = {}
    pim = np.array([[index.setdefault(p, len(index)) for p in pr] for pr in pairs], np.int32).reshape(-1, 2)
    table = np.array([record(cams[n]) for n in index])
    ms = matcher._original_pixel_rows(results)
    off = np.concatenate([[0], np.cumsum([len(m) for m in ms])]).astype(np.int32)
    rows = np.concatenate(ms) if len(ms) else np.zeros((0, 4), np.float32)
    sides = []
    for s in (0, 1):
        rc, out, st, flags = host_points(rows, 2 * s, off, pim[:, s], table)
        assert rc == 0 and not flags.any()
        sides.append((out, st))
    res, status = [], []
    for p, r in enumerate(results):
        b, e = off[p], off[p + 1]
        k0, k1 = sides[0][0][b:e].copy(), sides[1][0][b:e].copy()
        m = np.concatenate([k0, k1], 1)
        res.append((m, k0, k1, r[3], np.ones(4)) if len(r) > 4 else (m, k0, k1, r[3]))
        status.append(np.stack([sides[0][1][b:e], sides[1][1][b:e]], 1))
    return res, status


def with_uv_of_results(scene, results):
    """the scene whose uv table holds, per image, the coordinates `results` has for each planted point (NaN where it has none): what
    planted_points_of looks keypoints up in"""
    uv = np.full_like(scene['uv'], np.nan)
    for (a, b), r0, r in zip(scene['pairs'], scene['results'], results):
        for side, name in enumerate((a, b)):
            i = scene['names'].index(name)
            table = {p.tobytes(): k for k, p in enumerate(scene['uv'][i])}
            sel = np.array([table[np.ascontiguousarray(p, np.float32).tobytes()] for p in r0[0][:, 2 * side:2 * side + 2]])
            uv[i][sel] = r[0][:, 2 * side:2 * side + 2]
    return dict(scene, uv=uv, results=results)


def point_errors(scene, cm, tt):
    """distance of every triangulated point from the planted point its observations belong to (a track holds one planted point's)"""
    import triangulate_cases as C
    planted = C.planted_of_keypoints(scene, cm)
    err = np.zeros(len(tt.points))
    for k in range(len(tt.points)):
        a, b = tt.obs_offsets[k], tt.obs_offsets[k + 1]
        ids = {int(planted[i][kp]) for i, kp in zip(tt.obs_image[a:b], tt.obs_keypoint[a:b])}
        assert len(ids) == 1
        err[k] = np.linalg.norm(tt.points[k] - scene['X'][ids.pop()])
    return err
