"""Shared inputs of the homography-pair tests (test_homo_data_cpu.py, test_homo_data_gpu.py): images, the homographies of the issue,
PPM files, and the host build of csrc/warp_spec.h (geoformer_amd/csrc/host/warp_host.cpp, TEST INFRASTRUCTURE built by
geoformer_amd/build.py)."""
import ctypes
import os

import numpy as np

H37, W53 = 37, 53
M_IDENTITY = np.eye(3)
M_SHIFT = np.array([[1., 0., 3.], [0., 1., -2.], [0., 0., 1.]])
M_HALF = np.array([[1., 0., .5], [0., 1., 0.], [0., 0., 1.]])
M_OUTSIDE = np.array([[1., 0., 1000.], [0., 1., 1000.], [0., 0., 1.]])
M_PERSPECTIVE = np.array([[0.9, 0.15, 2.], [-0.1, 1.05, 1.5], [0.002, -0.003, 1.]])
MINV_HORIZON = np.array([[1., 0., 0.], [0., 1., 0.], [0., -0.05, 1.]])        # W = 1 - 0.05 y: exactly 0 on row 20, negative below
M_HORIZON = np.linalg.inv(MINV_HORIZON)
# source = 1.3 * destination - (4.3, 2.6): negative source coordinates with a fraction for the first destination pixels of every
# row and column (floor and truncation differ there), inside the source for the rest
M_NEGATIVE = np.linalg.inv(np.array([[1.3, 0., -4.3], [0., 1.3, -2.6], [0., 0., 1.]]))
NAMED = {'identity': M_IDENTITY, 'shift': M_SHIFT, 'half': M_HALF, 'outside': M_OUTSIDE, 'perspective': M_PERSPECTIVE,
         'horizon': M_HORIZON, 'negative': M_NEGATIVE}


def smooth_noisy(h=H37, w=W53, seed=5):
    """A smooth image plus +-6 noise, uint8 [h, w]."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 128 + 70 * np.sin(x / 9.0) * np.cos(y / 7.0) + 20 * np.sin((x + y) / 13.0)
    return np.clip(np.rint(base) + rng.integers(-6, 7, size=(h, w)), 0, 255).astype(np.uint8)


def random_u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def write_ppm(path, rgb):
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    with open(path, 'wb') as f:
        f.write(b'P6\n%d %d\n255\n' % (rgb.shape[1], rgb.shape[0]))
        f.write(rgb.tobytes())


def textured_rgb(h, w, seed):
    """A colour texture with structure at several scales (so a warped copy is recognisably the same picture)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((h, w, 3), dtype=np.uint8)
    for c in range(3):
        f = rng.uniform(5, 17, size=4)
        base = 128 + 50 * np.sin(x / f[0] + c) * np.cos(y / f[1]) + 40 * np.sin((x - y) / f[2]) * np.sin(y / f[3])
        out[..., c] = np.clip(np.rint(base) + rng.integers(-12, 13, size=(h, w)), 0, 255)
    return out


def make_image_dir(root, shapes, seed=0):
    """One generated PPM per (h, w) of `shapes` under root (some in a subdirectory); returns the sorted paths."""
    os.makedirs(os.path.join(root, 'sub'), exist_ok=True)
    paths = []
    for k, (h, w) in enumerate(shapes):
        p = os.path.join(root, 'sub' if k % 3 == 2 else '', f'img{k:02d}.ppm')
        write_ppm(p, textured_rgb(h, w, seed + k))
        paths.append(p)
    return sorted(paths)


_host = None


def host_lib():
    global _host
    if _host is None:
        from geoformer_amd import build
        if not os.path.exists(build.WARP_HOST_LIB):
            build.build_warp_host(verbose=False)
        h = ctypes.CDLL(build.WARP_HOST_LIB)
        h.gf_warp_host_perspective_u8.restype = ctypes.c_int
        h.gf_warp_host_perspective_u8.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p,
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        h.gf_warp_host_position.restype = None
        h.gf_warp_host_position.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        h.gf_warp_host_brightness_contrast.restype = None
        h.gf_warp_host_brightness_contrast.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float]
        _host = h
    return _host


def host_warp(src, M, w, h):
    """csrc/warp_spec.h through its host build: cv2.warpPerspective(src, M, (w, h)) for gray uint8 src."""
    src = np.ascontiguousarray(src, dtype=np.uint8)
    minv = np.ascontiguousarray(np.linalg.inv(np.asarray(M, dtype=np.float64)))
    dst = np.empty((h, w), dtype=np.uint8)
    rc = host_lib().gf_warp_host_perspective_u8(src.ctypes.data, src.shape[0], src.shape[1], src.strides[0], minv.ctypes.data, h, w, dst.ctypes.data)
    assert rc == 0
    return dst


def host_brightness_contrast(values, alpha, beta):
    v = np.ascontiguousarray(values, dtype=np.uint8).copy()
    host_lib().gf_warp_host_brightness_contrast(v.ctypes.data, v.size, alpha, beta)
    return v
