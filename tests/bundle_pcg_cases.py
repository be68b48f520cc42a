"""The PCG solver of the bundle adjustment (csrc/ba_pcg_spec.h) on the host build, for the CPU tests and as the reference of the GPU tests:
the ctypes wrapper of gf_ba_host_adjust_pcg (run_host_pcg) and the host stand-in of matcher._refine_device.  The scenes are
bundle_cases.py's."""
import ctypes

import numpy as np

import bundle_cases as bc

_bound = False


def host_lib():
    global _bound
    h = bc.host_lib()
    if not _bound:
        h.gf_ba_host_adjust_pcg.restype = ctypes.c_int
        h.gf_ba_host_adjust_pcg.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_double] + [ctypes.c_void_p] * 11
        _bound = True
    return h


def run_host_pcg(obs_off, obs_image, uv, K, R, t, X, free, thr=4.0, iters=16, cg_iters=64, cg_tol=1e-6, cam_free=None, img_off=None, img_obs=None):
    """The host build with the PCG solver on numpy arrays -> (status code, dict like ops.bundle_adjust(solver='pcg')'s)."""
    c = lambda a, d: np.ascontiguousarray(a, dtype=d)
    obs_off, obs_image, uv, K = c(obs_off, np.int32), c(obs_image, np.int32), c(uv, np.float32).reshape(-1, 2), c(K, np.float32).reshape(-1, 9)
    R, t, X = c(R, np.float64).reshape(-1, 9), c(t, np.float64).reshape(-1, 3), c(X, np.float64).reshape(-1, 3)
    n, T, N = len(K), len(obs_off) - 1, len(obs_image)
    free = np.asarray(free).astype(bool)
    if cam_free is None:
        cam_free = np.where(free, np.cumsum(free) - 1, -1)
    cam_free = c(cam_free, np.int32)
    F = int((cam_free >= 0).sum())
    if img_off is None:
        img_off, img_obs = bc.image_major(obs_image, n)
    img_off, img_obs = c(img_off, np.int32), c(img_obs, np.int32)
    iters_a = min(max(int(iters), 0), 64)
    room = max(iters_a, 1)
    o = {'R': np.zeros_like(R), 't': np.zeros_like(t), 'X': np.zeros_like(X), 'inliers': np.zeros(N, np.uint8), 'n_inliers': np.zeros(T, np.int32),
         'cost': np.zeros(iters_a + 1), 'lam': np.zeros(iters_a + 1), 'status': np.zeros(1, np.int32)}
    acc, used, res = np.zeros(room, np.int32), np.zeros(room, np.int32), np.zeros(room)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    rc = host_lib().gf_ba_host_adjust_pcg(p(obs_off), T, N, p(obs_image), p(uv), p(img_off), p(img_obs), p(cam_free), n, F, p(K), p(R), p(t), p(X),
                                          float(thr), int(iters), int(cg_iters), float(cg_tol), p(o['R']), p(o['t']), p(o['X']), p(o['inliers']),
                                          p(o['n_inliers']), p(o['cost']), p(acc), p(o['lam']), p(o['status']), p(used), p(res))
    o['accepted'], o['cg_used'], o['cg_res'] = acc[:iters_a], used[:iters_a], res[:iters_a]
    o['R'] = o['R'].reshape(-1, 3, 3)
    return rc, o


def run_host_pcg_scene(s, free, thr=4.0, iters=16, cg_iters=64, cg_tol=1e-6):
    rc, o = run_host_pcg(s.obs_off, s.obs_image, s.uv, s.K, s.R, s.t, s.X, free, thr, iters, cg_iters, cg_tol)
    assert rc == 0
    return o


def host_refine_device_pcg(a, thrs, iters, device=None, solver='dense', cg_iters=64, cg_tol=1e-6):
    """matcher._refine_device on the host build, either solver: the same inputs and outputs, for the tests without a GPU"""
    if solver == 'dense':
        return bc.host_refine_device(a, thrs, iters, device)
    R, t, X = a['R'], a['t'], a['X']
    costs, accs, used = [], [], []
    for thr in thrs:
        rc, o = run_host_pcg(a['obs_off'], a['obs_image'], a['uv'], a['K'], R, t, X, a['free'], thr, iters, cg_iters, cg_tol)
        assert rc == 0
        R, t, X = o['R'], o['t'], o['X']
        costs.append(o['cost'])
        accs.append(o['accepted'])
        used.append(o['cg_used'])
    return dict(R=R.reshape(-1, 9), t=t, X=X, cost=np.concatenate(costs), accepted=np.concatenate(accs), inliers=o['inliers'],
                cg_used=np.concatenate(used))
