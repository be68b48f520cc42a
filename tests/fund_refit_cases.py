"""Noisy planted scenes for the refit of the fundamental matrix on its inliers (the `refit` rule of geoformer_amd/csrc/fund_solver.h), an
independent numpy restatement of that rule with numpy.linalg.svd, and the ctypes front end of the host build's refit entries
(gf_fund_host_ransac_lo, gf_fund_host_refit_once of geoformer_amd/csrc/host/fund_host.cpp).  Built on tests/fund_cases.py.

noisy_scene(seed, n, outlier_frac, sigma), in this order of draws: rng = default_rng(seed); geometry(rng); visible_points(rng, R, t, n);
visible_points(rng, R, t, 200) held out and exact; p0 += normal(0, sigma), then p1 += normal(0, sigma); the outliers are the first
round(frac n) of rng.permutation(n), each with p1 redrawn uniformly in the image; rows cast to fp32.
"""
import ctypes

import numpy as np

import fund_cases as C

MAX_ROUNDS = 8
MIN_INLIERS = 8


def noisy_scene(seed, n, outlier_frac=0.3, sigma=0.5):
    """-> dict(m fp32 [n,4], F planted, outlier bool [n], h0, h1 [200,2] exact held-out correspondences)"""
    rng = np.random.default_rng(seed)
    R, t, F = C.geometry(rng)
    p0, p1 = C.visible_points(rng, R, t, n)
    h0, h1 = C.visible_points(rng, R, t, 200)
    p0 = p0 + rng.normal(0, sigma, p0.shape)
    p1 = p1 + rng.normal(0, sigma, p1.shape)
    outlier = np.zeros(n, bool)
    outlier[rng.permutation(n)[:int(round(outlier_frac * n))]] = True
    for i in np.flatnonzero(outlier):
        p1[i] = [rng.uniform(0, C.W), rng.uniform(0, C.H)]
    return {'m': np.c_[p0, p1].astype(np.float32), 'F': F, 'outlier': outlier, 'h0': h0, 'h1': h1}


def heldout_error(F, h0, h1):
    """median distance in pixels of the held-out points from their epipolar lines, both directions"""
    return float(np.median(np.r_[C.line_distance_px(F, h0, h1), C.line_distance_px(F.T, h1, h0)]))


def _transforms(norm):
    T0 = np.array([[1 / norm[2], 0, -norm[0] / norm[2]], [0, 1 / norm[2], -norm[1] / norm[2]], [0, 0, 1]])
    T1 = np.array([[1 / norm[5], 0, -norm[3] / norm[5]], [0, 1 / norm[5], -norm[4] / norm[5]], [0, 0, 1]])
    return T0, T1


def numpy_fit(m, mask, norm):
    """normalised eight-point fit on the rows of mask: null vector and rank 2 by SVD; pixels, Frobenius norm 1; None when it fails"""
    md = np.asarray(m, np.float32).astype(np.float64)[np.asarray(mask, bool)]
    T0, T1 = _transforms(norm)
    x0, x1 = np.c_[md[:, :2], np.ones(len(md))] @ T0.T, np.c_[md[:, 2:], np.ones(len(md))] @ T1.T
    A = np.einsum('ni,nj->nij', x1, x0).reshape(-1, 9)
    F = np.linalg.svd(A, full_matrices=True)[2][8].reshape(3, 3)
    U, S, Vt = np.linalg.svd(F)
    F = U @ np.diag([S[0], S[1], 0.0]) @ Vt
    F = T1.T @ (F / np.linalg.norm(F)) @ T0
    nn = np.linalg.norm(F)
    if not (np.isfinite(F).all() and nn > 0):
        return None
    return F / nn


def numpy_refit(m, F, mask, norm, thr, rounds):
    """The accept / stop rule of fund_solver.h around numpy_fit; m: the surviving rows.  -> F, mask, accepted rounds"""
    md = np.asarray(m, np.float32).astype(np.float64)
    mask = np.asarray(mask, bool).copy()
    done = 0
    for _ in range(rounds):
        if mask.sum() < MIN_INLIERS:
            break
        G = numpy_fit(m, mask, norm)
        if G is None:
            break
        cand = C.sampson_px(G, md[:, :2], md[:, 2:]) ** 2 < thr * thr
        if cand.sum() < mask.sum():
            break
        same = np.array_equal(cand, mask)
        F, mask, done = G, cand, done + 1
        if same:
            break
    return F, mask, done


# ---------------------------------------------------------------------------------------------------------------- host build
_bound = False


def host_lib():
    global _bound
    h = C.host_lib()
    if not _bound:
        h.gf_fund_host_ransac_lo.restype = ctypes.c_int
        h.gf_fund_host_ransac_lo.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_int,
                                             ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int] + [ctypes.c_void_p] * 5
        h.gf_fund_host_refit_once.restype = ctypes.c_int
        h.gf_fund_host_refit_once.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _bound = True
    return h


def host_ransac_lo(m, scores=None, sc_thres=0.25, thr=1.0, iters=256, seed=C.SEED, sample=0, refit=0):
    """as fund_cases.host_ransac, with `rounds`"""
    m = np.ascontiguousarray(m, np.float32).reshape(-1, 4)
    n = len(m)
    mm = m if n else np.zeros((1, 4), np.float32)
    sc = None if scores is None else np.ascontiguousarray(scores, np.float32)
    F, hyp, nin, mask = np.zeros((3, 3)), np.zeros(2, np.int32), np.zeros(1, np.int32), np.zeros(max(n, 1), np.uint8)
    rounds = np.full(1, -1, np.int32)
    rc = host_lib().gf_fund_host_ransac_lo(mm.ctypes.data, None if sc is None or n == 0 else sc.ctypes.data, n, float(sc_thres),
                                           float(np.float32(thr)), int(iters), int(seed), int(sample), int(refit), F.ctypes.data,
                                           hyp.ctypes.data, nin.ctypes.data, mask.ctypes.data, rounds.ctypes.data)
    return {'status': rc, 'valid': int(rc == 1), 'F': F, 'hyp': hyp, 'n_inliers': int(nin[0]), 'inliers': mask[:n].astype(bool),
            'rounds': int(rounds[0])}


def host_refit_once(m, mask, norm):
    """one refit of the host build from the inlier set `mask` over the rows m (all taken as surviving) -> F or None"""
    m = np.ascontiguousarray(m, np.float32).reshape(-1, 4)
    mk = np.ascontiguousarray(mask, np.uint8)
    norm = np.ascontiguousarray(norm, np.float64)
    F = np.zeros((3, 3))
    ok = host_lib().gf_fund_host_refit_once(m.ctypes.data, len(m), mk.ctypes.data, norm.ctypes.data, F.ctypes.data)
    return F if ok else None
