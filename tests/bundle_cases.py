"""Planted scenes for the bundle-adjustment tests, shared by the CPU tests (host build of csrc/ba_spec.h) and the GPU tests: cameras on an
arc, points in front of them, visibility by projection plus a random drop, pixel noise, optional gross outliers and pose perturbation.
Also the ctypes wrapper of the host build (run_host) and small geometry helpers."""
import ctypes

import numpy as np

W_IMG, H_IMG, FOCAL = 640.0, 480.0, 500.0


def rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-300:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def look_at(centre, target):
    z = target - centre
    z = z / np.linalg.norm(z)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ centre


def project(K, R, t, X):
    Y = X @ R.T + t
    return np.stack([K[0] * Y[:, 0] / Y[:, 2] + K[2], K[4] * Y[:, 1] / Y[:, 2] + K[5]], 1), Y[:, 2]


class Scene:
    """K fp32 [n,9], R_true / t_true and R / t (the perturbed start) fp64, X_true / X fp64 [T,3], obs_off int32 [T+1], obs_image int32 [N],
    uv fp32 [N,2], outlier bool [N] (planted gross outliers)."""

    def centres(self, R=None, t=None):
        R = self.R if R is None else R
        t = self.t if t is None else t
        return -np.einsum('nji,nj->ni', R.reshape(-1, 3, 3), t)


def make_scene(seed, n_cams=12, n_points=400, noise=0.5, drop=0.2, outliers=0.0, rot_deg=1.0, trans=0.05, point_noise=0.02, min_track=2,
               exact=False):
    """exact: fp64-exact observations are impossible (pixels are fp32), so the points are kept and `uv` is the fp32 rounding of the true
    projection: the residual of the true state is then about 2^-24 of a pixel coordinate."""
    rng = np.random.default_rng(seed)
    s = Scene()
    ang = np.linspace(-0.6, 0.6, n_cams)
    centres = np.stack([6.0 * np.sin(ang), 0.3 * np.cos(3 * ang), -6.0 * np.cos(ang) + 6.0], 1)
    Rs, ts = zip(*(look_at(c, np.array([0.0, 0.0, 6.0])) for c in centres))
    s.R_true, s.t_true = np.stack(Rs).reshape(n_cams, 9), np.stack(ts)
    s.K = np.tile(np.array([FOCAL, 0, W_IMG / 2, 0, FOCAL, H_IMG / 2, 0, 0, 1], np.float32), (n_cams, 1))
    X = np.stack([rng.uniform(-2.5, 2.5, n_points), rng.uniform(-1.5, 1.5, n_points), rng.uniform(4.0, 8.0, n_points)], 1)
    off, img, uv, out, keep_pts = [0], [], [], [], []
    proj = [project(s.K[i].astype(np.float64), s.R_true[i].reshape(3, 3), s.t_true[i], X) for i in range(n_cams)]
    for p in range(n_points):
        seen = [i for i in range(n_cams) if proj[i][1][p] > 0 and 0 <= proj[i][0][p, 0] < W_IMG and 0 <= proj[i][0][p, 1] < H_IMG
                and rng.random() >= drop]
        if len(seen) < min_track:
            continue
        keep_pts.append(p)
        for i in seen:
            px = proj[i][0][p] + (0.0 if exact else rng.normal(0, noise, 2))
            bad = rng.random() < outliers
            if bad:
                a = rng.uniform(0, 2 * np.pi)
                px = px + rng.uniform(20.0, 60.0) * np.array([np.cos(a), np.sin(a)])
            img.append(i); uv.append(px); out.append(bad)
        off.append(len(img))
    s.X_true = X[keep_pts]
    s.obs_off, s.obs_image = np.array(off, np.int32), np.array(img, np.int32)
    s.uv, s.outlier = np.array(uv, np.float32).reshape(-1, 2), np.array(out, bool)
    s.R, s.t = s.R_true.copy(), s.t_true.copy()
    if rot_deg > 0 or trans > 0:
        for i in range(n_cams):
            w = rng.normal(size=3)
            w *= np.deg2rad(rot_deg) / np.linalg.norm(w)
            d = rng.normal(size=3)
            d *= trans / np.linalg.norm(d)
            Rn = rodrigues(w) @ s.R_true[i].reshape(3, 3)
            c = -s.R_true[i].reshape(3, 3).T @ s.t_true[i] + d
            s.R[i], s.t[i] = Rn.reshape(9), -Rn @ c
    s.X = s.X_true + (0.0 if exact else rng.normal(0, point_noise, s.X_true.shape))
    return s


def free_flags(scene, fixed=(0, -1)):
    f = np.ones(len(scene.K), bool)
    for i in fixed:
        f[i] = False
    return f


def keep_fixed_true(scene, free):
    """the fixed cameras of a test scene hold their true poses"""
    scene.R[~free], scene.t[~free] = scene.R_true[~free], scene.t_true[~free]
    return scene


def image_major(obs_image, n_images):
    order = np.argsort(obs_image, kind='stable').astype(np.int32)
    off = np.concatenate([[0], np.cumsum(np.bincount(obs_image, minlength=n_images))]).astype(np.int32)
    return off, order


_host = None


def host_lib():
    global _host
    if _host is None:
        from geoformer_amd import build
        _host = ctypes.CDLL(build.build_ba_host(verbose=False))
        _host.gf_ba_host_adjust.restype = ctypes.c_int
        _host.gf_ba_host_adjust.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_int] + [ctypes.c_void_p] * 9
    return _host


def run_host(obs_off, obs_image, uv, K, R, t, X, free, thr=4.0, iters=16, cam_free=None, img_off=None, img_obs=None):
    """The host build on numpy arrays -> (status code, dict like ops.bundle_adjust's).  cam_free / img_off / img_obs override the tables
    derived from `free` and obs_image (for the error tests)."""
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
        img_off, img_obs = image_major(obs_image, n)
    img_off, img_obs = c(img_off, np.int32), c(img_obs, np.int32)
    iters_a = max(int(iters), 0) if int(iters) <= 64 else 64
    o = {'R': np.zeros_like(R), 't': np.zeros_like(t), 'X': np.zeros_like(X), 'inliers': np.zeros(N, np.uint8), 'n_inliers': np.zeros(T, np.int32),
         'cost': np.zeros(iters_a + 1), 'accepted': np.zeros(max(iters_a, 1), np.int32)[:iters_a], 'lam': np.zeros(iters_a + 1),
         'status': np.zeros(1, np.int32)}
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    acc = np.zeros(max(iters_a, 1), np.int32)
    rc = host_lib().gf_ba_host_adjust(p(obs_off), T, N, p(obs_image), p(uv), p(img_off), p(img_obs), p(cam_free), n, F, p(K), p(R), p(t), p(X),
                                      float(thr), int(iters), p(o['R']), p(o['t']), p(o['X']), p(o['inliers']), p(o['n_inliers']), p(o['cost']),
                                      p(acc), p(o['lam']), p(o['status']))
    o['accepted'] = acc[:iters_a]
    o['R'] = o['R'].reshape(-1, 3, 3)
    return rc, o


def run_host_scene(s, free, thr=4.0, iters=16):
    rc, o = run_host(s.obs_off, s.obs_image, s.uv, s.K, s.R, s.t, s.X, free, thr, iters)
    assert rc == 0
    return o


def centre_errors(R, t, s):
    c = -np.einsum('nji,nj->ni', np.asarray(R).reshape(-1, 3, 3), np.asarray(t).reshape(-1, 3))
    return np.linalg.norm(c - s.centres(s.R_true, s.t_true), axis=1)


def gold_fit(s, free, inlier_mask):
    """scipy least_squares over all free poses (rotation vector on the left of the start, translation) and all points at once, on the
    observations of inlier_mask, the other cameras fixed -> (R [n,3,3], t [n,3], X [T,3])."""
    from scipy.optimize import least_squares
    from scipy.sparse import lil_matrix
    n, T = len(s.K), len(s.X)
    fidx = np.where(free)[0]
    slot = {int(i): k for k, i in enumerate(fidx)}
    pt = np.repeat(np.arange(T), np.diff(s.obs_off))
    sel = np.where(inlier_mask)[0]
    K = s.K.astype(np.float64)
    R0, t0 = s.R.reshape(n, 3, 3), s.t
    uv = s.uv.astype(np.float64)

    def unpack(x):
        R, t = R0.copy(), t0.copy()
        for k, i in enumerate(fidx):
            R[i] = rodrigues(x[6 * k:6 * k + 3]) @ R0[i]
            t[i] = x[6 * k + 3:6 * k + 6]
        return R, t, x[6 * len(fidx):].reshape(T, 3)

    def fun(x):
        R, t, X = unpack(x)
        Y = np.einsum('nij,nj->ni', R[s.obs_image[sel]], X[pt[sel]]) + t[s.obs_image[sel]]
        Kk = K[s.obs_image[sel]]
        return np.concatenate([Kk[:, 0] * Y[:, 0] / Y[:, 2] + Kk[:, 2] - uv[sel, 0], Kk[:, 4] * Y[:, 1] / Y[:, 2] + Kk[:, 5] - uv[sel, 1]])

    m = len(sel)
    A = lil_matrix((2 * m, 6 * len(fidx) + 3 * T), dtype=int)
    for r, o in enumerate(sel):
        i = int(s.obs_image[o])
        for half in (0, m):
            if i in slot:
                A[half + r, 6 * slot[i]:6 * slot[i] + 6] = 1
            A[half + r, 6 * len(fidx) + 3 * pt[o]:6 * len(fidx) + 3 * pt[o] + 3] = 1
    x0 = np.concatenate([np.concatenate([np.zeros(3), t0[i]]) for i in fidx] + [s.X.reshape(-1)])
    res = least_squares(fun, x0, jac_sparsity=A, method='trf', x_scale='jac', ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=200)
    return unpack(res.x)


def to_consolidated(s, names=None):
    """The scene as `pairs --keypoints` would have left it: every observation is a keypoint of its image (in observation order), and
    every two observations of a point are a match of their images' pair -> (names, keypoints, pair_images, matches, obs_keypoint)."""
    n = len(s.K)
    names = names or [f'db/im{i:03d}.png' for i in range(n)]
    obs_kp = np.zeros(len(s.obs_image), np.int32)
    count = np.zeros(n, np.int64)
    for o, i in enumerate(s.obs_image):
        obs_kp[o] = count[i]
        count[i] += 1
    keypoints = [s.uv[s.obs_image == i].astype(np.float32) for i in range(n)]
    pairs = {}
    for p in range(len(s.obs_off) - 1):
        obs = range(s.obs_off[p], s.obs_off[p + 1])
        for a in obs:
            for b in obs:
                if s.obs_image[a] < s.obs_image[b]:
                    pairs.setdefault((int(s.obs_image[a]), int(s.obs_image[b])), []).append((obs_kp[a], obs_kp[b]))
    keys = sorted(pairs)
    return names, keypoints, np.array(keys, np.int32).reshape(-1, 2), [np.array(pairs[k], np.int32) for k in keys], obs_kp


def host_refine_device(a, thrs, iters, device=None):
    """matcher._refine_device on the host build: the same inputs and outputs, for the tests without a GPU"""
    R, t, X = a['R'], a['t'], a['X']
    costs, accs = [], []
    for thr in thrs:
        rc, o = run_host(a['obs_off'], a['obs_image'], a['uv'], a['K'], R, t, X, a['free'], thr, iters)
        assert rc == 0
        R, t, X = o['R'], o['t'], o['X']
        costs.append(o['cost'])
        accs.append(o['accepted'])
    return dict(R=R.reshape(-1, 9), t=t, X=X, cost=np.concatenate(costs), accepted=np.concatenate(accs), inliers=o['inliers'])


# ------------------------------------------------------------------------------------------------ scene surgery for the edge cases
def select_obs(s, keep):
    """Only the observations of `keep` (bool [N]); a point left without any is dropped."""
    keep = np.asarray(keep, bool)
    pt = np.repeat(np.arange(len(s.X)), np.diff(s.obs_off))
    cnt = np.bincount(pt[keep], minlength=len(s.X))
    alive = cnt > 0
    s.X, s.X_true = s.X[alive], s.X_true[alive]
    s.obs_off = np.concatenate([[0], np.cumsum(cnt[alive])]).astype(np.int32)
    s.obs_image, s.uv, s.outlier = s.obs_image[keep], s.uv[keep], s.outlier[keep]
    return s


def first_points(s, T):
    return select_obs(s, np.arange(len(s.uv)) < s.obs_off[T])


def limit_camera(s, cam, n_obs):
    """camera `cam` keeps its first n_obs observations"""
    mine = np.where(s.obs_image == cam)[0]
    keep = np.ones(len(s.uv), bool)
    keep[mine[n_obs:]] = False
    return select_obs(s, keep)


def cut_tracks(s, lengths):
    """point p keeps its first lengths[p % len(lengths)] observations (None: all)"""
    keep = np.ones(len(s.uv), bool)
    for p in range(len(s.X)):
        L = lengths[p % len(lengths)]
        if L is not None:
            keep[s.obs_off[p] + L:s.obs_off[p + 1]] = False
    return select_obs(s, keep)


def append_camera(s, R, t, K=None):
    s.K = np.concatenate([s.K, (s.K[:1] if K is None else np.asarray(K, np.float32).reshape(1, 9))])
    for name in ('R', 'R_true'):
        setattr(s, name, np.concatenate([getattr(s, name), np.asarray(R, np.float64).reshape(1, 9)]))
    for name in ('t', 't_true'):
        setattr(s, name, np.concatenate([getattr(s, name), np.asarray(t, np.float64).reshape(1, 3)]))
    return len(s.K) - 1


def append_point(s, X, obs):
    """obs: [(image, (u, v)), ...] with ascending images"""
    s.X = np.concatenate([s.X, np.asarray(X, np.float64).reshape(1, 3)])
    s.X_true = np.concatenate([s.X_true, np.asarray(X, np.float64).reshape(1, 3)])
    s.obs_image = np.concatenate([s.obs_image, np.array([i for i, _ in obs], np.int32)])
    s.uv = np.concatenate([s.uv, np.array([u for _, u in obs], np.float32).reshape(-1, 2)])
    s.outlier = np.concatenate([s.outlier, np.zeros(len(obs), bool)])
    s.obs_off = np.concatenate([s.obs_off, [s.obs_off[-1] + len(obs)]]).astype(np.int32)
    return len(s.X) - 1
