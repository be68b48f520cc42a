"""Bundle adjustment on the device (csrc/k_bundle.hip) against the host build of the same csrc/ba_spec.h, bit for bit, at the smallest shapes
where the kernels can go wrong; the limits and the status codes."""
import numpy as np
import pytest
import torch

import bundle_cases as bc

pytestmark = pytest.mark.gpu
KEYS = ('R', 't', 'X', 'inliers', 'n_inliers', 'cost', 'accepted', 'lam', 'status')
CX, CY = bc.W_IMG / 2, bc.H_IMG / 2


def run_device(s, free, thr, iters, host=True):
    from geoformer_amd import ops
    d = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device='cuda')
    h = {'obs_off': s.obs_off, 'obs_image': s.obs_image, 'free': free} if host else None
    o = ops.bundle_adjust(d(s.obs_off, torch.int32), d(s.obs_image, torch.int32), d(s.uv, torch.float32), d(s.K, torch.float32),
                          d(s.R, torch.float64), d(s.t, torch.float64), d(s.X, torch.float64), d(free, torch.bool), thr=thr, iters=iters, host=h)
    return {k: v.cpu().numpy() for k, v in o.items()}


def both(s, free, thr=20.0, iters=4, host=True):
    dev = run_device(s, free, thr, iters, host)
    ref = bc.run_host_scene(s, free, thr, iters)
    for k in KEYS:
        a, b = np.asarray(dev[k]), np.asarray(ref[k])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
    return dev


def free_cams(s, *cams):
    f = np.zeros(len(s.K), bool)
    f[list(cams)] = True
    return f


@pytest.mark.parametrize('n_free', (1, 2))
def test_one_and_two_free_cameras(n_free):
    s = bc.make_scene(31, n_cams=4, n_points=60)
    o = both(s, free_cams(s, *range(1, 1 + n_free)), iters=16)
    assert o['accepted'].sum() >= 3 and o['status'][0] == 0


def test_128_free_cameras_with_few_observations_each():
    s = bc.make_scene(32, n_cams=130, n_points=150, drop=0.93, min_track=2)
    free = bc.free_flags(s)
    assert free.sum() == 128 and np.bincount(s.obs_image, minlength=130).max() < 40
    o = both(s, free, iters=2)
    assert o['accepted'].any()


def test_cameras_with_5_6_7_observations_and_one_with_outliers_only():
    s = bc.make_scene(33, n_cams=7, n_points=90)
    for cam, n in ((1, 5), (2, 6), (3, 7)):
        bc.limit_camera(s, cam, n)
    s.uv[s.obs_image == 4] += np.float32(100.0)                            # every observation of camera 4 is an outlier: it moves nowhere
    assert np.bincount(s.obs_image)[1:4].tolist() == [5, 6, 7]
    o = both(s, free_cams(s, 1, 2, 3, 4, 5), iters=8)
    assert o['accepted'].any() and not o['inliers'][s.obs_image == 4].any()
    assert np.array_equal(o['R'][4].reshape(9), s.R[4]) and np.array_equal(o['t'][4], s.t[4])


def test_track_lengths_2_3_and_above_64():
    s = bc.make_scene(34, n_cams=70, n_points=24, drop=0.0)
    bc.cut_tracks(s, (2, 3, None, 5))
    L = np.diff(s.obs_off)
    assert (L == 2).any() and (L == 3).any() and L.max() > 64
    o = both(s, bc.free_flags(s, fixed=(0, 1, 35, 69)), iters=3)
    assert o['accepted'].any()


@pytest.mark.parametrize('T', (255, 256, 257))
def test_point_counts_at_the_block_edge(T):
    s = bc.first_points(bc.make_scene(35, n_cams=5, n_points=300, drop=0.1), T)
    assert len(s.X) == T
    both(s, bc.free_flags(s), iters=4)


def test_fixed_only_point_held_point_poseless_image_and_no_free_camera():
    s = bc.make_scene(36, n_cams=6, n_points=80)
    # a point seen by the two fixed cameras only
    p = int(np.argmax([(set(s.obs_image[s.obs_off[q]:s.obs_off[q + 1]]) >= {0, 5}) for q in range(len(s.X))]))
    keep = np.ones(len(s.uv), bool)
    sl = slice(s.obs_off[p], s.obs_off[p + 1])
    keep[sl] = np.isin(s.obs_image[sl], (0, 5))
    bc.select_obs(s, keep)
    # a held point: two fixed cameras on one ray along the world's z axis, so the point's z is free and its damped diagonal entry exactly 0
    a = bc.append_camera(s, np.eye(3), np.zeros(3))
    b = bc.append_camera(s, np.eye(3), np.array([0.0, 0.0, 1.0]))
    bc.append_point(s, [0.0, 0.0, 5.0], [(a, (CX, CY)), (b, (CX, CY))])
    # an image without a pose, with observations
    s.R[3], s.t[3] = np.nan, np.nan
    o = both(s, free_cams(s, 1, 2, 4), iters=6)
    assert o['status'][0] == 2 and o['accepted'].any()
    assert np.array_equal(o['X'][-1], [0.0, 0.0, 5.0]) and np.isnan(o['R'][3]).all()
    # declared free without a pose: status 4, and it still takes no part
    o = both(s, free_cams(s, 1, 2, 3, 4), iters=3)
    assert o['status'][0] == 2 | 4
    # no free camera at all: points only
    o = both(s, free_cams(s), iters=3)
    assert o['accepted'].any() and np.array_equal(np.nan_to_num(o['R'].reshape(-1, 9)), np.nan_to_num(s.R))


def test_a_failed_factorisation_is_a_rejected_step_and_lambda_grows():
    """A free camera whose only observation lies on its optical axis has two columns of exact zeros in its block (rotation about and
    translation along the axis): damping scales the diagonal, so the pivot is 0 at every lambda and every step fails on the device.  (The
    damped Schur complement of a system whose diagonal is positive is positive definite in exact arithmetic - coplanar points seen frontally
    by free cameras factor without trouble - so an exact zero is what makes the factorisation fail at the first lambda.)"""
    s = bc.make_scene(37, n_cams=4, n_points=40)
    a = bc.append_camera(s, np.eye(3), np.zeros(3))
    bc.append_point(s, [0.0, 0.0, 5.0], [(0, bc.project(s.K[0].astype(np.float64), s.R[0].reshape(3, 3), s.t[0], np.array([[0.0, 0.0, 5.0]]))[0][0]),
                                         (a, (CX, CY))])
    o = both(s, free_cams(s, 1, 2, a), iters=5)
    assert o['status'][0] & 1 and not o['accepted'].any()
    assert np.array_equal(o['lam'], 1e-4 * 10.0 ** np.arange(6)) and np.all(o['cost'] == o['cost'][0])
    assert np.array_equal(o['R'].reshape(-1, 9), s.R) and np.array_equal(o['X'], s.X)
    # coplanar points seen frontally, every camera free: the scene that has no anchor.  It must agree bit for bit whatever it does.
    f = bc.make_scene(38, n_cams=3, n_points=50, drop=0.0)
    f.X[:, 2] = 6.0
    both(f, np.ones(3, bool), iters=6)


@pytest.mark.parametrize('iters', (1, 16))
def test_iteration_counts_and_rejected_steps(iters):
    s = bc.make_scene(39, n_cams=6, n_points=120)
    o = both(s, bc.free_flags(s), iters=iters)
    assert o['cost'].shape == (iters + 1,) and np.all(np.diff(o['cost']) <= 0)
    if iters == 16:
        assert o['accepted'].any() and not o['accepted'].all()              # accept and reject both ran on the device


def test_twice_gives_the_same_bits_and_the_tables_may_come_from_the_device():
    s = bc.make_scene(40, n_cams=6, n_points=120, outliers=0.1)
    free = bc.free_flags(s)
    a = both(s, free, iters=8)
    b = run_device(s, free, 20.0, 8, host=False)
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_limits_and_status_codes():
    from geoformer_amd import _lib, ops
    s = bc.make_scene(41, n_cams=4, n_points=30)
    free = bc.free_flags(s)
    for kw in ({'iters': 0}, {'iters': 65}, {'thr': 0.0}, {'thr': float('nan')}):
        with pytest.raises(ValueError):
            run_device(s, free, kw.get('thr', 4.0), kw.get('iters', 4))
    big = bc.make_scene(41, n_cams=4, n_points=30)
    for _ in range(127):
        bc.append_camera(big, big.R[0], big.t[0])
    with pytest.raises(ValueError, match='128'):
        run_device(big, np.ones(131, bool), 4.0, 2)                         # 131 free
    fr = np.ones(131, bool)
    fr[[0, 3]] = False
    with pytest.raises(ValueError, match='129 free cameras, the limit is 128'):
        run_device(big, fr, 4.0, 2)
    fr[1] = False
    both(big, fr, iters=1)                                                  # 128: accepted
    # the entry point's own codes: GF_ERR_INVALID_ARGUMENT (-1) and GF_ERR_WORKSPACE (-2)
    L = _lib.lib()
    d = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device='cuda')
    n, T, N = 4, len(s.X), len(s.uv)
    io, ob = bc.image_major(s.obs_image, n)
    cf = np.where(free, np.cumsum(free) - 1, -1).astype(np.int32)
    dev = [d(x, dt) for x, dt in ((s.obs_off, torch.int32), (s.obs_image, torch.int32), (s.uv, torch.float32), (io, torch.int32), (ob, torch.int32),
                                  (cf, torch.int32), (s.K, torch.float32), (s.R, torch.float64), (s.t, torch.float64), (s.X, torch.float64))]
    outs = [torch.zeros(k, dtype=dt, device='cuda') for k, dt in ((9 * n, torch.float64), (3 * n, torch.float64), (3 * T, torch.float64), (N, torch.uint8),
                                                                   (T, torch.int32), (5, torch.float64), (4, torch.int32), (5, torch.float64), (1, torch.int32))]
    ws = torch.zeros(L.gf_bundle_workspace_bytes(T, N, n, 2), dtype=torch.uint8, device='cuda')
    assert ws.numel() > 0 and L.gf_bundle_workspace_bytes(T, N, n, 129) == 0
    p = lambda x: x.data_ptr()
    hp = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data

    def call(obs_off_host=s.obs_off, cam_free_host=cf, F=2, thr=4.0, iters=4, ws_bytes=None):
        keep = [np.ascontiguousarray(x, np.int32) for x in (obs_off_host, s.obs_image, io, ob, cam_free_host)]
        return L.gf_bundle_adjust(*[k.ctypes.data for k in keep], p(dev[0]), T, N, p(dev[1]), p(dev[2]), p(dev[3]), p(dev[4]), p(dev[5]), n, F,
                                  p(dev[6]), p(dev[7]), p(dev[8]), p(dev[9]), thr, iters, *[p(x) for x in outs], p(ws),
                                  ws.numel() if ws_bytes is None else ws_bytes, torch.cuda.current_stream().cuda_stream)
    assert call() == 0
    torch.cuda.synchronize()
    assert outs[6].sum().item() >= 1
    assert call(ws_bytes=16) == -2 and b'workspace' in L.gf_last_error()
    assert call(iters=65) == -1 and b'iters' in L.gf_last_error()
    assert call(thr=-1.0) == -1 and b'thr' in L.gf_last_error()
    assert call(F=3) == -1 and b'free' in L.gf_last_error()
    bad = s.obs_off.copy()
    bad[1], bad[2] = bad[2], bad[1]
    assert call(obs_off_host=bad) == -1 and b'ascend' in L.gf_last_error()
    assert call(cam_free_host=np.array([-1, 1, 0, -1])) == -1 and b'cam_free' in L.gf_last_error()
