"""Bundle adjustment with the PCG solver on the device (the ba_pcg_* kernels of csrc/k_bundle.hip) against the host build of the same
csrc/ba_pcg_spec.h, bit for bit on every output, the two CG logs included, at the smallest shapes where each kernel can go wrong; the limits
and the status codes of gf_bundle_adjust_pcg."""
import numpy as np
import pytest
import torch

import bundle_cases as bc
import bundle_pcg_cases as pc

pytestmark = pytest.mark.gpu
KEYS = ('R', 't', 'X', 'inliers', 'n_inliers', 'cost', 'accepted', 'lam', 'status')
PCG_KEYS = KEYS + ('cg_used', 'cg_res')
CX, CY = bc.W_IMG / 2, bc.H_IMG / 2


def run_device(s, free, thr, iters, host=True, **kw):
    from geoformer_amd import ops
    d = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device='cuda')
    h = {'obs_off': s.obs_off, 'obs_image': s.obs_image, 'free': free} if host else None
    o = ops.bundle_adjust(d(s.obs_off, torch.int32), d(s.obs_image, torch.int32), d(s.uv, torch.float32), d(s.K, torch.float32),
                          d(s.R, torch.float64), d(s.t, torch.float64), d(s.X, torch.float64), d(free, torch.bool), thr=thr, iters=iters, host=h,
                          **kw)
    return {k: v.cpu().numpy() for k, v in o.items()}


def both(s, free, thr=20.0, iters=4, host=True, cg_iters=64, cg_tol=1e-6):
    dev = run_device(s, free, thr, iters, host, solver='pcg', cg_iters=cg_iters, cg_tol=cg_tol)
    ref = pc.run_host_pcg_scene(s, free, thr, iters, cg_iters, cg_tol)
    assert set(dev) == set(PCG_KEYS)
    for k in PCG_KEYS:
        a, b = np.asarray(dev[k]), np.asarray(ref[k])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
    assert np.all(dev['cg_used'] <= cg_iters)
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


def test_129_free_cameras_most_of_which_see_nothing():
    """the 131-camera scene of test_bundle_gpu.py's limits test: one more free camera than the dense solver takes"""
    big = bc.make_scene(41, n_cams=4, n_points=30)
    for _ in range(127):
        bc.append_camera(big, big.R[0], big.t[0])
    fr = np.ones(131, bool)
    fr[[0, 3]] = False
    o = both(big, fr, thr=4.0, iters=2)
    assert np.array_equal(o['R'].reshape(-1, 9)[4:], big.R[4:]) and np.array_equal(o['t'][4:], big.t[4:])   # identity blocks move nowhere
    with pytest.raises(ValueError, match='129 free cameras, the limit is 128'):
        run_device(big, fr, 4.0, 2)


@pytest.mark.parametrize('F', (255, 256, 257))
def test_free_camera_counts_at_the_block_edge_of_the_inner_product(F):
    s = bc.make_scene(32, n_cams=F + 2, n_points=150, drop=0.93, min_track=2)
    free = bc.free_flags(s)
    assert free.sum() == F
    o = both(s, free, iters=2)
    assert o['accepted'].any() and o['cg_used'].min() >= 1


@pytest.mark.parametrize('n', (255, 256, 257))
def test_cameras_with_1_n_and_more_than_512_observations(n):
    s = bc.make_scene(33, n_cams=5, n_points=700, drop=0.1)
    bc.limit_camera(s, 1, 1)
    bc.limit_camera(s, 2, n)
    cnt = np.bincount(s.obs_image, minlength=5)
    assert cnt[1] == 1 and cnt[2] == n and cnt[3] > 512
    o = both(s, free_cams(s, 1, 2, 3), iters=4)
    assert o['accepted'].any()


def test_a_camera_with_outliers_only_gets_the_identity_block():
    s = bc.make_scene(33, n_cams=7, n_points=90)
    s.uv[s.obs_image == 4] += np.float32(100.0)
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
    p = int(np.argmax([(set(s.obs_image[s.obs_off[q]:s.obs_off[q + 1]]) >= {0, 5}) for q in range(len(s.X))]))
    keep = np.ones(len(s.uv), bool)
    sl = slice(s.obs_off[p], s.obs_off[p + 1])
    keep[sl] = np.isin(s.obs_image[sl], (0, 5))                            # a point seen by the two fixed cameras only
    bc.select_obs(s, keep)
    a = bc.append_camera(s, np.eye(3), np.zeros(3))                        # a held point: see test_bundle_gpu.py
    b = bc.append_camera(s, np.eye(3), np.array([0.0, 0.0, 1.0]))
    bc.append_point(s, [0.0, 0.0, 5.0], [(a, (CX, CY)), (b, (CX, CY))])
    s.R[3], s.t[3] = np.nan, np.nan                                        # an image without a pose, with observations
    o = both(s, free_cams(s, 1, 2, 4), iters=6)
    assert o['status'][0] == 2 and o['accepted'].any()
    assert np.array_equal(o['X'][-1], [0.0, 0.0, 5.0]) and np.isnan(o['R'][3]).all()
    o = both(s, free_cams(s, 1, 2, 3, 4), iters=3)                         # declared free without a pose: status 4, an identity block
    assert o['status'][0] == 2 | 4
    o = both(s, free_cams(s), iters=3)                                     # no free camera at all: points only, no CG
    assert o['accepted'].any() and np.array_equal(np.nan_to_num(o['R'].reshape(-1, 9)), np.nan_to_num(s.R))
    assert not o['cg_used'].any() and not o['cg_res'].any()


def test_a_singular_camera_block_fails_every_step_and_lambda_grows():
    """The optical-axis camera of test_bundle_gpu.py: two columns of exact zeros in M_f at every lambda, so gs_solve<6> fails its pivot test."""
    s = bc.make_scene(37, n_cams=4, n_points=40)
    a = bc.append_camera(s, np.eye(3), np.zeros(3))
    bc.append_point(s, [0.0, 0.0, 5.0], [(0, bc.project(s.K[0].astype(np.float64), s.R[0].reshape(3, 3), s.t[0], np.array([[0.0, 0.0, 5.0]]))[0][0]),
                                         (a, (CX, CY))])
    o = both(s, free_cams(s, 1, 2, a), iters=5)
    assert o['status'][0] & 1 and not o['accepted'].any() and not o['cg_used'].any()
    assert np.array_equal(o['lam'], 1e-4 * 10.0 ** np.arange(6)) and np.all(o['cost'] == o['cost'][0])
    assert np.array_equal(o['R'].reshape(-1, 9), s.R) and np.array_equal(o['X'], s.X)
    f = bc.make_scene(38, n_cams=3, n_points=50, drop=0.0)                 # coplanar points, every camera free: whatever it does, the same bits
    f.X[:, 2] = 6.0
    both(f, np.ones(3, bool), iters=6)


def test_cg_stopping_by_the_cap_by_rho_and_by_the_tolerance():
    s = bc.make_scene(39, n_cams=6, n_points=120)
    free = bc.free_flags(s)
    o = both(s, free, iters=6, cg_iters=1)                                 # never converges: the steps are still judged by their cost
    assert np.all(o['cg_used'] == 1) and np.all(o['cg_res'] > 1e-12) and np.all(np.diff(o['cost']) <= 0) and o['accepted'].any()
    o = both(s, free_cams(s, 2), iters=4, cg_iters=256, cg_tol=0.0)        # F = 1: until rho' <= 0, or the cap
    assert np.all(o['cg_used'] >= 1)
    o = both(s, free, iters=6)                                             # the defaults stop early: the remaining launches return
    assert (o['cg_used'] < 64).any() and np.all(o['cg_res'][o['cg_used'] < 64] <= 1e-12)


@pytest.mark.parametrize('iters', (1, 16))
def test_iteration_counts_and_rejected_steps(iters):
    s = bc.make_scene(39, n_cams=6, n_points=120)
    o = both(s, bc.free_flags(s), iters=iters)
    assert o['cost'].shape == (iters + 1,) and o['cg_used'].shape == (iters,) and np.all(np.diff(o['cost']) <= 0)
    if iters == 16:
        assert o['accepted'].any() and not o['accepted'].all()


def test_twice_gives_the_same_bits_and_the_tables_may_come_from_the_device():
    s = bc.make_scene(40, n_cams=6, n_points=120, outliers=0.1)
    free = bc.free_flags(s)
    a = both(s, free, iters=8)
    b = run_device(s, free, 20.0, 8, host=False, solver='pcg')
    for k in PCG_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_the_dense_solver_is_untouched_by_the_new_arguments():
    s = bc.make_scene(40, n_cams=6, n_points=120, outliers=0.1)
    free = bc.free_flags(s)
    dev = run_device(s, free, 20.0, 8, solver='dense', cg_iters=3, cg_tol=0.5)
    ref = bc.run_host_scene(s, free, 20.0, 8)
    assert set(dev) == set(KEYS)
    for k in KEYS:
        assert np.asarray(dev[k]).tobytes() == np.asarray(ref[k]).tobytes(), k


def test_limits_and_status_codes():
    from geoformer_amd import _lib
    s = bc.make_scene(41, n_cams=4, n_points=30)
    free = bc.free_flags(s)
    for kw in ({'cg_iters': 0}, {'cg_iters': 257}, {'cg_tol': -1.0}, {'cg_tol': 1.0}, {'cg_tol': float('nan')}, {'iters': 0}, {'iters': 65},
               {'thr': 0.0}, {'solver': 'cholesky'}):
        kw = dict({'solver': 'pcg'}, **kw)
        with pytest.raises(ValueError):
            run_device(s, free, kw.pop('thr', 4.0), kw.pop('iters', 4), **kw)
    L = _lib.lib()
    d = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device='cuda')
    n, T, N = 4, len(s.X), len(s.uv)
    io, ob = bc.image_major(s.obs_image, n)
    cf = np.where(free, np.cumsum(free) - 1, -1).astype(np.int32)
    dev = [d(x, dt) for x, dt in ((s.obs_off, torch.int32), (s.obs_image, torch.int32), (s.uv, torch.float32), (io, torch.int32), (ob, torch.int32),
                                  (cf, torch.int32), (s.K, torch.float32), (s.R, torch.float64), (s.t, torch.float64), (s.X, torch.float64))]
    outs = [torch.zeros(k, dtype=dt, device='cuda') for k, dt in ((9 * n, torch.float64), (3 * n, torch.float64), (3 * T, torch.float64), (N, torch.uint8),
                                                                   (T, torch.int32), (5, torch.float64), (4, torch.int32), (5, torch.float64), (1, torch.int32),
                                                                   (4, torch.int32), (4, torch.float64))]
    ws = torch.zeros(L.gf_bundle_pcg_workspace_bytes(T, N, n, 2), dtype=torch.uint8, device='cuda')
    assert ws.numel() > 0 and L.gf_bundle_pcg_workspace_bytes(T, N, n, 129) > 0 and L.gf_bundle_pcg_workspace_bytes(T, N, 70000, 65536) > 0
    assert L.gf_bundle_pcg_workspace_bytes(T, N, 70000, 65537) == 0 and L.gf_bundle_pcg_workspace_bytes(0, N, n, 2) == 0
    assert L.gf_bundle_workspace_bytes(T, N, n, 129) == 0                   # the dense solver's limit stands
    # O(n_obs + T + F): 1000 more free cameras cost 1000 x (36 + 36 + 5 x 6 + 1) doubles and their image number, and no more
    assert L.gf_bundle_pcg_workspace_bytes(T, N, 3000, 2000) - L.gf_bundle_pcg_workspace_bytes(T, N, 3000, 1000) <= 1000 * (103 * 8 + 4) + 16 * 256
    p = lambda x: x.data_ptr()

    def call(obs_off_host=s.obs_off, cam_free_host=cf, F=2, thr=4.0, iters=4, cg_iters=64, cg_tol=1e-6, ws_bytes=None, n_images=n):
        keep = [np.ascontiguousarray(x, np.int32) for x in (obs_off_host, s.obs_image, io, ob, cam_free_host)]
        return L.gf_bundle_adjust_pcg(*[k.ctypes.data for k in keep], p(dev[0]), T, N, p(dev[1]), p(dev[2]), p(dev[3]), p(dev[4]), p(dev[5]), n_images,
                                      F, p(dev[6]), p(dev[7]), p(dev[8]), p(dev[9]), thr, iters, cg_iters, cg_tol, *[p(x) for x in outs], p(ws),
                                      ws.numel() if ws_bytes is None else ws_bytes, torch.cuda.current_stream().cuda_stream)
    assert call() == 0
    torch.cuda.synchronize()
    assert outs[6].sum().item() >= 1 and outs[9].min().item() >= 1
    assert call(ws_bytes=16) == -2 and b'workspace' in L.gf_last_error()
    assert call(iters=65) == -1 and b'iters' in L.gf_last_error()
    assert call(thr=-1.0) == -1 and b'thr' in L.gf_last_error()
    assert call(cg_iters=0) == -1 and b'cg_iters' in L.gf_last_error()
    assert call(cg_iters=257) == -1 and b'cg_iters' in L.gf_last_error()
    for tol in (-1.0, 1.0, float('nan')):
        assert call(cg_tol=tol) == -1 and b'cg_tol' in L.gf_last_error()
    assert call(F=65537, n_images=70000) == -1 and b'65536' in L.gf_last_error()     # rejected before any table is read
    assert call(F=3) == -1 and b'free' in L.gf_last_error()
    bad = s.obs_off.copy()
    bad[1], bad[2] = bad[2], bad[1]
    assert call(obs_off_host=bad) == -1 and b'ascend' in L.gf_last_error()
    assert call(cam_free_host=np.array([-1, 1, 0, -1])) == -1 and b'cam_free' in L.gf_last_error()
