"""Bundle adjustment with the PCG solver of the reduced camera system, host build of csrc/ba_pcg_spec.h (gf_ba_host_adjust_pcg in
csrc/host/ba_host.cpp): more than 128 free cameras, the invariants of the rule, the dense host build at F <= 128, the gold fit (scipy) at
F > 128, gross outliers, the limits.  No GPU."""
import numpy as np
import pytest

import bundle_cases as bc
import bundle_pcg_cases as pc

SEEDS = (1, 2, 3, 4)
SCHEDULE = (20.0, 8.0, 4.0)     # test_bundle_cpu.py's
GATE = 1.01                     # test_bundle_cpu.py's ratio gate
KEYS = ('R', 't', 'X', 'inliers', 'n_inliers', 'cost', 'accepted', 'lam', 'status')


def big_scene(seed):
    s = bc.make_scene(seed, n_cams=132, n_points=300, drop=0.8)
    free = bc.free_flags(s)
    return bc.keep_fixed_true(s, free), free


def staged(run, s, free, schedule=SCHEDULE, iters=16):
    R, t, X = s.R, s.t, s.X
    for thr in schedule:
        rc, o = run(s.obs_off, s.obs_image, s.uv, s.K, R, t, X, free, thr, iters)
        assert rc == 0
        R, t, X = o['R'], o['t'], o['X']
    return o


def test_130_free_cameras_run_with_pcg_and_not_with_the_dense_solver():
    s, free = big_scene(50)
    assert free.sum() == 130
    a = (s.obs_off, s.obs_image, s.uv, s.K, s.R, s.t, s.X, free, 20.0, 4)
    rc, o = pc.run_host_pcg(*a)
    assert rc == 0 and o['accepted'].any() and o['cost'][-1] < o['cost'][0] and o['status'][0] == 0
    assert bc.run_host(*a)[0] == -1


@pytest.fixture(scope='module')
def noisy():
    s = bc.make_scene(11, n_cams=6, n_points=120)
    free = bc.free_flags(s)
    return s, free, pc.run_host_pcg_scene(s, free, thr=20.0, iters=16)


def test_cost_never_increases_and_a_rejected_step_changes_nothing(noisy):
    s, free, o = noisy
    assert np.all(np.diff(o['cost']) <= 0)
    assert o['accepted'].sum() >= 3 and (o['accepted'] == 0).any()          # both branches ran
    for k in np.where(o['accepted'] == 0)[0]:
        assert o['cost'][k + 1] == o['cost'][k] and o['lam'][k + 1] == min(o['lam'][k] * 10.0, 1e12)
    for k in np.where(o['accepted'] == 1)[0]:
        assert o['cost'][k + 1] < o['cost'][k] and o['lam'][k + 1] == max(o['lam'][k] / 10.0, 1e-12)
    prev = pc.run_host_pcg_scene(s, free, thr=20.0, iters=1)
    for k in range(1, 8):
        nxt = pc.run_host_pcg_scene(s, free, thr=20.0, iters=k + 1)
        assert np.array_equal(nxt['cost'][:k + 1], prev['cost']) and np.array_equal(nxt['cg_used'][:k], prev['cg_used'])
        if nxt['accepted'][k] == 0:
            for key in ('R', 't', 'X', 'inliers', 'n_inliers'):
                assert np.array_equal(nxt[key], prev[key]), key
        prev = nxt


def test_the_cg_logs_respect_the_cap_and_the_tolerance(noisy):
    s, free, o = noisy
    assert o['status'][0] == 0                                               # no step failed
    assert o['cg_used'].dtype == np.int32 and o['cg_res'].dtype == np.float64 and o['cg_used'].shape == o['cg_res'].shape == (16,)
    assert np.all(o['cg_used'] >= 1) and np.all(o['cg_used'] <= 64)
    early = o['cg_used'] < 64
    assert early.any() and np.all(o['cg_res'][early] <= 1e-6 ** 2)
    for cap, tol in ((1, 1e-6), (3, 1e-6), (64, 1e-2), (256, 0.0)):
        q = pc.run_host_pcg_scene(s, free, thr=20.0, iters=6, cg_iters=cap, cg_tol=tol)
        assert np.all(q['cg_used'] <= cap) and np.all(np.diff(q['cost']) <= 0)
        ok = (q['cg_used'] < cap) & (q['status'][0] & 1 == 0)
        assert np.all(q['cg_res'][ok] <= tol * tol), (cap, tol)
        if cap <= 3:
            assert np.all(q['cg_used'] == cap) and np.all(q['cg_res'] > tol * tol) and q['accepted'].any()   # never converged, judged by cost


def test_fixed_and_poseless_images_keep_their_bits():
    s = bc.make_scene(12, n_cams=6, n_points=100)
    free = bc.free_flags(s, fixed=(0, 3))
    s.R[4], s.t[4] = np.nan, np.nan
    free[4] = False
    o = pc.run_host_pcg_scene(s, free, thr=20.0, iters=8)
    for i in (0, 3, 4):
        assert o['R'][i].tobytes() == s.R[i].tobytes() and o['t'][i].tobytes() == s.t[i].tobytes()
    assert o['accepted'].sum() >= 2 and not o['inliers'][s.obs_image == 4].any()
    assert all(not np.array_equal(o['R'][i].reshape(9), s.R[i]) for i in range(6) if free[i])
    free[4] = True                                                           # declared free all the same: an identity block, status 4
    o2 = pc.run_host_pcg_scene(s, free, thr=20.0, iters=8)
    assert o2['status'][0] & 4 and o2['accepted'].sum() >= 2
    assert o2['R'][4].tobytes() == s.R[4].tobytes() and o2['t'][4].tobytes() == s.t[4].tobytes()


def test_two_runs_give_the_same_bits(noisy):
    s, free, o = noisy
    again = pc.run_host_pcg_scene(s, free, thr=20.0, iters=16)
    for key in o:
        assert np.asarray(o[key]).tobytes() == np.asarray(again[key]).tobytes(), key


def test_no_free_camera_equals_the_dense_host_build_bit_for_bit():
    s = bc.make_scene(14, n_cams=5, n_points=40, rot_deg=0.0, trans=0.0, point_noise=0.05)
    free = np.zeros(5, bool)
    d = bc.run_host_scene(s, free, thr=40.0, iters=3)
    o = pc.run_host_pcg_scene(s, free, thr=40.0, iters=3)
    assert o['accepted'].any() and not np.array_equal(o['X'], s.X)
    for key in KEYS:
        assert np.asarray(o[key]).tobytes() == np.asarray(d[key]).tobytes(), key
    assert not o['cg_used'].any() and not o['cg_res'].any()


def test_a_camera_block_that_cannot_be_inverted_fails_every_step():
    """The optical-axis camera of test_bundle_gpu.py: two columns of exact zeros in its block at every lambda."""
    s = bc.make_scene(37, n_cams=4, n_points=40)
    a = bc.append_camera(s, np.eye(3), np.zeros(3))
    X = np.array([[0.0, 0.0, 5.0]])
    bc.append_point(s, X[0], [(0, bc.project(s.K[0].astype(np.float64), s.R[0].reshape(3, 3), s.t[0], X)[0][0]), (a, (bc.W_IMG / 2, bc.H_IMG / 2))])
    free = np.zeros(len(s.K), bool)
    free[[1, 2, a]] = True
    o = pc.run_host_pcg_scene(s, free, thr=20.0, iters=5)
    assert o['status'][0] & 1 and not o['accepted'].any() and not o['cg_used'].any() and np.all(o['cg_res'] == 1.0)
    assert np.array_equal(o['lam'], 1e-4 * 10.0 ** np.arange(6)) and np.all(o['cost'] == o['cost'][0])
    assert np.array_equal(o['R'].reshape(-1, 9), s.R) and np.array_equal(o['X'], s.X)


@pytest.fixture(scope='module')
def dense_table():
    rows = []
    med = lambda v: float(np.median(v))
    for outliers in (0.0, 0.1):
        for seed in SEEDS:
            s = bc.make_scene(seed, outliers=outliers)
            free = bc.free_flags(s)
            bc.keep_fixed_true(s, free)
            d, o = staged(bc.run_host, s, free), staged(pc.run_host_pcg, s, free)
            rows.append(dict(outliers=outliers, seed=seed, scene=s, out=o,
                             cd=med(bc.centre_errors(d['R'], d['t'], s)[free]), cp=med(bc.centre_errors(o['R'], o['t'], s)[free]),
                             pd=med(np.linalg.norm(d['X'] - s.X_true, axis=1)), pp=med(np.linalg.norm(o['X'] - s.X_true, axis=1))))
    print('\noutliers seed | centre dense pcg ratio | point dense pcg ratio')
    for r in rows:
        print('%.1f %d | %.6f %.6f %.9f | %.6f %.6f %.9f' % (r['outliers'], r['seed'], r['cd'], r['cp'], r['cp'] / r['cd'], r['pd'], r['pp'],
                                                             r['pp'] / r['pd']))
    return rows


def test_against_the_dense_host_build(dense_table):
    """12 cameras, seeds 1 - 4, schedule (20, 8, 4), 16 iterations each: the medians of pcg within GATE of dense's."""
    for r in dense_table:
        if r['outliers'] == 0.0:
            assert r['cp'] <= GATE * r['cd'], (r['seed'], r['cp'] / r['cd'])
            assert r['pp'] <= GATE * r['pd'], (r['seed'], r['pp'] / r['pd'])


def test_no_outlier_is_an_inlier_at_the_end(dense_table):
    for r in dense_table:
        if r['outliers'] == 0.0:
            continue
        s, o = r['scene'], r['out']
        assert s.outlier.sum() > 300
        assert not o['inliers'][s.outlier].any(), r['seed']
        assert o['inliers'][~s.outlier].mean() > 0.99
        assert np.array_equal(o['n_inliers'], np.add.reduceat(o['inliers'].astype(np.int32), s.obs_off[:-1]))


def test_one_step_at_a_tiny_shape_equals_the_dense_solve():
    """3 cameras (two free, F = 2), 8 points, one LM iteration, cg_tol = 0 and cg_iters = 12 = 6 F: CG on a 12 x 12 system has then run its
    full Krylov space, so its x is the dense Cholesky's solution up to round-off, and so is the candidate.  The relative difference (the
    largest absolute difference of R, t and X over the largest absolute entry of the dense result) measured on this CPU over the four seeds
    16 - 19: 4.7e-14, 1.0e-14, 3.5e-14 and 1.3e-13; the maximum is 1.3e-13.  The gate is ten times that maximum, 1.3e-12: the factor covers
    round-off that depends on the compiler version, nothing else."""
    worst = 0.0
    for seed in (16, 17, 18, 19):
        s = bc.make_scene(seed, n_cams=3, n_points=8, drop=0.0)
        free = np.array([False, True, True])
        d = bc.run_host_scene(s, free, thr=40.0, iters=1)
        o = pc.run_host_pcg_scene(s, free, thr=40.0, iters=1, cg_iters=12, cg_tol=0.0)
        assert d['accepted'].tolist() == [1] and o['accepted'].tolist() == [1] and o['cg_used'][0] <= 12
        rel = max(np.abs(o[k] - d[k]).max() / np.abs(d[k]).max() for k in ('R', 't', 'X'))
        print('\nseed', seed, 'relative difference to the dense host build', rel)
        worst = max(worst, rel)
    assert worst <= 1.3e-12


@pytest.mark.parametrize('seed', (50, 51))
def test_against_the_gold_fit_beyond_128_free_cameras(seed):
    """130 free cameras, about 7 900 observations, thr 20, 16 iterations, cg_iters 64 and cg_tol 1e-6 (the defaults): the median centre
    error within GATE of scipy's fit over all free poses and all points at once."""
    s, free = big_scene(seed)
    o = pc.run_host_pcg_scene(s, free, thr=20.0, iters=16)
    Rg, tg, _ = bc.gold_fit(s, free, np.ones(len(s.uv), bool))
    c0 = float(np.median(bc.centre_errors(s.R, s.t, s)[free]))
    c1 = float(np.median(bc.centre_errors(o['R'], o['t'], s)[free]))
    cg = float(np.median(bc.centre_errors(Rg, tg, s)[free]))
    print('\nseed', seed, 'centre before', c0, 'after', c1, 'gold', cg, 'ratio', c1 / cg, 'cg_used', o['cg_used'].tolist())
    assert c1 < 0.5 * c0
    assert c1 <= GATE * cg, c1 / cg


def test_limits_are_errors():
    s = bc.make_scene(13, n_cams=4, n_points=30)
    free = bc.free_flags(s)
    a = (s.obs_off, s.obs_image, s.uv, s.K, s.R, s.t, s.X, free)
    assert pc.run_host_pcg(*a, 4.0, 2, 1, 0.0)[0] == 0 and pc.run_host_pcg(*a, 4.0, 2, 256, 0.5)[0] == 0
    for cg_iters in (0, -1, 257):
        assert pc.run_host_pcg(*a, 4.0, 2, cg_iters, 1e-6)[0] == -1
    for cg_tol in (-1.0, 1.0, float('nan'), float('inf')):
        assert pc.run_host_pcg(*a, 4.0, 2, 64, cg_tol)[0] == -1
    for iters in (0, 65):
        assert pc.run_host_pcg(*a, 4.0, iters)[0] == -1
    assert pc.run_host_pcg(*a, 0.0, 2)[0] == -1
    # 65537 free cameras (65536 is accepted): cameras that see nothing are enough for the limit
    for n, rc in ((65538, 0), (65539, -1)):
        K, R, t = np.tile(s.K[:1], (n, 1)), np.tile(s.R[:1], (n, 1)), np.tile(s.t[:1], (n, 1))
        K[:4], R[:4], t[:4] = s.K, s.R, s.t
        fr = np.ones(n, bool)
        fr[[0, 3]] = False
        assert pc.run_host_pcg(s.obs_off, s.obs_image, s.uv, K, R, t, s.X, fr, 4.0, 1, 2)[0] == rc, n
    off = s.obs_off.copy()
    off[1], off[2] = off[2], off[1]
    assert pc.run_host_pcg(off, *a[1:], 4.0, 2)[0] == -1
    assert pc.run_host_pcg(*a, 4.0, 2, cam_free=np.array([-1, 1, 0, -1]))[0] == -1
    # the Python layers name their limits before anything touches a device
    from geoformer_amd import matcher, ops
    assert ops.BA_PCG_MAX_FREE == 65536 and ops.BA_MAX_FREE == 128
    for kw in ({'solver': 'sparse'}, {'solver': 'pcg', 'cg_iters': 0}, {'solver': 'pcg', 'cg_iters': 257}, {'solver': 'pcg', 'cg_tol': -1.0},
               {'solver': 'pcg', 'cg_tol': 1.0}, {'solver': 'pcg', 'cg_tol': float('nan')}):
        with pytest.raises(ValueError, match='solver|cg_iters|cg_tol'):
            ops.bundle_adjust(None, None, None, None, None, None, None, None, **kw)
        with pytest.raises(ValueError, match='solver|cg_iters|cg_tol'):
            matcher.refine(None, None, None, None, **kw)
