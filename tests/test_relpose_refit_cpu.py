"""The refit rule (step 7) of csrc/rel_solver.h on the CPU (host build, csrc/host/relpose_host.cpp) against the gold standard: scipy's
Levenberg-Marquardt on the same residual over the planted inliers.  Scenes: tests/relpose_cases.py."""
import numpy as np
import pytest

import pose_cases as P
import relpose_cases as C

SEEDS = range(700, 724)
ITERS, REFIT = 128, 4


def _tangent(t):
    k = int(np.argmin(np.abs(t)))
    b1 = np.cross(t, np.eye(3)[k])
    b1 /= np.linalg.norm(b1)
    return b1, np.cross(t, b1)


def gold_fit(sc):
    """scipy.optimize.least_squares (LM) of the signed Sampson residual over a rotation vector and two tangent coordinates of t on the
    planted inliers, started at the planted pose"""
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation
    x = C.normalise(C.rows(sc))[~sc['outlier']]
    t0 = sc['t'] / np.linalg.norm(sc['t'])
    b1, b2 = _tangent(t0)

    def pose(p):
        t = t0 + p[3] * b1 + p[4] * b2
        return Rotation.from_rotvec(p[:3]).as_matrix(), t / np.linalg.norm(t)
    p0 = np.r_[Rotation.from_matrix(sc['R']).as_rotvec(), 0.0, 0.0]
    p = least_squares(lambda q: C.sampson_signed(*pose(q), x), p0, method='lm', xtol=1e-15, ftol=1e-15, gtol=1e-15).x
    return pose(p)


@pytest.fixture(scope='module')
def runs():
    out = []
    for s in SEEDS:
        sc = C.noisy_scene(s)
        m = C.rows(sc)
        per_thr = {thr: (C.host_ransac(m, pixel_thr=thr, iters=ITERS, seed=s), C.host_ransac(m, pixel_thr=thr, iters=ITERS, seed=s, refit=REFIT))
                   for thr in (2.0, 1.0)}
        out.append((s, sc, per_thr, gold_fit(sc)))
    return out


def _report(runs, thr):
    e0, e1, ratio = [], [], []
    print(f'pixel_thr {thr}: scene  inliers  refit  rounds  rot deg  with refit  gold   t deg  with refit  gold  outliers kept')
    for s, sc, per_thr, (Rg, tg) in runs:
        plain, refit = per_thr[thr]
        a, b, g = (P.pose_errors(r['R'], r['t'], sc['R'], sc['t']) for r in (plain, refit, {'R': Rg, 't': tg}))
        e0.append(a); e1.append(b); ratio.append((b[0] / g[0], b[1] / g[1]))
        print(f'{s}  {plain["n_inliers"]:4d}  {refit["n_inliers"]:4d}  {refit["rounds"]}  {a[0]:.4f}  {b[0]:.4f}  {g[0]:.4f}   {a[1]:.4f}  {b[1]:.4f}  '
              f'{g[1]:.4f}  {int((refit["inliers"] & sc["outlier"]).sum())}')
    e0, e1, ratio = np.array(e0), np.array(e1), np.array(ratio)
    print(f'pixel_thr {thr}: median rotation error {np.median(e0[:, 0]):.4f} -> {np.median(e1[:, 0]):.4f} deg, translation direction '
          f'{np.median(e0[:, 1]):.4f} -> {np.median(e1[:, 1]):.4f} deg; ratio to the gold fit: median {np.median(ratio[:, 0]):.6f} / '
          f'{np.median(ratio[:, 1]):.6f}, worst {ratio[:, 0].max():.3f} / {ratio[:, 1].max():.3f} (ungated)')
    return e0, e1, ratio


def test_refit_against_the_gold_fit(runs):
    """C: 24 scenes (seeds 700 .. 723: scene(seed, 300, 0.3, 0.5) plus 0.5 px noise on image 0 of the planted inliers, 128 hypotheses,
    RANSAC seed = scene seed, pixel_thr 2 px, refit = 4, pose_cases.K for both images).  n_inliers never decreases, the hypothesis is
    kept, R is orthonormal and |t| = 1 to 1e-12, the median rotation and translation-direction errors with refit are each at most half
    the median without, and the median ratio to the gold fit is at most 1.1 for each error.  The same figures at 1 px are printed only."""
    for s, sc, per_thr, _ in runs:
        for thr, (plain, refit) in per_thr.items():
            assert plain['valid'] == refit['valid'] == 1
            assert refit['n_inliers'] >= plain['n_inliers'], (s, thr)
            assert tuple(refit['hyp']) == tuple(plain['hyp']) and refit['n_cheiral'] == plain['n_cheiral'], (s, thr)
            assert 0 <= refit['rounds'] <= REFIT and refit['n_inliers'] == int(refit['inliers'].sum()) and plain['rounds'] == 0
            assert np.abs(refit['R'] @ refit['R'].T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(refit['R']) - 1) < 1e-12
            assert abs(np.linalg.norm(refit['t']) - 1) < 1e-12 and abs(np.linalg.norm(refit['E']) - 1) < 1e-12
            if refit['rounds'] == 0:
                assert all(np.array_equal(plain[k], refit[k]) for k in ('E', 'R', 't', 'inliers'))
            else:
                En = P.cross_matrix(refit['t']) @ refit['R']
                assert np.abs(refit['E'] - En / np.linalg.norm(En)).max() < 1e-14
    e0, e1, ratio = _report(runs, 2.0)
    _report(runs, 1.0)
    assert np.median(e1[:, 0]) <= 0.5 * np.median(e0[:, 0])
    assert np.median(e1[:, 1]) <= 0.5 * np.median(e0[:, 1])
    assert np.median(ratio[:, 0]) <= 1.1 and np.median(ratio[:, 1]) <= 1.1


def test_a_winner_with_five_inliers_is_not_refitted():
    """D: below 6 inliers there is no round: rounds = 0 and every output carries the five-point winner's bits"""
    sc = P.scene(11, 40, 0.0, 0.0)
    m = C.rows(sc)[:5]
    plain, refit = C.host_ransac(m), C.host_ransac(m, refit=4)
    assert plain['valid'] == 1 and plain['n_inliers'] == 5 and refit['rounds'] == 0
    for k in ('E', 'R', 't', 'hyp', 'inliers', 'n_inliers', 'n_cheiral'):
        assert np.array_equal(plain[k], refit[k]), k


def test_jacobian_against_central_differences():
    """D: rs_gn_row's analytic derivatives of r = e / sqrt(s) by (w1, w2, w3, a, b) against central differences THROUGH rs_gn_update, the
    residual recomputed in numpy, on 20 random rows and poses.  Step h = 1e-5: the truncation error is h^2 |r'''| / 6 and the
    rounding error of the difference about 4 eps |r| / h.  On these rows (|x| < 1, s > 0.05) |r|, |r'| and |r'''| / 6 stay below 1e3,
    so the tolerance is 1e3 h^2 + 4e3 eps / h = 1.0e-7 + 8.9e-8."""
    h = 1e-5
    tol = 1e3 * h * h + 4e3 * np.finfo(float).eps / h
    rng = np.random.default_rng(5)
    done = 0
    while done < 20:
        R, t = P.random_pose(rng)
        x = rng.uniform(-0.6, 0.6, 4)
        ok, J, res = C.host_gn_row(R, t, x)
        assert ok == 1
        assert abs(res - C.sampson_signed(R, t, x[None])[0]) < 1e-13
        E = P.cross_matrix(t) @ R
        a, b = E @ np.r_[x[:2], 1], E.T @ np.r_[x[2:], 1]
        if a[0] ** 2 + a[1] ** 2 + b[0] ** 2 + b[1] ** 2 < 0.05:
            continue
        for p in range(5):
            d = np.zeros(5)
            d[p] = h
            (ok1, R1, t1), (ok2, R2, t2) = C.host_gn_update(d, R, t), C.host_gn_update(-d, R, t)
            assert ok1 == ok2 == 1
            fd = (C.sampson_signed(R1, t1, x[None])[0] - C.sampson_signed(R2, t2, x[None])[0]) / (2 * h)
            assert abs(fd - J[p]) < tol, (done, p, fd, J[p])
        done += 1


def test_update_stays_on_the_manifold():
    rng = np.random.default_rng(6)
    R, t = P.random_pose(rng)
    ok, R1, t1 = C.host_gn_update(np.array([0.02, -0.01, 0.03, 0.05, -0.04]), R, t)
    assert ok == 1 and np.abs(R1 @ R1.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.norm(t1) - 1) < 1e-15
    ok, R0, t0 = C.host_gn_update(np.zeros(5), R, t)
    assert ok == 1 and np.array_equal(R0, R) and np.abs(t0 - t).max() < 1e-15


def test_a_singular_system_is_a_failed_fit():
    """D: all inliers identical -> J^T J has rank 1, the pivot test of gs_solve<5> fails, the round fails and the pose keeps its bits; so
    does an empty set.  On exact rows the fit stays at the planted pose."""
    rng = np.random.default_rng(8)
    R, t = P.random_pose(rng)
    X = P.world_points(rng, 40)
    X1 = X @ R.T + t
    x = np.c_[X[:, :2] / X[:, 2:], X1[:, :2] / X1[:, 2:]]
    ok, R1, t1 = C.host_refit_once(x, np.ones(40, np.uint8), R, t)
    assert ok == 1 and np.abs(R1 - R).max() < 1e-9 and np.abs(t1 - t).max() < 1e-9
    same = np.tile(x[:1] + [0, 0, 1e-3, 0], (40, 1))
    ok, R2, t2 = C.host_refit_once(same, np.ones(40, np.uint8), R, t)
    assert ok == 0 and np.array_equal(R2, R) and np.array_equal(t2, t)
    ok, R3, t3 = C.host_refit_once(x, np.zeros(40, np.uint8), R, t)
    assert ok == 0 and np.array_equal(R3, R) and np.array_equal(t3, t)
