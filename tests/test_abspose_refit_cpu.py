"""The refit rule of csrc/abs_solver.h on the CPU (host build, csrc/host/abspose_host.cpp) against the gold standard: scipy's
Levenberg-Marquardt on the planted inliers.  Scenes: tests/abspose_cases.py."""
import numpy as np
import pytest

import abspose_cases as C

SEEDS = range(400, 424)
N, FRAC, NOISE, ITERS, THR, REFIT = 300, 0.3, 0.5, 128, 2.0, 4


def gold_fit(sc):
    """scipy.optimize.least_squares (LM) over a rotation vector and t on the planted inliers, started at the planted pose"""
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation
    keep = ~sc['outlier']
    p2, p3 = sc['p2d'][keep].astype(np.float64), sc['p3d'][keep].astype(np.float64)

    def res(x):
        Y = p3 @ Rotation.from_rotvec(x[:3]).as_matrix().T + x[3:]
        return ((Y[:, :2] / Y[:, 2:3]) * [C.K[0, 0], C.K[1, 1]] + [C.K[0, 2], C.K[1, 2]] - p2).ravel()
    x0 = np.r_[Rotation.from_matrix(sc['R']).as_rotvec(), sc['t']]
    x = least_squares(res, x0, method='lm', xtol=1e-15, ftol=1e-15, gtol=1e-15).x
    return Rotation.from_rotvec(x[:3]).as_matrix(), x[3:]


@pytest.fixture(scope='module')
def runs():
    out = []
    for s in SEEDS:
        sc = C.scene(s, N, FRAC, noise=NOISE)
        plain = C.host_ransac(sc['p2d'], sc['p3d'], thr=THR, iters=ITERS)
        refit = C.host_ransac(sc['p2d'], sc['p3d'], thr=THR, iters=ITERS, refit=REFIT)
        out.append((s, sc, plain, refit, gold_fit(sc)))
    return out


def _centre_error(r, sc):
    return float(np.linalg.norm(C.centre(r['R'], r['t']) - C.centre(sc['R'], sc['t'])))


def test_refit_against_the_gold_fit(runs):
    """24 scenes (seeds 400 .. 423, 300 rows, 30 % outliers, 0.5 px noise, 128 hypotheses, thr 2 px, refit=4).  n_inliers never
    decreases, the hypothesis is kept, the median camera-centre error with refit is at most half the median without, and the median
    ratio of the refit's centre error to the gold fit's is at most 1.1.
    Measured with the host build: median centre error 9.83e-3 without, 1.25e-3 with refit (world units), 1 - 2 rounds accepted per scene,
    no outlier accepted, the refit better in 23 of 24 scenes; ratio to the gold fit: median 1.000000, worst 1.516 (scene 412; printed,
    ungated)."""
    e0, e1, ratio = [], [], []
    print('scene  inliers  refit  rounds  centre error  with refit  gold fit  ratio  rot deg  with refit')
    for s, sc, plain, refit, (Rg, tg) in runs:
        assert plain['valid'] == refit['valid'] == 1
        assert refit['n_inliers'] >= plain['n_inliers'], s
        assert tuple(refit['hyp']) == tuple(plain['hyp']), s
        assert 0 <= refit['rounds'] <= REFIT and refit['n_inliers'] == int(refit['inliers'].sum())
        assert abs(np.linalg.det(refit['R']) - 1) < 1e-12 and np.abs(refit['R'] @ refit['R'].T - np.eye(3)).max() < 1e-12
        a, b = _centre_error(plain, sc), _centre_error(refit, sc)
        g = float(np.linalg.norm(C.centre(Rg, tg) - C.centre(sc['R'], sc['t'])))
        e0.append(a); e1.append(b); ratio.append(b / g)
        print(f'{s}  {plain["n_inliers"]:4d}  {refit["n_inliers"]:4d}  {refit["rounds"]}  {a:.3e}  {b:.3e}  {g:.3e}  {b / g:.4f}  '
              f'{C.rotation_error_deg(plain["R"], sc["R"]):.4f}  {C.rotation_error_deg(refit["R"], sc["R"]):.4f}  '
              f'outliers accepted {int((refit["inliers"] & sc["outlier"]).sum())}')
    print(f'median centre error {np.median(e0):.3e} -> {np.median(e1):.3e}; ratio to the gold fit: median {np.median(ratio):.6f}, '
          f'worst {max(ratio):.3f} (ungated)')
    assert np.median(e1) <= 0.5 * np.median(e0)
    assert np.median(ratio) <= 1.1


def test_rounds_zero_reproduces_the_p3p_winner(runs):
    """refit = 0 is the plain entry; a problem whose winner has fewer than 6 inliers is not refitted: rounds = 0 and every output carries
    the P3P winner's bits"""
    s, sc, plain, refit, _ = runs[0]
    five = C.host_ransac(sc['p2d'][~sc['outlier']][:5], sc['p3d'][~sc['outlier']][:5], thr=THR, iters=ITERS)
    five_r = C.host_ransac(sc['p2d'][~sc['outlier']][:5], sc['p3d'][~sc['outlier']][:5], thr=THR, iters=ITERS, refit=8)
    assert five['valid'] == 1 and five['n_inliers'] <= 5 and five_r['rounds'] == 0
    for k in ('R', 't', 'hyp', 'inliers'):
        assert np.array_equal(five[k], five_r[k]), k
    assert plain['rounds'] == 0
    for s, sc, plain, refit, _ in runs:
        if refit['rounds'] == 0:
            assert all(np.array_equal(plain[k], refit[k]) for k in ('R', 't', 'hyp', 'inliers'))
        else:
            assert not np.array_equal(plain['R'], refit['R'])


def test_one_round_alone_converges_on_the_planted_inliers(runs):
    """gf_abs_host_refit_once: three Gauss-Newton steps from a pose a few pixels off reach the gold fit's neighbourhood"""
    s, sc, plain, refit, (Rg, tg) = runs[3]
    nm = C.box_norm(sc['p3d'])
    keep = (~sc['outlier']).astype(np.uint8)
    R0 = C.rodrigues(np.array([0.004, -0.003, 0.002])) @ sc['R']
    t0c = (sc['t'] + R0 @ nm[:3]) / nm[3] + np.array([0.002, -0.001, 0.002])          # conditioned: t' = (t + R c) / s
    ok, R1, t1c = C.host_refit_once(sc['p2d'], sc['p3d'], keep, nm, R0, t0c)
    assert ok == 1
    t1 = nm[3] * t1c - R1 @ nm[:3]
    before = float(np.linalg.norm(C.centre(R0, nm[3] * t0c - R0 @ nm[:3]) - C.centre(Rg, tg)))
    after = float(np.linalg.norm(C.centre(R1, t1) - C.centre(Rg, tg)))
    print(f'distance of the camera centre from the gold fit: {before:.3e} -> {after:.3e}')
    assert after < 1e-6 and after < 1e-3 * before
    # an empty set cannot be solved: the round fails and the pose stays
    ok, R2, t2 = C.host_refit_once(sc['p2d'], sc['p3d'], np.zeros(N, np.uint8), nm, R0, t0c)
    assert ok == 0 and np.array_equal(R2, R0) and np.array_equal(t2, t0c)
