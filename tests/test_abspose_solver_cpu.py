"""The absolute-pose rule of csrc/abs_solver.h on the CPU: the host build (csrc/host/abspose_host.cpp) against an independent numpy P3P
(quartic by polynomial arithmetic, numpy.roots, Kabsch alignment by SVD) and a numpy RANSAC over the same draws.
Scenes: tests/abspose_cases.py."""
import numpy as np
import pytest

import abspose_cases as C

MINIMAL_SEEDS = range(1000, 1200)
# a solution must reproject the three points it was computed from.  The scenes are exact fp64, so the error is the solver's own: the
# quartic's root carried through two triangle frames, 1e-9 relative at worst for a badly conditioned root, times the focal length and the
# 1 / 3 .. 1 / 8 of the depth range.  1e-3 px is 500 times below the tightest inlier threshold any test uses (0.5 px would already be tight).
REPROJ_TOL_PX = 1e-3


def _closest(sols, R, t):
    if not sols:
        return np.inf, np.inf
    return min(((C.rotation_error_deg(R, r), float(np.linalg.norm(tt - t))) for r, tt in sols), key=lambda e: e[0])


def test_host_p3p_against_independent_numpy_p3p():
    """200 exact minimal scenes.  The planted pose is among the host build's solutions, within 10 times the independent numpy solver's OWN
    worst deviation from the planted pose over these scenes; every host solution reprojects its three points.
    Measured here: numpy's worst 2.41e-06 deg / 5.38e-07 world units (camera centre about 130 units from the origin), so the gate is
    2.41e-05 deg / 5.38e-06; the host build's worst 2.41e-06 deg / 1.96e-07, worst reprojection of a host solution 7.4e-06 px, 435
    host solutions in 200 scenes, the same number per scene as numpy's."""
    worst_np, worst_host, worst_px, nsol = [0.0, 0.0], [0.0, 0.0], 0.0, 0
    per_scene = []
    for s in MINIMAL_SEEDS:
        px, X, nm, R, t = C.minimal_scene(s)
        ref, host = C.numpy_p3p(px, X), C.host_p3p(px, X, nm)
        assert 1 <= len(host) <= 4, s
        nsol += len(host)
        en, eh = _closest(ref, R, t), _closest(host, R, t)
        per_scene.append((s, en, eh))
        worst_np = [max(worst_np[0], en[0]), max(worst_np[1], en[1])]
        worst_host = [max(worst_host[0], eh[0]), max(worst_host[1], eh[1])]
        for r, tt in host:
            assert np.isfinite(r).all() and np.isfinite(tt).all()
            assert abs(np.linalg.det(r) - 1) < 1e-9 and np.abs(r @ r.T - np.eye(3)).max() < 1e-9
            e = C.reproj_px(r, tt, px, X).max()
            worst_px = max(worst_px, e)
            assert e < REPROJ_TOL_PX, (s, e)
    print(f'numpy worst {worst_np[0]:.3g} deg {worst_np[1]:.3g}; host worst {worst_host[0]:.3g} deg {worst_host[1]:.3g}; '
          f'worst reprojection {worst_px:.3g} px; {nsol} host solutions')
    assert np.isfinite(worst_np).all()
    assert worst_host[0] <= 10 * worst_np[0] and worst_host[1] <= 10 * worst_np[1], (worst_np, worst_host)


def test_degenerate_input_gives_no_solution_and_no_nan():
    px, X, nm, R, t = C.minimal_scene(1000)
    # collinear 3-D points (exactly: small integers), then two coincident ones
    line = np.array([[1.0, 2, 3], [2, 4, 6], [4, 8, 12]]) + np.array([100.0, -40, 30])
    assert C.host_p3p(px, line, C.box_norm(np.r_[line, X])) == []
    twice = X.copy(); twice[2] = twice[0]
    assert C.host_p3p(px, twice, nm) == []
    # two equal bearings
    same = px.copy(); same[1] = same[0]
    assert C.host_p3p(same, X, nm) == []
    # a non-finite coordinate on either side, and a degenerate box
    for bad in (np.nan, np.inf, -np.inf):
        p2 = px.copy(); p2[1, 0] = bad
        assert C.host_p3p(p2, X, nm) == []
        X2 = X.copy(); X2[2, 1] = bad
        assert C.host_p3p(px, X2, nm) == []
        n2 = nm.copy(); n2[3] = bad
        assert C.host_p3p(px, X, n2) == []
    assert C.numpy_p3p(px, twice) == [] and C.numpy_p3p(px * np.nan, X) == []


def test_host_ransac_small_problems():
    sc = C.scene(250, 300, 0.0)
    for n, valid in ((0, 0), (3, 0), (4, 1), (5, 1)):
        r = C.host_ransac(sc['p2d'][:n], sc['p3d'][:n], iters=64)
        assert r['status'] >= 0 and r['valid'] == valid and r['n_inliers'] == (n if valid else 0)
        if not valid:
            assert not r['R'].any() and not r['t'].any() and tuple(r['hyp']) == (-1, -1)
    flat = sc['p3d'][:50].copy(); flat[:] = flat[0]                 # a box without extent
    assert C.host_ransac(sc['p2d'][:50], flat, iters=64)['valid'] == 0
    assert C.host_ransac(sc['p2d'], sc['p3d'], iters=100)['status'] == -1
    assert C.host_ransac(sc['p2d'], sc['p3d'], thr=0.0)['status'] == -1
    assert C.host_ransac(sc['p2d'], sc['p3d'], refit=9)['status'] == -1


RANSAC_SEEDS = range(300, 306)


@pytest.mark.parametrize('frac', [0.3, 0.5])
def test_host_ransac_against_numpy_ransac_over_the_same_draws(frac):
    """300 rows, thr 2 px, 256 hypotheses: the inlier masks are equal.  Seeds 300 .. 305 were chosen so that no row lies within 1e-6 px^2
    of the threshold under the numpy winner (asserted): the scenes carry no noise, so an inlier's squared error is about 1e-9 px^2 and an
    outlier's is thousands; the comparison cannot hinge on rounding."""
    for s in RANSAC_SEEDS:
        sc = C.scene(s, 300, frac)
        host = C.host_ransac(sc['p2d'], sc['p3d'], thr=2.0, iters=256)
        mask, R, t, margin = C.numpy_ransac(sc['p2d'], sc['p3d'], thr=2.0, iters=256)
        assert margin > 1e-6, (s, margin)
        assert host['valid'] == 1 and host['n_inliers'] == int(mask.sum())
        assert np.array_equal(host['inliers'], mask), s
        assert np.array_equal(host['inliers'], ~sc['outlier']) or host['n_inliers'] >= int((~sc['outlier']).sum())
        assert C.rotation_error_deg(host['R'], sc['R']) < 1e-3 and np.linalg.norm(C.centre(host['R'], host['t']) - C.centre(sc['R'], sc['t'])) < 1e-3
