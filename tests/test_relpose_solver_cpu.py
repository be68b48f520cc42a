"""The calibrated two-view rule of csrc/rel_solver.h on the CPU (host build, csrc/host/relpose_host.cpp): it is the old essential-matrix
RANSAC (csrc/host/pose_host.cpp) where the two rules coincide, and the row filter removes rows and nothing else.  Scenes:
tests/relpose_cases.py over tests/pose_cases.py."""
import numpy as np
import pytest

import pose_cases as P
import relpose_cases as C

COMMON = ('E', 'R', 't', 'hyp', 'n_inliers', 'inliers', 'valid')


def _same(a, b, keys=COMMON):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize('n', C.SIZES)
def test_equals_the_old_host_ransac_where_the_rules_coincide(n):
    """A: no scores, all rows finite, refit = 0, the same K, pixel_thr, iters, seed and pair index -> every common output bit for bit.
    Both the shared K of pose_cases and anisotropic K0 != K1; valid follows the size (from five rows on a pose is found)."""
    sc = P.scene(40 + n, n, 0.3, 0.3)
    m = C.rows(sc)
    for K0, K1, rows in ((P.K, P.K, m), (C.intrinsics(1), C.intrinsics(4), C.reproject(m, C.intrinsics(1), C.intrinsics(4)))):
        for iters, sample, thr in ((64, 0, 1.0), (128, 3, 0.5)):
            old = P.host_ransac(rows[:, :2], rows[:, 2:], K0, K1, pixel_thr=thr, iters=iters, seed=77, sample=sample)
            new = C.host_ransac(rows, None, K0, K1, pixel_thr=thr, iters=iters, seed=77, sample=sample)
            assert new['status'] == old['status'] and new['valid'] == (1 if n >= 5 else 0)
            _same(old, new)
            assert new['rounds'] == 0 and new['n_cheiral'] <= new['n_inliers'] and (new['n_cheiral'] > 0) == bool(new['valid'])


def test_filtered_rows_are_removed_and_nothing_else():
    """B: low and NaN scores, NaN / +-inf coordinates (also in the middle of a 64-row group): the result is that of the list without
    those rows, filtered rows are never inliers; a pair with every row filtered and one left with four rows are not valid"""
    b = C.batch(filtered=True)
    off = b['offsets']
    left = [int((~b['gone'][off[n]:off[n + 1]]).sum()) for n in range(8)]
    assert left[3] == 0 and left[4] == 4 and min(left[5:]) >= 5
    for refit in (0, 4):
        for n, r in enumerate(C.host_batch(b, refit=refit)):
            keep = ~b['gone'][off[n]:off[n + 1]]
            s = C.host_ransac(b['m'][off[n]:off[n + 1]][keep], b['scores'][off[n]:off[n + 1]][keep], b['K0'][n], b['K1'][n], sample=n, refit=refit)
            _same(r, s, ('E', 'R', 't', 'hyp', 'n_inliers', 'n_cheiral', 'rounds', 'valid'))
            assert np.array_equal(r['inliers'][keep], s['inliers']) and not r['inliers'][~keep].any()
            assert r['valid'] == (1 if left[n] >= 5 else 0)
            if not r['valid']:
                assert r['n_inliers'] == 0 and not r['E'].any() and not r['R'].any() and tuple(r['hyp']) == (-1, -1)


@pytest.mark.parametrize('bad', (0.0, -500.0, np.nan, np.inf))
def test_a_bad_focal_length_is_not_valid_and_no_error(bad):
    m = C.rows(P.scene(7, 65, 0.3, 0.3))
    assert C.host_ransac(m)['valid'] == 1
    for which in range(4):
        K0, K1 = P.K.copy(), P.K.copy()
        (K0 if which < 2 else K1)[which % 2, which % 2] = bad
        r = C.host_ransac(m, None, K0, K1)
        assert r['status'] == 0 and r['valid'] == 0 and r['n_inliers'] == 0 and not r['inliers'].any() and not r['E'].any()


def test_argument_errors_of_the_host_entry():
    m = C.rows(P.scene(7, 65, 0.3, 0.3))
    for iters in (0, 100, -64, 32, 96):
        assert C.host_ransac(m, iters=iters)['status'] == -1
    assert C.host_ransac(m, pixel_thr=0.0)['status'] == -1 and C.host_ransac(m, refit=9)['status'] == -1
    assert C.host_ransac(m, refit=-1)['status'] == -1


def test_near_planar_and_planar_scenes():
    """The record behind the documented limits, printed; the gates are only what RANSAC itself promises.  12 near-planar scenes (300 rows, 90 %
    of the points on one plane, 20 % outliers, 0.3 px noise, 512 hypotheses): the off-plane planted inliers kept by the five-point rule and
    by the seven-point rule of fund_solver.h.  12 planar scenes: how often the planted pose comes back and how often its twin.
    With 20 % outliers a sample of five is outlier-free with probability 0.33, so among 512 hypotheses one is (1 - 1e-88): every scene is
    valid and the winner holds at least half of the planted inliers.
    Measured with the host builds: near-planar, every off-plane inlier kept by the five-point rule in 12 of 12 scenes, by the seven-point
    rule in 5 of 12; planar, the planted pose (rotation within 2 deg, direction within 10 deg) in 5 of 12 scenes, the twin in the others."""
    import fund_cases as F
    kept5 = kept7 = planted = 0
    for s in range(12):
        m, R, t, out, off = C.planar_scene(800 + s)
        a, b = C.host_ransac(m, iters=512, seed=s), F.host_ransac(m, iters=512, seed=s)
        want = off & ~out
        assert a['valid'] == 1 and a['n_inliers'] >= 0.5 * int((~out).sum())
        k5, k7 = int((a['inliers'] & want).sum()), int((b['inliers'] & want).sum())
        kept5 += k5 == int(want.sum())
        kept7 += k7 == int(want.sum())
        print(f'near-planar {800 + s}: off-plane planted {int(want.sum())}, kept by five points {k5}, by seven points {k7}')
    for s in range(12):
        m, R, t, out, off = C.planar_scene(900 + s, plane_frac=1.0)
        a = C.host_ransac(m, iters=512, seed=s)
        assert a['valid'] == 1 and a['n_inliers'] >= 0.5 * int((~out).sum())
        er, et = P.pose_errors(a['R'], a['t'], R, t)
        planted += er < 2 and et < 10
        print(f'planar {900 + s}: rotation error {er:.2f} deg, translation direction {et:.2f} deg')
    print(f'near-planar: every off-plane inlier kept in {kept5} (five points) / {kept7} (seven points) of 12 scenes; planar: the planted pose in '
          f'{planted} of 12')
