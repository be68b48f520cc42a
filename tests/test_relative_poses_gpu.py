"""matcher.relative_poses on the GPU: three planted pairs through one upload and one read back, against ops.ransac_relative_pose on the
packed rows, and into consolidate_matches.  Pairs: tests/relpose_cases.py."""
import numpy as np
import pytest
import torch

import pose_cases as P
import relpose_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def three():
    """pair 0: 300 rows; pair 1: 6 rows (a pose, but fewer inliers than min_inliers); pair 2: 129 rows, some filtered"""
    names = ['a.png', 'b.png', 'c.png']
    intr = {n: C.intrinsics(k) for k, n in enumerate(names)}
    pairs = [('a.png', 'b.png'), ('b.png', 'c.png'), ('a.png', 'c.png')]
    results = []
    for k, ((a, b), n) in enumerate(zip(pairs, (300, 6, 129))):
        m = C.reproject(C.rows(P.scene(950 + k, n, 0.3, 0.3)), intr[a], intr[b])
        s = np.full(n, 0.9, np.float32)
        if k == 2:
            m, s, _ = C.with_filtered(m)
        results.append((m.astype(np.float64), m[:, :2], m[:, 2:], s))
    return pairs, results, intr


@pytest.mark.parametrize('refit', [0, 4])
def test_relative_poses(three, refit):
    from geoformer_amd import matcher as MT, ops
    pairs, results, intr = three
    rp = MT.relative_poses(pairs, results, intr, thr=1.0, min_inliers=15, device=DEV, refit=refit)
    ms = [np.asarray(r[0], np.float32) for r in results]
    off = np.concatenate([[0], np.cumsum([len(m) for m in ms])]).astype(np.int32)
    t = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=DEV)
    rs = ops.ransac_relative_pose(t(np.concatenate(ms)), t(np.concatenate([r[3] for r in results])), t(off, torch.int32), 3,
                                  t(np.stack([intr[a] for a, _ in pairs])), t(np.stack([intr[b] for _, b in pairs])), pixel_thr=1.0, refit=refit)
    rs = {k: v.cpu().numpy() for k, v in rs.items()}
    for k in ('E', 'R', 't', 'n_inliers'):
        assert np.array_equal(getattr(rp, k), rs[k]), k
    assert np.array_equal(rp.rounds, rs['rounds'] if refit else np.zeros(3, np.int32))
    assert list(rs['valid']) == [1, 1, 1] and rs['n_inliers'][1] < 15
    assert list(rp.verified) == [True, False, True]
    for p in range(3):
        want = rs['inliers'][off[p]:off[p + 1]].astype(bool) if rp.verified[p] else np.zeros(len(ms[p]), bool)
        assert rp.masks[p].dtype == bool and np.array_equal(rp.masks[p], want)
        assert int(rp.masks[p].sum()) == (rp.n_inliers[p] if rp.verified[p] else 0)
    assert list(MT.relative_poses(pairs, results, intr, min_inliers=5, device=DEV, refit=refit).verified) == [True, True, True]
    # the planted poses (0.3 px noise): a degree or two for the five-point winner
    for p, seed in ((0, 950), (2, 952)):
        sc = P.scene(seed, (300, 6, 129)[p], 0.3, 0.3)
        er, et = P.pose_errors(rp.R[p], rp.t[p], sc['R'], sc['t'])
        assert er < 2.0 and et < 8.0, (p, er, et)
    # only the inliers of verified pairs are consolidated
    got = MT.consolidate_matches(pairs, results, device=DEV, keep=rp.masks)
    want = MT.consolidate_matches(pairs, [tuple(np.asarray(x)[k] for x in r) for r, k in zip(results, rp.masks)], device=DEV)
    assert all(np.array_equal(a, b) for a, b in zip(got.keypoints, want.keypoints))
    assert all(np.array_equal(a, b) for a, b in zip(got.matches, want.matches))
    assert len(got.matches[1]) == 0 and sum(len(x) for x in got.matches) > 0


def test_a_missing_image_is_an_error_before_any_upload(three, monkeypatch):
    from geoformer_amd import matcher as MT, ops
    pairs, results, intr = three
    monkeypatch.setattr(ops, 'ransac_relative_pose', lambda *a, **k: pytest.fail('the device was reached'))
    monkeypatch.setattr(torch, 'from_numpy', lambda *a, **k: pytest.fail('an upload was prepared'))
    with pytest.raises(ValueError, match=r"relative_poses: no intrinsics for 'c.png'"):
        MT.relative_poses(pairs, results, {k: v for k, v in intr.items() if k != 'c.png'}, device=DEV)
    with pytest.raises(ValueError, match='3 pairs but 2 results'):
        MT.relative_poses(pairs, results[:2], intr, device=DEV)


def test_no_pairs():
    from geoformer_amd import matcher as MT
    rp = MT.relative_poses([], [], {}, device=DEV)
    assert rp.E.shape == (0, 3, 3) and rp.t.shape == (0, 3) and rp.masks == [] and rp.verified.dtype == bool
