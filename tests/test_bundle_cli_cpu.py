"""`python -m geoformer_amd.matcher refine` on written files, read back; matcher.refine's host side and write_poses.  No GPU: the device
step (sfm._refine_device) is replaced by the host build of the same rule, which the GPU tests show to be bit-identical."""
import os

import numpy as np
import pytest

import bundle_cases as bc


@pytest.fixture()
def planted(monkeypatch):
    from geoformer_amd import matcher, sfm
    monkeypatch.setattr(sfm, '_refine_device', bc.host_refine_device)
    s = bc.make_scene(21, n_cams=6, n_points=150, outliers=0.05)
    free = bc.free_flags(s)
    bc.keep_fixed_true(s, free)
    names, kps, pim, ms, obs_kp = bc.to_consolidated(s)
    cm = matcher.ConsolidatedMatches(names, kps, pim, ms)
    T = len(s.X)
    pok = [np.full(len(k), -1, np.int32) for k in kps]
    for p in range(T):
        for o in range(s.obs_off[p], s.obs_off[p + 1]):
            pok[s.obs_image[o]][obs_kp[o]] = p
    tt = matcher.TriangulatedTracks(s.X.copy(), np.zeros(T), s.obs_off, s.obs_image, obs_kp, pok, T, 0, 0)
    intr = {nm: s.K[i].reshape(3, 3).astype(np.float64) for i, nm in enumerate(names)}
    poses = {nm: (s.R[i].reshape(3, 3), s.t[i]) for i, nm in enumerate(names)}
    return matcher, s, cm, tt, intr, poses, [names[0], names[-1]]


def test_refine_returns_refined_poses_and_inlier_tracks(planted):
    matcher, s, cm, tt, intr, poses, fixed = planted
    rs = matcher.refine(cm, tt, intr, poses, fixed=fixed, iters=16, thr=(20.0, 8.0, 4.0), min_obs=2)
    assert rs.n_free == 4 and rs.cost.shape == (51,) and rs.accepted.shape == (48,)
    assert list(rs.poses) == list(poses)
    for nm in fixed:
        assert rs.poses[nm][0].tobytes() == poses[nm][0].tobytes() and np.array_equal(rs.poses[nm][1], poses[nm][1])
    R = np.stack([rs.poses[nm][0] for nm in cm.names]).reshape(-1, 9)
    t = np.stack([rs.poses[nm][1] for nm in cm.names])
    before, after = bc.centre_errors(s.R, s.t, s), bc.centre_errors(R, t, s)
    assert np.median(after[1:-1]) < 0.2 * np.median(before[1:-1])
    tr = rs.tracks
    # the layout of TriangulatedTracks: inlier observations only, no planted outlier among them, every kept point with >= min_obs
    kept = set(zip(tr.obs_image.tolist(), tr.obs_keypoint.tolist()))
    _, _, _, _, obs_kp = bc.to_consolidated(s)
    outl = set(zip(s.obs_image[s.outlier].tolist(), obs_kp[s.outlier].tolist()))
    assert not (kept & outl) and len(kept) == len(tr.obs_image) >= 0.9 * (~s.outlier).sum()
    assert tr.obs_offsets[0] == 0 and tr.obs_offsets[-1] == len(tr.obs_image) and np.all(np.diff(tr.obs_offsets) >= 2)
    assert len(tr.points) == len(tr.errors) == len(tr.obs_offsets) - 1
    assert 0.2 < np.median(tr.errors) < 1.5                                # 0.5 px noise per coordinate
    for p in range(len(tr.points)):
        for o in range(tr.obs_offsets[p], tr.obs_offsets[p + 1]):
            assert tr.point_of_keypoint[tr.obs_image[o]][tr.obs_keypoint[o]] == p
    assert sum(int((pk >= 0).sum()) for pk in tr.point_of_keypoint) == len(tr.obs_image)
    assert tr.n_tracks == tt.n_tracks and tr.n_rejected == tt.n_rejected + len(tt.points) - len(tr.points)
    # the moved origin changes nothing a user sees: the same scene 1000 units away refines to the same poses, moved
    shift = np.array([1000.0, -2000.0, 500.0])
    poses2 = {nm: (Rn, tn - Rn @ shift) for nm, (Rn, tn) in poses.items()}
    tt2 = tt._replace(points=tt.points + shift)
    rs2 = matcher.refine(cm, tt2, intr, poses2, fixed=fixed, iters=16, thr=(20.0, 8.0, 4.0))
    assert np.abs(rs2.tracks.points - shift - tr.points).max() < 1e-9
    with pytest.raises(ValueError, match='not an image'):
        matcher.refine(cm, tt, intr, poses, fixed=['nowhere.png'])
    with pytest.raises(ValueError, match='iters'):
        matcher.refine(cm, tt, intr, poses, iters=65)


def test_more_than_128_free_images_is_a_value_error_that_names_the_limit(planted):
    matcher, s, cm, tt, intr, poses, fixed = planted
    n = 131
    names = [f'db/x{i:03d}.png' for i in range(n)]
    kps = [np.array([[10.0, 10.0]], np.float32)] * n
    cm2 = matcher.ConsolidatedMatches(names, kps, np.zeros((0, 2), np.int32), [])
    tt2 = matcher.TriangulatedTracks(np.array([[0.0, 0.0, 5.0]]), np.zeros(1), np.array([0, n], np.int32), np.arange(n, dtype=np.int32),
                                     np.zeros(n, np.int32), [np.zeros(1, np.int32)] * n, 1, 0, 0)
    K = np.array([[500.0, 0, 10], [0, 500.0, 10], [0, 0, 1]])
    with pytest.raises(ValueError, match='128'):
        matcher.refine(cm2, tt2, {nm: K for nm in names}, {nm: (np.eye(3), np.zeros(3)) for nm in names}, fixed=names[:2])
    rs = matcher.refine(cm2, tt2, {nm: K for nm in names}, {nm: (np.eye(3), np.zeros(3)) for nm in names}, fixed=names[:3], iters=1)
    assert rs.n_free == 128


def test_write_poses_is_what_read_poses_reads(tmp_path, planted):
    matcher, s, cm, tt, intr, poses, fixed = planted
    f = tmp_path / 'poses.txt'
    matcher.write_poses(str(f), poses)
    back = matcher.read_poses(str(f))
    assert list(back) == [str(tmp_path / nm) for nm in poses]
    for nm, (R, t) in poses.items():
        assert np.abs(back[str(tmp_path / nm)][0] - R).max() < 1e-12 and np.array_equal(back[str(tmp_path / nm)][1], t)


def test_refine_command_on_written_files(tmp_path, planted, capsys):
    matcher, s, cm, tt, intr, poses, fixed = planted
    kp = str(tmp_path / 'kp')
    matcher.write_consolidated(kp, cm)
    matcher.write_triangulated(str(tmp_path / 'pts.npz'), tt)
    matcher.write_poses(str(tmp_path / 'poses.txt'), poses)
    with open(tmp_path / 'intr.txt', 'w') as f:
        for nm, K in intr.items():
            f.write(' '.join([nm] + [repr(float(K[i, j])) for i, j in ((0, 0), (1, 1), (0, 2), (1, 2))]) + '\n')
    (tmp_path / 'fixed.txt').write_text('# trusted\n' + '\n'.join(fixed) + '\n')
    argv = ['refine', kp, '--points', str(tmp_path / 'pts.npz'), '--poses', str(tmp_path / 'poses.txt'), '--intrinsics', str(tmp_path / 'intr.txt'),
            '--fixed', str(tmp_path / 'fixed.txt'), '--thr', '20,8,4', '--out', str(tmp_path / 'pts2.npz'), '--out-poses', str(tmp_path / 'poses2.txt')]
    matcher.main(argv)
    said = capsys.readouterr().out
    assert '4 free and 2 fixed images' in said and 'pts2.npz' in said
    want = matcher.refine(cm, tt, intr, poses, fixed=fixed, iters=16, thr=(20.0, 8.0, 4.0))
    tt2 = matcher.read_triangulated(str(tmp_path / 'pts2.npz'))
    # (the poses went through quaternions in a text file: the last bits of the start differ, the integer tables must not)
    assert np.abs(tt2.points - want.tracks.points).max() < 1e-7 and np.abs(tt2.errors - want.tracks.errors).max() < 1e-6   # (units, pixels)
    for a, b in zip(tt2[2:5], want.tracks[2:5]):
        assert a.dtype == np.int32 and np.array_equal(a, b)
    assert all(np.array_equal(a, b) for a, b in zip(tt2.point_of_keypoint, want.tracks.point_of_keypoint))
    poses2 = matcher.read_poses(str(tmp_path / 'poses2.txt'))
    for nm in cm.names:
        R2, t2 = poses2[str(tmp_path / nm)]
        assert np.abs(R2 - want.poses[nm][0]).max() < 1e-7 and np.abs(t2 - want.poses[nm][1]).max() < 1e-7
    # `triangulate` and `localize-sparse` take these files as they are: the parser and the readers (their device halves are the GPU tests')
    ap = matcher.build_parser()
    a = ap.parse_args(['refine', 'kp', '--points', 'p', '--poses', 'q', '--intrinsics', 'k', '--out', 'o', '--out-poses', 'op'])
    assert (a.iters, a.thr, a.min_obs, a.fixed, a.device) == (16, '4.0', 2, None, 'cuda') and not hasattr(a, 'ckpt')
    for extra in (['--iters', '0'], ['--iters', '65'], ['--thr', '0'], ['--thr', 'x'], ['--min-obs', '1']):
        with pytest.raises(SystemExit):
            matcher.main(['refine', 'no_such_dir', '--points', 'p', '--poses', 'q', '--intrinsics', 'k', '--out', 'o', '--out-poses', 'op'] + extra)
    with pytest.raises(SystemExit):
        ap.parse_args(['refine', 'kp', '--points', 'p', '--poses', 'q', '--intrinsics', 'k', '--out', 'o'])
