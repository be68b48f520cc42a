"""The host-side pieces of `python -m geoformer_amd.matcher triangulate`: the consolidated directory read back, the poses file, the
parser's defaults and errors.  No GPU."""
import numpy as np
import pytest

import triangulate_cases as C


def test_consolidated_round_trip(tmp_path):
    from geoformer_amd import matcher
    rng = np.random.default_rng(5)
    cm = matcher.ConsolidatedMatches(['/data/a.png', 'db/b with space.png', 'c.png'],
                                     [rng.uniform(0, 600, (4, 2)).astype(np.float32), np.zeros((0, 2), np.float32),
                                      rng.uniform(0, 600, (7, 2)).astype(np.float32)],
                                     np.array([[0, 2], [2, 0], [1, 2]], np.int32),
                                     [rng.integers(0, 4, (5, 2)).astype(np.int32), rng.integers(0, 4, (3, 2)).astype(np.int32), np.zeros((0, 2), np.int32)])
    matcher.write_consolidated(str(tmp_path / 'kp'), cm)
    back = matcher.read_consolidated(str(tmp_path / 'kp'))
    assert back.names == cm.names and np.array_equal(back.pair_images, cm.pair_images) and back.pair_images.dtype == np.int32
    assert len(back.keypoints) == 3 and len(back.matches) == 3
    for a, b in zip(back.keypoints + back.matches, cm.keypoints + cm.matches):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    empty = matcher.ConsolidatedMatches([], [], np.zeros((0, 2), np.int32), [])
    matcher.write_consolidated(str(tmp_path / 'none'), empty)
    back = matcher.read_consolidated(str(tmp_path / 'none'))
    assert back.names == [] and back.keypoints == [] and back.matches == [] and back.pair_images.shape == (0, 2)


def test_read_poses_reads_what_localize_writes(tmp_path):
    from geoformer_amd import matcher
    K, R, t = C.make_cameras(5, 9)
    f = tmp_path / 'poses.txt'
    names = ['db/a.png', 'db/b.png', '/abs/c.png', 'd.png', 'e.png']
    with open(f, 'w') as out:                                           # the line `localize --out` writes
        out.write('# path qw qx qy qz tx ty tz\n\n')
        for name, Ri, ti in zip(names, R, t):
            out.write(' '.join([name] + [repr(float(v)) for v in (*matcher.rotation_to_quaternion(Ri), *ti)]) + '\n')
    poses = matcher.read_poses(str(f))
    want = [str(tmp_path / 'db' / 'a.png'), str(tmp_path / 'db' / 'b.png'), '/abs/c.png', str(tmp_path / 'd.png'), str(tmp_path / 'e.png')]
    assert list(poses) == want
    for name, Ri, ti in zip(want, R, t):
        assert np.abs(poses[name][0] - Ri).max() < 1e-12 and np.array_equal(poses[name][1], ti)
    q = np.array([0.5, -0.5, 0.5, 0.5])
    assert np.abs(matcher.quaternion_to_rotation(3 * q) - matcher.quaternion_to_rotation(q)).max() < 1e-15          # normalised first
    assert np.abs(matcher.rotation_to_quaternion(matcher.quaternion_to_rotation(q)) - q).max() < 1e-12
    f.write_text('a.png 1 0 0 0 1 2\n')
    with pytest.raises(ValueError, match='qw qx qy qz tx ty tz'):
        matcher.read_poses(str(f))
    f.write_text('a.png 0 0 0 0 1 2 3\n')
    with pytest.raises(ValueError, match='quaternion'):
        matcher.read_poses(str(f))
    f.write_text('a.png 1 0 0 0 1 nan 3\n')
    with pytest.raises(ValueError, match='not finite'):
        matcher.read_poses(str(f))


def test_parser_takes_the_triangulate_command(capsys):
    from geoformer_amd import matcher
    ap = matcher.build_parser()
    a = ap.parse_args(['triangulate', 'kp', '--poses', 'p.txt', '--intrinsics', 'k.txt'])
    assert (a.cmd, a.keypoints, a.poses, a.intrinsics, a.out, a.thr, a.min_angle, a.min_obs, a.refit, a.device) == \
        ('triangulate', 'kp', 'p.txt', 'k.txt', None, 4.0, 1.5, 2, 2, 'cuda')
    assert not hasattr(a, 'ckpt') and not hasattr(a, 'imsize')           # no model behind this command
    assert ap.parse_args(['triangulate', 'kp', '--poses', 'p', '--intrinsics', 'k', '--refit']).refit == 4
    b = ap.parse_args(['triangulate', 'kp', '--poses', 'p', '--intrinsics', 'k', '--refit', '0', '--thr', '2.5', '--min-angle', '3', '--min-obs', '3',
                       '--out', 'o.npz'])
    assert (b.refit, b.thr, b.min_angle, b.min_obs, b.out) == (0, 2.5, 3.0, 3, 'o.npz')
    for bad in (['triangulate', 'kp', '--poses', 'p'], ['triangulate', 'kp', '--intrinsics', 'k'], ['triangulate', '--poses', 'p', '--intrinsics', 'k']):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    # values the device entry point would reject are the command line's errors, before anything is read
    for extra in (['--min-obs', '1'], ['--refit', '9'], ['--thr', '0']):
        with pytest.raises(SystemExit):
            matcher.main(['triangulate', 'no_such_dir', '--poses', 'p', '--intrinsics', 'k'] + extra)
    assert 'triangulate: need' in capsys.readouterr().err
    # the other commands are as they were
    assert ap.parse_args(['localize', 'pairs.txt', '--xyz', 'maps', '--intrinsics', 'k.txt']).refit == 0
