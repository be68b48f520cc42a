"""The host-side pieces of `python -m geoformer_amd.matcher localize`: the parser, the intrinsics file, the quaternion of the output line."""
import numpy as np
import pytest

import abspose_cases as C


def test_parser_takes_the_localize_command():
    from geoformer_amd import matcher
    ap = matcher.build_parser()
    a = ap.parse_args(['localize', 'pairs.txt', '--xyz', 'maps', '--intrinsics', 'k.txt'])
    assert (a.cmd, a.list, a.xyz, a.intrinsics, a.out, a.thr, a.min_inliers, a.refit, a.sc_thres) == \
        ('localize', 'pairs.txt', 'maps', 'k.txt', None, 12.0, 12, 0, 0.25)
    assert a.imsize == 640 and a.batch == 8 and a.precision == 'fp16' and not a.no_match_upscale and a.cache_gb is None
    assert ap.parse_args(['localize', 'p', '--xyz', 'd', '--intrinsics', 'f', '--refit']).refit == 4
    assert ap.parse_args(['localize', 'p', '--xyz', 'd', '--intrinsics', 'f', '--refit', '2', '--thr', '5', '--out', 'o.txt']).refit == 2
    with pytest.raises(SystemExit):
        ap.parse_args(['localize', 'p', '--xyz', 'd'])


def test_read_intrinsics(tmp_path):
    from geoformer_amd import matcher
    f = tmp_path / 'k.txt'
    f.write_text('# query fx fy cx cy\nquery/a.png 500 510 320 240\n\n/abs/b.png 1 2 3 4\n')
    k = matcher.read_intrinsics(str(f))
    assert set(k) == {str(tmp_path / 'query' / 'a.png'), '/abs/b.png'}
    assert np.array_equal(k[str(tmp_path / 'query' / 'a.png')], [[500, 0, 320], [0, 510, 240], [0, 0, 1]])
    f.write_text('a.png 1 2 3\n')
    with pytest.raises(ValueError, match='fx fy cx cy'):
        matcher.read_intrinsics(str(f))


def test_rotation_to_quaternion():
    from geoformer_amd import matcher
    rng = np.random.default_rng(3)
    cases = [C.geometry(rng)[0] for _ in range(20)] + [np.eye(3), np.diag([1.0, -1, -1]), np.diag([-1.0, 1, -1]), np.diag([-1.0, -1, 1])]
    for R in cases:
        w, x, y, z = q = matcher.rotation_to_quaternion(R)
        back = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        assert w >= 0 and abs(np.linalg.norm(q) - 1) < 1e-12 and np.abs(back - R).max() < 1e-12
