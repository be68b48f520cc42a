"""Lens distortion on the host: the rule of csrc/camera_spec.h through its serial build (csrc/host/camera_host.cpp) against a numpy
longdouble gold that does not read the header, its edges, the camera files, the parser, and the chain undistort -> keypoints -> points on
the host builds (tests/camera_cases.py)."""
import os

import numpy as np
import pytest

import camera_cases as CC
import triangulate_cases as C

DISTORTING = [k for k in CC.CAMERAS if 'pinhole' not in k]
N = 1000


@pytest.fixture(scope='module')
def planted():
    """per camera: (record, the fp32 real-image pixels of N in-domain ideal points, the ideal normalised points)"""
    out = {}
    for seed, key in enumerate(CC.CAMERAS):
        rec = CC.record(CC.camera(key))
        x, y = CC.in_domain_points(rec, N, 100 + seed)
        out[key] = (rec, CC.distorted_pixels(rec, x, y), x, y)
    return out


@pytest.mark.parametrize('key', list(CC.CAMERAS))
def test_host_build_equals_the_longdouble_gold_to_one_ulp(planted, key):
    """Both sides are within 1e-9 normalised units of the pre-image before their one rounding to fp32, so they can differ only where
    that rounding falls on two sides of a boundary: at most 1 fp32 ulp, on every point."""
    rec, px, _, _ = planted[key]
    gold, res = CC.gold_undistort(rec, px)
    assert res < 1e-17                                                   # the reference itself has converged
    out, st = CC.host_one(CC.camera(key), px)
    assert not st.any() and np.isfinite(out).all()
    ulps = CC.ulps_apart(out, gold)
    print(f'{key}: {100.0 * (out == gold).all(1).mean():.1f} % of {len(px)} points equal the gold exactly, worst {ulps.max():.2f} ulp')
    assert ulps.max() <= 1.0


@pytest.mark.parametrize('key', DISTORTING)
def test_newton_steps_stay_far_below_the_cap(planted, key):
    rec, px, _, _ = planted[key]
    h = CC.host_lib()
    xy, steps, most = np.zeros(2), np.zeros(1, np.int32), 0
    for u, v in px[:200].astype(np.float64):
        assert h.gf_camera_host_undistort(CC._p(rec), (u - rec[2]) / rec[0], (v - rec[3]) / rec[1], CC._p(xy), CC._p(steps)) == 1
        most = max(most, int(steps[0]))
    assert most <= 16


@pytest.mark.parametrize('key', DISTORTING)
def test_round_trip_within_the_rounding_of_the_ideal_pixel(planted, key):
    """distort(undistort(p)) against p.  The ideal pixel is rounded to fp32 (half an ulp per coordinate), the closed form carries that
    through the camera's Jacobian (two entries per row, each at most the largest entry), and its own result is rounded once more: 1 ulp
    times the largest Jacobian entry of the camera over the planted points, plus 1 ulp.  The ulp is that of the largest coordinate
    involved, before or after."""
    rec, px, x, y = planted[key]
    cam = CC.camera(key)
    ideal, st = CC.host_one(cam, px)
    back, _ = CC.host_one(cam, ideal, inverse=0)
    assert not st.any()
    j00, j01, j10, j11 = CC.np_jacobian(rec, x, y)
    jmax = max(np.abs(j00).max(), np.abs(j01 * rec[0] / rec[1]).max(), np.abs(j10 * rec[1] / rec[0]).max(), np.abs(j11).max())
    ulp = np.spacing(np.maximum(np.abs(px).max(1), np.abs(ideal).max(1)).astype(np.float32)).astype(np.float64)
    err = np.abs(back.astype(np.float64) - px.astype(np.float64)).max(1)
    print(f'{key}: largest Jacobian entry {jmax:.3f}, worst round trip {np.max(err / ulp):.2f} ulp of {jmax + 1:.2f} allowed')
    assert np.all(err <= ulp * jmax + ulp)


@pytest.mark.parametrize('key', ['simple_pinhole', 'pinhole'])
def test_zero_distortion_returns_the_input_bits(key):
    rng = np.random.default_rng(3)
    px = rng.uniform(-500, 3000, (257, 2)).astype(np.float32)
    px[5] = [-0.0, 1e-30]
    for inverse in (1, 0):
        out, st = CC.host_one(CC.camera(key), px, inverse)
        assert out.tobytes() == px.tobytes() and not st.any()
    from geoformer_amd import matcher
    zero = matcher.Camera('OPENCV', 10, 10, (900.0, 950.0, 700.0, 500.0, 0.0, -0.0, 0.0, 0.0))
    out, st = CC.host_one(zero, px)
    assert out.tobytes() == px.tobytes() and not st.any()


def test_failures_and_non_finite_rows():
    from geoformer_amd import matcher
    cam = matcher.Camera('SIMPLE_RADIAL', 1600, 1200, (800.0, 800.0, 600.0, -0.3))
    nan, inf = np.float32('nan'), np.float32('inf')
    px = np.array([[800 + 800 * 0.69, 600], [800 + 800 * 0.71, 600], [800 + 800 * 2.0, 600], [nan, nan], [inf, 600], [800, -inf], [nan, 600],
                   [800, nan], [800, 600]], np.float32)
    out, st = CC.host_one(cam, px)
    assert st.tolist() == [0, 2, 2, 1, 1, 1, 1, 1, 0]
    assert np.isfinite(out[[0, 8]]).all() and np.isnan(out[1:8]).all()
    assert out[8].tolist() == [800.0, 600.0] and out[0, 0] > px[0, 0] and out[0, 1] == 600.0
    # a pinhole camera reports a non-finite row as well
    out, st = CC.host_one(matcher.Camera('PINHOLE', 1600, 1200, (800.0, 800.0, 800.0, 600.0)), px)
    assert st.tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 0] and np.isnan(out[3:8]).all() and out[:3].tobytes() == px[:3].tobytes()
    # the closed form has no failure; a non-finite row is NaN
    out, st = CC.host_one(cam, px, inverse=0)
    assert st.tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 0] and np.isnan(out[3:8]).all() and np.isfinite(out[:3]).all()


def test_a_point_beyond_the_fold_gets_the_pre_image_inside_it():
    """k = -0.3: the radial profile r (1 - 0.3 r^2) rises to 0.7027 at r = 1.054 and falls again; r = 1.3 lands on 0.6409, whose pre-image
    inside the fold is r = 0.8045..."""
    from geoformer_amd import matcher
    cam = matcher.Camera('SIMPLE_RADIAL', 1600, 1200, (800.0, 800.0, 600.0, -0.3))
    rd = 1.3 * (1 - 0.3 * 1.3 ** 2)
    out, st = CC.host_one(cam, np.array([[800 + 800 * rd, 600]], np.float32))
    r = (float(out[0, 0]) - 800) / 800
    assert st[0] == 0 and r < 1.054 and abs(r * (1 - 0.3 * r * r) - rd) < 1e-6


def test_argument_errors_of_the_list_form():
    rec = np.stack([CC.record(CC.camera(k)) for k in CC.CAMERAS])
    px = np.random.default_rng(5).uniform(300, 900, (40, 2)).astype(np.float32)
    rc, out, st, flags = CC.host_points(px, 0, [0, 10, 10, 40], [2, 99, 4], rec)
    assert rc == 0 and flags.tolist() == [0, 1] and not st.any()          # an empty segment's camera is checked too; no row belongs to it
    rc, out, st, flags = CC.host_points(px, 0, [0, 10, 40], [2, 7], rec)
    assert rc == 0 and flags.tolist() == [0, 1] and not st[:10].any() and (st[10:] == 3).all() and np.isnan(out[10:]).all()
    rc, out, st, flags = CC.host_points(px, 0, [0, 10, 40], [2, -1], rec)
    assert rc == 0 and flags.tolist() == [0, 1] and (st[10:] == 3).all()
    for off in ([0, 30, 20, 40], [1, 20, 40], [0, 20, 39], [0, 20, 50], [-3, 2 ** 30, 40]):
        rc, out, st, flags = CC.host_points(px, 0, off, [2, 4], rec)
        assert rc == 0 and flags.tolist() == [1, 0], off
    rc, out, st, flags = CC.host_points(px, 0, [0, 20, 39], [2, 4], rec)
    assert st[39] == 3 and np.isnan(out[39]).all() and not st[:39].any()
    assert CC.host_points(px, 0, [0, 40], [0], rec, P=-1)[0] == -1
    assert CC.host_points(px, 0, [0, 40], [0], rec[:0])[0] == -1          # C == 0 with points present
    assert CC.host_points(px, 0, [0], [], rec)[0] == -1                   # S == 0 with points present
    rc, out, st, flags = CC.host_points(px[:0], 0, [0], [], rec)
    assert rc == 0 and len(out) == 0 and not flags.any()                  # an empty call


# --------------------------------------------------------------------------------------------- files
def test_cameras_file_round_trip(tmp_path):
    from geoformer_amd import matcher
    f = tmp_path / 'cams.txt'
    f.write_text('# hloc query list\n\nq/a.jpg SIMPLE_RADIAL 1600 1200 1469.2 800 600 -0.0353\n'
                 f'{tmp_path}/db/b.png PINHOLE 640 480 500 501.5 320 240\nc.png SIMPLE_PINHOLE 10 20 7 5 10\n'
                 'd.png RADIAL 10 20 7 5 10 -0.2 0.05\ne.png OPENCV 10 20 7 8 5 10 -0.25 0.08 1e-3 -2e-3\n')
    cams = matcher.read_cameras(str(f))
    assert list(cams) == [str(tmp_path / 'q' / 'a.jpg'), str(tmp_path / 'db' / 'b.png')] + [str(tmp_path / n) for n in ('c.png', 'd.png', 'e.png')]
    a = cams[str(tmp_path / 'q' / 'a.jpg')]
    assert a == matcher.Camera('SIMPLE_RADIAL', 1600, 1200, (1469.2, 800.0, 600.0, -0.0353)) and isinstance(a.width, int)
    assert cams[str(tmp_path / 'e.png')].params == (7.0, 8.0, 5.0, 10.0, -0.25, 0.08, 1e-3, -2e-3)
    g = tmp_path / 'sub' / 'again.txt'
    os.makedirs(g.parent)
    matcher.write_cameras(str(g), cams)
    assert matcher.read_cameras(str(g)) == cams
    g2 = tmp_path / 'again.txt'
    matcher.write_cameras(str(g2), cams)
    assert matcher.read_cameras(str(g2)) == cams and g2.read_text().splitlines()[0].startswith('q/a.jpg SIMPLE_RADIAL 1600 1200 1469.2 ')


@pytest.mark.parametrize('line, message', [
    ('a.png FISHEYE 10 10 5 5 5', r"cams.txt:2: unknown camera model 'FISHEYE' (supported: SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV)"),
    ('a.png OPENCV_FISHEYE 10 10 5 5 5 5 0 0 0 0',
     r"cams.txt:2: unknown camera model 'OPENCV_FISHEYE' (supported: SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV)"),
    ('a.png SIMPLE_RADIAL 10 10 5 5 5', r'cams.txt:2: SIMPLE_RADIAL takes 4 parameters, got 3'),
    ('a.png PINHOLE 10 10 5 5 5 5 5', r'cams.txt:2: PINHOLE takes 4 parameters, got 5'),
    ('a.png SIMPLE_RADIAL 10 10 5 5 5 nan', r'cams.txt:2: a parameter that is not finite'),
    ('a.png RADIAL 10 10 5 5 inf 0 0', r'cams.txt:2: a parameter that is not finite'),
    ('a.png SIMPLE_RADIAL 10 10 0 5 5 0.1', r'cams.txt:2: a focal length that is not positive'),
    ('a.png OPENCV 10 10 5 -5 5 5 0 0 0 0', r'cams.txt:2: a focal length that is not positive'),
    ('a.png PINHOLE 10.5 10 5 5 5 5', r'cams.txt:2: W and H must be integers and the parameters numbers'),
    ('a.png PINHOLE 10 10 5 5 x 5', r'cams.txt:2: W and H must be integers and the parameters numbers'),
    ('a.png PINHOLE 10', r'cams.txt:2: expected `path MODEL W H params...`, got 3 fields'),
])
def test_cameras_file_errors_name_file_and_line(tmp_path, line, message):
    from geoformer_amd import matcher
    f = tmp_path / 'cams.txt'
    f.write_text('# one\n' + line + '\n')
    with pytest.raises(ValueError) as e:
        matcher.read_cameras(str(f))
    assert str(e.value) == str(tmp_path) + os.sep + message


def test_canonical_records_and_pinhole_of(tmp_path):
    from geoformer_amd import matcher
    cams = {k: CC.camera(k) for k in CC.CAMERAS}
    assert matcher.canonical_camera(cams['simple_pinhole']) == (1000.0, 1000.0, 640.0, 480.0, 0.0, 0.0, 0.0, 0.0)
    assert matcher.canonical_camera(cams['pinhole']) == (1000.0, 1010.0, 640.0, 480.0, 0.0, 0.0, 0.0, 0.0)
    assert matcher.canonical_camera(cams['simple_radial_m0.3']) == (1000.0, 1000.0, 640.0, 480.0, -0.3, 0.0, 0.0, 0.0)
    assert matcher.canonical_camera(cams['radial']) == (1000.0, 1000.0, 640.0, 480.0, -0.2, 0.05, 0.0, 0.0)
    assert matcher.canonical_camera(cams['opencv']) == (900.0, 950.0, 700.0, 500.0, -0.25, 0.08, 1e-3, -2e-3)
    with pytest.raises(ValueError):
        matcher.canonical_camera(matcher.Camera('FULL_OPENCV', 1, 1, (1.0,) * 12))
    with pytest.raises(ValueError):
        matcher.canonical_camera(matcher.Camera('RADIAL', 1, 1, (1.0,) * 4))
    Ks = matcher.pinhole_of(cams)
    assert list(Ks) == list(cams)
    assert np.array_equal(Ks['opencv'], [[900, 0, 700], [0, 950, 500], [0, 0, 1]]) and np.array_equal(Ks['radial'], [[1000, 0, 640], [0, 1000, 480], [0, 0, 1]])
    f = tmp_path / 'intrinsics.txt'
    matcher.write_intrinsics(str(f), {str(tmp_path / k): v for k, v in Ks.items()})
    back = matcher.read_intrinsics(str(f))
    assert all(np.array_equal(back[str(tmp_path / k)], v) for k, v in Ks.items())


def test_parser_cameras_flags():
    from geoformer_amd import matcher
    ap = matcher.build_parser()
    assert ap.parse_args(['pairs', 'list.txt']).cameras is None
    a = ap.parse_args(['pairs', 'list.txt', '--cameras', 'c.txt', '--keypoints', 'kp', '--verify'])
    assert (a.cameras, a.keypoints, a.verify) == ('c.txt', 'kp', True)
    a = ap.parse_args(['localize', 'p', '--xyz', 'd', '--cameras', 'c.txt'])
    assert (a.cameras, a.intrinsics, a.thr, a.min_inliers, a.refit) == ('c.txt', None, 12.0, 12, 0)
    a = ap.parse_args(['localize', 'p', '--xyz', 'd', '--intrinsics', 'k.txt'])
    assert (a.cameras, a.intrinsics) == (None, 'k.txt')
    for argv in (['localize', 'p', '--xyz', 'd', '--intrinsics', 'k.txt', '--cameras', 'c.txt'], ['localize', 'p', '--xyz', 'd']):
        with pytest.raises(SystemExit):
            ap.parse_args(argv)
    for cmd in (['triangulate', 'kp', '--poses', 'p', '--intrinsics', 'i'], ['localize-sparse', 'kp', '--points', 'p', '--queries', 'q', '--intrinsics', 'i']):
        assert not hasattr(ap.parse_args(cmd), 'cameras')                # they run unchanged on what `pairs --cameras` wrote


def test_cameras_of_the_command_line_are_keyed_by_the_pair_list(tmp_path):
    from geoformer_amd import matcher
    f = tmp_path / 'cams.txt'
    f.write_text('a.png PINHOLE 10 10 5 5 5 5\nsub/b.png SIMPLE_RADIAL 10 10 5 5 5 -0.1\n')
    a, b = str(tmp_path / 'a.png'), str(tmp_path / 'sub' / 'b.png')
    cams = matcher._cameras_for(str(f), [(a, b), (b, a)])
    assert set(cams) == {a, b} and cams[b].model == 'SIMPLE_RADIAL'
    with pytest.raises(SystemExit, match='no camera for'):
        matcher._cameras_for(str(f), [(a, str(tmp_path / 'c.png'))])
    # the intrinsics file `pairs --keypoints OUT --cameras FILE` writes names the images as names.txt does and reads back through read_intrinsics
    out = tmp_path / 'kp' / 'intrinsics.txt'
    os.makedirs(out.parent)
    matcher.write_intrinsics(str(out), matcher.pinhole_of(cams), [b, a])
    assert out.read_text().splitlines() == [f'{b} 5.0 5.0 5.0 5.0', f'{a} 5.0 5.0 5.0 5.0']
    assert list(matcher.read_intrinsics(str(out))) == [b, a]


def test_undistort_results_needs_every_camera():
    from geoformer_amd import matcher
    sc = C.matcher_scene(n_points=20)
    cams = CC.scene_cameras(sc, -0.2)
    del cams[sc['names'][4]]
    with pytest.raises(ValueError, match='no camera for'):
        matcher.undistort_results(sc['pairs'], sc['results'], cams)
    with pytest.raises(ValueError, match='27 pairs but 26 results'):
        matcher.undistort_results(sc['pairs'], sc['results'][:-1], CC.scene_cameras(sc, -0.2))


# --------------------------------------------------------------------------------------------- the chain on the host builds
def _host_chain(scene, results):
    cm = C.host_consolidated(dict(scene, results=results))
    return cm, C.host_triangulated(cm, scene['intrinsics'], scene['db_poses'])


@pytest.fixture(scope='module')
def base_chain():
    sc = C.matcher_scene()
    cm, tt = _host_chain(sc, sc['results'])
    return sc, float(np.median(CC.point_errors(sc, cm, tt))), len(tt.points)


@pytest.mark.parametrize('k', [-0.2, -0.05])
def test_chain_on_host_builds(base_chain, k):
    """matcher_scene's observations distorted with the radial term k, undistorted through the host build, then the host consolidation
    and triangulation: the median 3-D error is at most 1.01 times the undistorted scene's and every point is kept.  Measured: a ratio of
    0.999998 at k = -0.2 and 1.000004 at k = -0.05.  The same observations taken as pinhole are at least twice as bad at k = -0.2
    (measured: 4.24 times; 1.63 times at k = -0.05, where nothing is asserted)."""
    from geoformer_amd import matcher
    sc, base, n_base = base_chain
    cams = CC.scene_cameras(sc, k)
    assert all(np.array_equal(v, sc['intrinsics'][n]) for n, v in matcher.pinhole_of(cams).items())
    dist = CC.distorted_scene(sc, cams)
    res, status = CC.host_undistorted_results(dist['pairs'], dist['results'], cams)
    assert not any(s.any() for s in status)
    und = CC.with_uv_of_results(dist, res)
    cm, tt = _host_chain(und, res)
    e_und = float(np.median(CC.point_errors(und, cm, tt)))
    cmd, ttd = _host_chain(dist, dist['results'])
    e_pin = float(np.median(CC.point_errors(dist, cmd, ttd)))
    print(f'k = {k}: median 3-D error {base:.6f} undistorted scene, {e_und:.6f} undistorted first (ratio {e_und / base:.6f}), '
          f'{e_pin:.6f} taken as pinhole ({e_pin / base:.2f} x); {len(tt.points)} of {n_base} points')
    assert n_base == 300 and len(tt.points) == 300
    assert e_und <= 1.01 * base
    if k == -0.2:
        assert e_pin >= 2 * base
