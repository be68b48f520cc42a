"""`python -m geoformer_amd.matcher refine --solver pcg` on written files, and matcher.refine(solver='pcg')'s host side.  No GPU: the device
step (sfm._refine_device) is replaced by the host build of the same rules, which the GPU tests show to be bit-identical."""
import numpy as np
import pytest

import bundle_cases as bc
import bundle_pcg_cases as pc


def as_matcher_inputs(matcher, s):
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
    return cm, tt, intr, poses, [names[0], names[-1]]


@pytest.fixture(scope='module')
def scene130():
    s = bc.make_scene(50, n_cams=132, n_points=300, drop=0.8)
    free = bc.free_flags(s)
    return bc.keep_fixed_true(s, free)


@pytest.fixture()
def planted(monkeypatch, scene130):
    from geoformer_amd import matcher, sfm
    monkeypatch.setattr(sfm, '_refine_device', pc.host_refine_device_pcg)
    return (matcher, scene130) + as_matcher_inputs(matcher, scene130)


def test_refine_with_pcg_takes_130_free_images_and_dense_names_the_limit(planted):
    matcher, s, cm, tt, intr, poses, fixed = planted
    with pytest.raises(ValueError, match=r"130 free images, the limit is 128 .*solver='pcg'"):
        matcher.refine(cm, tt, intr, poses, fixed=fixed, iters=4, thr=20.0)
    rs = matcher.refine(cm, tt, intr, poses, fixed=fixed, iters=8, thr=(20.0, 8.0), solver='pcg')
    assert rs.n_free == 130 and rs.cost.shape == (18,) and rs.accepted.shape == (16,)
    assert rs.cg_used.shape == (16,) and rs.cg_used.dtype == np.int32 and rs.cg_used.min() >= 1 and rs.cg_used.max() <= 64
    assert rs._fields[:5] == ('poses', 'tracks', 'cost', 'accepted', 'n_free') and rs._fields[-1] == 'cg_used'
    for nm in fixed:
        assert rs.poses[nm][0].tobytes() == poses[nm][0].tobytes() and np.array_equal(rs.poses[nm][1], poses[nm][1])
    R = np.stack([rs.poses[nm][0] for nm in cm.names]).reshape(-1, 9)
    t = np.stack([rs.poses[nm][1] for nm in cm.names])
    before, after = bc.centre_errors(s.R, s.t, s), bc.centre_errors(R, t, s)
    assert np.median(after[1:-1]) < 0.5 * np.median(before[1:-1])
    # a smaller cap is passed through: every stage logs at most that many
    rs3 = matcher.refine(cm, tt, intr, poses, fixed=fixed, iters=2, thr=20.0, solver='pcg', cg_iters=3, cg_tol=1e-3)
    assert rs3.cg_used.tolist() == [3, 3]


def test_the_dense_solver_still_returns_no_cg_log(monkeypatch):
    from geoformer_amd import matcher, sfm
    monkeypatch.setattr(sfm, '_refine_device', pc.host_refine_device_pcg)
    s = bc.make_scene(21, n_cams=6, n_points=150, outliers=0.05)
    bc.keep_fixed_true(s, bc.free_flags(s))
    cm, tt, intr, poses, fixed = as_matcher_inputs(matcher, s)
    d = matcher.refine(cm, tt, intr, poses, fixed=fixed, iters=4, thr=20.0)
    p = matcher.refine(cm, tt, intr, poses, fixed=fixed, iters=4, thr=20.0, solver='pcg')
    assert d.cg_used is None and p.cg_used.shape == (4,) and d.n_free == p.n_free == 4
    assert len(matcher.RefinedStructure({}, tt, np.zeros(0), np.zeros(0, np.int32), 0)) == 6                 # five positional fields still build one


def test_refine_command_with_solver_pcg_on_written_files(tmp_path, planted, capsys):
    matcher, s, cm, tt, intr, poses, fixed = planted
    kp = str(tmp_path / 'kp')
    matcher.write_consolidated(kp, cm)
    matcher.write_triangulated(str(tmp_path / 'pts.npz'), tt)
    matcher.write_poses(str(tmp_path / 'poses.txt'), poses)
    with open(tmp_path / 'intr.txt', 'w') as f:
        for nm, K in intr.items():
            f.write(' '.join([nm] + [repr(float(K[i, j])) for i, j in ((0, 0), (1, 1), (0, 2), (1, 2))]) + '\n')
    (tmp_path / 'fixed.txt').write_text('\n'.join(fixed) + '\n')
    argv = ['refine', kp, '--points', str(tmp_path / 'pts.npz'), '--poses', str(tmp_path / 'poses.txt'), '--intrinsics', str(tmp_path / 'intr.txt'),
            '--fixed', str(tmp_path / 'fixed.txt'), '--thr', '20', '--iters', '8', '--out', str(tmp_path / 'pts2.npz'), '--out-poses',
            str(tmp_path / 'poses2.txt')]
    with pytest.raises(ValueError, match='130 free images, the limit is 128'):          # without the flag: the dense solver's limit
        matcher.main(argv)
    assert not (tmp_path / 'pts2.npz').exists()
    matcher.main(argv + ['--solver', 'pcg'])
    said = capsys.readouterr().out
    assert '130 free and 2 fixed images' in said and 'pts2.npz' in said
    want = matcher.refine(cm, tt, intr, poses, fixed=fixed, iters=8, thr=20.0, solver='pcg')
    tt2 = matcher.read_triangulated(str(tmp_path / 'pts2.npz'))
    assert len(tt2.points) == len(want.tracks.points) and np.abs(tt2.points - want.tracks.points).max() < 1e-7
    poses2 = matcher.read_poses(str(tmp_path / 'poses2.txt'))
    assert len(poses2) == 132
    for nm in cm.names:
        R2, t2 = poses2[str(tmp_path / nm)]
        assert np.abs(R2 - want.poses[nm][0]).max() < 1e-7 and np.abs(t2 - want.poses[nm][1]).max() < 1e-7
    # the parser: defaults, the choices, the ranges; no model is loaded
    ap = matcher.build_parser()
    base = ['refine', 'kp', '--points', 'p', '--poses', 'q', '--intrinsics', 'k', '--out', 'o', '--out-poses', 'op']
    a = ap.parse_args(base)
    assert (a.solver, a.cg_iters, a.cg_tol) == ('dense', 64, 1e-6) and not hasattr(a, 'ckpt')
    a = ap.parse_args(base + ['--solver', 'pcg', '--cg-iters', '32', '--cg-tol', '1e-3'])
    assert (a.solver, a.cg_iters, a.cg_tol) == ('pcg', 32, 1e-3)
    for extra in (['--solver', 'sparse'], ['--solver', 'pcg', '--cg-iters', '0'], ['--solver', 'pcg', '--cg-iters', '257'],
                  ['--solver', 'pcg', '--cg-tol', '1'], ['--solver', 'pcg', '--cg-tol', '-1']):
        with pytest.raises(SystemExit):
            matcher.main(['refine', 'no_such_dir', '--points', 'p', '--poses', 'q', '--intrinsics', 'k', '--out', 'o', '--out-poses', 'op'] + extra)
