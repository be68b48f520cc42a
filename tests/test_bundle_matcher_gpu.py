"""matcher.refine on the GPU inside the chain triangulate -> refine -> triangulate -> localize_queries_sparse, on the planted one-place
scene of tests/triangulate_cases.py (matcher_scene: six database cameras, two queries) with perturbed database poses, against the same
chain without refine.  The model is not run."""
import numpy as np
import pytest

import bundle_cases as bc
import triangulate_cases as TC

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SCHEDULE = (20.0, 8.0, 4.0)          # see test_bundle_cpu.py: the start is about 10 px off


@pytest.fixture(scope='module')
def chain():
    from geoformer_amd import matcher
    sc = TC.matcher_scene()
    cm = matcher.consolidate_matches(sc['pairs'], sc['results'], qt_psize=0, device=DEV)
    db_pair = np.flatnonzero([a not in sc['queries'] and b not in sc['queries'] for a, b in sc['pairs']])
    cm_db = cm._replace(pair_images=cm.pair_images[db_pair], matches=[cm.matches[p] for p in db_pair])
    rng = np.random.default_rng(7)
    db = [sc['names'][i] for i in TC.DB]
    fixed = [db[0], db[-1]]                                               # the two end cameras: trusted, at their true poses
    rough = {}
    for nm in db:
        R, t = sc['db_poses'][nm]
        if nm in fixed:
            rough[nm] = (R.copy(), t.copy())
            continue
        w, d = rng.normal(size=3), rng.normal(size=3)
        Rn = bc.rodrigues(w * np.deg2rad(1.0) / np.linalg.norm(w)) @ R
        rough[nm] = (Rn, -Rn @ (-R.T @ t + 0.05 * d / np.linalg.norm(d)))
    return matcher, sc, cm, cm_db, rough, fixed


def centre(R, t):
    return -np.asarray(R).T @ np.asarray(t)


def query_errors(matcher, sc, cm, tt):
    lq = matcher.localize_queries_sparse(cm, tt, sc['queries'], sc['intrinsics'], refit=2, device=DEV)
    assert lq.localized.all()
    return np.array([np.linalg.norm(centre(lq.R[k], lq.t[k]) - centre(*sc['poses'][nm])) for k, nm in enumerate(lq.names)])


def test_refine_lowers_the_query_error_of_the_chain(chain):
    matcher, sc, cm, cm_db, rough, fixed = chain
    intr = sc['intrinsics']
    plain = {thr: query_errors(matcher, sc, cm, matcher.triangulate(cm_db, intr, rough, thr=thr, device=DEV)) for thr in (4.0, 20.0)}
    tt0 = matcher.triangulate(cm_db, intr, rough, thr=20.0, device=DEV)    # loose: the rough poses are about 10 px off
    rs = matcher.refine(cm_db, tt0, intr, rough, fixed=fixed, iters=16, thr=SCHEDULE, device=DEV)
    assert rs.n_free == 4 and rs.accepted.sum() >= 3 and np.all(np.diff(rs.cost.reshape(3, 17), axis=1) <= 0)
    tt1 = matcher.triangulate(cm_db, intr, rs.poses, device=DEV)
    refined = query_errors(matcher, sc, cm, tt1)
    db_before = np.median([np.linalg.norm(centre(*rough[nm]) - centre(*sc['db_poses'][nm])) for nm in rough if nm not in fixed])
    db_after = np.median([np.linalg.norm(centre(*rs.poses[nm]) - centre(*sc['db_poses'][nm])) for nm in rough if nm not in fixed])
    print(f'\nmedian query centre error: no refine, triangulate at 4 px {np.median(plain[4.0]):.5f}, at 20 px {np.median(plain[20.0]):.5f}; '
          f'with refine {np.median(refined):.5f}; database centres {db_before:.5f} -> {db_after:.5f}; points {len(tt0.points)} -> '
          f'{len(rs.tracks.points)} refined -> {len(tt1.points)} re-triangulated')
    assert np.median(refined) < np.median(plain[4.0]) and np.median(refined) < np.median(plain[20.0])
    assert db_after < db_before
    for nm in fixed:
        assert rs.poses[nm][0].tobytes() == rough[nm][0].tobytes() and rs.poses[nm][1].tobytes() == rough[nm][1].tobytes()


def test_the_device_step_of_refine_equals_the_host_build(chain):
    matcher, sc, cm, cm_db, rough, fixed = chain
    tt0 = matcher.triangulate(cm_db, sc['intrinsics'], rough, thr=20.0, device=DEV)
    a = matcher._refine_inputs(cm_db, tt0, sc['intrinsics'], rough, fixed)
    dev, ref = matcher._refine_device(a, SCHEDULE, 8, DEV), bc.host_refine_device(a, SCHEDULE, 8)
    for k in ('R', 't', 'X', 'cost', 'accepted', 'inliers'):
        assert np.asarray(dev[k]).tobytes() == np.asarray(ref[k]).tobytes(), k


def test_refine_command_feeds_triangulate_and_localize_sparse(chain, tmp_path, capsys):
    matcher, sc, cm, cm_db, rough, fixed = chain
    kp = str(tmp_path / 'kp')
    matcher.write_consolidated(kp, cm)                                     # queries included: they have no pose and take no part
    matcher.write_poses(str(tmp_path / 'poses.txt'), rough)
    with open(tmp_path / 'intr.txt', 'w') as f:
        for nm, K in sc['intrinsics'].items():
            f.write(' '.join([nm] + [repr(float(K[i, j])) for i, j in ((0, 0), (1, 1), (0, 2), (1, 2))]) + '\n')
    (tmp_path / 'fixed.txt').write_text('\n'.join(fixed) + '\n')
    common = ['--intrinsics', str(tmp_path / 'intr.txt')]
    matcher.main(['triangulate', kp, '--poses', str(tmp_path / 'poses.txt'), '--thr', '20', '--out', str(tmp_path / 'pts.npz')] + common)
    matcher.main(['refine', kp, '--points', str(tmp_path / 'pts.npz'), '--poses', str(tmp_path / 'poses.txt'), '--fixed', str(tmp_path / 'fixed.txt'),
                  '--thr', '20,8,4', '--out', str(tmp_path / 'pts2.npz'), '--out-poses', str(tmp_path / 'poses2.txt')] + common)
    assert '4 free and 2 fixed images' in capsys.readouterr().out
    matcher.main(['triangulate', kp, '--poses', str(tmp_path / 'poses2.txt'), '--out', str(tmp_path / 'pts3.npz')] + common)
    back = matcher.read_triangulated(str(tmp_path / 'pts2.npz'))
    again = matcher.read_triangulated(str(tmp_path / 'pts3.npz'))
    assert len(back.points) > 200 and len(again.points) >= len(back.points) - 5
    assert np.median(again.errors) < 1.5
    (tmp_path / 'queries.txt').write_text('\n'.join(sc['queries']) + '\n')
    lq = matcher.main(['localize-sparse', kp, '--points', str(tmp_path / 'pts3.npz'), '--queries', str(tmp_path / 'queries.txt'), '--refit', '2',
                       '--out', str(tmp_path / 'qposes.txt')] + common)
    assert '2 of 2 queries localised' in capsys.readouterr().out
    qp = matcher.read_poses(str(tmp_path / 'qposes.txt'))
    for nm in sc['queries']:
        assert np.linalg.norm(centre(*qp[nm]) - centre(*sc['poses'][nm])) < 0.05
