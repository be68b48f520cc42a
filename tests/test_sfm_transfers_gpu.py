"""One upload and one read back per SfM stage: every stage of geoformer_amd.sfm goes through sfm._upload and sfm._download exactly once per
call, counted here on the smallest planted cases of the case modules.  What the stages compute is checked, bit for bit, by their own tests."""
import numpy as np
import pytest

import abspose_cases as AC
import camera_cases as CAM
import triangulate_cases as TC

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture()
def counts(monkeypatch):
    from geoformer_amd import sfm
    n = {'up': 0, 'down': 0}

    def counting(name, key):
        real = getattr(sfm, name)

        def wrapped(*a, **k):
            n[key] += 1
            return real(*a, **k)
        monkeypatch.setattr(sfm, name, wrapped)
    counting('_upload', 'up'), counting('_download', 'down')

    def taken():
        got = (n['up'], n['down'])
        n['up'] = n['down'] = 0
        return got
    return taken


@pytest.fixture(scope='module')
def scene():
    """matcher_scene with 40 points: 27 pairs of 28 rows; consolidated and triangulated once"""
    from geoformer_amd import sfm
    sc = TC.matcher_scene(n_points=40)
    cm = sfm.consolidate_matches(sc['pairs'], sc['results'], qt_psize=0, device=DEV)
    db_pair = np.flatnonzero([a not in sc['queries'] and b not in sc['queries'] for a, b in sc['pairs']])
    cm_db = cm._replace(pair_images=cm.pair_images[db_pair], matches=[cm.matches[p] for p in db_pair])
    tt = sfm.triangulate(cm_db, sc['intrinsics'], sc['db_poses'], device=DEV)
    assert len(tt.points) > 20
    return sc, cm, cm_db, tt


@pytest.fixture(scope='module')
def three(scene):
    """three pairs of the scene, the middle one without rows"""
    sc = scene[0]
    none = (np.zeros((0, 4), np.float32), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), np.zeros(0, np.float32))
    return sc['pairs'][:3], [sc['results'][0], none, sc['results'][2]], sc['intrinsics']


def test_the_pair_stages(three, counts):
    from geoformer_amd import sfm
    pairs, results, intr = three
    for refit in (0, 2):
        vm = sfm.verify_matches(pairs, results, thr=2.0, min_inliers=8, device=DEV, refit=refit)
        assert counts() == (1, 1) and list(vm.verified) == [True, False, True] and [len(m) for m in vm.masks] == [28, 0, 28]
        rp = sfm.relative_poses(pairs, results, intr, thr=2.0, min_inliers=8, device=DEV, refit=refit)
        assert counts() == (1, 1) and list(rp.verified) == [True, False, True] and [len(m) for m in rp.masks] == [28, 0, 28]
    und, _ = sfm.undistort_results(pairs, results, CAM.scene_cameras({'names': list(intr), 'intrinsics': intr}, -0.05), device=DEV)
    assert counts() == (1, 1) and [len(r[0]) for r in und] == [28, 0, 28] and [s.shape for s in und.status] == [(28, 2), (0, 2), (28, 2)]
    cm = sfm.consolidate_matches(pairs, results, device=DEV, keep=vm.masks)
    assert counts() == (1, 1) and len(cm.matches) == 3


def test_localize_queries(counts):
    """two queries, three pairs against the two maps of abspose_cases (one map twice): the maps are uploaded one by one, as documented, the
    rows of all pairs in one block"""
    from geoformer_amd import sfm
    maps = dict(zip(('db/a', 'db/b'), AC.lookup_maps()))
    rng = np.random.default_rng(3)
    pairs, results = [('q0', 'db/a'), ('q1', 'db/b'), ('q0', 'db/b')], []
    for _, d in pairs:
        db = AC.lookup_points(*maps[d].shape[:2], seed=len(results))
        m = np.c_[rng.uniform(0, 640, (len(db), 2)), db].astype(np.float32)
        results.append((m, m[:, :2], m[:, 2:], np.full(len(m), 0.9, np.float32)))
    lq = sfm.localize_queries(pairs, results, {'q0': AC.K, 'q1': AC.K}, maps, device=DEV, refit=2)
    assert counts() == (1, 1) and lq.names == ['q0', 'q1'] and [len(m) for m in lq.masks] == [len(r[0]) for r in results]


def test_triangulate(scene, counts):
    from geoformer_amd import sfm
    sc, cm, cm_db, tt = scene
    counts()
    again = sfm.triangulate(cm_db, sc['intrinsics'], sc['db_poses'], device=DEV)
    assert counts() == (1, 1) and again.points.tobytes() == tt.points.tobytes()
    # T == 0: rows that join a keypoint to itself make no track of two keypoints - the upload, the track kernels, nothing to read back
    loops = sfm.ConsolidatedMatches(cm_db.names[:2], [k[:2] for k in cm_db.keypoints[:2]], np.array([[0, 0]], np.int32),
                                    [np.array([[0, 0], [1, 1]], np.int32)])
    none = sfm.triangulate(loops, sc['intrinsics'], sc['db_poses'], device=DEV)
    assert counts() == (1, 0) and none.n_tracks == 0 and len(none.points) == 0


@pytest.mark.parametrize('solver', ['dense', 'pcg'])
def test_refine_with_a_schedule(scene, counts, solver):
    from geoformer_amd import sfm
    sc, cm, cm_db, tt = scene
    db = [sc['names'][i] for i in TC.DB]
    counts()
    rs = sfm.refine(cm_db, tt, sc['intrinsics'], sc['db_poses'], fixed=[db[0], db[-1]], iters=3, thr=(8.0, 4.0), device=DEV, solver=solver)
    assert counts() == (1, 1) and rs.n_free == 4 and rs.cost.shape == (8,) and (rs.cg_used is not None) == (solver == 'pcg')


def test_localize_queries_sparse(scene, counts):
    from geoformer_amd import sfm
    sc, cm, cm_db, tt = scene
    counts()
    lq = sfm.localize_queries_sparse(cm, tt, sc['queries'], sc['intrinsics'], refit=2, device=DEV)
    assert counts() == (1, 1) and lq.localized.all() and lq.n_clusters is None
    lq = sfm.localize_queries_sparse(cm, tt, sc['queries'], sc['intrinsics'], refit=2, device=DEV, covis_cluster=True, dedup=True)
    assert counts() == (1, 1) and lq.localized.all() and lq.n_clusters.tolist() == [1, 1]
    # M == 0: the database images have observations, but no matched keypoint has a point - no RANSAC, the clusters alone are read back
    bare = tt._replace(point_of_keypoint=[np.full_like(p, -1) for p in tt.point_of_keypoint])
    lq = sfm.localize_queries_sparse(cm, bare, sc['queries'], sc['intrinsics'], device=DEV, covis_cluster=True, dedup=True)
    assert counts() == (1, 1) and not lq.localized.any() and all(not c.any() for c in lq.cluster_inliers) and not lq.R.any()
