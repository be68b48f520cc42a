"""matcher.localize_queries_sparse with covisibility clustering and unique rows, on the GPU: the flags off, dedup on matcher_scene, two
places that look alike (tests/covis_cases.py: two_place_scene) and a query with a single cluster.  The model is not run."""
import numpy as np
import pytest
import torch

import covis_cases as CC
import triangulate_cases as TC

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CENTRE_FACTOR = 2.262        # see test_two_places_the_right_cluster_wins


@pytest.fixture(scope='module')
def chain():
    from geoformer_amd import matcher
    sc = TC.matcher_scene()
    cm = matcher.consolidate_matches(sc['pairs'], sc['results'], qt_psize=0, device=DEV)
    tt = matcher.triangulate(cm, sc['intrinsics'], sc['db_poses'], device=DEV)
    return sc, cm, tt


@pytest.fixture(scope='module')
def places():
    from geoformer_amd import matcher
    sc = CC.two_place_scene()
    cm = matcher.consolidate_matches(sc['pairs'], sc['results'], qt_psize=0, device=DEV)
    tt = matcher.triangulate(CC.database_only(cm, sc), sc['intrinsics'], sc['db_poses'], device=DEV)
    return sc, cm, tt


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_flags_off_is_todays_path(chain):
    """(a) both flags off: _sparse_rows and ops.ransac_absolute_pose over the queries, as before; the new fields are not filled."""
    from geoformer_amd import matcher, ops
    sc, cm, tt = chain
    lq = matcher.localize_queries_sparse(cm, tt, sc['queries'], sc['intrinsics'], refit=2, device=DEV)
    p2d, p3d, query_off, pair_off, used, owner = matcher._sparse_rows(cm, tt, sc['queries'])
    Ks = torch.tensor(np.stack([sc['intrinsics'][q].astype(np.float32).reshape(9) for q in sc['queries']]), device=DEV)
    rs = ops.ransac_absolute_pose(torch.from_numpy(p2d).to(DEV), torch.from_numpy(p3d).to(DEV), None, torch.from_numpy(query_off).to(DEV), 2, Ks,
                                  pixel_thr=12.0, refit=2)
    assert same(lq.R, rs['R'].cpu().numpy()) and same(lq.t, rs['t'].cpu().numpy()) and same(lq.n_inliers, rs['n_inliers'].cpu().numpy())
    assert same(lq.rounds, rs['rounds'].cpu().numpy()) and lq.localized.all()
    inl = rs['inliers'].cpu().numpy().astype(bool)
    for pos, p in enumerate(used):
        assert np.array_equal(lq.masks[p], inl[pair_off[pos]:pair_off[pos + 1]])
    assert lq.n_clusters is None and lq.cluster is None and lq.db_names is None and lq.db_cluster is None and lq.cluster_inliers is None


def test_dedup_counts_every_keypoint_point_pair_once(chain):
    """(b) the rows of a query are its distinct (keypoint, point) pairs; the masks on the original rows follow rule 9."""
    from geoformer_amd import matcher
    sc, cm, tt = chain
    lq = matcher.localize_queries_sparse(cm, tt, sc['queries'], sc['intrinsics'], refit=2, device=DEV, dedup=True)
    plain = matcher.localize_queries_sparse(cm, tt, sc['queries'], sc['intrinsics'], refit=2, device=DEV)
    assert lq.localized.all() and lq.n_clusters.tolist() == [1, 1] and lq.cluster.tolist() == [0, 0]
    tb = matcher._covis_tables(cm, tt, sc['queries'])
    with torch.cuda.device(DEV):
        n_rows = np.diff(matcher._device_rows(cm, tt, sc['queries'], sc['intrinsics'], tb, DEV, False, True)[3]['prob_off'].cpu().numpy())
    for q, name in enumerate(lq.names):
        qi = cm.names.index(name)
        seen, first, rows = {}, [], []
        for p in range(len(cm.matches)):                                # pair order, then row order
            i, j = cm.pair_images[p]
            if qi not in (i, j):
                continue
            col = 0 if i == qi else 1
            other = j if i == qi else i
            pt = tt.point_of_keypoint[other][cm.matches[p][:, 1 - col]]
            for r, (kq, x) in enumerate(zip(cm.matches[p][:, col], pt)):
                if x >= 0:
                    first.append(seen.setdefault((int(kq), int(x)), (p, r)))
                    rows.append((p, r))
                else:
                    assert not lq.masks[p][r]                            # a row without a point is nobody's inlier
        distinct = len(seen)
        assert n_rows[q] == distinct                                     # the rows RANSAC sees: every (keypoint, point) once
        assert len(rows) > 3 * distinct > 0                              # the scene repeats every correspondence about four times
        assert lq.cluster_inliers[q].tolist() == [lq.n_inliers[q]] and lq.n_inliers[q] <= distinct < plain.n_inliers[q]
        assert lq.n_inliers[q] >= 0.9 * distinct
        # rule 9: a repeated row carries the byte of its first occurrence, and the heads carry n_inliers bytes in all
        assert all(lq.masks[p][r] == lq.masks[fp][fr] for (p, r), (fp, fr) in zip(rows, first))
        assert sum(bool(lq.masks[p][r]) for (p, r) in set(first)) == lq.n_inliers[q]


def test_two_places_the_right_cluster_wins(places):
    """(c) The first query sees place A (6 database images, 70 % of the points per pair) and place B (3 images at a rigid copy of A's
    structure 100 units away, 50 % per pair).  Measured with the host chain (thr 12 px, 512 hypotheses, refit 2, no dedup): A's problem has
    1258 inliers of 1258 rows, B's 412 of 412 - a factor of 3.05, the winner does not rest on noise.  The camera-centre error of the
    clustered result is 0.00269 units against 0.00238 for estimate_absolute_pose on the PLANTED points of A's rows (same draws: sample =
    A's problem), a factor of 1.131; the gate is twice that factor (the rule of CENTRE_FACTOR in test_triangulate_matcher_gpu)."""
    from geoformer_amd import matcher
    sc, cm, tt = places
    q0 = sc['queries'][0]
    lq = matcher.localize_queries_sparse(cm, tt, [q0], sc['intrinsics'], refit=2, device=DEV, covis_cluster=True)
    pooled = matcher.localize_queries_sparse(cm, tt, [q0], sc['intrinsics'], refit=2, device=DEV, dedup=True)
    assert pooled.n_clusters.tolist() == [1] and len(pooled.db_names[0]) == 9                   # pooled: one problem over both places
    assert lq.n_clusters.tolist() == [2] and lq.localized.all()
    place = [sc['place'][nm] for nm in lq.db_names[0]]
    assert sorted(place) == ['A'] * 6 + ['B'] * 3 and lq.db_cluster[0].dtype == np.int32
    assert len({(pl, int(c)) for pl, c in zip(place, lq.db_cluster[0])}) == 2                   # the clusters separate A's images from B's
    a_cluster = int(lq.db_cluster[0][place.index('A')])
    assert lq.cluster.tolist() == [a_cluster]
    cin = lq.cluster_inliers[0]
    print(f'cluster inliers: A {cin[a_cluster]}, B {cin[1 - a_cluster]}')
    assert cin.dtype == np.int32 and cin.shape == (2,) and cin[a_cluster] == lq.n_inliers[0] and cin[a_cluster] >= 2 * cin[1 - a_cluster] > 0
    qi = cm.names.index(q0)
    a_rows = []
    for p, (i, j) in enumerate(cm.pair_images):
        if qi in (i, j) and sc['place'][cm.names[j if i == qi else i]] == 'B':
            assert len(lq.masks[p]) > 0 and not lq.masks[p].any()                               # every mask of a B pair is all False
        elif qi in (i, j):
            col = 0 if i == qi else 1
            has = tt.point_of_keypoint[j if i == qi else i][cm.matches[p][:, 1 - col]] >= 0
            a_rows.append(cm.matches[p][has, col])
    assert sum(int(m.sum()) for m in lq.masks) == lq.n_inliers[0]
    kp = np.concatenate(a_rows)                                                                  # A's rows in problem order
    table = {p.tobytes(): k for k, p in enumerate(sc['uv'][sc['names'].index(q0)])}
    planted = sc['X'][[table[p.tobytes()] for p in cm.keypoints[qi][kp]]]
    ref = matcher.estimate_absolute_pose(cm.keypoints[qi][kp], planted, sc['intrinsics'][q0], thr=12.0, refit=2, device=DEV, sample=a_cluster)
    c_true = TC.centre_of(*sc['poses'][q0])
    e_ref = np.linalg.norm(TC.centre_of(ref[0], ref[1]) - c_true)
    e_tri = np.linalg.norm(TC.centre_of(lq.R[0], lq.t[0]) - c_true)
    print(f'{q0}: centre error {e_tri:.5f} clustered, {e_ref:.5f} with the planted points, factor {e_tri / e_ref:.3f}')
    assert e_tri <= CENTRE_FACTOR * e_ref, (e_tri, e_ref)


def test_device_path_equals_the_host_chain(places):
    """every output of the device path against the serial host builds of the rule and of the absolute-pose RANSAC, byte for byte"""
    from geoformer_amd import matcher
    sc, cm, tt = places
    for cluster, dedup in ((True, False), (True, True), (False, True)):
        lq = matcher.localize_queries_sparse(cm, tt, sc['queries'], sc['intrinsics'], refit=2, device=DEV, covis_cluster=cluster, dedup=dedup)
        h = CC.host_localize(cm, tt, sc['queries'], sc['intrinsics'], cluster=cluster, dedup=dedup, refit=2)
        s, tb = h['sel'], h['tables']
        assert same(lq.R, s['R']) and same(lq.t, s['t']) and same(lq.n_inliers, s['n_inliers']) and same(lq.rounds, s['rounds'])
        assert same(lq.cluster, s['winner']) and same(lq.localized, s['localized'].astype(bool)) and same(lq.n_clusters, h['n_clusters'])
        assert same(np.concatenate(lq.db_cluster), h['cluster'])
        assert same(np.concatenate(lq.cluster_inliers), np.where(h['rs']['valid'] == 1, h['rs']['n_inliers'], 0).astype(np.int32))
        for c, p in enumerate(tb['used']):
            assert np.array_equal(lq.masks[p], s['mask'][tb['pair_row_off'][c]:tb['pair_row_off'][c + 1]].astype(bool))


def test_single_cluster_keeps_the_bits(places):
    """(d) the second query's database images all lie in A: with clustering on (dedup off) its pose has the bits of clustering off.  It is the
    only query of the call, so its problem index is its query index."""
    from geoformer_amd import matcher
    sc, cm, tt = places
    q1 = sc['queries'][1]
    on = matcher.localize_queries_sparse(cm, tt, [q1], sc['intrinsics'], refit=2, device=DEV, covis_cluster=True)
    off = matcher.localize_queries_sparse(cm, tt, [q1], sc['intrinsics'], refit=2, device=DEV)
    assert on.n_clusters.tolist() == [1] and on.cluster.tolist() == [0] and len(on.db_names[0]) == 6 and on.db_cluster[0].tolist() == [0] * 6
    assert on.localized.all() and same(on.R, off.R) and same(on.t, off.t) and same(on.n_inliers, off.n_inliers) and same(on.rounds, off.rounds)
    assert all(np.array_equal(a, b) for a, b in zip(on.masks, off.masks))


def test_cli_localize_sparse_runs_from_the_files_of_the_chain(places, tmp_path, capsys):
    """`localize-sparse` on what `pairs --keypoints` and `triangulate --out` write gives the poses of the direct call, in the pose-line
    format read_poses reads; names in the queries and intrinsics files resolve as written."""
    from geoformer_amd import matcher
    sc, cm, tt = places
    kdir, pts, qfile, kfile, out = (str(tmp_path / n) for n in ('kp', 'points.npz', 'queries.txt', 'intrinsics.txt', 'poses.txt'))
    matcher.write_consolidated(kdir, cm)
    matcher.write_triangulated(pts, tt)
    with open(qfile, 'w') as f:
        f.write('# the queries\n' + '\n'.join(sc['queries']) + '\n')
    with open(kfile, 'w') as f:
        for q in sc['queries']:
            K = sc['intrinsics'][q]
            f.write(' '.join([q] + [repr(float(v)) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2])]) + '\n')
    matcher.main(['localize-sparse', kdir, '--points', pts, '--queries', qfile, '--intrinsics', kfile, '--covis-cluster', '--dedup', '--refit', '2',
                  '--out', out, '--device', DEV])
    said = capsys.readouterr().out
    assert '2 of 2 queries localised' in said and '1 queries with more than one cluster' in said
    lq = matcher.localize_queries_sparse(cm, tt, sc['queries'], sc['intrinsics'], refit=2, device=DEV, covis_cluster=True, dedup=True)
    poses = matcher.read_poses(out)
    assert list(poses) == sc['queries']
    for q, name in enumerate(sc['queries']):
        R, t = poses[name]
        assert np.array_equal(t, lq.t[q]) and np.abs(R - lq.R[q]).max() < 1e-12       # (R goes through a quaternion and back)


def test_pairs_without_rows_still_cluster_by_the_points():
    """rules 2 and 3 do not look at the match rows: a query whose two pairs are empty, over two images that share no point, has two
    clusters, no winner and no pose"""
    from geoformer_amd import matcher
    c = CC.make_case(5, [0], [(1, 3), (2, 4)], [(0, 1, 0), (0, 2, 0)])
    names = [f'im{i}' for i in range(5)]
    kps = [np.zeros((c['kp_off'][i + 1] - c['kp_off'][i], 2), np.float32) for i in range(5)]
    cm = matcher.ConsolidatedMatches(names, kps, c['pair_images'], [np.zeros((0, 2), np.int32)] * 2)
    tt = matcher.TriangulatedTracks(np.zeros((2, 3)), np.zeros(2), c['obs_offsets'], c['obs_image'], np.zeros(4, np.int32),
                                    [c['pok'][c['kp_off'][i]:c['kp_off'][i + 1]] for i in range(5)], 2, 0, 0)
    for cluster, want in ((True, [2]), (False, [1])):
        lq = matcher.localize_queries_sparse(cm, tt, ['im0'], {'im0': np.eye(3)}, device=DEV, covis_cluster=cluster, dedup=True)
        assert lq.n_clusters.tolist() == want and lq.cluster.tolist() == [-1] and not lq.localized.any() and lq.db_names == [['im1', 'im2']]
        assert lq.db_cluster[0].tolist() == ([0, 1] if cluster else [0, 0]) and lq.cluster_inliers[0].tolist() == [0] * want[0]
        assert not lq.R.any() and [len(m) for m in lq.masks] == [0, 0]
