"""The covisibility rule on the CPU: the serial host build (csrc/host/covis_host.cpp over csrc/covis_spec.h, the text the kernels compile)
against a restatement of steps 1 - 5 in plain Python (tests/covis_cases.py: sets and a breadth-first search), the pair-level bookkeeping
of matcher._covis_tables against the host build, and the command line of the last link.  No GPU."""
import numpy as np
import pytest

import covis_cases as CC

CASES = CC.rule_cases()


def run_host(c, cluster, dedup):
    rc, tb = CC.host_lists(c)
    assert rc == 0
    st, cl, ncl = CC.host_cluster(c, tb, enable=cluster)
    assert st == 0
    st, rows = CC.host_rows(c, tb, cl, ncl, dedup=dedup)
    assert st == 0
    return dict(tb, cluster=cl, n_clusters=ncl, **rows)


@pytest.mark.parametrize('name', sorted(CASES))
@pytest.mark.parametrize('cluster,dedup', [(True, False), (True, True), (False, True), (False, False)])
def test_host_build_equals_the_python_rule(name, cluster, dedup):
    c = CASES[name]
    got, ref = run_host(c, cluster, dedup), CC.python_rule(c, cluster, dedup)
    for k in CC.TABLE_KEYS + ('cluster', 'n_clusters', 'prob_base') + CC.ROW_KEYS:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k


def clusters_of(name, cluster=True):
    got = run_host(CASES[name], cluster, False)
    return got['list_img'].tolist(), got['cluster'].tolist(), got['n_clusters'].tolist()


def test_the_named_cases_cluster_as_stated():
    assert clusters_of('no_pairs') == ([], [], [0])
    assert clusters_of('one_database_image') == ([1], [0], [1])
    assert clusters_of('two_images_no_shared_point') == ([1, 2], [0, 1], [2])
    assert clusters_of('bridge_outside_the_list') == ([1, 3], [0, 1], [2])              # a path through an image outside the list links nothing
    assert clusters_of('bridge_inside_the_list') == ([1, 3, 2], [0, 0, 0], [1])
    assert clusters_of('star') == (list(range(1, 8)), [0] * 7, [1])
    assert clusters_of('image_without_points') == ([1, 2], [0, 0], [1])                 # image 3 has no point: not listed
    assert clusters_of('query_on_the_second_side') == ([0, 1, 2], [0, 0, 0], [1])
    assert clusters_of('pair_listed_twice') == ([1, 2], [0, 0], [1])
    assert clusters_of('two_images_no_shared_point', cluster=False) == ([1, 2], [0, 0], [1])
    img, cl, n = clusters_of('chain_1024')
    assert img == list(range(1024, 0, -1)) and cl == [0] * 1024 and n == [1]


def test_a_pair_listed_twice_contributes_twice():
    got = run_host(CASES['pair_listed_twice'], True, False)
    assert got['pairs'][:, 2].tolist() == [1, 2, 1] and got['pairs'][:, 6].tolist() == [0, 1, 0] and len(got['keep']) == 13


def test_dedup_drops_exactly_the_repeated_rows():
    """repeated_rows: the query's rows are (keypoint, point) = (2,0) (2,1) (2,0) (3,-) | (2,0) (2,-) (1,-): one problem."""
    c = CASES['repeated_rows']
    plain, uniq = run_host(c, True, False), run_host(c, True, True)
    assert plain['keep'].tolist() == [1, 1, 1, 0, 1, 0, 0]
    assert plain['first_of'].tolist() == [0, 1, 2, -1, 4, -1, -1] and plain['sel'].tolist() == [0, 1, 2, 4]
    assert uniq['first_of'].tolist() == [0, 1, 0, -1, 0, -1, -1] and uniq['sel'].tolist() == [0, 1]
    assert uniq['slot'].tolist() == [0, 1, 0, -1, 0, -1, -1]
    for name in sorted(CASES):                                           # everywhere: the kept rows are the distinct (problem, keypoint, point)
        u = run_host(CASES[name], True, True)
        k = u['keep'].astype(bool)
        triples = np.stack([u['row_prob'], u['row_kp'], u['row_pt']], 1)[k]
        assert len(u['sel']) == len({tuple(x) for x in triples.tolist()})
        first = u['first_of'][k]
        assert np.all(first <= np.flatnonzero(k)) and np.array_equal(np.stack([u['row_prob'], u['row_kp'], u['row_pt']], 1)[first], triples)


def test_a_list_of_1025_is_an_error():
    c = CC.chain_case(1025)
    rc, _ = CC.host_lists(c)
    assert rc == -2 and CC.python_rule(c) is None
    # and the cluster entry refuses such a list whoever built it
    ok = CC.chain_case(1024)
    _, tb = CC.host_lists(ok)
    tb = dict(tb, list_off=np.array([0, 1025], np.int32), list_img=np.r_[tb['list_img'], 1].astype(np.int32),
              sorted_img=np.r_[tb['sorted_img'], 1].astype(np.int32), sorted_pos=np.r_[tb['sorted_pos'], 0].astype(np.int32))
    assert CC.host_cluster(ok, tb)[0] == -2


def test_select_rule_on_the_host():
    """Step 8 and 9: most inliers among the valid problems, then the lowest cluster; masks only on the winner's rows, through slot."""
    prob_base = np.array([0, 3, 3, 5], np.int32)                         # three queries: 3, 0 and 2 problems
    rs = {'valid': np.array([1, 0, 1, 1, 1], np.int32), 'n_inliers': np.array([7, 99, 7, 20, 20], np.int32),
          'R': np.arange(45, dtype=np.float64).reshape(5, 3, 3), 't': np.arange(15, dtype=np.float64).reshape(5, 3),
          'rounds': np.array([1, 2, 3, 4, 5], np.int32), 'inliers': np.array([1, 0, 1, 1, 1, 0], np.uint8)}
    row_prob = np.array([0, 0, 2, 2, 3, 4, 4, -1], np.int32)
    slot = np.array([0, 0, 2, 3, 4, 5, -1, -1], np.int32)
    s = CC.host_select(prob_base, rs, row_prob, slot, min_inliers=10)
    assert s['winner'].tolist() == [0, -1, 0] and s['localized'].tolist() == [0, 0, 1] and s['n_inliers'].tolist() == [7, 0, 20]
    assert s['rounds'].tolist() == [1, 0, 4] and np.array_equal(s['R'][0], rs['R'][0]) and np.array_equal(s['R'][2], rs['R'][3])
    assert not s['R'][1].any() and np.array_equal(s['t'][2], rs['t'][3])
    assert s['mask'].tolist() == [1, 1, 0, 0, 1, 0, 0, 0]


# --------------------------------------------------------------------------------------------- matcher bookkeeping and the command line
def as_matcher_inputs(c):
    from geoformer_amd import matcher
    names = [f'im{i}' for i in range(c['n_images'])]
    kps = [np.zeros((c['kp_off'][i + 1] - c['kp_off'][i], 2), np.float32) for i in range(c['n_images'])]
    cm = matcher.ConsolidatedMatches(names, kps, c['pair_images'], [c['ids'][c['id_off'][p]:c['id_off'][p + 1]] for p in range(len(c['pair_images']))])
    tt = matcher.TriangulatedTracks(np.zeros((c['T'], 3)), np.zeros(c['T']), c['obs_offsets'], c['obs_image'], np.zeros(len(c['obs_image']), np.int32),
                                    [c['pok'][c['kp_off'][i]:c['kp_off'][i + 1]] for i in range(c['n_images'])], c['T'], 0, 0)
    queries = [names[i] for i in np.argsort(np.where(c['image_q'] >= 0, c['image_q'], 1 << 30))[:c['Q']]]
    return cm, tt, queries


@pytest.mark.parametrize('name', sorted(CASES))
def test_matcher_tables_equal_the_host_build(name):
    from geoformer_amd import matcher
    c = CASES[name]
    tb = matcher._covis_tables(*as_matcher_inputs(c))
    _, ref = CC.host_lists(c)
    for k in CC.TABLE_KEYS:
        assert tb[k].dtype == np.int32 and np.array_equal(tb[k], ref[k]), k


def test_matcher_refuses_a_list_of_1025():
    from geoformer_amd import matcher
    with pytest.raises(ValueError, match='1025 database images'):
        matcher._covis_tables(*as_matcher_inputs(CC.chain_case(1025)))


def test_cli_localize_sparse_parses():
    from geoformer_amd import matcher
    a = matcher.build_parser().parse_args(['localize-sparse', 'kp', '--points', 'p.npz', '--queries', 'q.txt', '--intrinsics', 'k.txt'])
    assert (a.cmd, a.keypoints, a.points, a.queries, a.intrinsics) == ('localize-sparse', 'kp', 'p.npz', 'q.txt', 'k.txt')
    assert (a.covis_cluster, a.dedup, a.thr, a.min_inliers, a.refit, a.out) == (False, False, 12.0, 12, 0, None)
    a = matcher.build_parser().parse_args(['localize-sparse', 'kp', '--points', 'p.npz', '--queries', 'q.txt', '--intrinsics', 'k.txt', '--covis-cluster',
                                           '--dedup', '--thr', '8', '--min-inliers', '20', '--refit', '--out', 'poses.txt'])
    assert (a.covis_cluster, a.dedup, a.thr, a.min_inliers, a.refit, a.out) == (True, True, 8.0, 20, 4, 'poses.txt')
    with pytest.raises(SystemExit):
        matcher.build_parser().parse_args(['localize-sparse', 'kp', '--queries', 'q.txt', '--intrinsics', 'k.txt'])


def test_cli_read_triangulated_round_trips(tmp_path):
    from geoformer_amd import matcher
    _, tt, _ = as_matcher_inputs(CASES['random_03'])
    tt = tt._replace(points=np.random.default_rng(1).normal(size=(len(tt.points), 3)), n_conflict=4, n_rejected=2)
    path = str(tmp_path / 'points.npz')
    matcher.write_triangulated(path, tt)
    back = matcher.read_triangulated(path)
    for a, b in zip(tt[:5] + tuple(tt.point_of_keypoint), back[:5] + tuple(back.point_of_keypoint)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert len(back.point_of_keypoint) == len(tt.point_of_keypoint)
    assert (back.n_tracks, back.n_conflict, back.n_rejected) == (tt.n_tracks, 4, 2)


def test_cli_old_format_reads_with_unknown_counts(tmp_path):
    from geoformer_amd import matcher
    _, tt, _ = as_matcher_inputs(CASES['star'])
    path = str(tmp_path / 'old.npz')
    np.savez(path, points=tt.points, errors=tt.errors, obs_offsets=tt.obs_offsets, obs_image=tt.obs_image, obs_keypoint=tt.obs_keypoint,
             point_of_keypoint=np.concatenate(tt.point_of_keypoint),
             kp_offsets=np.concatenate([[0], np.cumsum([len(p) for p in tt.point_of_keypoint])]).astype(np.int32))
    back = matcher.read_triangulated(path)
    assert (back.n_tracks, back.n_conflict, back.n_rejected) == (-1, -1, -1)
    assert np.array_equal(back.obs_image, tt.obs_image) and len(back.point_of_keypoint) == len(tt.point_of_keypoint)
