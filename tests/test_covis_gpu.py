"""The covisibility kernels against the serial host build (csrc/host/covis_host.cpp, the same csrc/covis_spec.h): ops.covis_clusters,
ops.sparse_rows and ops.select_cluster byte for byte on every case of tests/covis_cases.py, run to run, and against matcher._sparse_rows."""
import numpy as np
import pytest
import torch

import covis_cases as CC
import triangulate_cases as TC

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CASES = CC.rule_cases()
MODES = [(True, False), (True, True), (False, True), (False, False)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_rule(c, tb, cluster, dedup):
    """the three ops on a case -> numpy dict with the keys of the host run (the RANSAC outputs of the selection are made up, seeded)"""
    from geoformer_amd import ops
    d = {k: dev(c[k]) for k in ('kp_off', 'pok', 'obs_offsets', 'obs_image', 'ids')}
    t = {k: dev(tb[k]) for k in CC.TABLE_KEYS}
    cl, ncl, status = ops.covis_clusters(d['kp_off'], d['pok'], d['obs_offsets'], d['obs_image'], t['list_off'], t['list_img'], t['sorted_img'],
                                         t['sorted_pos'], tb, enable=cluster)
    rows = ops.sparse_rows(t['pairs'], t['pair_row_off'], d['ids'], d['kp_off'], d['pok'], c['T'], t['list_off'], cl, ncl, tb, dedup=dedup, status=status)
    rs = fake_ransac(rows['N'], rows['M'])
    sel = ops.select_cluster(rows['prob_base'], {k: dev(v) for k, v in rs.items()}, rows['row_prob'], rows['slot'], min_inliers=12)
    out = {'cluster': cl, 'n_clusters': ncl, **{k: rows[k] for k in CC.ROW_KEYS + ('prob_base',)}, **{'sel_' + k: sel[k] for k in CC.SELECT_KEYS}}
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out['sel'] = out['sel'].astype(np.int32)
    return out, rs, rows['N'], rows['M']


def fake_ransac(N, M):
    rng = np.random.default_rng(N * 7919 + M)
    return {'valid': (rng.random(N) < 0.8).astype(np.int32), 'n_inliers': rng.integers(0, 30, N).astype(np.int32), 'R': rng.normal(size=(N, 3, 3)),
            't': rng.normal(size=(N, 3)), 'rounds': rng.integers(0, 3, N).astype(np.int32), 'inliers': (rng.random(M) < 0.5).astype(np.uint8)}


def host_rule(c, tb, cluster, dedup, rs):
    st, cl, ncl = CC.host_cluster(c, tb, enable=cluster)
    assert st == 0
    st, rows = CC.host_rows(c, tb, cl, ncl, dedup=dedup)
    assert st == 0
    sel = CC.host_select(rows['prob_base'], rs, rows['row_prob'], rows['slot'], 12)
    return {'cluster': cl, 'n_clusters': ncl, **{k: rows[k] for k in CC.ROW_KEYS + ('prob_base',)}, **{'sel_' + k: sel[k] for k in CC.SELECT_KEYS}}


@pytest.mark.parametrize('name', sorted(CASES))
def test_ops_equal_the_host_build_and_repeat(name):
    c = CASES[name]
    rc, tb = CC.host_lists(c)
    assert rc == 0
    for cluster, dedup in MODES:
        got, rs, N, M = device_rule(c, tb, cluster, dedup)
        ref = host_rule(c, tb, cluster, dedup, rs)
        assert set(got) == set(ref)
        for k in ref:
            assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape and got[k].tobytes() == ref[k].tobytes(), (k, cluster, dedup)
        again = device_rule(c, tb, cluster, dedup)[0]
        assert all(again[k].tobytes() == got[k].tobytes() for k in got), (cluster, dedup)


def test_entry_points_refuse_bad_tables_before_the_device():
    from geoformer_amd import ops, _lib
    c = CC.chain_case(1024)
    _, tb = CC.host_lists(c)
    d = {k: dev(c[k]) for k in ('kp_off', 'pok', 'obs_offsets', 'obs_image', 'ids')}
    long = dict(tb, list_off=np.array([0, 1025], np.int32), list_img=np.r_[tb['list_img'], 1].astype(np.int32),
                sorted_img=np.r_[tb['sorted_img'], 1].astype(np.int32), sorted_pos=np.r_[tb['sorted_pos'], 0].astype(np.int32))
    t = {k: dev(long[k]) for k in CC.TABLE_KEYS}
    with pytest.raises(_lib.GeoFormerHipError, match='more than 1024'):
        ops.covis_clusters(d['kp_off'], d['pok'], d['obs_offsets'], d['obs_image'], t['list_off'], t['list_img'], t['sorted_img'], t['sorted_pos'], long)
    bad = dict(tb, list_img=np.where(np.arange(1024) == 5, 5000, tb['list_img']).astype(np.int32))
    t = {k: dev(bad[k]) for k in CC.TABLE_KEYS}
    with pytest.raises(_lib.GeoFormerHipError, match='outside'):
        ops.covis_clusters(d['kp_off'], d['pok'], d['obs_offsets'], d['obs_image'], t['list_off'], t['list_img'], t['sorted_img'], t['sorted_pos'], bad)
    t = {k: dev(tb[k]) for k in CC.TABLE_KEYS}
    cl, ncl, status = ops.covis_clusters(d['kp_off'], d['pok'], d['obs_offsets'], d['obs_image'], t['list_off'], t['list_img'], t['sorted_img'],
                                         t['sorted_pos'], tb)
    pairs = tb['pairs'].copy()
    pairs[3, 4] = len(c['ids']) + 7                                       # a row range past ids
    with pytest.raises(_lib.GeoFormerHipError, match='outside ids'):
        ops.sparse_rows(dev(pairs), t['pair_row_off'], d['ids'], d['kp_off'], d['pok'], c['T'], t['list_off'], cl, ncl, dict(tb, pairs=pairs))
    # what only the device sees: a keypoint index its image does not have is skipped, flagged and raised after the one read
    ids = c['ids'].copy()
    ids[10, 1] = 9
    with pytest.raises(_lib.GeoFormerHipError, match='keypoint'):
        ops.sparse_rows(t['pairs'], t['pair_row_off'], dev(ids), d['kp_off'], d['pok'], c['T'], t['list_off'], cl, ncl, tb)


@pytest.fixture(scope='module')
def chain():
    from geoformer_amd import matcher
    sc = TC.matcher_scene()
    cm = matcher.consolidate_matches(sc['pairs'], sc['results'], qt_psize=0, device=DEV)
    tt = matcher.triangulate(cm, sc['intrinsics'], sc['db_poses'], device=DEV)
    return sc, cm, tt


@pytest.mark.parametrize('thinned', [False, True])
def test_device_rows_equal_sparse_rows_without_its_nan_rows(chain, thinned):
    """thinned: every third keypoint of an image loses its point (matcher_scene triangulates every track, so it has no NaN row of its own)"""
    from geoformer_amd import matcher, ops
    sc, cm, tt = chain
    if thinned:
        tt = tt._replace(point_of_keypoint=[np.where(np.arange(len(p)) % 3 == 1, -1, p).astype(np.int32) for p in tt.point_of_keypoint])
    names = sc['queries']
    p2d, p3d, query_off, pair_off, used, owner = matcher._sparse_rows(cm, tt, names)
    fin = np.isfinite(p3d).all(1)
    assert (0 < (~fin).sum() < len(fin)) if thinned else fin.all()
    tb = matcher._covis_tables(cm, tt, names)
    assert tb['used'] == sorted(used) and len(used) == 12
    kp_off = np.concatenate([[0], np.cumsum([len(k) for k in cm.keypoints])]).astype(np.int32)
    ids = np.concatenate(cm.matches).astype(np.int32)
    t = {k: dev(tb[k]) for k in CC.TABLE_KEYS}
    kpo, pok = dev(kp_off), dev(np.concatenate(tt.point_of_keypoint))
    cl, ncl, status = ops.covis_clusters(kpo, pok, dev(tt.obs_offsets), dev(tt.obs_image), t['list_off'], t['list_img'], t['sorted_img'],
                                         t['sorted_pos'], tb, enable=False)
    rows = ops.sparse_rows(t['pairs'], t['pair_row_off'], dev(ids), kpo, pok, len(tt.points), t['list_off'], cl, ncl, tb, dedup=False, status=status,
                           keypoints=dev(np.concatenate(cm.keypoints)), points=dev(tt.points.astype(np.float32)))
    assert rows['N'] == 2 and rows['M'] == int(fin.sum())
    assert rows['p2d'].cpu().numpy().tobytes() == p2d[fin].tobytes() and rows['p3d'].cpu().numpy().tobytes() == p3d[fin].tobytes()
    assert rows['prob_off'].cpu().numpy().tolist() == [0] + [int(fin[:query_off[q + 1]].sum()) for q in range(2)]
