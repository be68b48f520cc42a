"""Localisation on the GPU: gf_abspose_ransac and gf_xyz_lookup (csrc/k_abspose.hip behind ops.ransac_absolute_pose / ops.xyz_lookup)
against the host build of the same abs_solver.h (csrc/host/abspose_host.cpp), bit for bit.
Scenes, maps and points: tests/abspose_cases.py."""
import numpy as np
import pytest
import torch

import abspose_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SIZES = (0, 3, 4, 5, 63, 64, 65, 129, 300)  # empty, below the minimum, minimal, one more, the wave boundary on both sides, two waves and a tail, many
THR = 2.0


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def device(p2d, p3d, offsets, scores=None, thr=THR, sc_thres=0.25, iters=256, seed=C.SEED, refit=0):
    from geoformer_amd import ops
    N = len(offsets) - 1
    rs = ops.ransac_absolute_pose(_t(np.asarray(p2d, np.float32).reshape(-1, 2)), _t(np.asarray(p3d, np.float32).reshape(-1, 3)),
                                  None if scores is None else _t(scores), _t(offsets, torch.int32), N, _t(C.K9.reshape(3, 3)), pixel_thr=thr,
                                  sc_thres=sc_thres, iters=iters, seed=seed, refit=refit)
    assert rs['R'].dtype == torch.float64 and rs['inliers'].dtype == torch.uint8 and rs['R'].shape == (N, 3, 3) and rs['t'].shape == (N, 3)
    return {k: v.cpu().numpy() for k, v in rs.items()}


def assert_equals_host(dev, p2d, p3d, offsets, scores=None, n0=0, **kw):
    """every output of every problem, bit for bit; n0: the launch index of the first problem"""
    kw.setdefault('thr', THR)
    for n in range(len(offsets) - 1):
        a, b = offsets[n], offsets[n + 1]
        host = C.host_ransac(p2d[a:b], p3d[a:b], None if scores is None else scores[a:b], sample=n0 + n, **kw)
        assert host['status'] >= 0
        assert int(dev['valid'][n]) == host['valid'], n
        assert tuple(dev['hypothesis'][n]) == tuple(host['hyp']), n
        assert int(dev['n_inliers'][n]) == host['n_inliers'], n
        assert int(dev['rounds'][n]) == host['rounds'], n
        assert np.array_equal(dev['inliers'][a:b].astype(bool), host['inliers']), n
        assert np.array_equal(dev['R'][n].view(np.int64), host['R'].view(np.int64)), (n, np.abs(dev['R'][n] - host['R']).max())
        assert np.array_equal(dev['t'][n].view(np.int64), host['t'].view(np.int64)), (n, np.abs(dev['t'][n] - host['t']).max())


@pytest.fixture(scope='module')
def nine_problems():
    scenes = [C.scene(200 + i, n, 0.3 if n >= 63 else 0.0) for i, n in enumerate(SIZES)]
    p2d = np.concatenate([s['p2d'] for s in scenes])
    p3d = np.concatenate([s['p3d'] for s in scenes])
    offsets = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    return scenes, p2d, p3d, offsets


@pytest.mark.parametrize('iters', [C.HYP_PER_WG, 2 * C.HYP_PER_WG, 256])
def test_device_equals_host_build(nine_problems, iters):
    scenes, p2d, p3d, offsets = nine_problems
    dev = device(p2d, p3d, offsets, iters=iters)
    assert_equals_host(dev, p2d, p3d, offsets, iters=iters)
    assert list(dev['valid']) == [0, 0, 1, 1, 1, 1, 1, 1, 1]
    assert dev['n_inliers'][2] == 4 and not dev['inliers'][:3].any() and not dev['R'][:2].any() and not dev['t'][:2].any()
    assert not dev['rounds'].any()
    sc = scenes[8]
    assert C.rotation_error_deg(dev['R'][8], sc['R']) < 1e-3 and np.array_equal(dev['inliers'][offsets[8]:].astype(bool), ~sc['outlier'])


def test_device_equals_host_build_with_filtered_rows(nine_problems):
    """scores that filter rows in the middle of a wave, NaN / inf planted in 2-D and in 3-D coordinates, a problem whose rows are all
    filtered and one left with three survivors"""
    scenes, p2d, p3d, offsets = nine_problems
    p2d, p3d = p2d.copy(), p3d.copy()
    rng = np.random.default_rng(9)
    scores = rng.uniform(0.3, 1.0, len(p2d)).astype(np.float32)
    o = offsets
    scores[o[8] + np.array([3, 30, 31, 32, 33, 70, 100, 130, 131, 190, 299])] = 0.1      # the 300-row problem
    scores[o[8] + 150] = np.nan
    scores[o[7] + np.arange(20, 45)] = 0.2                                               # the 129-row problem
    scores[o[5]:o[6]] = 0.0                                                              # 64 rows, none survive
    scores[o[4] + 3:o[5]] = 0.24                                                         # 63 rows, three survive
    p2d[o[8] + 17, 0] = np.nan; p2d[o[8] + 66, 1] = np.inf; p3d[o[8] + 67, 2] = np.nan; p3d[o[7] + 64, 0] = -np.inf; p3d[o[6] + 1, 1] = np.nan
    dev = device(p2d, p3d, offsets, scores)
    assert_equals_host(dev, p2d, p3d, offsets, scores)
    keep = (scores >= 0.25) & np.isfinite(p2d).all(1) & np.isfinite(p3d).all(1)
    assert not dev['inliers'][~keep].any()
    assert list(dev['valid']) == [0, 0, 1, 1, 0, 0, 1, 1, 1]
    # the result is that of the list with the filtered rows removed
    a, b = o[8], o[9]
    host = C.host_ransac(p2d[a:b][keep[a:b]], p3d[a:b][keep[a:b]], None, sample=8)
    assert np.array_equal(dev['inliers'][a:b].astype(bool)[keep[a:b]], host['inliers'])
    assert np.array_equal(dev['R'][8].view(np.int64), host['R'].view(np.int64)) and np.array_equal(dev['t'][8].view(np.int64), host['t'].view(np.int64))


@pytest.fixture(scope='module')
def noisy_problems():
    scenes = [C.scene(s, 300, 0.3, noise=0.5) for s in (400, 402, 409)] + [C.scene(410, 5, 0.0)]
    p2d = np.concatenate([s['p2d'] for s in scenes])
    p3d = np.concatenate([s['p3d'] for s in scenes])
    return scenes, p2d, p3d, np.array([0, 300, 600, 900, 905], np.int32)


@pytest.mark.parametrize('refit', [1, 4, 8])
def test_refit_equals_host_build(noisy_problems, refit):
    scenes, p2d, p3d, offsets = noisy_problems
    dev = device(p2d, p3d, offsets, iters=128, refit=refit)
    assert_equals_host(dev, p2d, p3d, offsets, iters=128, refit=refit)
    plain = device(p2d, p3d, offsets, iters=128)
    assert (dev['rounds'][:3] >= 1).all() and (dev['rounds'] <= refit).all() and dev['rounds'][3] == 0
    assert (dev['n_inliers'] >= plain['n_inliers']).all() and np.array_equal(dev['hypothesis'], plain['hypothesis'])
    for k in ('R', 't'):
        assert np.array_equal(dev[k][3], plain[k][3])                    # five rows: never refitted, the P3P winner's bits
    for n in range(3):
        err = [np.linalg.norm(C.centre(r['R'][n], r['t'][n]) - C.centre(scenes[n]['R'], scenes[n]['t'])) for r in (plain, dev)]
        assert err[1] < err[0], (n, err)


@pytest.mark.parametrize('refit', [1, 4])
def test_refit_equals_host_build_with_filtered_rows(noisy_problems, refit):
    """the refit reads its first set from the mask and writes its last one back THROUGH the list of surviving rows: the first problem gets
    rows that take no part - low scores in the middle of waves and on both sides of row 255 / 256, a NaN score, a NaN pixel, an inf point -
    so that surviving row i is not row i.  The comparison is worth something only when a refit of that problem is accepted and moves rows in
    and out of the set: the host build alone says that it does (at 1 px; at the 2 px of the other tests the accepted refit keeps the set)."""
    scenes, p2d, p3d, offsets = noisy_problems
    p2d, p3d = p2d.copy(), p3d.copy()
    scores = np.random.default_rng(60).uniform(0.3, 1.0, len(p2d)).astype(np.float32)
    scores[[3, 30, 31, 100, 130, 200, 255, 256, 299]] = 0.1
    scores[150] = np.nan
    p2d[17, 0] = np.nan; p3d[70, 2] = np.inf
    keep = (scores >= 0.25) & np.isfinite(p2d).all(1) & np.isfinite(p3d).all(1)
    assert keep[:300].sum() == 300 - 12 and keep[300:].all()
    plain, host = (C.host_ransac(p2d[:300], p3d[:300], scores[:300], sample=0, iters=128, refit=r, thr=1.0) for r in (0, refit))
    changed = np.flatnonzero(plain['inliers'] != host['inliers'])
    assert host['rounds'] >= 1 and changed.min() < 255 and changed.max() > 256
    dev = device(p2d, p3d, offsets, scores, thr=1.0, iters=128, refit=refit)
    assert_equals_host(dev, p2d, p3d, offsets, scores, thr=1.0, iters=128, refit=refit)
    assert dev['rounds'][0] >= 1 and not dev['inliers'][~keep].any()
    assert (dev['n_inliers'] == [int(dev['inliers'][offsets[n]:offsets[n + 1]].sum()) for n in range(len(offsets) - 1)]).all()


def test_refit_of_problems_that_cannot_be_refitted_equals_host_build(nine_problems):
    """the refit stage launched over empty problems, problems below the minimum and a minimal one: rounds 0 and the P3P winner's bits where
    nothing is refitted, against the host build"""
    scenes, p2d, p3d, offsets = nine_problems
    dev = device(p2d, p3d, offsets, refit=4)
    assert_equals_host(dev, p2d, p3d, offsets, refit=4)
    assert not dev['rounds'][:3].any() and list(dev['valid'][:3]) == [0, 0, 1]


def test_refit_zero_is_the_plain_entry(noisy_problems):
    scenes, p2d, p3d, offsets = noisy_problems
    a, b = device(p2d, p3d, offsets, iters=128, refit=0), device(p2d, p3d, offsets, iters=128)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert not a['rounds'].any()
    assert_equals_host(a, p2d, p3d, offsets, iters=128, refit=0)


def test_two_calls_give_the_same_bits(nine_problems):
    scenes, p2d, p3d, offsets = nine_problems
    a, b = device(p2d, p3d, offsets, refit=4), device(p2d, p3d, offsets, refit=4)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert tuple(device(p2d, p3d, offsets, seed=1234)['hypothesis'][8]) != tuple(device(p2d, p3d, offsets)['hypothesis'][8])


def test_a_problem_depends_on_its_index_not_on_its_neighbours(nine_problems):
    """the draw is keyed by (seed, n, t): the 300-row problem at index 2 of two different launches gives the same bits"""
    scenes, p2d, p3d, offsets = nine_problems
    big = scenes[8]
    la = [scenes[6], scenes[7], big]
    lb = [scenes[2], big, scenes[4], scenes[6]]
    oa = np.array([0, 65, 194, 494], np.int32)
    ob = np.array([0, 4, 4, 304, 367, 432], np.int32)                 # index 1 is an empty problem
    a2, a3 = (np.concatenate([s[k] for s in la]) for k in ('p2d', 'p3d'))
    b2, b3 = (np.concatenate([s[k] for s in lb]) for k in ('p2d', 'p3d'))
    a, b = device(a2, a3, oa), device(b2, b3, ob)
    for k in ('R', 't', 'valid', 'n_inliers', 'hypothesis'):
        assert np.array_equal(a[k][2], b[k][2]), k
    assert np.array_equal(a['inliers'][194:494], b['inliers'][4:304])
    assert_equals_host(b, b2, b3, ob)


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a.view(np.uint32)[~np.isnan(a)], b.view(np.uint32)[~np.isnan(b)])


def test_lookup_equals_host_build():
    """the CPU test's maps and points; a two-pair table whose maps differ in size; the keypoints read out of a [M, 4] match list"""
    from geoformer_amd import ops
    a, b = C.lookup_maps()
    pa, pb = C.lookup_points(5, 7, 5), C.lookup_points(33, 65, 6)
    pts = np.concatenate([pa, pb, pb[:4]])
    off = np.array([0, len(pa), len(pa) + len(pb)], np.int32)          # the last four rows belong to no pair
    host = C.host_xyz_lookup([a, b], off, pts)
    da, db = _t(a), _t(b)
    table = ops.xyz_map_table([da, db], DEV)
    got = ops.xyz_lookup(table, _t(off, torch.int32), _t(pts)).cpu().numpy()
    assert _same(got, host) and np.isnan(got[-4:]).all() and np.isfinite(got).all(1).sum() > 60
    m4 = _t(np.c_[np.zeros((len(pts), 2), np.float32), pts])
    assert _same(ops.xyz_lookup(table, _t(off, torch.int32), m4[:, 2:]).cpu().numpy(), host)
    for m, dm, p in ((a, da, pa), (b, db, pb)):                       # each map alone (the table holds addresses: da, db stay alive)
        got = ops.xyz_lookup(ops.xyz_map_table([dm], DEV), _t([0, len(p)], torch.int32), _t(p)).cpu().numpy()
        assert _same(got, C.host_xyz_lookup([m], [0, len(p)], p))
    none = ops.xyz_lookup(ops.xyz_map_table([None], DEV), _t([0, len(pa)], torch.int32), _t(pa)).cpu().numpy()
    assert np.isnan(none).all()


def test_argument_errors():
    from geoformer_amd import _lib, ops
    sc = C.scene(300, 50, 0.3)
    a, b, off, K = _t(sc['p2d']), _t(sc['p3d']), _t([0, 50], torch.int32), _t(C.K9.reshape(3, 3))
    for iters in (0, 100, -64, C.HYP_PER_WG + 1):
        with pytest.raises(_lib.GeoFormerHipError, match=r'\(-1\).*multiple of 64'):
            ops.ransac_absolute_pose(a, b, None, off, 1, K, iters=iters)
    for thr in (0.0, -1.0):
        with pytest.raises(_lib.GeoFormerHipError, match=r'\(-1\).*pixel_thr'):
            ops.ransac_absolute_pose(a, b, None, off, 1, K, pixel_thr=thr)
    for refit in (-1, 9):
        with pytest.raises(_lib.GeoFormerHipError, match=r'\(-1\).*refit_rounds'):
            ops.ransac_absolute_pose(a, b, None, off, 1, K, refit=refit)
    with pytest.raises(_lib.GeoFormerHipError, match=r'\(-1\).*N out of range'):
        ops.ransac_absolute_pose(a, b, None, _t([0], torch.int32), 0, K)
    with pytest.raises(ValueError):
        ops.ransac_absolute_pose(a, b, None, off, 2, K)
    h = _lib.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()

    def raw(p2d=p, N=1, iters=256, thr=2.0, refit=0, ws=4096):
        return h.gf_abspose_ransac(p2d, p, None, p, N, 50, p, 0.25, thr, iters, 1, refit, p, p, p, p, p, p, p, p, ws, None)
    assert raw(p2d=None) == -1 and b'null pointer' in h.gf_last_error()
    assert raw(N=0) == -1 and b'N out of range' in h.gf_last_error()
    assert raw(N=5000000) == -1 and b'N out of range' in h.gf_last_error()
    assert raw(iters=96) == -1 and b'multiple of 64' in h.gf_last_error()
    assert raw(thr=0.0) == -1 and b'pixel_thr' in h.gf_last_error()
    assert raw(refit=9) == -1 and b'refit_rounds' in h.gf_last_error()
    assert raw(refit=-1) == -1 and b'refit_rounds' in h.gf_last_error()
    assert raw(ws=16) == -2 and b'workspace too small' in h.gf_last_error()
    assert h.gf_abspose_workspace_bytes(1, 50, 256) > 50 * 4 + 2 * 50 + 4 * 9 * 8 and h.gf_abspose_workspace_bytes(0, 50, 256) == 0
    assert h.gf_xyz_lookup(None, 1, p, p, 2, 5, p, None) == -1 and b'null pointer' in h.gf_last_error()
    assert h.gf_xyz_lookup(p, 0, p, p, 2, 5, p, None) == -1 and h.gf_xyz_lookup(p, 1, p, p, 1, 5, p, None) == -1
