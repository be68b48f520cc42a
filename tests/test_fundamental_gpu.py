"""Two-view verification on the GPU: gf_fundamental_ransac (csrc/k_fundamental.hip behind ops.ransac_fundamental) against the host
build of the same fund_solver.h (csrc/host/fund_host.cpp), bit for bit, and against the planted geometry.
Scenes: tests/fund_cases.py; the outcome checks and their scene seeds: tests/test_fund_solver_cpu.py."""
import numpy as np
import pytest
import torch

import fund_cases as C
import test_fund_solver_cpu as CPU

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SIZES = (0, 6, 7, 63, 64, 65, 129, 300)     # empty, below the minimum, minimal, the wave boundary on both sides, two waves and a tail, many


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def device(m, offsets, scores=None, thr=1.0, sc_thres=0.25, iters=256, seed=C.SEED):
    from geoformer_amd import ops
    N = len(offsets) - 1
    rs = ops.ransac_fundamental(_t(np.asarray(m, np.float32).reshape(-1, 4)), None if scores is None else _t(scores), _t(offsets, torch.int32), N,
                                pixel_thr=thr, sc_thres=sc_thres, iters=iters, seed=seed)
    assert rs['F'].dtype == torch.float64 and rs['inliers'].dtype == torch.uint8 and rs['F'].shape == (N, 3, 3)
    return {k: v.cpu().numpy() for k, v in rs.items()}


def assert_equals_host(dev, m, offsets, scores=None, n0=0, **kw):
    """every output of every pair, bit for bit; n0: the launch index of the first pair"""
    for n in range(len(offsets) - 1):
        a, b = offsets[n], offsets[n + 1]
        host = C.host_ransac(m[a:b], None if scores is None else scores[a:b], sample=n0 + n, **kw)
        assert host['status'] >= 0
        assert int(dev['valid'][n]) == host['valid'], n
        assert tuple(dev['hypothesis'][n]) == tuple(host['hyp']), n
        assert int(dev['n_inliers'][n]) == host['n_inliers'], n
        assert np.array_equal(dev['inliers'][a:b].astype(bool), host['inliers']), n
        assert np.array_equal(dev['F'][n].view(np.int64), host['F'].view(np.int64)), (n, np.abs(dev['F'][n] - host['F']).max())


@pytest.fixture(scope='module')
def eight_pairs():
    scenes = [C.scene(200 + i, n, 0.3 if n >= 63 else 0.0) for i, n in enumerate(SIZES)]
    m = np.concatenate([s['m'] for s in scenes])
    offsets = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    return scenes, m, offsets


@pytest.mark.parametrize('iters', [C.HYP_PER_WG, 2 * C.HYP_PER_WG, 256])
def test_device_equals_host_build(eight_pairs, iters):
    scenes, m, offsets = eight_pairs
    dev = device(m, offsets, iters=iters)
    assert_equals_host(dev, m, offsets, iters=iters)
    assert list(dev['valid']) == [0, 0, 1, 1, 1, 1, 1, 1]
    assert dev['n_inliers'][2] == 7 and not dev['inliers'][:6].any() and not dev['F'][:2].any()


def test_device_equals_host_build_with_filtered_rows(eight_pairs):
    """scores that filter rows in the middle of a wave, NaN / inf coordinates planted in some rows, a pair whose rows are all filtered and
    one left with six"""
    scenes, m, offsets = eight_pairs
    m = m.copy()
    rng = np.random.default_rng(9)
    scores = rng.uniform(0.3, 1.0, len(m)).astype(np.float32)
    o = offsets
    scores[o[7] + np.array([3, 30, 31, 32, 33, 70, 100, 130, 131, 190, 299])] = 0.1      # the 300-row pair
    scores[o[7] + 150] = np.nan
    scores[o[6] + np.arange(20, 45)] = 0.2                                               # the 129-row pair
    scores[o[4]:o[5]] = 0.0                                                              # 64 rows, none survive
    scores[o[3] + 6:o[4]] = 0.24                                                         # 63 rows, six survive
    m[o[7] + 17, 0] = np.nan; m[o[7] + 66, 3] = np.inf; m[o[6] + 64, 2] = -np.inf; m[o[5] + 1, 1] = np.nan
    dev = device(m, offsets, scores)
    assert_equals_host(dev, m, offsets, scores)
    keep = (scores >= 0.25) & np.isfinite(m).all(1)
    assert not dev['inliers'][~keep].any()
    assert list(dev['valid']) == [0, 0, 1, 0, 0, 1, 1, 1]
    # the result is that of the list with the filtered rows removed
    a, b = o[7], o[8]
    host = C.host_ransac(m[a:b][keep[a:b]], None, sample=7)
    assert np.array_equal(dev['inliers'][a:b].astype(bool)[keep[a:b]], host['inliers'])
    assert np.array_equal(dev['F'][7].view(np.int64), host['F'].view(np.int64))


def test_two_calls_give_the_same_bits(eight_pairs):
    scenes, m, offsets = eight_pairs
    a, b = device(m, offsets), device(m, offsets)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert tuple(device(m, offsets, seed=1234)['hypothesis'][7]) != tuple(a['hypothesis'][7])


def test_a_pair_depends_on_its_index_not_on_its_neighbours(eight_pairs):
    """the draw is keyed by (seed, n, t): the 300-row pair at index 2 of two different launches gives the same bits"""
    scenes, m, offsets = eight_pairs
    big = scenes[7]['m']
    la = np.concatenate([scenes[5]['m'], scenes[6]['m'], big])
    lb = np.concatenate([scenes[2]['m'], big, scenes[3]['m'], scenes[5]['m']])
    oa = np.array([0, 65, 194, 494], np.int32)
    ob = np.array([0, 7, 7, 307, 370, 435], np.int32)                 # index 1 is an empty pair
    a, b = device(la, oa), device(lb, ob)
    for k in ('F', 'valid', 'n_inliers', 'hypothesis'):
        assert np.array_equal(a[k][2], b[k][2]), k
    assert np.array_equal(a['inliers'][194:494], b['inliers'][7:307])
    assert_equals_host(b, lb, ob)


@pytest.mark.parametrize('frac, seeds, outcome', [(0.3, CPU.SEEDS_30, CPU.outcome_30), (0.5, CPU.SEEDS_50, CPU.outcome_50)])
def test_outcome_on_planted_scenes(frac, seeds, outcome):
    """the outcome cases of tests/test_fund_solver_cpu.py (same scenes, same RANSAC seeds, pair index 0) through ops.ransac_fundamental"""
    for s in seeds:
        sc = C.scene(s, 300, frac)
        off = np.array([0, 300], np.int32)
        dev = device(sc['m'], off, thr=CPU.THR, iters=256, seed=s - 100)
        ok, missed, extra = outcome(sc, dev['inliers'].astype(bool))
        print(f'{int(frac * 100)} % outliers, scene {s}: {missed} planted inliers missed, {extra} extra rows accepted')
        assert dev['valid'][0] == 1 and ok and dev['n_inliers'][0] == int(dev['inliers'].sum())
        assert abs(np.linalg.norm(dev['F'][0]) - 1) < 1e-12
        assert_equals_host(dev, sc['m'], off, thr=CPU.THR, iters=256, seed=s - 100)


def test_argument_errors():
    from geoformer_amd import _lib, ops
    sc = C.scene(300, 50, 0.3)
    m, off = _t(sc['m']), _t([0, 50], torch.int32)
    for iters in (0, 100, -64, C.HYP_PER_WG + 1):
        with pytest.raises(_lib.GeoFormerHipError, match=r'\(-1\).*multiple of 64'):
            ops.ransac_fundamental(m, None, off, 1, iters=iters)
    with pytest.raises(_lib.GeoFormerHipError, match=r'\(-1\).*pixel_thr'):
        ops.ransac_fundamental(m, None, off, 1, pixel_thr=0.0)
    h = _lib.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    assert h.gf_fundamental_ransac(None, None, p, 1, 50, 0.25, 1.0, 256, 1, p, p, p, p, p, p, 4096, None) == -1 and b'null pointer' in h.gf_last_error()
    assert h.gf_fundamental_ransac(p, None, p, 0, 50, 0.25, 1.0, 256, 1, p, p, p, p, p, p, 4096, None) == -1 and b'N out of range' in h.gf_last_error()
    assert h.gf_fundamental_ransac(p, None, p, 5000000, 50, 0.25, 1.0, 256, 1, p, p, p, p, p, p, 4096, None) == -1 and b'N out of range' in h.gf_last_error()
    assert h.gf_fundamental_ransac(p, None, p, 1, 50, 0.25, 1.0, 256, 1, p, p, p, p, p, p, 16, None) == -2 and b'workspace too small' in h.gf_last_error()
    assert h.gf_fundamental_workspace_bytes(1, 50, 256) > 50 * 4 + 4 * 9 * 8 and h.gf_fundamental_workspace_bytes(0, 50, 256) == 0
