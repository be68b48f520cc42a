"""Keypoint consolidation for SfM on the device (csrc/k_keypoints.hip behind ops.consolidate_keypoints / matcher.consolidate_matches):
against what the reference's matches_to_keypoint_ids recorded (tests/golden/g19_keypoint_quantize.npz) and, bit for bit - keypoints, ids and
order - against the serial host build of the same rule (csrc/host/keypoint_host.cpp over csrc/keypoint_spec.h)."""
import os

import numpy as np
import pytest
import torch

import keypoint_cases as KC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def device_consolidate(m, sc, off, im, n_images, sc_thres=0.25, psize=48.0, dthres=4.0, unique=True):
    from geoformer_amd import ops
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (np.asarray(m, np.float32).reshape(-1, 4), np.asarray(sc, np.float32),
                                                                     np.asarray(off, np.int32), np.asarray(im, np.int32).reshape(-1, 2))]
    out = ops.consolidate_keypoints(*t, n_images, sc_thres, psize, dthres, unique)
    assert [o.dtype for o in out] == [torch.float32, torch.int32, torch.int32, torch.int32]
    return tuple(o.cpu().numpy() for o in out)


def both(case, **kw):
    dev = device_consolidate(*case, **kw)
    host = KC.host_consolidate(*case, **kw)
    KC.assert_same(dev, host)
    return dev, host


@pytest.fixture(scope='module')
def golden_g19():
    return KC.golden_cases()


@pytest.mark.parametrize('case', range(7))
def test_device_reproduces_the_reference(golden_g19, case):
    inputs, cases = golden_g19
    psize, dthres, unique, exp = cases[case]
    res = device_consolidate(inputs['matches'], inputs['scores'], inputs['pair_offsets'], inputs['pair_images'], inputs['n_images'],
                             inputs['sc_thres'], psize, dthres, unique)
    KC.check_against_golden(res, psize, dthres, unique, exp)


def test_one_cell_with_thousands_of_centres():
    # every chunking path (registers, scratch chunks, a partly filled last chunk) and the merge path in one group
    for unique in (True, False):
        dev, host = both(KC.lattice_case(), psize=48.0, dthres=0.5, unique=unique)
        assert host[4]['most_centres'] >= 2304 and host[4]['groups'] == 2
        assert host[4]['K'] < 2 * 2804                                    # jittered points merged


def test_long_sequential_groups():
    dev, host = both(KC.long_groups_case())
    assert host[4]['groups'] == 6 and host[4]['longest_group'] == 2000


def test_interleaved_images_and_pairs():
    case = KC.interleaved_case()
    for kw in (dict(), dict(unique=False), dict(psize=16.0, dthres=6.0), dict(sc_thres=0.0, psize=48.0, dthres=0.5)):
        dev, host = both(case, **kw)
        assert host[4]["flags"] == 0 and 0 < len(dev[2]) <= len(case[0])
    assert all(k > 0 for k in np.diff(dev[1]))                            # every image has keypoints


def test_empty_inputs():
    z4, z1 = np.zeros((0, 4), np.float32), np.zeros(0, np.float32)
    dev, host = both((z4, z1, np.array([0], np.int32), np.zeros((0, 2), np.int32), 3))                      # no pairs
    assert dev[0].shape == (0, 2) and dev[1].tolist() == [0, 0, 0, 0] and dev[2].shape == (0, 2) and dev[3].tolist() == [0]
    dev, host = both((z4, z1, np.array([0, 0, 0], np.int32), np.array([[0, 1], [1, 2]], np.int32), 3))     # pairs without rows
    assert dev[3].tolist() == [0, 0, 0]
    m, sc, off, im, n = KC.interleaved_case()
    dev, host = both((m, sc, off, im, n), sc_thres=2.0)                                                       # all rows below the threshold
    assert dev[0].shape == (0, 2) and dev[2].shape == (0, 2) and not dev[1].any() and not dev[3].any()
    dev, host = both((m[:17], sc[:17], np.array([0, 0, 17, 17], np.int32), np.array([[0, 1], [1, 0], [0, 1]], np.int32), 2), sc_thres=0.0)
    assert dev[3].tolist()[0] == 0 and dev[3][2] == dev[3][3] == len(dev[2])                                  # a pair with 0 rows on either side


def test_boundary_coordinates():
    case = KC.boundary_case()
    for psize, dthres in ((48.0, 4.0), (16.0, 6.0)):
        dev, host = both(case, psize=psize, dthres=dthres)
        assert host[4]['flags'] == 0 and host[4]['points'] == 2 * len(case[0])
    both(case, psize=-1.0, dthres=-1.0)


def test_exact_mode():
    case = KC.exact_case()
    dev, host = both(case, sc_thres=0.0, psize=-1.0, dthres=-1.0)
    assert len(dev[2]) == len(case[0]) and dev[2][:4, 0].tolist() == [0, 0, 0, 0]
    both(case, sc_thres=0.5, psize=48.0, dthres=0.0)
    both(KC.interleaved_case(), psize=0.0, dthres=4.0)


def test_equal_scores_under_the_filter():
    dev, host = both(KC.equal_scores_case(), psize=48.0, dthres=6.0)
    assert host[4]['dropped'] > 0


def test_same_call_twice_same_bits():
    case = KC.lattice_case()
    KC.assert_same(device_consolidate(*case, psize=48.0, dthres=0.5), device_consolidate(*case, psize=48.0, dthres=0.5))
    case = KC.interleaved_case()
    KC.assert_same(device_consolidate(*case), device_consolidate(*case))


def test_ranges_are_status_codes_before_any_launch():
    from geoformer_amd import _lib, ops
    h = _lib.lib()
    # nothing but the arguments is looked at: every pointer is null
    assert h.gf_keypoint_keys(None, None, None, None, 1, 1, (1 << 19) + 1, 0.25, 48.0, 4.0, None, None, None, None, None, None, None) == -1
    assert b'image index range' in h.gf_last_error()
    assert h.gf_keypoint_keys(None, None, None, None, 1, 1, 4, 0.25, 2.0, 4.0, None, None, None, None, None, None, None) == -1
    assert b'cell index range' in h.gf_last_error()
    assert h.gf_keypoint_keys(None, None, None, None, 1, 1, 4, 0.25, float('inf'), 4.0, None, None, None, None, None, None, None) == -1
    assert b'cell index range' in h.gf_last_error()
    assert h.gf_keypoint_keys(None, None, None, None, 1, 1 << 30, 4, 0.25, 48.0, 4.0, None, None, None, None, None, None, None) == -1
    with pytest.raises(_lib.GeoFormerHipError, match='cell index range'):
        device_consolidate(*KC.interleaved_case(), psize=1.5)
    # what only the data can break is reported after the call, and nothing wraps
    m = np.array([[1, 1, 2, 2], [5e6, 1, 2, 2]], np.float32)
    with pytest.raises(_lib.GeoFormerHipError, match='coordinate'):
        device_consolidate(m, np.ones(2, np.float32), [0, 2], [[0, 1]], 2)
    assert len(device_consolidate(m, np.ones(2, np.float32), [0, 2], [[0, 1]], 2, psize=-1.0)[2]) == 2       # the exact mode has no cells
    with pytest.raises(_lib.GeoFormerHipError, match='pair_images'):
        device_consolidate(m[:1], np.ones(1, np.float32), [0, 1], [[0, 2]], 2)
    assert ops.KP_FLAG_COORD_RANGE == 1 and ops.KP_FLAG_IMAGE_RANGE == 2


# ------------------------------------------------------------------------------------------------------------------------------
# matcher level: three random images, the deterministic-init matcher, both return conventions
# ------------------------------------------------------------------------------------------------------------------------------
def _write_images(root):
    from PIL import Image
    rng = np.random.default_rng(11)
    paths = []
    for name, (w, h) in (('a', (200, 168)), ('b', (280, 210)), ('c', (240, 168))):
        paths.append(os.path.join(root, name + '.png'))
        Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(paths[-1])
    return paths


_shared = {}


def _matcher():
    if 'm' not in _shared:
        from geoformer_amd import matcher as MT
        from geoformer_amd.weights import deterministic_init_
        m = MT.GeoFormerMatcher(imsize=160, match_threshold=0.0, no_match_upscale=True, precision='fp16')
        deterministic_init_(m.model)
        m.model.fine_matching.thr = 0.0
        _shared['m'] = m
    return _shared['m']


def _host_of(pairs, results, **kw):
    names = {}
    im = np.array([[names.setdefault(p, len(names)) for p in pr] for pr in pairs], np.int32)
    ms = [np.asarray(r[0], np.float32).reshape(-1, 4) for r in results]
    ss = [np.asarray(r[3], np.float32) for r in results]
    off = np.concatenate([[0], np.cumsum([len(x) for x in ms])]).astype(np.int32)
    return list(names), im, KC.host_consolidate(np.concatenate(ms), np.concatenate(ss), off, im, len(names), **kw)


def _check_record(cm, pairs, results, sc_thres, unique):
    names, im, (kp, kpo, ids, ido, st) = _host_of(pairs, results, sc_thres=sc_thres, unique=unique)
    assert cm.names == names and np.array_equal(cm.pair_images, im) and cm.pair_images.dtype == np.int32
    assert len(cm.keypoints) == len(names) and len(cm.matches) == len(pairs) and st['rows'] > 0
    for i, k in enumerate(cm.keypoints):
        assert k.dtype == np.float32 and np.array_equal(k.view(np.uint32), kp[kpo[i]:kpo[i + 1]].view(np.uint32))
    for q, mt in enumerate(cm.matches):
        assert mt.dtype == np.int32 and mt.shape[1:] == (2,) and np.array_equal(mt, ids[ido[q]:ido[q + 1]])
        for s in range(2):
            assert (mt[:, s] >= 0).all() and (mt[:, s] < len(cm.keypoints[im[q, s]])).all()            # every id names a keypoint of its image
            if unique:
                assert len(np.unique(mt[:, s])) == len(mt)                                               # no id repeats within a pair
    return st


@pytest.mark.parametrize('no_match_upscale', [True, False])
def test_consolidate_matches_equals_the_host_build(tmp_path, no_match_upscale):
    from geoformer_amd import matcher as MT
    a, b, c = _write_images(str(tmp_path))
    pairs = [(a, b), (c, a), (b, c), (a, b)]                   # one pair in reversed first-appearance order, one listed twice
    m = _matcher()
    m.no_match_upscale = no_match_upscale
    try:
        results = m.match_many(pairs)
    finally:
        m.no_match_upscale = True
    assert len(results[0]) == (5 if no_match_upscale else 4) and (results[0][0].dtype == np.float64) == (not no_match_upscale)
    scores = np.concatenate([r[3] for r in results])
    for sc_thres in (0.0, float(np.median(scores))):
        st_u = _check_record(MT.consolidate_matches(pairs, results, sc_thres=sc_thres, device=DEV), pairs, results, sc_thres, True)
        st_a = _check_record(MT.consolidate_matches(pairs, results, sc_thres=sc_thres, qt_unique=False, device=DEV), pairs, results, sc_thres, False)
        assert st_a['dropped'] == 0 and st_u['rows'] + st_u['dropped'] == st_a['rows']
    empty = MT.consolidate_matches(pairs, results, sc_thres=2.0, device=DEV)
    assert [k.shape for k in empty.keypoints] == [(0, 2)] * 3 and [x.shape for x in empty.matches] == [(0, 2)] * 4


def test_cli_writes_names_keypoints_and_matches(tmp_path, monkeypatch):
    from geoformer_amd import matcher as MT
    img = tmp_path / 'img'
    img.mkdir()
    paths = _write_images(str(img))
    m = _matcher()
    monkeypatch.setattr(MT, 'GeoFormerMatcher', lambda *a, **k: m)          # the command line's matcher: the deterministic one of this file
    out = str(tmp_path / 'sfm')
    MT.main(['pairs', '--all-pairs', str(img), '--keypoints', out, '--sc-thres', '0', '--imsize', '160', '--match-threshold', '0',
             '--no-match-upscale'])
    pairs = MT.all_pairs(str(img))
    want = MT.consolidate_matches(pairs, m.match_many(pairs), sc_thres=0.0, device=DEV)
    assert sorted(os.listdir(out)) == ['keypoints.npz', 'matches.npz', 'names.txt']
    assert open(os.path.join(out, 'names.txt')).read().split('\n')[:-1] == want.names == paths
    kz, mz = np.load(os.path.join(out, 'keypoints.npz')), np.load(os.path.join(out, 'matches.npz'))
    assert sorted(kz.files) == [f'k{i:05d}' for i in range(3)] and sorted(mz.files) == [f'm{q:05d}' for q in range(3)] + ['pairs']
    assert np.array_equal(mz['pairs'], want.pair_images) and sum(len(x) for x in want.matches) > 0
    for i in range(3):
        assert kz[f'k{i:05d}'].dtype == np.float32 and np.array_equal(kz[f'k{i:05d}'].view(np.uint32), want.keypoints[i].view(np.uint32))
        assert mz[f'm{i:05d}'].dtype == np.int32 and np.array_equal(mz[f'm{i:05d}'], want.matches[i])
    # every match of every pair reads as two keypoints
    for q, (i0, i1) in enumerate(mz['pairs']):
        ids = mz[f'm{q:05d}']
        assert kz[f'k{i0:05d}'][ids[:, 0]].shape == kz[f'k{i1:05d}'][ids[:, 1]].shape == (len(ids), 2)
