"""Two-view verification at the matcher level: matcher.verify_matches / estimate_fundamental over ops.ransac_fundamental,
consolidate_matches(keep=...) and `pairs --verify` on the command line.  Scenes: tests/fund_cases.py."""
import os

import numpy as np
import pytest
import torch

import fund_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _result(m, scores=None):
    """a tuple as match_many returns it: matches, kpts1, kpts2, scores"""
    m = np.asarray(m, np.float32).reshape(-1, 4)
    return m, m[:, :2], m[:, 2:], np.ones(len(m), np.float32) if scores is None else np.asarray(scores, np.float32)


@pytest.fixture(scope='module')
def four_pairs():
    """two planted geometries (one with low scores on some rows), one pure-outlier pair, one empty pair"""
    a, b = C.scene(500, 300, 0.3), C.scene(501, 200, 0.3)
    rng = np.random.default_rng(3)
    junk = np.c_[rng.uniform(0, 640, 60), rng.uniform(0, 480, 60), rng.uniform(0, 640, 60), rng.uniform(0, 480, 60)].astype(np.float32)
    sb = rng.uniform(0.3, 1.0, 200).astype(np.float32)
    sb[[5, 64, 65, 130]] = 0.1
    pairs = [('a', 'b'), ('b', 'c'), ('a', 'c'), ('c', 'd')]
    results = [_result(a['m']), _result(b['m'], sb), _result(junk), _result(np.zeros((0, 4)))]
    return pairs, results, (a, b)


def test_verify_matches_on_four_pairs(four_pairs):
    from geoformer_amd import matcher as MT, ops
    pairs, results, (a, b) = four_pairs
    vm = MT.verify_matches(pairs, results, thr=1.0, min_inliers=15, sc_thres=0.25, device=DEV)
    assert vm.F.shape == (4, 3, 3) and vm.F.dtype == np.float64 and vm.n_inliers.shape == (4,) and vm.verified.dtype == bool
    assert list(vm.verified) == [True, True, False, False]
    assert [m.shape for m in vm.masks] == [(300,), (200,), (60,), (0,)] and all(m.dtype == bool for m in vm.masks)
    assert not vm.masks[2].any() and vm.n_inliers[3] == 0 and not vm.F[3].any()
    # the planted pairs: every planted inlier that takes part is kept; the filtered rows are not
    assert vm.masks[0][~a['outlier']].all()
    took_part = results[1][3] >= 0.25
    assert vm.masks[1][~b['outlier'] & took_part].all() and not vm.masks[1][~took_part].any()
    # the masks are ops.ransac_fundamental's
    ms = np.concatenate([r[0] for r in results])
    ss = np.concatenate([r[3] for r in results])
    off = np.array([0, 300, 500, 560, 560], np.int32)
    rs = ops.ransac_fundamental(torch.from_numpy(ms).to(DEV), torch.from_numpy(ss).to(DEV), torch.from_numpy(off).to(DEV), 4, pixel_thr=1.0, sc_thres=0.25)
    inl = rs['inliers'].cpu().numpy().astype(bool)
    assert np.array_equal(rs['F'].cpu().numpy().view(np.int64), vm.F.view(np.int64)) and np.array_equal(rs['n_inliers'].cpu().numpy(), vm.n_inliers)
    for p in (0, 1):
        assert np.array_equal(vm.masks[p], inl[off[p]:off[p + 1]]) and vm.n_inliers[p] == vm.masks[p].sum()
    # the junk pair: RANSAC may well return a model of a few inliers; min_inliers is what rejects it
    assert rs['n_inliers'][2].item() < 15
    lax = MT.verify_matches(pairs, results, min_inliers=0, device=DEV)
    assert list(lax.verified) == [True, True, bool(rs['valid'][2].item()), False]
    with pytest.raises(ValueError):
        MT.verify_matches(pairs[:3], results, device=DEV)
    assert MT.verify_matches([], [], device=DEV).F.shape == (0, 3, 3)


def test_estimate_fundamental_is_the_batch_entry_at_index_zero(four_pairs):
    from geoformer_amd import matcher as MT
    pairs, results, (a, b) = four_pairs
    F, mask = MT.estimate_fundamental(a['m'], thr=1.0, device=DEV)
    vm = MT.verify_matches(pairs[:1], results[:1], thr=1.0, device=DEV)
    assert np.array_equal(F.view(np.int64), vm.F[0].view(np.int64)) and np.array_equal(mask, vm.masks[0]) and mask.dtype == bool
    assert abs(np.linalg.norm(F) - 1) < 1e-12 and C.sampson_px(F, a['m'][mask, :2].astype(np.float64), a['m'][mask, 2:].astype(np.float64)).max() < 1.0
    assert MT.estimate_fundamental(a['m'][:6], device=DEV) is None
    assert MT.estimate_fundamental(np.repeat(a['m'][:1], 30, 0), device=DEV) is None


def _same(x, y):
    assert x.names == y.names and np.array_equal(x.pair_images, y.pair_images)
    assert len(x.keypoints) == len(y.keypoints) and len(x.matches) == len(y.matches)
    for k, l in zip(x.keypoints, y.keypoints):
        assert k.dtype == l.dtype == np.float32 and k.shape == l.shape and np.array_equal(k.view(np.uint32), l.view(np.uint32))
    for k, l in zip(x.matches, y.matches):
        assert k.dtype == l.dtype == np.int32 and k.shape == l.shape and np.array_equal(k, l)


def test_consolidate_matches_with_masks(four_pairs):
    from geoformer_amd import matcher as MT
    pairs, results, _ = four_pairs
    vm = MT.verify_matches(pairs, results, device=DEV)
    rng = np.random.default_rng(4)
    for keep in (vm.masks, [rng.random(len(r[0])) < 0.5 for r in results]):
        got = MT.consolidate_matches(pairs, results, keep=keep, device=DEV)
        want = MT.consolidate_matches(pairs, [tuple(np.asarray(x)[k] for x in r) for r, k in zip(results, keep)], device=DEV)
        _same(got, want)
        assert sum(len(m) for m in got.matches) > 0
    _same(MT.consolidate_matches(pairs, results, keep=None, device=DEV), MT.consolidate_matches(pairs, results, device=DEV))
    none = MT.consolidate_matches(pairs, results, keep=[np.zeros(len(r[0]), bool) for r in results], device=DEV)
    assert [m.shape for m in none.matches] == [(0, 2)] * 4 and all(m.dtype == np.int32 for m in none.matches)
    with pytest.raises(ValueError):
        MT.consolidate_matches(pairs, results, keep=vm.masks[:2], device=DEV)
    with pytest.raises(ValueError):
        MT.consolidate_matches(pairs, results, keep=[m[:-1] if len(m) else m for m in vm.masks], device=DEV)


# ------------------------------------------------------------------------------------------------------------------------------
# command line: three tiny generated PPM images, the deterministic-init matcher
# ------------------------------------------------------------------------------------------------------------------------------
def _write_images(root):
    from PIL import Image
    rng = np.random.default_rng(11)
    paths = []
    for name, (w, h) in (('a', (200, 168)), ('b', (280, 210)), ('c', (240, 168))):
        paths.append(os.path.join(root, name + '.ppm'))
        Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(paths[-1])
    return paths


def _npz(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def _same_arrays(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def test_cli_verify(tmp_path, monkeypatch):
    """Without --verify: what the command writes is what it wrote before the flag existed - the same keys and bytes of every array (the
    arrays are compared, not the .npz containers: a zip member carries its time of writing).  With --verify: the new keys, two_view.npz,
    and only verified inliers consolidated."""
    from geoformer_amd import matcher as MT
    from geoformer_amd.weights import deterministic_init_
    img = tmp_path / 'img'
    img.mkdir()
    _write_images(str(img))
    m = MT.GeoFormerMatcher(imsize=160, match_threshold=0.0, no_match_upscale=True, precision='fp16')
    deterministic_init_(m.model)
    m.model.fine_matching.thr = 0.0
    monkeypatch.setattr(MT, 'GeoFormerMatcher', lambda *a, **k: m)
    common = ['pairs', '--all-pairs', str(img), '--sc-thres', '0', '--imsize', '160', '--match-threshold', '0', '--no-match-upscale']
    plain, ver = tmp_path / 'plain', tmp_path / 'ver'
    MT.main(common + ['--out', str(plain / 'm'), '--keypoints', str(plain / 'k')])
    MT.main(common + ['--out', str(ver / 'm'), '--keypoints', str(ver / 'k'), '--verify', '--verify-thr', '3', '--min-inliers', '7'])
    pairs = MT.all_pairs(str(img))
    results = m.match_many(pairs)
    # ---- flag absent: the parent's code path, restated
    files = sorted(os.listdir(plain / 'm'))
    assert len(files) == 3 and sorted(os.listdir(plain / 'k')) == ['keypoints.npz', 'matches.npz', 'names.txt']
    cm = MT.consolidate_matches(pairs, results, sc_thres=0.0, device=DEV)
    MT.write_consolidated(str(tmp_path / 'want'), cm)
    for k, (f, res) in enumerate(zip(files, results)):
        assert f.startswith(f'{k:05d}_')
        _same_arrays(_npz(plain / 'm' / f), {'matches': res[0], 'kpts1': res[1], 'kpts2': res[2], 'scores': res[3]})
    for f in ('keypoints.npz', 'matches.npz'):
        _same_arrays(_npz(plain / 'k' / f), _npz(tmp_path / 'want' / f))
    assert open(plain / 'k' / 'names.txt', 'rb').read() == open(tmp_path / 'want' / 'names.txt', 'rb').read()
    # ---- --verify
    vm = MT.verify_matches(pairs, results, thr=3.0, min_inliers=7, sc_thres=0.0, device=DEV)
    assert sorted(os.listdir(ver / 'm')) == files and sorted(os.listdir(ver / 'k')) == ['keypoints.npz', 'matches.npz', 'names.txt', 'two_view.npz']
    for k, (f, res) in enumerate(zip(files, results)):
        z = _npz(ver / 'm' / f)
        assert sorted(z) == ['F', 'inliers', 'kpts1', 'kpts2', 'matches', 'scores', 'verified']
        assert z['F'].shape == (3, 3) and z['F'].dtype == np.float64 and z['inliers'].shape == (len(res[0]),) and z['inliers'].dtype == bool
        assert z['verified'].shape == () and z['verified'].dtype == bool
        assert np.array_equal(z['F'], vm.F[k]) and np.array_equal(z['inliers'], vm.masks[k]) and bool(z['verified']) == bool(vm.verified[k])
        _same_arrays({q: z[q] for q in ('matches', 'kpts1', 'kpts2', 'scores')}, _npz(plain / 'm' / f))
    tv = _npz(ver / 'k' / 'two_view.npz')
    assert sorted(tv) == ['F', 'n_inliers', 'pairs', 'verified']
    assert tv['pairs'].shape == (3, 2) and tv['F'].shape == (3, 3, 3) and tv['n_inliers'].shape == (3,) and tv['verified'].shape == (3,)
    assert np.array_equal(tv['pairs'], cm.pair_images) and np.array_equal(tv['verified'], vm.verified) and np.array_equal(tv['n_inliers'], vm.n_inliers)
    MT.write_consolidated(str(tmp_path / 'want_v'), MT.consolidate_matches(pairs, results, sc_thres=0.0, device=DEV, keep=vm.masks))
    for f in ('keypoints.npz', 'matches.npz'):
        _same_arrays(_npz(ver / 'k' / f), _npz(tmp_path / 'want_v' / f))
    mz = _npz(ver / 'k' / 'matches.npz')
    for q in range(3):
        assert len(mz[f'm{q:05d}']) <= int(vm.masks[q].sum())
