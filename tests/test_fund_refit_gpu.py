"""The refit of the fundamental matrix on its inliers on the GPU: gf_fundamental_ransac_lo (rt_refit<FundModel> of csrc/k_fundamental.hip behind
ops.ransac_fundamental(refit=R)) against the host build of the same fund_solver.h, bit for bit, then matcher.verify_matches(refit=R),
consolidate_matches(keep=...) and `pairs --verify --verify-refit`.  Scenes: tests/fund_refit_cases.py."""
import os

import numpy as np
import pytest
import torch

import fund_cases as C
import fund_refit_cases as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ITERS = 64
# SURVIVING rows per pair: the eight-inlier minimum on both sides, the 64-lane tree on both sides, the 256 partial sums on both sides (255:
# the last partial stays +0.0; 257: the first partial is the only one with two rows), many rows per partial.  One more pair is pure outliers.
SURVIVORS = (7, 8, 9, 63, 64, 65, 255, 256, 257, 600)
SCENES = (700, 705, 705, 703, 704, 705, 706, 707, 708, 709)      # scene seeds; at 8 and 9 rows: seeds whose refit the host build accepts
FILTERED = 8                      # the index of the pair that also carries filtered and non-finite rows (257 of its 270 rows survive)
KEYS = ('F', 'valid', 'n_inliers', 'hypothesis', 'rounds', 'inliers')


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def device(m, scores, offsets, refit, thr=1.0, sc_thres=0.25, iters=ITERS, seed=C.SEED):
    from geoformer_amd import ops
    N = len(offsets) - 1
    rs = ops.ransac_fundamental(_t(np.asarray(m, np.float32).reshape(-1, 4)), None if scores is None else _t(scores), _t(offsets, torch.int32), N,
                                pixel_thr=thr, sc_thres=sc_thres, iters=iters, seed=seed, refit=refit)
    return {k: v.cpu().numpy() for k, v in rs.items()}


def device_lo(m, scores, offsets, refit, thr=1.0, sc_thres=0.25, iters=ITERS, seed=C.SEED):
    """gf_fundamental_ransac_lo itself (ops.ransac_fundamental calls it for refit > 0 only)"""
    from geoformer_amd import _lib
    h = _lib.lib()
    N, M = len(offsets) - 1, len(m)
    dm, ds, do = _t(m), _t(scores), _t(offsets, torch.int32)
    out = {'F': torch.empty(N, 3, 3, dtype=torch.float64, device=DEV), 'valid': torch.empty(N, dtype=torch.int32, device=DEV),
           'n_inliers': torch.empty(N, dtype=torch.int32, device=DEV), 'hypothesis': torch.empty(N, 2, dtype=torch.int32, device=DEV),
           'inliers': torch.zeros(M, dtype=torch.uint8, device=DEV), 'rounds': torch.full((N,), -1, dtype=torch.int32, device=DEV)}
    ws = torch.empty(h.gf_fundamental_lo_workspace_bytes(N, M, iters), dtype=torch.uint8, device=DEV)
    rc = h.gf_fundamental_ransac_lo(dm.data_ptr(), ds.data_ptr(), do.data_ptr(), N, M, sc_thres, thr, iters, seed, out['F'].data_ptr(),
                                    out['valid'].data_ptr(), out['n_inliers'].data_ptr(), out['hypothesis'].data_ptr(), out['inliers'].data_ptr(),
                                    refit, out['rounds'].data_ptr(), ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def host(m, scores, offsets, refit, order=None, **kw):
    """the host build pair by pair; order[n]: the launch index of pair n"""
    out = []
    for n in range(len(offsets) - 1):
        a, b = offsets[n], offsets[n + 1]
        out.append(R.host_ransac_lo(m[a:b], scores[a:b], iters=ITERS, sample=n if order is None else order[n], refit=refit, **kw))
        assert out[-1]['status'] >= 0
    return out


def assert_equals_host(dev, hst, offsets):
    for n, h in enumerate(hst):
        a, b = offsets[n], offsets[n + 1]
        assert int(dev['valid'][n]) == h['valid'], n
        assert tuple(dev['hypothesis'][n]) == tuple(h['hyp']), n
        assert int(dev['rounds'][n]) == h['rounds'], n
        assert int(dev['n_inliers'][n]) == h['n_inliers'], n
        assert np.array_equal(dev['inliers'][a:b].astype(bool), h['inliers']), n
        assert np.array_equal(dev['F'][n].view(np.int64), h['F'].view(np.int64)), (n, np.abs(dev['F'][n] - h['F']).max())


def make_pairs():
    """sigma = 0.5 px scenes with the surviving row counts of SURVIVORS (no outliers below 63 rows, 30 % from there on), then 60 rows of
    pure outliers.  Pair FILTERED has 13 more rows that take no part: low and NaN scores, NaN / inf coordinates, in the middle of waves."""
    ms, ss = [], []
    for i, n in enumerate(SURVIVORS):
        extra = 13 if i == FILTERED else 0
        m = R.noisy_scene(SCENES[i], n + extra, 0.3 if n >= 63 else 0.0, 0.5)['m']
        s = np.random.default_rng(50 + i).uniform(0.3, 1.0, len(m)).astype(np.float32)
        if extra:
            s[[3, 64, 65, 66, 130, 200, 255, 256, 269]] = 0.1
            s[150] = np.nan
            m[17, 0] = np.nan; m[70, 3] = np.inf; m[128, 2] = -np.inf
        ms.append(m)
        ss.append(s)
    rng = np.random.default_rng(3)
    ms.append(np.c_[rng.uniform(0, 640, 60), rng.uniform(0, 480, 60), rng.uniform(0, 640, 60), rng.uniform(0, 480, 60)].astype(np.float32))
    ss.append(np.ones(60, np.float32))
    offsets = np.concatenate([[0], np.cumsum([len(m) for m in ms])]).astype(np.int32)
    m, s = np.concatenate(ms), np.concatenate(ss)
    keep = (s >= 0.25) & np.isfinite(m).all(1)
    assert [int(keep[offsets[i]:offsets[i + 1]].sum()) for i in range(len(SURVIVORS))] == list(SURVIVORS)
    return ms, ss, m, s, offsets, keep


@pytest.fixture(scope='module')
def pairs11():
    return make_pairs()


@pytest.fixture(scope='module')
def host_runs(pairs11):
    ms, ss, m, s, offsets, keep = pairs11
    return {r: host(m, s, offsets, r) for r in (0, 1, 4, 8)}


def test_the_scenes_reach_the_edges(host_runs):
    """what the bit comparisons below are worth: the refit runs (and is accepted) on both sides of every boundary, not at seven rows"""
    r8 = host_runs[8]
    assert r8[0]['rounds'] == 0 and r8[0]['n_inliers'] == 7                         # seven inliers: not refitted
    assert all(r8[i]['rounds'] > 0 for i in range(1, len(SURVIVORS))), [h['rounds'] for h in r8]
    assert max(h['rounds'] for h in r8) > 1
    assert all(b['n_inliers'] >= a['n_inliers'] for a, b in zip(host_runs[0], r8))


@pytest.mark.parametrize('refit', [1, 4, 8])
def test_device_equals_host_build(pairs11, host_runs, refit):
    ms, ss, m, s, offsets, keep = pairs11
    dev = device(m, s, offsets, refit)
    assert dev['rounds'].dtype == np.int32 and dev['rounds'].shape == (len(ms),)
    assert_equals_host(dev, host_runs[refit], offsets)
    assert not dev['inliers'][~keep].any()
    assert (dev['n_inliers'] == [int(dev['inliers'][offsets[n]:offsets[n + 1]].sum()) for n in range(len(ms))]).all()


def test_zero_rounds_is_gf_fundamental_ransac(pairs11, host_runs):
    ms, ss, m, s, offsets, keep = pairs11
    plain = device(m, s, offsets, 0)
    assert 'rounds' not in plain
    rc, lo = device_lo(m, s, offsets, 0)
    assert rc == 0 and not lo['rounds'].any()
    for k in plain:
        assert np.array_equal(plain[k].view(np.uint8), lo[k].view(np.uint8)), k
    assert_equals_host(lo, host_runs[0], offsets)
    # rounds[n] == 0 after a refit: the seven-point winner's bits
    rc, lo8 = device_lo(m, s, offsets, 8)
    assert rc == 0
    for n in np.flatnonzero(lo8['rounds'] == 0):
        assert np.array_equal(lo8['F'][n].view(np.int64), plain['F'][n].view(np.int64)) and lo8['n_inliers'][n] == plain['n_inliers'][n]
        assert np.array_equal(lo8['inliers'][offsets[n]:offsets[n + 1]], plain['inliers'][offsets[n]:offsets[n + 1]])
    assert np.array_equal(lo8['hypothesis'], plain['hypothesis']) and (lo8['n_inliers'] >= plain['n_inliers']).all()


def test_refit_of_pairs_that_cannot_be_refitted_equals_host_build():
    """the refit stage launched over the pairs of tests/test_fundamental_gpu.py - an empty pair, one below the minimum, a minimal one (seven
    inliers: not refitted), 63 .. 300 rows - through gf_fundamental_ransac_lo itself: rounds 0 and the seven-point winner's bits where
    nothing is refitted, against the host build"""
    sizes = (0, 6, 7, 63, 64, 65, 129, 300)
    m = np.concatenate([C.scene(200 + i, n, 0.3 if n >= 63 else 0.0)['m'] for i, n in enumerate(sizes)])
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    scores = np.ones(len(m), np.float32)
    rc, dev = device_lo(m, scores, offsets, 4)
    assert rc == 0
    assert_equals_host(dev, host(m, scores, offsets, 4), offsets)
    assert list(dev['valid']) == [0, 0, 1, 1, 1, 1, 1, 1] and not dev['rounds'][:3].any() and dev['n_inliers'][2] == 7


def test_two_calls_give_the_same_bits(pairs11):
    ms, ss, m, s, offsets, keep = pairs11
    a, b = device(m, s, offsets, 4), device(m, s, offsets, 4)
    for k in KEYS:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def test_a_pair_depends_on_its_index_not_on_its_neighbours(pairs11):
    """the pairs in another order: every pair against the host build with its new launch index as `sample`; the 600-row pair at the same
    index next to other neighbours gives the same bits"""
    ms, ss, m, s, offsets, keep = pairs11
    order = [3, 10, 9, 8, 0, 6, 1, 5, 2, 7, 4]
    lm, ls = [ms[i] for i in order], [ss[i] for i in order]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lm])]).astype(np.int32)
    mm, sm = np.concatenate(lm), np.concatenate(ls)
    dev = device(mm, sm, off, 4)
    assert_equals_host(dev, host(mm, sm, off, 4), off)
    lm2, ls2 = [ms[5], ms[1], ms[9], ms[2]], [ss[5], ss[1], ss[9], ss[2]]     # the 600-row pair at index 2 again
    off2 = np.concatenate([[0], np.cumsum([len(x) for x in lm2])]).astype(np.int32)
    dev2 = device(np.concatenate(lm2), np.concatenate(ls2), off2, 4)
    for k in ('F', 'valid', 'n_inliers', 'hypothesis', 'rounds'):
        assert np.array_equal(dev[k][2], dev2[k][2]), k
    assert np.array_equal(dev['inliers'][off[2]:off[3]], dev2['inliers'][off2[2]:off2[3]])


def test_matcher_level(pairs11):
    from geoformer_amd import matcher as MT
    ms, ss, m, s, offsets, keep = pairs11
    names = [(f'i{n}', f'j{n}') for n in range(len(ms))]
    results = [(x, x[:, :2], x[:, 2:], y) for x, y in zip(ms, ss)]
    op = device(m, s, offsets, 4, iters=512)
    vm = MT.verify_matches(names, results, thr=1.0, min_inliers=8, sc_thres=0.25, device=DEV, refit=4)
    assert vm.rounds.dtype == np.int32 and np.array_equal(vm.rounds, op['rounds']) and np.array_equal(vm.n_inliers, op['n_inliers'])
    assert np.array_equal(vm.F.view(np.int64), op['F'].view(np.int64))
    assert np.array_equal(vm.verified, (op['valid'] == 1) & (op['n_inliers'] >= 8)) and vm.verified[1:10].all() and not vm.verified[0]
    for n in range(len(ms)):
        want = op['inliers'][offsets[n]:offsets[n + 1]].astype(bool) if vm.verified[n] else np.zeros(len(ms[n]), bool)
        assert np.array_equal(vm.masks[n], want), n
    plain = MT.verify_matches(names, results, thr=1.0, min_inliers=8, sc_thres=0.25, device=DEV)
    assert plain.rounds.dtype == np.int32 and plain.rounds.shape == (len(ms),) and not plain.rounds.any()
    assert (vm.n_inliers >= plain.n_inliers).all() and vm.n_inliers.sum() > plain.n_inliers.sum()
    assert MT.verify_matches([], [], device=DEV, refit=4).rounds.shape == (0,)
    # the masks of the refined models go where the seven-point masks went
    got = MT.consolidate_matches(names, results, keep=vm.masks, device=DEV)
    want = MT.consolidate_matches(names, [tuple(np.asarray(x)[k] for x in r) for r, k in zip(results, vm.masks)], device=DEV)
    assert len(got.matches) == len(want.matches) and all(np.array_equal(a, b) for a, b in zip(got.matches, want.matches))
    assert sum(len(x) for x in got.matches) > 0
    # one pair
    F, mask = MT.estimate_fundamental(ms[9], thr=1.0, device=DEV, refit=4)
    one = device(ms[9], None, np.array([0, 600], np.int32), 4, iters=512)
    assert np.array_equal(F.view(np.int64), one['F'][0].view(np.int64)) and np.array_equal(mask, one['inliers'].astype(bool))


def test_argument_errors(pairs11):
    from geoformer_amd import _lib, ops
    ms, ss, m, s, offsets, keep = pairs11
    dm, off = _t(ms[4]), _t([0, 64], torch.int32)
    for refit in (-1, 9, 64):
        with pytest.raises(_lib.GeoFormerHipError, match=r'\(-1\).*gf_fundamental_ransac_lo.*refit_rounds'):
            ops.ransac_fundamental(dm, None, off, 1, iters=ITERS, refit=refit)
    with pytest.raises(_lib.GeoFormerHipError, match=r'\(-1\).*gf_fundamental_ransac_lo.*multiple of 64'):
        ops.ransac_fundamental(dm, None, off, 1, iters=100, refit=4)
    h = _lib.lib()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    assert h.gf_fundamental_ransac_lo(p, None, p, 1, 50, 0.25, 1.0, 64, 1, p, p, p, p, p, 4, None, p, 1 << 16, None) == -1
    assert b'gf_fundamental_ransac_lo: null pointer' in h.gf_last_error()
    small = h.gf_fundamental_workspace_bytes(1, 50, 64)
    assert h.gf_fundamental_lo_workspace_bytes(1, 50, 64) >= small + 2 * 50 and h.gf_fundamental_lo_workspace_bytes(0, 50, 64) == 0
    assert h.gf_fundamental_ransac_lo(p, None, p, 1, 50, 0.25, 1.0, 64, 1, p, p, p, p, p, 4, p, p, small, None) == -2
    assert b'gf_fundamental_ransac_lo: workspace too small' in h.gf_last_error()


# ------------------------------------------------------------------------------------------------------------------------------
# command line: three tiny generated PPM images, the deterministic-init matcher
# ------------------------------------------------------------------------------------------------------------------------------
def _npz(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def test_cli_writes_refit_rounds(tmp_path, monkeypatch, capsys):
    from PIL import Image
    from geoformer_amd import matcher as MT
    from geoformer_amd.weights import deterministic_init_
    img = tmp_path / 'img'
    img.mkdir()
    rng = np.random.default_rng(11)
    for name, (w, h) in (('a', (200, 168)), ('b', (280, 210)), ('c', (240, 168))):
        Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(os.path.join(str(img), name + '.ppm'))
    m = MT.GeoFormerMatcher(imsize=160, match_threshold=0.0, no_match_upscale=True, precision='fp16')
    deterministic_init_(m.model)
    m.model.fine_matching.thr = 0.0
    monkeypatch.setattr(MT, 'GeoFormerMatcher', lambda *a, **k: m)
    common = ['pairs', '--all-pairs', str(img), '--sc-thres', '0', '--imsize', '160', '--match-threshold', '0', '--no-match-upscale', '--verify',
              '--verify-thr', '3', '--min-inliers', '7']
    assert MT.build_parser().parse_args(common + ['--verify-refit']).verify_refit == 4 and MT.build_parser().parse_args(common).verify_refit == 0
    out = tmp_path / 'out'
    MT.main(common + ['--out', str(out / 'm'), '--keypoints', str(out / 'k'), '--verify-refit', '2'])
    pairs = MT.all_pairs(str(img))
    results = m.match_many(pairs)
    vm = MT.verify_matches(pairs, results, thr=3.0, min_inliers=7, sc_thres=0.0, device=DEV, refit=2)
    files = sorted(os.listdir(out / 'm'))
    assert len(files) == 3
    for k, f in enumerate(files):
        z = _npz(out / 'm' / f)
        assert sorted(z) == ['F', 'inliers', 'kpts1', 'kpts2', 'matches', 'refit_rounds', 'scores', 'verified']
        assert z['refit_rounds'].shape == () and z['refit_rounds'].dtype == np.int32 and int(z['refit_rounds']) == int(vm.rounds[k])
        assert np.array_equal(z['F'], vm.F[k]) and np.array_equal(z['inliers'], vm.masks[k])
    tv = _npz(out / 'k' / 'two_view.npz')
    assert sorted(tv) == ['F', 'n_inliers', 'pairs', 'refit_rounds', 'verified']
    assert np.array_equal(tv['refit_rounds'], vm.rounds) and np.array_equal(tv['n_inliers'], vm.n_inliers)
    assert f'the refit on the inliers (up to 2 rounds) changed {int((vm.rounds > 0).sum())} pairs' in capsys.readouterr().out
