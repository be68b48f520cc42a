"""Relative pose on the GPU: gf_pose_essential_ransac against the host build of the same pose_solver.h (bit for bit) and against the
planted truth, gf_epipolar_errors against the formula in numpy fp64, compute_pose_errors and the validation step.
Scenes: tests/pose_cases.py."""
import numpy as np
import pytest
import torch

import pose_cases as P

pytestmark = pytest.mark.gpu
DEV = 'cuda'
COUNTS = (300, 130, 5, 4, 0)        # 130: two waves and a tail; 5: the exact minimum; 4: below it; 0: empty


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _K(n):
    return _t(np.repeat(P.K[None], n, 0))


@pytest.fixture(scope='module')
def five_pairs():
    scenes = [P.scene(200 + i, n, 0.3) if n else None for i, n in enumerate(COUNTS)]
    mk0 = np.concatenate([s['mk0'] for s in scenes if s is not None])
    mk1 = np.concatenate([s['mk1'] for s in scenes if s is not None])
    counts = np.array([sum(COUNTS), *COUNTS], np.int32)
    return scenes, mk0, mk1, counts


def _device(mk0, mk1, counts, iters=256, seed=0x5EED, N=None):
    from geoformer_amd import ops
    N = len(counts) - 1 if N is None else N
    rs = ops.ransac_essential(_t(mk0), _t(mk1), _t(counts, torch.int32), N, _K(N), _K(N), iters=iters, seed=seed)
    return {k: v.cpu().numpy() for k, v in rs.items()}


@pytest.mark.parametrize('iters', [32, 64, 256])
def test_device_equals_host_build(five_pairs, iters):
    """32 hypotheses: one workgroup per pair; 64: two; 256: eight.  The 5-match pair is the tie case - every hypothesis that solves has
    5 inliers - so the winner must be the smallest hypothesis and its smallest root across all workgroups, as on the host."""
    scenes, mk0, mk1, counts = five_pairs
    dev = _device(mk0, mk1, counts, iters=iters)
    off = 0
    for n, cnt in enumerate(COUNTS):
        host = P.host_ransac(mk0[off:off + cnt], mk1[off:off + cnt], iters=iters, sample=n)
        assert int(dev['valid'][n]) == host['valid'] == (1 if cnt >= 5 else 0), n
        assert tuple(dev['hypothesis'][n]) == tuple(host['hyp']), n
        assert int(dev['n_inliers'][n]) == host['n_inliers'], n
        assert np.array_equal(dev['inliers'][off:off + cnt].astype(bool), host['inliers']), n
        for k in ('E', 'R', 't'):                                   # bit-equal: same text, fp64, contraction off on both sides
            assert np.array_equal(dev[k][n].view(np.int64), host[k].view(np.int64)), (n, k, np.abs(dev[k][n] - host[k]).max())
        off += cnt


def test_a_pair_depends_on_its_index_not_on_its_neighbours(five_pairs):
    """the draw is keyed by (seed, n, t): the 130-match scene at index 2 of a 3-pair and of a 5-pair launch (index 1 empty there) gives the
    same bits"""
    scenes = five_pairs[0]
    mid = scenes[1]
    la = [scenes[2], scenes[3], mid]
    lb = [scenes[0], None, mid, scenes[2], scenes[3]]
    out = []
    for lst in (la, lb):
        cnts = [0 if s is None else len(s['mk0']) for s in lst]
        mk0 = np.concatenate([s['mk0'] for s in lst if s is not None])
        mk1 = np.concatenate([s['mk1'] for s in lst if s is not None])
        dev = _device(mk0, mk1, np.array([sum(cnts), *cnts], np.int32))
        off = sum(cnts[:2])
        out.append({**{k: dev[k][2] for k in ('E', 'R', 't', 'valid', 'n_inliers', 'hypothesis')}, 'inliers': dev['inliers'][off:off + cnts[2]]})
    assert out[0]['valid'] == 1 and len(out[0]['inliers']) == COUNTS[1]
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


def test_argument_errors_launch_nothing():
    from geoformer_amd import _lib
    h = _lib.lib()
    buf = torch.zeros(1 << 18, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()

    def call(N, iters, ws_bytes):
        return h.gf_pose_essential_ransac(p, p, p, N, 64, p, p, 0.5, iters, 1, p, p, p, p, p, p, p, p, ws_bytes, None)
    assert call(0, 256, 1 << 18) == -1 and b'need N' in h.gf_last_error()
    need = h.gf_pose_workspace_bytes(2, 256)
    assert 0 < need <= 1 << 18 and h.gf_pose_workspace_bytes(0, 256) == 0
    assert call(2, 256, need - 1) == -2 and b'workspace too small' in h.gf_last_error()


def test_device_recovers_the_planted_pose(five_pairs):
    scenes, mk0, mk1, counts = five_pairs
    dev = _device(mk0, mk1, counts)
    off = 0
    for n, cnt in enumerate(COUNTS):
        sc = scenes[n]
        if cnt >= 5:
            assert dev['valid'][n] == 1
            assert np.array_equal(dev['inliers'][off:off + cnt].astype(bool), ~sc['outlier'])
            assert dev['n_inliers'][n] == int((~sc['outlier']).sum())
            assert abs(np.linalg.norm(dev['E'][n]) - 1) < 1e-12 and abs(np.linalg.det(dev['R'][n]) - 1) < 1e-9
            assert abs(np.linalg.norm(dev['t'][n]) - 1) < 1e-12
            if cnt > 5:                 # (five matches alone fit every root of their own minimal problem: valid, 5 inliers, no more is known)
                re, te = P.pose_errors(dev['R'][n], dev['t'][n], sc['R'], sc['t'])
                print(f'pair {n} ({cnt} matches): R_err {re:.2e} t_err {te:.2e} deg')
                assert re < 0.05 and te < 0.05
        else:
            assert dev['valid'][n] == 0 and dev['n_inliers'][n] == 0 and not dev['inliers'][off:off + cnt].any()
            assert not dev['R'][n].any() and not dev['t'][n].any()
        off += cnt


def test_deterministic_seeded_nan_isolated_and_bad_iters(five_pairs):
    from geoformer_amd import _lib, ops
    scenes, mk0, mk1, counts = five_pairs
    a, b = _device(mk0, mk1, counts), _device(mk0, mk1, counts)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    c = _device(mk0, mk1, counts, seed=1234)
    assert tuple(c['hypothesis'][0]) != tuple(a['hypothesis'][0])
    # a NaN keypoint in pair 1: pairs 0, 2, 3, 4 keep their bits; pair 1 loses exactly that match
    bad = mk1.copy()
    victim = COUNTS[0] + int(np.flatnonzero(~scenes[1]['outlier'])[3])
    bad[victim, 1] = np.nan
    d = _device(mk0, bad, counts)
    for n in (0, 2, 3, 4):
        for k in ('E', 'R', 't', 'valid', 'n_inliers', 'hypothesis'):
            assert np.array_equal(a[k][n], d[k][n]), (n, k)
    keep = np.ones(len(mk0), bool)
    keep[COUNTS[0]:COUNTS[0] + COUNTS[1]] = False
    assert np.array_equal(a['inliers'][keep], d['inliers'][keep])
    want = ~scenes[1]['outlier']
    want[victim - COUNTS[0]] = False
    assert d['valid'][1] == 1 and np.array_equal(d['inliers'][COUNTS[0]:COUNTS[0] + COUNTS[1]].astype(bool), want)
    for iters in (0, 100, -32):
        with pytest.raises(_lib.GeoFormerHipError, match=r'\(-1\).*multiple of 32'):
            ops.ransac_essential(_t(mk0), _t(mk1), _t(counts, torch.int32), 5, _K(5), _K(5), iters=iters)


def _epi_reference(p0, p1, bids, T, K0, K1):
    """metrics.py:30-47 with E = [t]x R (:55-56) in numpy fp64, sums associated left to right as written."""
    T, K0, K1 = T[bids], K0[bids], K1[bids]
    t, R = T[:, :3, 3], T[:, :3, :3]
    E = np.stack([t[:, 1, None] * R[:, 2] - t[:, 2, None] * R[:, 1], t[:, 2, None] * R[:, 0] - t[:, 0, None] * R[:, 2],
                  t[:, 0, None] * R[:, 1] - t[:, 1, None] * R[:, 0]], 1)
    x0, y0 = (p0[:, 0] - K0[:, 0, 2]) / K0[:, 0, 0], (p0[:, 1] - K0[:, 1, 2]) / K0[:, 1, 1]
    x1, y1 = (p1[:, 0] - K1[:, 0, 2]) / K1[:, 0, 0], (p1[:, 1] - K1[:, 1, 2]) / K1[:, 1, 1]
    Ep0 = [(E[:, r, 0] * x0 + E[:, r, 1] * y0) + E[:, r, 2] for r in range(3)]
    Etp1 = [(E[:, 0, c] * x1 + E[:, 1, c] * y1) + E[:, 2, c] for c in range(2)]
    p1Ep0 = (x1 * Ep0[0] + y1 * Ep0[1]) + Ep0[2]
    return (p1Ep0 * p1Ep0) * (1.0 / (Ep0[0] * Ep0[0] + Ep0[1] * Ep0[1]) + 1.0 / (Etp1[0] * Etp1[0] + Etp1[1] * Etp1[1]))


def test_epipolar_errors_against_fp64_numpy():
    from geoformer_amd import ops
    sizes = (500, 300, 200)
    scenes = [P.scene(300 + i, n, 0.3) for i, n in enumerate(sizes)]
    p0 = np.concatenate([s['mk0'] for s in scenes])
    p1 = np.concatenate([s['mk1'] for s in scenes])
    outlier = np.concatenate([s['outlier'] for s in scenes])
    bids = np.repeat(np.arange(3), sizes)
    K0 = np.repeat(P.K[None], 3, 0).astype(np.float32)
    K1 = K0.copy()
    K1[:, 0, 0] = 510.0; K1[:, 1, 2] = 236.0                       # (only the formula is compared below for these intrinsics)
    T = np.stack([s['T_0to1'] for s in scenes]).astype(np.float32)
    for k1 in (K0, K1):
        got = ops.epipolar_errors(_t(p0), _t(p1), _t(bids, torch.int64), _t(T), _t(K0), _t(k1)).cpu().numpy()
        want = _epi_reference(p0.astype(np.float64), p1.astype(np.float64), bids, T.astype(np.float64), K0.astype(np.float64),
                              k1.astype(np.float64)).astype(np.float32)
        assert got.dtype == np.float32
        rel = np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), np.finfo(np.float32).tiny)
        print(f'worst relative difference to fp32(numpy fp64): {rel.max():.3e}')
        assert rel.max() <= 2.0 ** -23                              # the kernel computes in fp64 and rounds once
        if k1 is K0:
            assert (got[~outlier] < 5e-4).all() and (got[outlier] > 5e-4).all()


def test_compute_pose_errors_two_planted_pairs_and_an_empty_one():
    from geoformer_amd.train import metrics as MT
    scenes = [P.scene(400, 300, 0.3), P.scene(401, 200, 0.3)]
    data = {'mkpts0_f': _t(np.concatenate([s['mk0'] for s in scenes])), 'mkpts1_f': _t(np.concatenate([s['mk1'] for s in scenes])),
            'm_bids': _t(np.repeat([0, 1], [300, 200]), torch.int64), 'K0': _K(3), 'K1': _K(3),
            'T_0to1': _t(np.stack([scenes[0]['T_0to1'], scenes[1]['T_0to1'], np.eye(4)]))}
    MT.compute_pose_errors(data, {'ransac_pixel_thr': 0.5, 'ransac_conf': 0.99999})
    MT.compute_symmetrical_epipolar_errors(data)
    assert len(data['R_errs']) == len(data['t_errs']) == len(data['inliers']) == 3
    for b, sc in enumerate(scenes):
        print(f'pair {b}: R_err {data["R_errs"][b]:.2e} t_err {data["t_errs"][b]:.2e} deg')
        assert data['R_errs'][b] < 0.05 and data['t_errs'][b] < 0.05
        assert np.array_equal(data['inliers'][b], ~sc['outlier'])
    assert data['R_errs'][2] == np.inf and data['t_errs'][2] == np.inf and data['inliers'][2].shape == (0,)
    assert data['epi_errs'].shape == (500,) and data['epi_errs'].dtype == torch.float32


def test_estimate_relative_pose_front_end():
    from geoformer_amd import matcher
    sc = P.scene(402, 300, 0.3)
    R, t, mask = matcher.estimate_relative_pose(np.c_[sc['mk0'], sc['mk1']], P.K, P.K, thr=0.5)
    re, te = P.pose_errors(R, t, sc['R'], sc['t'])
    assert re < 0.05 and te < 0.05 and np.array_equal(mask, ~sc['outlier'])
    assert matcher.estimate_relative_pose(np.c_[sc['mk0'], sc['mk1']][:4], P.K, P.K) is None


def test_validation_step_on_a_synthetic_megadepth_batch():
    from geoformer_amd.model.cvpr_ds_config import get_default_cfg
    from geoformer_amd.model.full_model import GeoFormer
    from geoformer_amd.model.geo_config import get_cfg_model
    from geoformer_amd.train import ValidationStep, synthetic_megadepth_batch
    from geoformer_amd.weights import deterministic_init_
    gcfg = get_cfg_model()
    gcfg.update(precision='fp32')
    model = deterministic_init_(GeoFormer(get_default_cfg(), gcfg)).to(DEV)
    model.train()
    batch = synthetic_megadepth_batch(2, (96, 128), 5, device=DEV)
    out = ValidationStep(model)(batch)['metrics']
    assert model.training                                            # the step leaves the model's mode as it found it
    assert set(out) == {'identifiers', 'epi_errs', 'R_errs', 't_errs', 'inliers'}
    assert len(out['identifiers']) == len(set(out['identifiers'])) == 2
    assert all(len(out[k]) == 2 for k in out)
    assert sum(len(e) for e in out['epi_errs']) == len(batch['m_bids'])
    for b in range(2):
        n = int((batch['m_bids'] == b).sum())
        assert len(out['epi_errs'][b]) == n
        assert len(out['inliers'][b]) in (0, n)                      # empty without a pose, else one flag per match of the pair
        assert np.isinf(out['R_errs'][b]) == np.isinf(out['t_errs'][b]) == (len(out['inliers'][b]) == 0)
    agg = ValidationStep(model).aggregate([{'metrics': out}])
    assert set(agg) == {'auc@5', 'auc@10', 'auc@20', 'prec@5e-04'}


def test_train_entry_point_validates_after_training(capsys):
    """`--validate K`: after the steps, K batches through the validation step, one line with the four aggregated numbers."""
    import re
    from geoformer_amd.train import run
    run.main(['--steps', '1', '--batch', '2', '--size', '96', '128', '--validate', '2'])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('validation: ')]
    assert len(lines) == 1
    m = re.fullmatch(r'validation: auc@5 (\S+) auc@10 (\S+) auc@20 (\S+) prec@5e-04 (\S+)', lines[0])
    assert m and all(0.0 <= float(v) <= 1.0 for v in m.groups())
