"""Calibrated two-view verification on the GPU: gf_relpose_ransac / gf_relpose_ransac_lo (csrc/k_relpose.hip behind
ops.ransac_relative_pose) against the host build of the same rel_solver.h (csrc/host/relpose_host.cpp), bit for bit, and against
ops.ransac_essential where the two rules coincide.  Pairs: tests/relpose_cases.py."""
import numpy as np
import pytest
import torch

import relpose_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'
OUT = ('E', 'R', 't')


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def device(b, thr=1.0, iters=128, seed=0x5EED, refit=0, m=None, scores='batch', offsets=None, K0=None, K1=None):
    from geoformer_amd import ops
    offsets = b['offsets'] if offsets is None else offsets
    N = len(offsets) - 1
    sc = b['scores'] if isinstance(scores, str) else scores
    rs = ops.ransac_relative_pose(_t(b['m'] if m is None else m), None if sc is None else _t(sc), _t(offsets, torch.int32), N,
                                  _t(b['K0'] if K0 is None else K0), _t(b['K1'] if K1 is None else K1), pixel_thr=thr, sc_thres=C.SC_THRES,
                                  iters=iters, seed=seed, refit=refit)
    assert rs['E'].dtype == torch.float64 and rs['inliers'].dtype == torch.uint8 and rs['E'].shape == (N, 3, 3) and rs['t'].shape == (N, 3)
    assert ('rounds' in rs) == bool(refit)
    return {k: v.cpu().numpy() for k, v in rs.items()}


def assert_equals_host(dev, b, refit, **kw):
    off = b['offsets']
    for n, host in enumerate(C.host_batch(b, refit=refit, **kw)):
        assert host['status'] >= 0
        assert int(dev['valid'][n]) == host['valid'], n
        assert tuple(dev['hypothesis'][n]) == tuple(host['hyp']), n
        assert int(dev['n_inliers'][n]) == host['n_inliers'] and int(dev['n_cheiral'][n]) == host['n_cheiral'], n
        assert np.array_equal(dev['inliers'][off[n]:off[n + 1]].astype(bool), host['inliers']), n
        for k in OUT:
            assert np.array_equal(dev[k][n].view(np.int64), host[k].view(np.int64)), (n, k, np.abs(dev[k][n] - host[k]).max())
        if refit:
            assert int(dev['rounds'][n]) == host['rounds'], n


@pytest.fixture(scope='module')
def batches():
    return {False: C.batch(False), True: C.batch(True)}


@pytest.mark.parametrize('filtered', [False, True])
@pytest.mark.parametrize('refit', [0, 4])
@pytest.mark.parametrize('iters', [64, 128, 256])
def test_device_equals_host_build(batches, iters, refit, filtered):
    """F: eight pairs of sizes (0, 4, 5, 63, 64, 65, 129, 300) in one call, per-pair different anisotropic K0, K1: every output of every pair
    bit for bit"""
    b = batches[filtered]
    dev = device(b, iters=iters, refit=refit)
    assert_equals_host(dev, b, refit, iters=iters)
    assert list(dev['valid']) == ([0, 0, 0, 0, 0, 1, 1, 1] if filtered else [0, 0, 1, 1, 1, 1, 1, 1])
    assert not dev['inliers'][b['gone']].any()
    if refit:
        assert dev['rounds'].max() >= 1                   # the refit ran somewhere


def test_runs_repeat_and_pairs_do_not_see_their_neighbours(batches):
    """G: two calls give the same bits, another seed another hypothesis; the 300-row pair at index 2 of two different launches - one with
    an empty pair before it - gives the same bits; refit = 0 through the _lo entry is the plain entry"""
    b = batches[False]
    a1, a2 = device(b, refit=4), device(b, refit=4)
    for k in a1:
        assert np.array_equal(a1[k], a2[k]), k
    other = device(b, refit=4, seed=0x5EED + 1)
    assert not np.array_equal(other['hypothesis'][7], a1['hypothesis'][7])
    off = b['offsets']
    big, mid = b['m'][off[7]:off[8]], b['m'][off[6]:off[7]]
    K0, K1 = b['K0'][[5, 6, 7]], b['K1'][[5, 6, 7]]
    l1 = device(b, refit=4, scores=None, m=np.concatenate([mid, big]), offsets=np.array([0, 0, len(mid), len(mid) + len(big)], np.int32), K0=K0, K1=K1)
    l2 = device(b, refit=4, scores=None, m=np.concatenate([mid[:70], mid[:60], big]),
                offsets=np.array([0, 70, 130, 130 + len(big)], np.int32), K0=K0[[1, 0, 2]], K1=K1[[1, 0, 2]])
    assert l1['valid'][2] == 1 and l1['valid'][0] == 0
    for k in ('E', 'R', 't', 'valid', 'n_inliers', 'n_cheiral', 'hypothesis', 'rounds'):
        assert np.array_equal(l1[k][2], l2[k][2]), k
    assert np.array_equal(l1['inliers'][len(mid):], l2['inliers'][130:])
    # the _lo entry with refit_rounds = 0
    from geoformer_amd import _lib
    plain = device(b)
    h = _lib.lib()
    N, M = 8, len(b['m'])
    m, o, k0, k1 = _t(b['m']), _t(off, torch.int32), _t(b['K0']), _t(b['K1'])
    E, R = torch.empty(N, 9, dtype=torch.float64, device=DEV), torch.empty(N, 9, dtype=torch.float64, device=DEV)
    t = torch.empty(N, 3, dtype=torch.float64, device=DEV)
    ints = torch.full((6, N), 7, dtype=torch.int32, device=DEV)
    inl = torch.zeros(M, dtype=torch.uint8, device=DEV)
    ws = torch.empty(h.gf_relpose_lo_workspace_bytes(N, M, 128), dtype=torch.uint8, device=DEV)
    rc = h.gf_relpose_ransac_lo(m.data_ptr(), None, o.data_ptr(), N, M, k0.data_ptr(), k1.data_ptr(), C.SC_THRES, 1.0, 128, 0x5EED, E.data_ptr(),
                                R.data_ptr(), t.data_ptr(), ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(), ints[3].data_ptr(),
                                inl.data_ptr(), 0, ints[5].data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc == 0, h.gf_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(E.cpu().numpy().reshape(N, 3, 3), plain['E']) and np.array_equal(R.cpu().numpy().reshape(N, 3, 3), plain['R'])
    assert np.array_equal(t.cpu().numpy(), plain['t']) and np.array_equal(inl.cpu().numpy(), plain['inliers'])
    assert np.array_equal(ints[0].cpu().numpy(), plain['valid']) and np.array_equal(ints[1].cpu().numpy(), plain['n_inliers'])
    assert np.array_equal(ints[2].cpu().numpy(), plain['n_cheiral']) and not ints[5].cpu().numpy().any()
    assert np.array_equal(torch.stack([ints[3], ints[4]]).cpu().numpy().reshape(-1)[:2 * N].reshape(N, 2), plain['hypothesis'])


def test_equals_ransac_essential_where_the_rules_coincide(batches):
    """H: no filtered row, refit = 0: E, R, t, valid, n_inliers, hypothesis and the mask of ops.ransac_essential, bit for bit"""
    from geoformer_amd import ops
    b = batches[False]
    off = b['offsets']
    counts = np.concatenate([[off[-1]], np.diff(off)]).astype(np.int32)
    for iters, thr in ((64, 1.0), (256, 0.5)):
        new = device(b, thr=thr, iters=iters, seed=99)
        old = ops.ransac_essential(_t(b['m'][:, :2]), _t(b['m'][:, 2:]), _t(counts, torch.int32), 8, _t(b['K0']), _t(b['K1']), pixel_thr=thr,
                                   iters=iters, seed=99)
        for k in ('E', 'R', 't', 'valid', 'n_inliers', 'hypothesis', 'inliers'):
            assert np.array_equal(new[k], old[k].cpu().numpy()), k
        assert list(new['valid']) == [0, 0, 1, 1, 1, 1, 1, 1]


def test_argument_errors(batches):
    """I"""
    from geoformer_amd import _lib, ops
    b = batches[False]
    m, off, k = _t(b['m']), _t(b['offsets'], torch.int32), _t(b['K0'])
    for iters in (0, 100, -64, 32, 96):
        for refit in (0, 2):
            with pytest.raises(_lib.GeoFormerHipError, match=r'\(-1\).*multiple of 64'):
                ops.ransac_relative_pose(m, None, off, 8, k, k, iters=iters, refit=refit)
    for thr in (0.0, float('inf')):
        with pytest.raises(_lib.GeoFormerHipError, match=r'\(-1\).*pixel_thr'):
            ops.ransac_relative_pose(m, None, off, 8, k, k, pixel_thr=thr)
    with pytest.raises(_lib.GeoFormerHipError, match=r'\(-1\).*refit_rounds'):
        ops.ransac_relative_pose(m, None, off, 8, k, k, refit=9)
    h = _lib.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()

    def plain(matches=p, N=1, ws=4096):
        return h.gf_relpose_ransac(matches, None, p, N, 50, p, p, 0.25, 1.0, 256, 1, p, p, p, p, p, p, p, p, p, ws, None)

    def lo(rounds=p, N=1, ws=4096, refit=2):
        return h.gf_relpose_ransac_lo(p, None, p, N, 50, p, p, 0.25, 1.0, 256, 1, p, p, p, p, p, p, p, p, refit, rounds, p, ws, None)
    assert plain(matches=None) == -1 and b'gf_relpose_ransac: null pointer' in h.gf_last_error()
    assert lo(rounds=None) == -1 and b'gf_relpose_ransac_lo: null pointer' in h.gf_last_error()
    assert plain(N=0) == -1 and b'N out of range' in h.gf_last_error()
    assert plain(N=3000000) == -1 and b'N out of range' in h.gf_last_error()          # 3e6 * 256 / 32 > 2^24 (and fine for a 64-wide tile)
    assert lo(N=0) == -1 and lo(N=3000000) == -1 and b'N * (iters / 32)' in h.gf_last_error()
    assert plain(ws=16) == -2 and b'workspace too small' in h.gf_last_error()
    assert lo(ws=16) == -2 and lo(refit=-1) == -1 and b'refit_rounds' in h.gf_last_error()
    assert h.gf_relpose_workspace_bytes(1, 50, 256) > 50 * 4 + 8 * 9 * 8
    assert h.gf_relpose_lo_workspace_bytes(1, 50, 256) >= h.gf_relpose_workspace_bytes(1, 50, 256) + 100
    assert h.gf_relpose_workspace_bytes(0, 50, 256) == 0 and h.gf_relpose_lo_workspace_bytes(0, 50, 256) == 0
