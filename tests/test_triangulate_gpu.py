"""Triangulation on the GPU: gf_triangulate (csrc/k_triangulate.hip behind ops.triangulate_tracks) against the host build of the same
tri_solver.h (csrc/host/tri_host.cpp), every output bit for bit.  Cameras and tracks: tests/triangulate_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

import triangulate_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'
N_CAMERAS = 44
# hypotheses per track: 2 -> 1, 3 -> 3, 4 -> 6, 11 -> 55, 12 and longer -> 64
LENGTH_SETS = {
    'mixed': [2, 3, 11, 12, 13, 40],                 # 251 slots: every pair up to 11, draws from 12 on
    'slots_63': [11, 4, 2, 2],                       # one slot short of a wave
    'slots_64': [11, 4, 2, 2, 2],                    # a wave exactly
    'slots_65': [11, 4, 2, 2, 2, 2],                 # one slot into the second wave
    'one_track': [5],
    'many_blocks': ([2, 3, 2, 5, 2, 4, 3, 12] * 80)[:601],      # three blocks of 256 tracks, the last with 89: the two-level slot search
}


@pytest.fixture(scope='module')
def cams():
    return C.make_cameras(N_CAMERAS, 31)


def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def device(tr_off, img, uv, K, R, t, **kw):
    from geoformer_amd import ops
    rs = ops.triangulate_tracks(_t(tr_off, torch.int32), _t(img, torch.int32), _t(np.asarray(uv, np.float32).reshape(-1, 2), torch.float32),
                                _t(K, torch.float32), _t(R, torch.float64), _t(t, torch.float64), **kw)
    T = len(tr_off) - 1
    assert rs['X'].dtype == torch.float64 and rs['X'].shape == (T, 3) and rs['inliers'].dtype == torch.uint8 and rs['err2'].dtype == torch.float64
    return {k: v.cpu().numpy() for k, v in rs.items()}


def assert_bits(a, b, what=''):
    for k in C.OUT_KEYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), (what, k, np.flatnonzero(np.atleast_1d(a[k] != b[k]).reshape(len(a[k]), -1).any(1))[:8])


def spoiled(K, R, t, tr):
    """the planted tracks with every special kind among them: a conflict, a pose-less image, one effective observation, a NaN pixel"""
    img, uv = tr['obs_image'].copy(), tr['obs_uv'].copy()
    off = tr['track_off']
    Rn = R.copy()
    Rn[N_CAMERAS - 1] = np.nan                                           # the last camera has no pose
    T = len(off) - 1
    if T >= 4:
        img[off[1] + 1] = img[off[1]]                                    # track 1: an image twice
        img[off[2]] = N_CAMERAS - 1 if off[3] - off[2] == 2 else img[off[2]]      # a length-2 track 2 keeps one effective observation
        uv[off[3], 0] = np.nan                                           # track 3: a NaN pixel
    return img, uv, Rn


@pytest.mark.parametrize('refit', [0, 1, 4])
@pytest.mark.parametrize('name', list(LENGTH_SETS))
def test_device_equals_host_build(cams, name, refit):
    K, R, t = cams
    tr = C.planted_tracks(K, R, t, LENGTH_SETS[name], seed=40, noise=0.5, outlier_frac=0.2)
    kw = dict(pixel_thr=4.0, min_angle_deg=1.5, min_obs=2, refit=refit)
    rc, host = C.host_triangulate(tr['track_off'], tr['obs_image'], tr['obs_uv'], K, R, t, **kw)
    assert rc == 0
    dev = device(tr['track_off'], tr['obs_image'], tr['obs_uv'], K, R, t, **kw)
    assert_bits(dev, host, name)
    assert host['valid'].sum() >= 0.9 * len(host['valid']) and (refit == 0) == (host['rounds'].max() == 0)
    if name == 'mixed':                                                  # outlier observations are planted from length 5 up and left out
        assert np.array_equal(host['inliers'].astype(bool), tr['planted'])
    assert_bits(device(tr['track_off'], tr['obs_image'], tr['obs_uv'], K, R, t, **kw), dev, 'second run')


@pytest.mark.parametrize('min_obs', [2, 3])
def test_conflict_poseless_short_and_nan_tracks(cams, min_obs):
    K, R, t = cams
    for name in ('mixed', 'many_blocks'):
        lengths = [3, 3, 2, 3] + LENGTH_SETS[name]
        tr = C.planted_tracks(K, R, t, lengths, seed=41, noise=0.5, outlier_frac=0.2)
        img, uv, Rn = spoiled(K, R, t, tr)
        rc, host = C.host_triangulate(tr['track_off'], img, uv, K, Rn, t, refit=2, min_obs=min_obs)
        dev = device(tr['track_off'], img, uv, K, Rn, t, refit=2, min_obs=min_obs)
        assert rc == 0
        assert_bits(dev, host, name)
        assert dev['conflict'][:4].tolist() == [0, 1, 0, 0] and dev['conflict'].sum() == 1
        assert dev['valid'][1] == 0 and dev['hypothesis'][1] == -1 and dev['valid'][2] == 0 and dev['hypothesis'][2] == -1
        assert dev['valid'][3] == (min_obs == 2) and dev['n_inliers'][3] == 2 and dev['hypothesis'][3] == 2      # the pair without the NaN pixel
        assert np.all(dev['X'][dev['valid'] == 0] == 0)
        bad = np.repeat(dev['valid'] == 0, np.diff(tr['track_off']))
        assert not dev['inliers'][bad].any() and not dev['inliers'][img == N_CAMERAS - 1].any()


def test_zero_tracks(cams):
    K, R, t = cams
    dev = device(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros((0, 2), np.float32), K, R, t)
    assert all(len(dev[k]) == 0 for k in C.OUT_KEYS)


def test_another_launch_position_changes_only_drawn_tracks(cams):
    K, R, t = cams
    lengths = LENGTH_SETS['mixed'] + LENGTH_SETS['slots_65']
    tr = C.planted_tracks(K, R, t, lengths, seed=42, noise=0.5, outlier_frac=0.2)
    off = tr['track_off']
    order = np.arange(len(lengths))[::-1]
    seg = [np.arange(off[k], off[k + 1]) for k in order]
    perm = np.concatenate(seg)
    off2 = np.concatenate([[0], np.cumsum([len(s) for s in seg])]).astype(np.int32)
    a = device(off, tr['obs_image'], tr['obs_uv'], K, R, t, refit=2)
    b = device(off2, tr['obs_image'][perm], tr['obs_uv'][perm], K, R, t, refit=2)
    rc, host = C.host_triangulate(off2, tr['obs_image'][perm], tr['obs_uv'][perm], K, R, t, refit=2)
    assert_bits(b, host)
    for j, k in enumerate(order):
        if lengths[k] >= 12:                                             # the draw is keyed by the track index
            continue
        for key in ('X', 'valid', 'conflict', 'n_inliers', 'hypothesis', 'rounds', 'err2'):
            assert a[key][k].tobytes() == b[key][j].tobytes(), (key, k)
        assert np.array_equal(a['inliers'][off[k]:off[k + 1]], b['inliers'][off2[j]:off2[j + 1]])


def test_argument_errors_come_back_as_status_codes():
    from geoformer_amd import _lib
    h = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(T=1, n_obs=2, n_images=2, thr=4.0, cosm=0.9996, min_obs=2, refit=0, ws=p, ws_bytes=1 << 20, first=p):
        return h.gf_triangulate(first, T, n_obs, p, p, p, p, p, n_images, thr, cosm, min_obs, refit, 1, p, p, p, p, p, p, p, p, ws, ws_bytes, None)
    for kw, word in ((dict(T=-1), b'T'), (dict(T=1 << 25), b'2^31'), (dict(n_obs=-1), b'n_obs'), (dict(thr=0.0), b'pixel_thr'),
                     (dict(thr=float('inf')), b'pixel_thr'), (dict(cosm=float('nan')), b'cos_min_angle'), (dict(min_obs=1), b'min_obs'),
                     (dict(refit=-1), b'refit'), (dict(refit=9), b'refit'), (dict(first=None), b'null pointer'), (dict(n_images=0), b'no images'),
                     (dict(n_obs=0), b'no observations')):
        assert call(**kw) == -1 and b'gf_triangulate' in h.gf_last_error() and word in h.gf_last_error(), (kw, h.gf_last_error())
    assert call(ws=None) == -2 and call(ws_bytes=16) == -2 and b'workspace' in h.gf_last_error()
    assert h.gf_triangulate_workspace_bytes(0, 4) == 0 and h.gf_triangulate_workspace_bytes(1000, 16) >= 1000 * (3 * 4 + 8) + 16 * 28
    assert call(T=0, first=None) == 0                                    # no tracks: nothing is read, nothing is launched
