"""The homography-pair generator on the GPU: gf_image_warp_resize (csrc/k_homo_pair.hip behind ops.image_warp_resize) against the host
path matcher.cv2_resize_linear_u8(homo_data.cv2_warp_perspective_u8(cv2_gray_u8(src), M, w, h), wt, ht), which
tests/test_homo_data_cpu.py pins; HomoPairs' two preprocess modes against each other; the training entry point on a directory.
Integer byte work on fp64 positions that host and device round identically: the bound everywhere is ZERO differing bytes / bits."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import homo_cases as C

pytestmark = pytest.mark.gpu

DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (ht, wt) for the 37 x 53 source: reduce, enlarge, same size (53 is no multiple of 4 either), a width that is no multiple of 4
TARGETS = [(24, 32), (40, 56), (37, 53), (26, 35)]


def host_path(src, M, wt, ht, warp_size=None, bc=None):
    from geoformer_amd import matcher as MT
    from geoformer_amd.train import homo_data as D
    gray = MT.cv2_gray_u8(src) if src.ndim == 3 else src
    w, h = warp_size or (gray.shape[1], gray.shape[0])
    im = MT.cv2_resize_linear_u8(D.cv2_warp_perspective_u8(gray, M, w, h), wt, ht)
    return im if bc is None else D.brightness_contrast_u8(im, *bc)


def device_u8(d_src, M, wt, ht, **kw):
    from geoformer_amd import ops
    return ops.image_warp_resize(d_src, M, wt, ht, normalised=False, **kw).cpu().numpy()


def source(kind, h=C.H37, w=C.W53):
    """numpy source and the device tensor that holds it: gray, RGB, RGB inside rows 21 bytes longer than w * 3."""
    if kind == 'gray':
        src = C.smooth_noisy(h, w)
        return src, torch.from_numpy(src).to(DEV)
    src = C.textured_rgb(h, w, 9)
    if kind == 'rgb':
        return src, torch.from_numpy(src).to(DEV)
    wide = torch.full((h, w + 7, 3), 255, dtype=torch.uint8, device=DEV)
    wide[:, :w] = torch.from_numpy(src).to(DEV)
    d = wide[:, :w]
    assert d.stride(0) == (w + 7) * 3
    return src, d


@pytest.mark.parametrize('kind', ['gray', 'rgb', 'rgb_strided'])
def test_kernel_equals_host_path(kind):
    src, d = source(kind)
    for ht, wt in TARGETS:
        for name, M in C.NAMED.items():
            got, want = device_u8(d, M, wt, ht), host_path(src, M, wt, ht)
            assert got.shape == want.shape == (ht, wt)
            assert np.array_equal(got, want), f'{kind} {name} -> {ht} x {wt}: {(got != want).sum()} bytes differ'
    assert host_path(src, C.M_NEGATIVE, 53, 37)[:, 3].any() and not host_path(src, C.M_OUTSIDE, 32, 24).any()


@pytest.mark.parametrize('kind', ['gray', 'rgb'])
def test_exact_2x_branch_and_more_than_one_block(kind):
    """48 x 64 -> 24 x 32 takes the (a + b + c + d + 2) >> 2 branch over four warped pixels; 300 x 1100 at the same size spans five
    blocks across (256 output pixels each) and 75 down, with a ragged last block."""
    src, d = source(kind, 48, 64)
    for name, M in C.NAMED.items():
        assert np.array_equal(device_u8(d, M, 32, 24), host_path(src, M, 32, 24)), name
    src, d = source(kind, 300, 1100)
    M = np.array([[0.95, 0.05, 12.], [-0.03, 1.02, -7.], [4e-5, -6e-5, 1.]])
    assert np.array_equal(device_u8(d, M, 1100, 300), host_path(src, M, 1100, 300))
    assert np.array_equal(device_u8(d, M, 1027, 290), host_path(src, M, 1027, 290))


def test_warp_size_other_than_the_source():
    src, d = source('rgb')
    for warp_size, (ht, wt) in (((41, 29), (24, 32)), ((64, 48), (24, 32)), ((32, 24), (24, 32))):
        got = device_u8(d, C.M_PERSPECTIVE, wt, ht, warp_size=warp_size)
        assert np.array_equal(got, host_path(src, C.M_PERSPECTIVE, wt, ht, warp_size=warp_size)), warp_size


def test_output_kinds():
    from geoformer_amd import ops
    src, d = source('rgb')
    u8 = torch.from_numpy(host_path(src, C.M_PERSPECTIVE, 32, 24))
    assert u8.unique().numel() > 100
    quotient = ops.image_warp_resize(d, C.M_PERSPECTIVE, 32, 24)
    assert quotient.shape == (1, 1, 24, 32) and quotient.dtype == torch.float32
    assert torch.equal(quotient.cpu()[0, 0], u8.float() / 255.0)                                   # the correctly rounded quotient
    product = ops.image_warp_resize(d, C.M_PERSPECTIVE, 32, 24, reciprocal=True)
    assert torch.equal(product.cpu()[0, 0], u8.float() * torch.tensor(1.0 / 255.0, dtype=torch.float32))
    # the identity at the source's size is gf_image_gray_resize's path
    assert torch.equal(ops.image_warp_resize(d, np.eye(3), 32, 24), ops.image_gray_resize(d, 32, 24))


@pytest.mark.parametrize('bc', [(1.3, 0.0), (1.0, -0.2), (0.7, 0.0), (1.0, 0.2)])
def test_brightness_contrast_in_the_same_launch(bc):
    from geoformer_amd import ops
    src, d = source('rgb')
    for M in (C.M_PERSPECTIVE, C.M_IDENTITY):                 # the warp kernel and the identity path apply it identically
        for ht, wt in ((24, 32), (37, 53)):
            want = host_path(src, M, wt, ht, bc=bc)
            assert not np.array_equal(want, host_path(src, M, wt, ht))
            assert np.array_equal(device_u8(d, M, wt, ht, brightness_contrast=bc), want)
            f = ops.image_warp_resize(d, M, wt, ht, brightness_contrast=bc).cpu()[0, 0]
            assert torch.equal(f, torch.from_numpy(want).float() / 255.0)


def test_writes_one_slice_of_a_batch_and_nothing_else():
    from geoformer_amd import ops
    src, d = source('gray')
    for ht, wt in ((24, 32), (26, 35)):                       # 35: the slice starts at an address no 16-byte store may assume
        batch = torch.full((3, 1, ht, wt), -7.0, device=DEV)
        r = ops.image_warp_resize(d, C.M_PERSPECTIVE, wt, ht, out=batch[1])
        assert r.data_ptr() == batch[1].data_ptr()
        assert torch.equal(batch[1, 0].cpu(), torch.from_numpy(host_path(src, C.M_PERSPECTIVE, wt, ht)).float() / 255.0)
        assert (batch[0] == -7.0).all() and (batch[2] == -7.0).all()
        b8 = torch.full((3, 1, ht, wt), 99, dtype=torch.uint8, device=DEV)
        ops.image_warp_resize(d, C.M_PERSPECTIVE, wt, ht, out=b8[1], normalised=False)
        assert np.array_equal(b8[1, 0].cpu().numpy(), host_path(src, C.M_PERSPECTIVE, wt, ht))
        assert (b8[0] == 99).all() and (b8[2] == 99).all()


def test_bad_arguments_are_errors_not_faults():
    import ctypes
    from geoformer_amd import _lib, ops
    _, d = source('gray')
    nan = np.eye(3)
    nan[1, 1] = np.nan
    for M in (nan, np.zeros((3, 3)), np.array([[1., 2., 3.], [2., 4., 6.], [0., 0., 1.]]), np.eye(4)):
        with pytest.raises(ValueError):
            ops.image_warp_resize(d, M, 32, 24)
    for kw in ({'wt': 0, 'ht': 24}, {'wt': 32, 'ht': 0}, {'wt': 32, 'ht': 24, 'warp_size': (0, 5)}):
        with pytest.raises(ValueError):
            ops.image_warp_resize(d, np.eye(3), **kw)
    with pytest.raises(ValueError):
        ops.image_warp_resize(d, np.eye(3), 32, 24, brightness_contrast=(float('nan'), 0.0))
    with pytest.raises(ValueError):
        ops.image_warp_resize(d, np.eye(3), 32, 24, out=torch.empty(24, 33, device=DEV))
    with pytest.raises(ValueError):
        ops.image_warp_resize(d.float(), np.eye(3), 32, 24)
    # the C entry itself answers with a status code
    h = _lib.lib()
    out = torch.empty(24, 32, dtype=torch.uint8, device=DEV)
    eye = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    bad = (ctypes.c_double * 9)(1, 0, 0, 0, float('inf'), 0, 0, 0, 1)
    p, q = ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(out.data_ptr())

    def call(minv=eye, hs=37, ws=53, stride=53, hw=37, ww=53, ht=24, wt=32, kind=0, ch=1, bc=None):
        return h.gf_image_warp_resize(p, ch, hs, ws, stride, minv, hw, ww, q, kind, ht, wt, bc, None)
    assert call(minv=bad) == -1 and b'non-finite' in h.gf_last_error()
    assert call(minv=None) == -1 and call(ht=0) == -1 and call(wt=0) == -1 and call(hw=0) == -1 and call(ww=-3) == -1 and call(hs=0) == -1
    assert call(stride=52) == -1 and call(kind=3) == -1 and call(ch=2) == -1
    assert call(bc=(ctypes.c_float * 2)(float('nan'), 0)) == -1
    torch.cuda.synchronize()


SHAPES = [(96, 128), (128, 96), (120, 160), (128, 96), (192, 256), (90, 120)]      # portrait and landscape; copy, exact 2x, reduce, enlarge


@pytest.fixture(scope='module')
def image_dir(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('homo_gpu'))
    return root, C.make_image_dir(root, SHAPES)


def test_homopairs_device_equals_host(image_dir):
    from geoformer_amd.train.homo_data import HomoPairs
    root, _ = image_dir
    dev, host = (HomoPairs(root, size=(96, 128), seed=3, device=DEV, preprocess=p) for p in ('device', 'host'))
    assert len(dev) == 6
    seen, augmented = set(), 0
    for epoch in range(2):
        lists = list(dev.batches(2, epoch))
        assert lists == list(host.batches(2, epoch)) and sorted(i for b in lists for i in b) == list(range(6))
        for indices in lists:
            assert len({dev.target_hw(i) for i in indices}) == 1
            a, b = dev.batch(indices, epoch), host.batch(indices, epoch)
            assert set(a) == set(b) == {'image0', 'image1', 'H_0to1', 'H_1to0', 'is_negs', 'dataset_name', 'pair_id', 'pair_names'}
            for k in a:
                if torch.is_tensor(a[k]):
                    assert a[k].device.type == 'cuda' and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (k, indices, epoch)
                else:
                    assert a[k] == b[k], k
            assert a['image0'].shape == (len(indices), 1, *dev.target_hw(indices[0])) and a['image0'].max() <= 1.0 and a['image1'].std() > 0.02
            seen.add(dev.target_hw(indices[0]))
            augmented += sum(dev.sample(i, epoch)[k] is not None for i in indices for k in ('aug_orig', 'aug_warp'))
    assert seen == {(96, 128), (96, 64)} and augmented > 0
    with pytest.raises(ValueError, match='different target shapes'):
        dev.batch([0, 1])


def test_train_run_on_an_image_directory(image_dir):
    """`python -m geoformer_amd.train.run --data DIR` in a child process: two steps at 96 x 128, a finite loss, the files' names."""
    root, paths = image_dir
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE')}
    r = subprocess.run([sys.executable, '-m', 'geoformer_amd.train.run', '--steps', '2', '--batch', '2', '--size', '96', '128', '--coarse-thr', '0.0',
                        '--data', root, '--data-seed', '1'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('step')]
    assert len(lines) == 2, r.stdout
    names = {os.path.basename(p) + '_0' for p in paths}
    for ln in lines:
        assert np.isfinite(float(ln.split()[3])), ln
        got = ln.split(' pairs ')[1].split(',')
        assert len(got) == 2 and set(got) <= names, ln
