"""Device-side image preprocessing (csrc/k_image_pre.hip behind ops.image_gray_resize and preprocess='device') against the host
restatement `MT.cv2_resize_linear_u8(MT.cv2_gray_u8(rgb), wt, ht)`, which tests/test_matcher_cpu.py pins by hand-derived vectors.
The arithmetic is integer byte work, so the bound everywhere is ZERO differing bytes / bits."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _host(src, wt, ht):
    from geoformer_amd import matcher as MT
    return MT.cv2_resize_linear_u8(MT.cv2_gray_u8(src) if src.ndim == 3 else src, wt, ht)


def _device_u8(src, wt, ht):
    from geoformer_amd import ops
    return ops.image_gray_resize(torch.from_numpy(src).to(DEV), wt, ht, normalised=False).cpu().numpy()


def _content(kind, h, w, ch, seed=0):
    rng = np.random.default_rng(seed)
    shape = (h, w, 3) if ch == 3 else (h, w)
    if kind == 'random':
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == 'zeros':
        return np.zeros(shape, np.uint8)
    if kind == 'full':
        return np.full(shape, 255, np.uint8)
    if kind == 'hramp':
        g = np.broadcast_to(np.round(np.linspace(0, 255, w)).astype(np.uint8)[None, :], (h, w))
    elif kind == 'vramp':
        g = np.broadcast_to(np.round(np.linspace(0, 255, h)).astype(np.uint8)[:, None], (h, w))
    elif kind == 'checker':
        g = (((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255).astype(np.uint8)
    else:
        raise KeyError(kind)
    if ch == 1:
        return g.copy()
    # colour: the three channels differ, so a swapped coefficient order shows
    return np.ascontiguousarray(np.stack([g, 255 - g, np.roll(g, 1, axis=1)], axis=-1))


# (source h, source w) -> (target h, target w)
SHAPES = [
    ((768, 1024), (480, 640)), ((1200, 1600), (480, 640)), ((600, 800), (480, 640)),            # non-integer downscale
    ((240, 320), (480, 640)), ((2, 2), (8, 8)), ((3, 5), (16, 24)),                              # upscale
    ((960, 1280), (480, 640)), ((480, 640), (240, 320)), ((6, 10), (3, 5)),                      # exact 2x both ways: the area form
    ((480, 640), (480, 320)), ((480, 640), (240, 640)),                                          # 2x one way only: generic
    ((480, 640), (480, 640)), ((7, 13), (7, 13)),                                                # same size
    ((16, 2000), (8, 640)), ((2000, 16), (640, 8)),                                              # extreme aspect ratios
    ((479, 641), (240, 320)), ((479, 641), (239, 321)), ((479, 641), (480, 640)),                # odd source (and target) sizes
    ((37, 53), (1, 1)), ((37, 53), (5, 3)), ((1, 1), (8, 8)), ((64, 64), (63, 2)),               # tiny / non-multiple-of-4 targets
]
CONTENTS = ['random', 'zeros', 'full', 'hramp', 'vramp', 'checker']


def _sid(s):
    return f'{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}'


@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_uint8_rgb_matches_host(shape, content):
    (hs, ws), (ht, wt) = shape
    src = _content(content, hs, ws, 3, seed=hs * 7 + ws)
    got, want = _device_u8(src, wt, ht), _host(src, wt, ht)
    assert got.shape == want.shape == (ht, wt) and got.dtype == np.uint8
    assert int((got != want).sum()) == 0, f'{int((got != want).sum())} differing bytes'


@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_uint8_single_channel_matches_host(shape, content):
    (hs, ws), (ht, wt) = shape
    src = _content(content, hs, ws, 1, seed=hs * 5 + ws)
    got, want = _device_u8(src, wt, ht), _host(src, wt, ht)
    assert int((got != want).sum()) == 0, f'{int((got != want).sum())} differing bytes'


@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_uint8_padded_row_stride(shape):
    """A crop of a wider / taller tensor: rows are further apart than W * channels bytes and nothing outside the crop is read into
    the result (the surroundings hold other values)."""
    from geoformer_amd import ops
    (hs, ws), (ht, wt) = shape
    rng = np.random.default_rng(hs + 3 * ws)
    for ch in (3, 1):
        wide = rng.integers(0, 256, (hs + 5, ws + 37) + ((3,) if ch == 3 else ()), dtype=np.uint8)
        crop = wide[2:2 + hs, 11:11 + ws]
        d = torch.from_numpy(wide).to(DEV)[2:2 + hs, 11:11 + ws]
        assert not d.is_contiguous() or hs == 1
        got = ops.image_gray_resize(d, wt, ht, normalised=False).cpu().numpy()
        want = _host(np.ascontiguousarray(crop), wt, ht)
        assert int((got != want).sum()) == 0, (ch, int((got != want).sum()))


@pytest.mark.parametrize('ssize', [1000, 777])
def test_coefficients_every_destination_size(ssize):
    """The device's coefficient arithmetic, indirectly: a one-row and a one-column image resized to every destination width /
    height in 8 .. 1024 step 8.  (d + 0.5) * scale - 0.5 contracted into a fused multiply-add moves single weights by one unit
    for some (size, position) pairs - a steep ramp and random bytes turn that into differing output bytes."""
    rng = np.random.default_rng(ssize)
    lines = [rng.integers(0, 256, ssize, dtype=np.uint8), ((np.arange(ssize) * 37) % 256).astype(np.uint8),
             ((np.arange(ssize) & 1) * 255).astype(np.uint8)]
    bad = []
    for dsize in range(8, 1025, 8):
        for k, line in enumerate(lines):
            row, col = np.ascontiguousarray(line[None, :]), np.ascontiguousarray(line[:, None])
            for src, wt, ht in ((row, dsize, 1), (col, 1, dsize)):
                diff = int((_device_u8(src, wt, ht) != _host(src, wt, ht)).sum())
                if diff:
                    bad.append((src.shape, (ht, wt), k, diff))
            rgb = np.ascontiguousarray(np.stack([line, line[::-1], np.roll(line, 3)], -1)[None])       # [1, ssize, 3]
            diff = int((_device_u8(rgb, dsize, 1) != _host(rgb, dsize, 1)).sum())
            if diff:
                bad.append((rgb.shape, (1, dsize), k, diff))
    assert not bad, f'{len(bad)} (source, target) cases with differing bytes, first: {bad[:5]}'


def _want_f32(u8, device='cpu'):
    """The normalised tensor as torch computes it.  On the CPU `/ 255.0` is the correctly rounded fp32 division.  On the device torch
    turns a Python-scalar divisor into a multiplication by fp32(1 / 255) - 126 of the 256 byte values come out one unit in the last
    place away from the quotient - and that is what the matcher's host path (load_gray_scale_tensor: the uint8 image goes to the
    device as fp32 and is divided there) hands the model.  image_gray_resize has both: reciprocal=False / True."""
    return torch.from_numpy(u8).to(device=device, dtype=torch.float32)[None, None] / 255.0


@pytest.mark.parametrize('where', ['cpu', DEV])
@pytest.mark.parametrize('shape', [((768, 1024), (480, 640)), ((480, 640), (240, 320)), ((480, 640), (480, 640)), ((479, 641), (239, 321)),
                                   ((1, 256), (1, 256))], ids=_sid)
def test_fp32_output_bitwise(shape, where):
    """fp32 output against torch.from_numpy(u8).to(torch.float32)[None, None] / 255.0, torch.equal on the int32 view: as torch
    evaluates it on the CPU (reciprocal=False) and as torch evaluates it on the device (reciprocal=True, what the matcher uses)."""
    from geoformer_amd import ops
    (hs, ws), (ht, wt) = shape
    if hs == 1:
        src = np.arange(256, dtype=np.uint8)[None, :]                     # every byte value once
    else:
        src = _content('random', hs, ws, 3, seed=5)
    u8 = _host(src, wt, ht)
    got = ops.image_gray_resize(torch.from_numpy(src).to(DEV), wt, ht, reciprocal=(where != 'cpu'))
    want = _want_f32(u8, where)
    assert got.shape == want.shape == (1, 1, ht, wt) and got.dtype == torch.float32 and got.is_contiguous()
    got = got.to(want.device)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), \
        f'{int((got.view(torch.int32) != want.view(torch.int32)).sum())} differing fp32 words'


def test_out_slices_of_a_batch():
    from geoformer_amd import ops
    ht, wt = 96, 136
    sizes = [(200, 300), (192, 272), (96, 136), (333, 517), (50, 70)]
    rng = np.random.default_rng(11)
    srcs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    for normalised, recip, dtype, fill in ((True, False, torch.float32, -7.0), (True, True, torch.float32, -7.0), (False, False, torch.uint8, 171)):
        batch = torch.full((len(sizes) + 2, 1, ht, wt), fill, dtype=dtype, device=DEV)
        for i, s in enumerate(srcs):
            r = ops.image_gray_resize(torch.from_numpy(s).to(DEV), wt, ht, out=batch[i + 1], normalised=normalised, reciprocal=recip)
            assert r.data_ptr() == batch[i + 1].data_ptr()
        assert bool((batch[0] == fill).all()) and bool((batch[-1] == fill).all())          # bytes outside the slices untouched
        for i, s in enumerate(srcs):
            single = ops.image_gray_resize(torch.from_numpy(s).to(DEV), wt, ht, normalised=normalised, reciprocal=recip)
            assert torch.equal(batch[i + 1].reshape(ht, wt), single.reshape(ht, wt)), i
            want = _want_f32(_host(s, wt, ht), DEV if recip else 'cpu').reshape(ht, wt).cpu().numpy() if normalised else _host(s, wt, ht)
            assert np.array_equal(batch[i + 1].reshape(ht, wt).cpu().numpy(), want), i
    with pytest.raises(ValueError):
        ops.image_gray_resize(torch.from_numpy(srcs[0]).to(DEV), wt, ht, out=torch.empty(ht, wt + 1, device=DEV))
    with pytest.raises(ValueError):
        ops.image_gray_resize(torch.from_numpy(srcs[0]).to(DEV), wt, ht, out=torch.empty(ht, wt, dtype=torch.uint8, device=DEV))


def test_non_default_stream():
    from geoformer_amd import ops
    src = _content('random', 600, 800, 3, seed=3)
    d = torch.from_numpy(src).to(DEV)
    base_u8 = ops.image_gray_resize(d, 640, 480, normalised=False)
    base_f = ops.image_gray_resize(d, 640, 480)
    assert torch.equal(base_f.cpu().view(torch.int32), _want_f32(_host(src, 640, 480)).view(torch.int32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        u8 = ops.image_gray_resize(d, 640, 480, normalised=False)
        f = ops.image_gray_resize(d, 640, 480)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(u8, base_u8) and torch.equal(f.view(torch.int32), base_f.view(torch.int32))
    assert np.array_equal(u8.cpu().numpy(), _host(src, 640, 480))


def _write_files(tmp_path):
    """PNG, PPM / PGM and JPEG files, colour and gray, of sizes that reach the three resize forms at imsize 160."""
    from PIL import Image
    rng = np.random.default_rng(21)
    paths = []
    for k, (h, w) in enumerate([(168, 200), (320, 400), (160, 184), (210, 280), (481, 643)]):
        yy, xx = np.mgrid[0:h, 0:w]
        base = (127 + 90 * np.sin(xx / 7.0 + k) * np.cos(yy / 5.0)).astype(np.int64)
        rgb = np.clip(base[..., None] + rng.integers(-30, 30, (h, w, 3)), 0, 255).astype(np.uint8)
        gray = rgb[..., 1].copy()
        for ext, im in (('png', rgb), ('ppm', rgb), ('jpg', rgb), ('png', gray), ('pgm', gray), ('jpg', gray)):
            p = str(tmp_path / f'im{k}_{"c" if im.ndim == 3 else "g"}.{ext}')
            Image.fromarray(im).save(p, **({'quality': 92} if ext == 'jpg' else {}))
            paths.append(p)
    return paths


def test_files_device_equals_host(tmp_path):
    from geoformer_amd import matcher as MT
    for p in _write_files(tmp_path):
        for imsize in (160, 480, None):
            th, sh = MT.load_gray_scale_tensor(p, DEV, imsize=imsize, dfactor=8, value_to_scale=min, preprocess='host')
            td, sd = MT.load_gray_scale_tensor(p, DEV, imsize=imsize, dfactor=8, value_to_scale=min, preprocess='device')
            assert sh == sd, (p, imsize)
            assert td.shape == th.shape and td.dtype == th.dtype == torch.float32 and td.device == th.device
            assert torch.equal(td.view(torch.int32), th.view(torch.int32)), (os.path.basename(p), imsize,
                                                                              int((td.view(torch.int32) != th.view(torch.int32)).sum()))


def _matcher(preprocess):
    from geoformer_amd import matcher as MT
    torch.manual_seed(1234)
    m = MT.GeoFormerMatcher(imsize=160, match_threshold=0.0, no_match_upscale=True, precision='fp16', preprocess=preprocess)
    m.model.fine_matching.thr = 0.0
    return m


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def test_matcher_device_equals_host(tmp_path):
    """GeoFormerMatcher (random weights under a fixed seed, fp16) on two files of unequal size.  Premise: the host path repeats itself
    bit for bit; then the device path must return identical matches, kpts, scores and upscale - on one pair, and on 50
    alternating pairs through one matcher object (the staging buffers are reused with images of changing size)."""
    import sys
    from PIL import Image
    import golden_inputs as GI
    i0, i1 = GI.textured_pair(168, 200, 77)
    big = torch.nn.functional.interpolate(i1, size=(210, 280), mode='bilinear', align_corners=False)
    pa, pb = str(tmp_path / 'a.png'), str(tmp_path / 'b.ppm')
    a = (i0[0, 0] * 255).round().byte().numpy()
    b = (big[0, 0] * 255).round().byte().numpy()
    Image.fromarray(np.stack([a, np.roll(a, 1, 0), np.roll(a, 1, 1)], -1)).save(pa)        # colour files: the gray conversion runs
    Image.fromarray(np.stack([b, np.roll(b, 2, 1), np.roll(b, 2, 0)], -1)).save(pb)
    host, dev = _matcher('host'), _matcher('device')
    assert all(torch.equal(v, dev.model.state_dict()[k]) for k, v in host.model.state_dict().items())
    orders = [(pa, pb), (pb, pa)]
    want = []
    for o in orders:
        h1, h2 = host.match_pairs(*o), host.match_pairs(*o)
        if not _same(h1, h2):
            pytest.fail(f'the host path does not repeat itself on {[os.path.basename(p) for p in o]} ({len(h1[0])} vs {len(h2[0])} matches): '
                        'nothing can be said about the device path')
        want.append(h1)
    print(f'matches per order: {[len(w[0]) for w in want]}', file=sys.stderr)
    got = dev.match_pairs(*orders[0])
    assert len(got) == 5
    for name, x, y in zip(('matches', 'kpts1', 'kpts2', 'scores', 'upscale'), got, want[0]):
        assert np.array_equal(x, y), name
    # the tensors the model consumed, whatever the number of matches
    for p in (pa, pb):
        assert torch.equal(dev.load_im(p)[0].view(torch.int32), host.load_im(p)[0].view(torch.int32))
    for k in range(50):
        got = dev.match_pairs(*orders[k & 1])
        again = host.match_pairs(*orders[k & 1])
        if not _same(again, want[k & 1]):
            pytest.fail(f'the host path does not repeat itself at pair {k}: nothing can be said about the device path')
        for name, x, y in zip(('matches', 'kpts1', 'kpts2', 'scores', 'upscale'), got, want[k & 1]):
            assert np.array_equal(x, y), (k, name)


def test_cpu_device_raises():
    from geoformer_amd import matcher as MT
    with pytest.raises(ValueError, match='preprocess'):
        MT.GeoFormerMatcher(imsize=160, match_threshold=0.2, device='cpu', preprocess='device')
    with pytest.raises(ValueError, match='preprocess'):
        MT.load_gray_scale_tensor('does-not-matter.png', 'cpu', imsize=160, preprocess='device')
    with pytest.raises(ValueError, match='preprocess'):
        MT.load_gray_scale_tensor('does-not-matter.png', DEV, imsize=160, preprocess='gpu')
