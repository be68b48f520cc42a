"""Host side of the device preprocessing path, without a GPU: the decoder split of `load_gray_image`, the argument checks of
preprocess='device', the command line flag."""
import numpy as np
import pytest


def _files(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(4)
    rgb = rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)
    gray = rgb[..., 0].copy()
    out = {}
    for name, im in (('c.png', rgb), ('c.ppm', rgb), ('c.jpg', rgb), ('g.png', gray), ('g.pgm', gray), ('g.jpg', gray)):
        out[name] = str(tmp_path / name)
        Image.fromarray(im).save(out[name])
    pal = str(tmp_path / 'p.png')
    Image.fromarray(rgb).convert('P').save(pal)
    out['p.png'] = pal
    return rgb, gray, out


def test_decoder_split_keeps_load_gray_image(tmp_path):
    from geoformer_amd import matcher as MT
    rgb, gray, files = _files(tmp_path)
    for name in ('c.png', 'c.ppm', 'p.png'):                      # colour that still needs the fixed-point gray
        im = MT.load_image_u8(files[name])
        assert im.shape == (40, 56, 3) and im.dtype == np.uint8
        np.testing.assert_array_equal(MT.load_gray_image(files[name]), MT.cv2_gray_u8(im))
    np.testing.assert_array_equal(MT.load_image_u8(files['c.ppm']), rgb)
    for name in ('c.jpg', 'g.jpg', 'g.png', 'g.pgm'):             # final already: the JPEG luma plane, mode L files
        im = MT.load_image_u8(files[name])
        assert im.shape == (40, 56) and im.dtype == np.uint8
        np.testing.assert_array_equal(MT.load_gray_image(files[name]), im)
    np.testing.assert_array_equal(MT.load_image_u8(files['g.png']), gray)


def test_device_preprocessing_needs_a_cuda_device(tmp_path):
    from geoformer_amd import matcher as MT
    _, _, files = _files(tmp_path)
    with pytest.raises(ValueError, match="preprocess='device'"):
        MT.load_gray_scale_tensor(files['c.png'], 'cpu', imsize=32, preprocess='device')
    with pytest.raises(ValueError, match="preprocess='device'"):
        MT.GeoFormerMatcher(imsize=160, match_threshold=0.2, device='cpu', preprocess='device')
    with pytest.raises(ValueError, match='preprocess must be one of'):
        MT.load_gray_scale_tensor(files['c.png'], 'cpu', imsize=32, preprocess='gpu')
    t, scale = MT.load_gray_scale_tensor(files['c.png'], 'cpu', imsize=32, preprocess='host')          # the default, spelled out
    t2, scale2 = MT.load_gray_scale_tensor(files['c.png'], 'cpu', imsize=32)
    assert scale == scale2 and t.equal(t2) and t.shape == (1, 1, 32, 40)


def test_command_line_flag():
    from geoformer_amd import matcher as MT
    for argv in (['match', 'a.png', 'b.png', '--preprocess', 'gpu'], ['hpatches', 'root', '--preprocess', 'gpu']):
        with pytest.raises(SystemExit):
            MT.main(argv)
    import inspect
    assert inspect.signature(MT.GeoFormerMatcher.__init__).parameters['preprocess'].default == 'host'
    assert inspect.signature(MT.load_gray_scale_tensor).parameters['preprocess'].default == 'host'
