"""Kept feature maps on the GPU: the address-table kernels against their siblings on torch.stack of the same maps, the model's
match_features against forward_features / forward, and the matcher's match_many against match_pairs.  Every comparison is on bits
(torch.equal / np.array_equal): the new path reads the same values through another address computation, there is nothing to tolerate."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
TABLE = [2, 0, 2]               # not in allocation order, one map named twice
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
TYPE_PAIRS = [(F32, F32), (F16, F16), (BF16, BF16), (BF16, F16), (F16, BF16)]


def _map(c, h, w, dtype, layout, seed, offset=0):
    """One [C,H,W] map in an allocation of its own.  layout 'nhwc': channels-last (stride 1 on C); 'nchw': contiguous.
    offset: elements between the start of the allocation and the map (1: the map is not 32-byte aligned)."""
    g = torch.Generator().manual_seed(seed)
    flat = torch.zeros(c * h * w + offset, dtype=dtype, device=DEV)
    flat[offset:] = (torch.randn(c * h * w, generator=g) * 3).to(dtype).to(DEV)
    body = flat[offset:]
    return body.view(h, w, c).permute(2, 0, 1) if layout == 'nhwc' else body.view(c, h, w)


def _stack(maps):
    """torch.stack of the maps, in the maps' own memory layout (a channels-last map stays channels-last in the batch)."""
    if maps[0].stride(0) == 1 and maps[0].shape[0] > 1:
        return torch.stack([m.permute(1, 2, 0) for m in maps]).permute(0, 3, 1, 2)
    return torch.stack(maps)


# ------------------------------------------------------------------------------------------------------------------------------
# kernel level
# ------------------------------------------------------------------------------------------------------------------------------
PE_FORMS = {                       # name -> (C, layout, offset of map 0 in its allocation)
    'vector': (256, 'nhwc', 0),                # dense channels-last, C % 8 == 0, every entry 32-byte aligned
    'scalar_c20': (20, 'nhwc', 0),             # channels-last, C % 8 != 0
    'scalar_unaligned': (256, 'nhwc', 1),      # C = 256, but one table entry starts one element into its allocation
    'nchw': (40, 'nchw', 0),                   # contiguous NCHW: partial 32 x 32 tiles in both directions (35 positions, 40 channels)
}


@pytest.mark.parametrize('tin,tout', TYPE_PAIRS, ids=lambda t: str(t).split('.')[-1])
@pytest.mark.parametrize('form', list(PE_FORMS))
def test_pos_encode_table_equals_stacked(form, tin, tout):
    from geoformer_amd import ops
    C, layout, off = PE_FORMS[form]
    H, W = 5, 7
    maps = [_map(C, H, W, tin, layout, 10 + k, offset=off if k == 0 else 0) for k in range(3)]
    if form == 'scalar_unaligned':
        assert maps[0].data_ptr() % 32 != 0 and maps[1].data_ptr() % 32 == 0
    elif layout == 'nhwc':
        assert all(m.data_ptr() % 32 == 0 for m in maps)
    pe = torch.randn(H, W, C, generator=torch.Generator().manual_seed(5)).to(DEV)
    batch = ops.MapBatch([maps[k] for k in TABLE])
    got = ops.pos_encode(batch, pe, tout)
    want = ops.pos_encode(_stack([maps[k] for k in TABLE]), pe, tout)
    assert got.shape == (3, H * W, C) and got.dtype == tout
    assert torch.equal(got, want)
    assert torch.equal(want, (_stack([maps[k] for k in TABLE]).float() + pe.permute(2, 0, 1)).to(tout).flatten(2).transpose(1, 2))
    into = torch.empty(5, H * W, C, dtype=tout, device=DEV)                       # the `out=` form the model uses (halves of one buffer)
    assert ops.pos_encode(batch, pe, tout, out=into[2:]).data_ptr() == into[2:].data_ptr() and torch.equal(into[2:], want)


FG_FORMS = [('rows', F16, F16), ('rows', BF16, BF16), ('rows', BF16, F16), ('general', F32, F32)]


@pytest.mark.parametrize('drop', [0, 1], ids=['M60', 'M59'])
@pytest.mark.parametrize('form,tin,tout', FG_FORMS, ids=lambda t: str(t).split('.')[-1])
def test_fine_gather_table_equals_stacked(form, tin, tout, drop):
    """Side 0: fine maps [128,16,20] over a 4 x 5 coarse grid; side 1: [128,12,16] over 3 x 4; stride 4, window 5, CC = 256.  Every
    (sample, cell of image 0) with j = i % 12: all four corner cells and their zero padding, M = 60.  One match dropped: M = 59, 2M % 4 != 0,
    the last workgroup of the one-wave-per-window form is partly empty."""
    from geoformer_amd import ops
    layout = 'nhwc' if form == 'rows' else 'nchw'
    maps0 = [_map(128, 16, 20, tin, layout, 20 + k) for k in range(3)]
    maps1 = [_map(128, 12, 16, tin, layout, 30 + k) for k in range(3)]
    t0, t1 = TABLE, [1, 1, 0]
    g = torch.Generator().manual_seed(7)
    c0 = torch.randn(3, 20, 256, generator=g).to(tout).to(DEV)
    c1 = torch.randn(3, 12, 256, generator=g).to(tout).to(DEV)
    b = torch.arange(3).repeat_interleave(20)
    i = torch.arange(20).repeat(3)
    keep = torch.ones(60, dtype=torch.bool)
    if drop:
        keep[17] = False
    b, i = b[keep].to(DEV), i[keep].to(DEV)
    j = i % 12
    M = int(keep.sum())
    args = (c0, c1, b, i, j, 5, 4, 4, 5, tout)
    win, ccat = ops.fine_gather(ops.MapBatch([maps0[k] for k in t0]), ops.MapBatch([maps1[k] for k in t1]), *args)
    win_ref, ccat_ref = ops.fine_gather(_stack([maps0[k] for k in t0]), _stack([maps1[k] for k in t1]), *args)
    assert win.shape == (2 * M, 25, 128) and ccat.shape == (2 * M, 256) and win.dtype == tout
    assert torch.equal(win, win_ref) and torch.equal(ccat, ccat_ref)
    # and the reference is what it should be: F.unfold windows of the stacked maps, converted once
    s0 = _stack([maps0[k] for k in t0]).float()
    unf = torch.nn.functional.unfold(s0, kernel_size=5, stride=4, padding=2).view(3, 128, 25, 20)
    assert torch.equal(win_ref[:M], unf[b, :, :, i].permute(0, 2, 1).to(tout))
    assert bool((win_ref[:M][(b == 0) & (i == 0)][0, 0] == 0).all())                  # a corner cell: its first window position is padding


def test_wrappers_refuse_batches_that_do_not_agree():
    from geoformer_amd import ops
    a, b = _map(128, 16, 20, F16, 'nhwc', 1), _map(128, 16, 24, F16, 'nhwc', 2)
    with pytest.raises(ValueError, match='shape'):
        ops.MapBatch([a, b])
    with pytest.raises(ValueError, match='strides'):
        ops.MapBatch([a, _map(128, 16, 20, F16, 'nchw', 3)])
    one, two = ops.MapBatch([a]), ops.MapBatch([a, a])
    c = torch.zeros(2, 20, 256, dtype=F16, device=DEV)
    ids = torch.zeros(1, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match='maps on side'):
        ops.fine_gather(one, two, c, c, ids, ids, ids, 5, 5, 4, 5, F16)
    with pytest.raises(TypeError):
        ops.fine_gather(one, a[None], c, c, ids, ids, ids, 5, 5, 4, 5, F16)


# ------------------------------------------------------------------------------------------------------------------------------
# model level: imsize 160, thresholds 0, images of 160 x 184 and 160 x 208
# ------------------------------------------------------------------------------------------------------------------------------
TENSOR_KEYS = ('mkpts0_c', 'mkpts1_c', 'mkpts0_f', 'mkpts1_f', 'mconf', 'b_ids', 'i_ids', 'j_ids', 'm_bids')
_models = {}


def _model(precision):
    if precision not in _models:
        from geoformer_amd.model.cvpr_ds_config import get_default_cfg
        from geoformer_amd.model.full_model import GeoFormer
        from geoformer_amd.model.geo_config import get_cfg_model
        from geoformer_amd.weights import deterministic_init_
        conf, gcfg = get_default_cfg(), get_cfg_model()
        conf['match_coarse']['thr'] = 0.0
        gcfg.update(coarse_thr=0.0, fine_thr=0.0, precision=precision)
        _models[precision] = deterministic_init_(GeoFormer(conf, gcfg)).eval().to(DEV)
    return _models[precision]


def _images(n, h, w, seed):
    import golden_inputs as GI
    return torch.cat([GI.textured_pair(h, w, seed + k)[k % 2] for k in range(n)]).to(DEV)


def _assert_same(out, ref):
    assert len(ref['b_ids']) > 20 and len(ref['mkpts0_f']) > 4, (len(ref['b_ids']), len(ref['mkpts0_f']))
    for k in TENSOR_KEYS:
        assert out[k].shape == ref[k].shape and torch.equal(out[k], ref[k]), k


def _stacked(recs, field):
    return _stack([getattr(r, field) for r in recs])


@pytest.mark.parametrize('precision', ['fp16', 'bf16_fp16', 'fp32'])
def test_match_features_equals_forward_features_on_the_stacked_maps(precision):
    m = _model(precision)
    img0, img1 = _images(2, 160, 184, 100), _images(2, 160, 208, 200)
    with torch.no_grad():
        e0, e1 = m.extract_features(img0), m.extract_features(img1)
        recs0, recs1 = [e0[1], e0[0]], [e1[0], e1[1]]                       # side 0 not in the order of its storage
        assert recs0[0].coarse.shape == (256, 20, 23) and recs1[0].fine.shape == (128, 80, 104)
        assert recs0[0].coarse.dtype == m.backbone_dtype and recs0[0].image_size == (160, 184)
        out = m.match_features(recs0, recs1)
        ref = m.forward_features({'image0': img0.flip(0), 'image1': img1}, _stacked(recs0, 'coarse'), _stacked(recs0, 'fine'),
                                 _stacked(recs1, 'coarse'), _stacked(recs1, 'fine'))
    _assert_same(out, ref)
    assert int(out['m_bids'].max()) == 1 and tuple(out['hw0_i'].tolist()) == (160, 184) and int(out['bs']) == 2


def test_one_query_broadcast_against_three_candidates():
    m = _model('fp16')
    with torch.no_grad():
        query = m.extract_features(_images(1, 160, 184, 300))[0]
        cands = m.extract_features(_images(3, 160, 208, 400))
        out = m.match_features([query] * 3, cands)                           # the same record object three times
        ref = m.forward_features({'image0': torch.zeros(3, 1, 160, 184, device=DEV), 'image1': torch.zeros(3, 1, 160, 208, device=DEV)},
                                 query.coarse[None].expand(3, -1, -1, -1).contiguous(), query.fine[None].expand(3, -1, -1, -1).contiguous(),
                                 _stacked(cands, 'coarse'), _stacked(cands, 'fine'))
    _assert_same(out, ref)
    assert sorted(set(out['m_bids'].tolist())) == [0, 1, 2]


def test_extract_then_match_equals_forward():
    """Equal shapes, fp16: forward runs both images through the backbone as one batch of two - exactly extract_features(cat) - and
    keeps both position-encoded maps in one buffer, as match_features does for equal shapes."""
    m = _model('fp16')
    img = _images(2, 160, 184, 500)
    img0, img1 = img[:1], img[1:]
    with torch.no_grad():
        recs = m.extract_features(torch.cat([img0, img1]))
        out = m.match_features([recs[0]], [recs[1]])
        ref = m({'image0': img0, 'image1': img1})
    _assert_same(out, ref)


def test_match_features_refuses_mixed_sides_and_training_mode():
    m = _model('fp16')
    with torch.no_grad():
        a = m.extract_features(_images(1, 160, 184, 600))[0]
        b = m.extract_features(_images(1, 160, 208, 700))[0]
        with pytest.raises(ValueError):
            m.match_features([a, b], [b, b])
        with pytest.raises(ValueError):
            m.match_features([a], [b, b])
    m.train()
    try:
        with pytest.raises(RuntimeError, match='eval'):
            m.match_features([a], [b])
    finally:
        m.eval()


# ------------------------------------------------------------------------------------------------------------------------------
# matcher level: fp16, image files of three sizes (forward runs the backbone per image too: the same launches on both paths)
# ------------------------------------------------------------------------------------------------------------------------------
def _write_images(root):
    from PIL import Image
    rng = np.random.default_rng(11)
    paths = []
    for name, (w, h) in (('a', (200, 168)), ('b', (280, 210)), ('c', (240, 168))):          # -> 160 x 184, 160 x 208, 160 x 224
        paths.append(os.path.join(root, name + '.png'))
        Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(paths[-1])
    return paths


def _matcher(**kw):
    from geoformer_amd import matcher as MT
    from geoformer_amd.weights import deterministic_init_
    m = MT.GeoFormerMatcher(imsize=160, match_threshold=0.0, no_match_upscale=True, precision='fp16', **kw)
    deterministic_init_(m.model)
    m.model.fine_matching.thr = 0.0
    return m


def _assert_results_equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w) and len(w[0]) > 4
        for x, y in zip(g, w):
            assert np.asarray(x).shape == np.asarray(y).shape and np.array_equal(x, y)


def test_match_many_equals_match_pairs_and_extracts_each_image_once(tmp_path):
    from geoformer_amd import matcher as MT
    a, b, c = _write_images(str(tmp_path))
    pairs = [(a, b), (a, c), (b, c)]
    m = _matcher()
    assert [m.resized_shape(p) for p in (a, b, c)] == [(160, 184), (160, 208), (160, 224)]
    want = [m.match_pairs(*p) for p in pairs]
    got = m.match_many(pairs)
    _assert_results_equal(got, want)
    assert len(got[0]) == 5 and (m.store.extractions, m.store.hits, len(m.store)) == (3, 3, 3)
    _assert_results_equal(m.match_many(pairs), want)                                      # everything from the store
    assert (m.store.extractions, m.store.hits) == (3, 9)
    rec = m.extract(a)
    assert rec.scale == (200 / 184, 168 / 160) and rec.features.image_size == (160, 184) and m.store.extractions == 3
    _assert_results_equal([m.match_features(m.extract(a), m.extract(b))], want[:1])
    # the other return convention: keypoints scaled back to the original images
    m.no_match_upscale = False
    want_up = [m.match_pairs(*p) for p in pairs]
    got_up = m.match_many(pairs)
    assert len(got_up[0]) == 4
    _assert_results_equal(got_up, want_up)
    # a byte budget that holds two images: the same results, images extracted again after their eviction
    sizes = sorted(m.extract(p).nbytes for p in (a, b, c))
    m.no_match_upscale = True
    m.store = MT.FeatureStore(max_bytes=sizes[1] + sizes[2])
    _assert_results_equal(m.match_many(pairs), want)
    assert m.store.extractions == 4 and m.store.evictions == 2 and len(m.store) == 2 and m.store.nbytes <= m.store.max_bytes
    _assert_results_equal(m.match_many(pairs), want)
    assert m.store.extractions > 4


def test_hpatches_with_reused_features_prints_the_same_auc(tmp_path):
    from PIL import Image
    from geoformer_amd import matcher as MT
    rng = np.random.default_rng(3)
    d = tmp_path / 'v_synth'
    d.mkdir()
    for k in range(1, 7):
        Image.fromarray(rng.integers(0, 255, (168, 200, 3), dtype=np.uint8)).save(str(d / f'{k}.ppm'))
        if k > 1:
            np.savetxt(str(d / f'H_1_{k}'), np.array([[1., 0, 4], [0, 1, -3], [0, 0, 1]]))
    m = _matcher()
    plain, reused = [], []
    out0 = MT.eval_hpatches(m, str(tmp_path), log=plain.append)
    assert m.store.extractions == 0                                                        # off by default: the store is not touched
    out1 = MT.eval_hpatches(m, str(tmp_path), log=reused.append, reuse_features=True)
    assert [s for s in plain if 'AUC' in s] == [s for s in reused if 'AUC' in s] and len([s for s in plain if 'AUC' in s]) == 1
    assert (m.store.extractions, m.store.hits) == (6, 4) and out0['pairs'] == out1['pairs'] == 5
