"""Padded batches of unequal image sizes on the GPU: the two ragged kernels against their tensor siblings on the maps zero-padded and
stacked, the model's match_features(pad=True) against the existing masked path (forward_features with masks built here) and against the
fp32 oracle, and the matcher's match_many(pad=True).  Every comparison is on bits (torch.equal / np.array_equal) unless stated: the new
path reads the same values through another address computation and substitutes the same zeros.

In the kernel tests every map lies inside a larger allocation whose other elements are 77: a read past a map's extent (or past its
allocation's used part) shows up as a wrong value, not as a silent zero."""
import os

import numpy as np
import pytest
import torch

import geoformer_oracle as O
import golden_inputs as GI
import ransac_oracle as RO

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
TYPE_PAIRS = [(F32, F32), (F16, F16), (BF16, BF16), (BF16, F16), (F16, BF16)]
MARGIN = 64                     # elements of 77 in front of and behind every map (keeps 32-byte alignment for every dtype)


def _map(c, h, w, dtype, layout, seed, offset=0):
    """One [C,h,w] map inside an allocation of its own: MARGIN + offset elements of 77, the map, MARGIN elements of 77.
    layout 'nhwc': channels-last (stride 1 on C); 'nchw': contiguous.  offset 1: the map is not 32-byte aligned."""
    g = torch.Generator().manual_seed(seed)
    n = c * h * w
    flat = torch.full((MARGIN + offset + n + MARGIN,), 77.0, dtype=dtype, device=DEV)
    body = flat[MARGIN + offset:MARGIN + offset + n]
    body.copy_((torch.randn(n, generator=g) * 3).to(dtype))
    return body.view(h, w, c).permute(2, 0, 1) if layout == 'nhwc' else body.view(c, h, w)


def _pad_stack(maps, H, W):
    """The maps zero-padded at the right and bottom to H x W and stacked, in the maps' own memory layout."""
    c = maps[0].shape[0]
    if maps[0].stride(0) == 1 and c > 1:
        out = torch.zeros(len(maps), H, W, c, dtype=maps[0].dtype, device=maps[0].device).permute(0, 3, 1, 2)
    else:
        out = torch.zeros(len(maps), c, H, W, dtype=maps[0].dtype, device=maps[0].device)
    for n, m in enumerate(maps):
        out[n, :, :m.shape[1], :m.shape[2]] = m
    return out


def _extent_mask(extents, H, W):
    """bool [N,H,W], true inside each sample's extent - from arange comparisons, not from any kernel."""
    hs = torch.tensor([e[0] for e in extents], device=DEV)[:, None, None]
    ws = torch.tensor([e[1] for e in extents], device=DEV)[:, None, None]
    return (torch.arange(H, device=DEV)[None, :, None] < hs) & (torch.arange(W, device=DEV)[None, None, :] < ws)


# ------------------------------------------------------------------------------------------------------------------------------
# kernel level
# ------------------------------------------------------------------------------------------------------------------------------
PE_FORMS = {                       # name -> (C, layout, offset of map 0 in its allocation)
    'vector': (256, 'nhwc', 0),                # channels-last, C % 8 == 0, every entry 32-byte aligned: 8 channels per lane
    'scalar_c20': (20, 'nhwc', 0),             # channels-last, C % 8 != 0
    'scalar_unaligned': (256, 'nhwc', 1),      # C = 256, but one table entry starts one element off 32-byte alignment
    'nchw': (40, 'nchw', 0),                   # contiguous [C,h,w]: partial 32 x 32 tiles in both directions (35 positions, 40 channels)
}
PE_EXTENTS = [(5, 7), (3, 7), (5, 4), (1, 1)]
PE_TABLE = [2, 0, 3, 2, 1]          # not in allocation order, one map named twice


@pytest.mark.parametrize('tin,tout', TYPE_PAIRS, ids=lambda t: str(t).split('.')[-1])
@pytest.mark.parametrize('form', list(PE_FORMS))
def test_pos_encode_ragged_equals_padded_stack(form, tin, tout):
    from geoformer_amd import ops
    C, layout, off = PE_FORMS[form]
    H, W = 5, 7
    maps = [_map(C, h, w, tin, layout, 10 + k, offset=off if k == 0 else 0) for k, (h, w) in enumerate(PE_EXTENTS)]
    if form == 'scalar_unaligned':
        assert maps[0].data_ptr() % 32 != 0 and maps[1].data_ptr() % 32 == 0
    else:
        assert all(m.data_ptr() % 32 == 0 for m in maps)
    ms, ext = [maps[k] for k in PE_TABLE], [PE_EXTENTS[k] for k in PE_TABLE]
    N = len(ms)
    for (Hc, Wc), canvas in (((H, W), None), ((6, 8), (6, 8))):                     # the default canvas; an explicit one larger than every map
        pe = torch.randn(Hc, Wc, C, generator=torch.Generator().manual_seed(5)).to(DEV)
        batch = ops.RaggedMapBatch(ms, canvas=canvas)
        assert batch.shape == (N, C, Hc, Wc)
        mask = torch.full((N, Hc, Wc), 9, dtype=torch.uint8, device=DEV)
        got = ops.pos_encode(batch, pe, tout, mask_out=mask)
        padded = _pad_stack(ms, Hc, Wc)
        want = ops.pos_encode(padded, pe, tout)
        assert got.shape == (N, Hc * Wc, C) and got.dtype == tout
        assert torch.equal(got, want)
        assert torch.equal(want, (padded.float() + pe.permute(2, 0, 1)).to(tout).flatten(2).transpose(1, 2))
        assert torch.equal(mask, _extent_mask(ext, Hc, Wc).to(torch.uint8))
        assert torch.equal(ops.pos_encode(batch, pe, tout), want)                                # without a mask
        into = torch.full((N + 2, Hc * Wc, C), 5, dtype=tout, device=DEV)                       # the `out=` form the model uses (halves of one buffer)
        bmask = torch.zeros(N, Hc, Wc, dtype=torch.bool, device=DEV)
        assert ops.pos_encode(batch, pe, tout, out=into[2:], mask_out=bmask).data_ptr() == into[2:].data_ptr()
        assert torch.equal(into[2:], want) and bool((into[:2] == 5).all()) and torch.equal(bmask, _extent_mask(ext, Hc, Wc))
    with pytest.raises(ValueError, match='mask_out'):
        ops.pos_encode(padded, pe, tout, mask_out=mask)                                          # only a ragged batch has padding to report


FG_FORMS = [('rows', F16, F16), ('rows', BF16, BF16), ('rows', BF16, F16), ('general', F32, F32)]
FG_EXT0, FG_EXT1 = [(4, 5), (3, 5), (4, 3)], [(3, 4), (2, 4), (3, 2)]       # coarse extents on canvases of 4 x 5 and 3 x 4 cells


def _cells(ext, wc, reach=False):
    """Flat canvas indices of the cells of an h x w extent; reach=True: also the first cells past its right and bottom edges that the
    canvas has (their windows straddle the edge: two rows / columns of taps inside the map, three outside)."""
    h, w = ext
    return [y * wc + x for y in range(h + reach) for x in range(w + reach) if x < wc]


@pytest.mark.parametrize('matches', ['M47', 'M46', 'past_edge'])
@pytest.mark.parametrize('form,tin,tout', FG_FORMS, ids=lambda t: str(t).split('.')[-1])
def test_fine_gather_ragged_equals_padded_stack(form, tin, tout, matches):
    """Side 0: fine canvas [128,16,20] over 4 x 5 coarse cells; side 1: [128,12,16] over 3 x 4; stride 4, window 5, CC = 256.
    M47: every valid cell of every sample on side 0, j cycling through the sample's valid cells on side 1 - all cells on the borders of
    the valid regions and all corners with their zero padding; 2M % 4 != 0, the last workgroup of the one-wave form is partly empty.
    M46: one match dropped.  With stride 4 and a 5 x 5 window a VALID cell's window ends two fine pixels inside its map, so
    past_edge adds the first padded cells on both sides (canvas rows / columns the masks exclude in the model): their windows cross the
    map's edge, where the memory behind the map (the next row of the map itself, the 77s) must not be read."""
    from geoformer_amd import ops
    layout = 'nhwc' if form == 'rows' else 'nchw'
    maps0 = [_map(128, 4 * h, 4 * w, tin, layout, 20 + k) for k, (h, w) in enumerate(FG_EXT0)]
    maps1 = [_map(128, 4 * h, 4 * w, tin, layout, 30 + k) for k, (h, w) in enumerate(FG_EXT1)]
    g = torch.Generator().manual_seed(7)
    c0 = torch.randn(3, 20, 256, generator=g).to(tout).to(DEV)
    c1 = torch.randn(3, 12, 256, generator=g).to(tout).to(DEV)
    reach = matches == 'past_edge'
    b, i, j = [], [], []
    for n in range(3):
        ci = _cells(FG_EXT0[n], 5, reach)
        cj = _cells(FG_EXT1[n], 4, reach)
        ci = [c for c in ci if c < 20]
        cj = [c for c in cj if c < 12]
        b += [n] * len(ci)
        i += ci
        j += [cj[k % len(cj)] for k in range(len(ci))]
    if matches == 'M46':
        del b[17], i[17], j[17]
    M = len(b)
    assert matches == 'past_edge' or M == {'M47': 47, 'M46': 46}[matches]
    b, i, j = (torch.tensor(v, device=DEV) for v in (b, i, j))
    args = (c0, c1, b, i, j, 5, 4, 4, 5, tout)
    rb0, rb1 = ops.RaggedMapBatch(maps0), ops.RaggedMapBatch(maps1)
    assert rb0.shape == (3, 128, 16, 20) and rb1.shape == (3, 128, 12, 16)
    win, ccat = ops.fine_gather(rb0, rb1, *args)
    p0, p1 = _pad_stack(maps0, 16, 20), _pad_stack(maps1, 12, 16)
    win_ref, ccat_ref = ops.fine_gather(p0, p1, *args)
    assert win.shape == (2 * M, 25, 128) and ccat.shape == (2 * M, 256) and win.dtype == tout
    assert torch.equal(win, win_ref) and torch.equal(ccat, ccat_ref)
    # and the reference is what it should be: F.unfold windows of the padded stacked maps, converted once
    unf = torch.nn.functional.unfold(p0.float(), kernel_size=5, stride=4, padding=2).view(3, 128, 25, 20)
    assert torch.equal(win_ref[:M], unf[b, :, :, i].permute(0, 2, 1).to(tout))
    assert bool((win[:M][(b == 0) & (i == 0)][0, 0] == 0).all())                      # a corner cell: its first window position is padding
    if reach:
        # sample 1 of side 0 has 3 of the canvas's 4 rows of cells: cell (3, 0) is the first padded one, its window covers fine rows 10 .. 14
        # of a 12-row map: window rows 0, 1 are the map's (columns 2 .. 4: non-zero with randn data), rows 2 .. 4 lie past its extent
        w = win[:M][(b == 1) & (i == 15)][0].view(5, 5, 128).float()
        assert bool((w[2:] == 0).all()) and bool((w[:2, 2:] != 0).any()) and bool((w[:2, :2] == 0).all())
        # sample 2 of side 0 is 3 of 5 cells wide: cell (0, 3), window columns 2 .. 4 are past the extent (its rows 0, 1 are F.unfold's padding)
        w = win[:M][(b == 2) & (i == 3)][0].view(5, 5, 128).float()
        assert bool((w[:, 2:] == 0).all()) and bool((w[2:, :2] != 0).any())


def test_wrappers_refuse_batches_that_do_not_agree():
    from geoformer_amd import ops
    a, b = _map(128, 16, 20, F16, 'nhwc', 1), _map(128, 12, 20, F16, 'nhwc', 2)
    ragged, one = ops.RaggedMapBatch([a, b]), ops.RaggedMapBatch([a])
    c = torch.zeros(2, 20, 256, dtype=F16, device=DEV)
    ids = torch.zeros(1, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match='maps on side'):
        ops.fine_gather(one, ragged, c, c, ids, ids, ids, 5, 5, 4, 5, F16)
    with pytest.raises(TypeError):
        ops.fine_gather(ragged, ops.MapBatch([a, a]), c, c, ids, ids, ids, 5, 5, 4, 5, F16)
    with pytest.raises(TypeError):
        ops.fine_gather(ragged, torch.stack([a, a]), c, c, ids, ids, ids, 5, 5, 4, 5, F16)
    with pytest.raises(ValueError, match='canvas'):
        ops.pos_encode(ragged, torch.zeros(16, 21, 128, device=DEV), F16)                       # a table of another size than the canvas


# ------------------------------------------------------------------------------------------------------------------------------
# model level, against the existing masked path: imsize 160, thresholds 0
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


def _image(h, w, seed):
    return GI.textured_pair(h, w, seed)[seed % 2].to(DEV)


_recs = {}


def _records(m, sizes, seed):
    """One record per (h, w), each from a backbone call of its own; computed once per model and shared between the tests."""
    out = []
    for k, (h, w) in enumerate(sizes):
        key = (m.precision, h, w, seed + k)
        if key not in _recs:
            _recs[key] = m.extract_features(_image(h, w, seed + k))[0]
        out.append(_recs[key])
    return out


SIDE0 = [(160, 184), (160, 208)]
CASES = {'A_equal_canvases': [(160, 208), (128, 208)], 'B_unequal_canvases': [(128, 184), (128, 160)],
         'C_padding_on_both_sides_of_a_sample': [(128, 208), (160, 184)]}
# In A and B every sample has padding on at most one side.  In C sample 0 has it on both, and there the masked path itself - the reference's
# masked_fill with a FINITE -1e9 (coarse_matching.py:123-124), which K1 reproduces - leaves conf = 1 / (L S) > 0 at (padded row, padded
# column): both softmaxes are uniform there.  At the threshold 0 of these tests such entries can pass as matches, in the masked path and in
# the padded batch alike (they are compared on bits); any threshold above 1 / (L S) excludes them.


@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('precision', ['fp16', 'bf16_fp16', 'fp32'])
def test_match_features_padded_equals_the_masked_path_on_padded_maps(precision, case):
    m = _model(precision)
    with torch.no_grad():
        recs0, recs1 = _records(m, SIDE0, 100), _records(m, CASES[case], 200)
        out = m.match_features(recs0, recs1, pad=True)
        sides = []
        for recs in (recs0, recs1):
            hi, wi = max(r.image_size[0] for r in recs), max(r.image_size[1] for r in recs)
            ext = [tuple(r.coarse.shape[1:]) for r in recs]
            sides.append((hi, wi, ext, _pad_stack([r.coarse for r in recs], hi // 8, wi // 8), _pad_stack([r.fine for r in recs], hi // 2, wi // 2),
                          _extent_mask(ext, hi // 8, wi // 8)))
        (h0, w0, ext0, c0, f0, m0), (h1, w1, ext1, c1, f1, m1) = sides
        assert (h0, w0) == (160, 208) and (h1, w1) == ((128, 184) if case.startswith('B') else (160, 208))
        ref = m.forward_features({'image0': torch.zeros(2, 1, h0, w0, device=DEV), 'image1': torch.zeros(2, 1, h1, w1, device=DEV),
                                  'mask0': m0, 'mask1': m1}, c0, f0, c1, f1)
    assert len(ref['b_ids']) > 20 and sorted(set(ref['b_ids'].tolist())) == [0, 1], len(ref['b_ids'])
    for k in TENSOR_KEYS:
        assert out[k].shape == ref[k].shape and torch.equal(out[k], ref[k]), k
    assert out['mask0'].dtype == torch.bool and torch.equal(out['mask0'], m0) and torch.equal(out['mask1'], m1)
    assert tuple(out['hw0_i'].tolist()) == (h0, w0) and tuple(out['hw1_i'].tolist()) == (h1, w1) and int(out['bs']) == 2
    assert tuple(out['hw0_c'].tolist()) == (h0 // 8, w0 // 8) and tuple(out['hw1_f'].tolist()) == (h1 // 2, w1 // 2)
    # every coarse match lies inside its own sample's extents on both sides - or, in C, outside on both (see CASES): a pair of one valid
    # and one padded cell has conf = 0 exactly and never passes
    b = out['b_ids'].tolist()
    inside = [[c // wc < ext[n][0] and c % wc < ext[n][1] for n, c in zip(b, ids)]
              for ids, ext, wc in ((out['i_ids'].tolist(), ext0, w0 // 8), (out['j_ids'].tolist(), ext1, w1 // 8))]
    assert inside[0] == inside[1] and sum(inside[0]) > 20
    assert case.startswith('C') or all(inside[0])
    assert all(n == 0 for n, ok in zip(b, inside[0]) if not ok)              # only sample 0 of C has padding on both sides


def test_uniform_sides_with_pad_are_the_unpadded_call_and_mixed_sides_without_pad_are_refused():
    m = _model('fp16')
    with torch.no_grad():
        recs0, recs1 = _records(m, [(160, 184)] * 2, 300), _records(m, [(160, 208)] * 2, 400)
        out, ref = m.match_features(recs0, recs1, pad=True), m.match_features(recs0, recs1)
        assert len(ref['b_ids']) > 20 and 'mask0' not in out
        for k in TENSOR_KEYS:
            assert out[k].shape == ref[k].shape and torch.equal(out[k], ref[k]), k
        mixed = _records(m, SIDE0, 100)
        with pytest.raises(ValueError, match='one size'):
            m.match_features(mixed, recs1)
        with pytest.raises(ValueError, match='one size'):
            m.match_features(recs0, mixed, pad=False)
        # one mixed side, one uniform: the uniform side's mask is all true
        out = m.match_features(mixed, recs1, pad=True)
        assert bool(out['mask1'].all()) and not bool(out['mask0'].all()) and tuple(out['hw0_i'].tolist()) == (160, 208)


def test_geo_module_encodes_a_ragged_batch_itself_when_the_two_encodings_differ():
    """GeoModule adds its own position encoding when its temp_bug_fix flag differs from the coarse level's: that call reads the ragged
    batch a second time, and must give what it gives on the padded maps."""
    m = _model('fp16')
    with torch.no_grad():
        recs0, recs1 = _records(m, SIDE0, 100), _records(m, CASES['B_unequal_canvases'], 200)
        m.geo_module.pos_encoding.temp_bug_fix = not m.pos_encoding.temp_bug_fix
        try:
            out = m.match_features(recs0, recs1, pad=True)
            ext0, ext1 = [tuple(r.coarse.shape[1:]) for r in recs0], [tuple(r.coarse.shape[1:]) for r in recs1]
            ref = m.forward_features({'image0': torch.zeros(2, 1, 160, 208, device=DEV), 'image1': torch.zeros(2, 1, 128, 184, device=DEV),
                                      'mask0': _extent_mask(ext0, 20, 26), 'mask1': _extent_mask(ext1, 16, 23)},
                                     _pad_stack([r.coarse for r in recs0], 20, 26), _pad_stack([r.fine for r in recs0], 80, 104),
                                     _pad_stack([r.coarse for r in recs1], 16, 23), _pad_stack([r.fine for r in recs1], 64, 92))
        finally:
            m.geo_module.pos_encoding.temp_bug_fix = m.pos_encoding.temp_bug_fix
            m.geo_module.pos_encoding._tables.clear()                 # tables of the flipped kind: the cache is keyed by size only
    assert len(ref['b_ids']) > 20
    for k in TENSOR_KEYS:
        assert out[k].shape == ref[k].shape and torch.equal(out[k], ref[k]), k


# ------------------------------------------------------------------------------------------------------------------------------
# model level, against the oracle: fp32, N = 2, canvas 8 x 10, planted correspondences
# ------------------------------------------------------------------------------------------------------------------------------
ORACLE_EXT0, ORACLE_EXT1 = [(7, 10), (8, 9)], [(8, 8), (6, 10)]        # the masks of test_e2e_gpu.test_megadepth_style_batch_inference
ORACLE_SEED = 1301            # the oracle alone finds 93 coarse matches over both samples with it (checked on the CPU)


def test_padded_batch_against_the_oracle_on_zero_padded_maps_with_masks():
    from geoformer_amd.model.cvpr_ds_config import get_default_cfg
    from geoformer_amd.model.full_model import GeoFormer, ImageFeatures
    from geoformer_amd.model.geo_config import get_cfg_model
    (c0, f0), (c1, f1) = GI.planted_features(2, 8, 10, 8, 10, ORACLE_SEED)
    gc = get_cfg_model()
    gc.update(coarse_thr=0.2, fine_thr=0.1, precision='fp32')
    m = GeoFormer(get_default_cfg(), gc).eval()
    m.load_state_dict(O.make_weights())
    m = m.to(DEV)

    def crop(c, f, ext):           # the records: each sample's own part of the maps, in an allocation of its own
        return [ImageFeatures(c[n, :, :h, :w].contiguous().to(DEV), f[n, :, :4 * h, :4 * w].contiguous().to(DEV), (8 * h, 8 * w))
                for n, (h, w) in enumerate(ext)]

    def padded(t, ext, r):         # the oracle's input: the same parts, zeros elsewhere
        out = torch.zeros_like(t)
        for n, (h, w) in enumerate(ext):
            out[n, :, :h * r, :w * r] = t[n, :, :h * r, :w * r]
        return out

    with torch.no_grad():
        out = m.match_features(crop(c0, f0, ORACLE_EXT0), crop(c1, f1, ORACLE_EXT1), pad=True)
    feats = ((padded(c0, ORACLE_EXT0, 1), padded(f0, ORACLE_EXT0, 4)), (padded(c1, ORACLE_EXT1, 1), padded(f1, ORACLE_EXT1, 4)))
    data = {'image0': torch.zeros(2, 1, 64, 80), 'image1': torch.zeros(2, 1, 64, 80),
            'mask0': _extent_mask(ORACLE_EXT0, 8, 10).cpu(), 'mask1': _extent_mask(ORACLE_EXT1, 8, 10).cpu()}
    ref = O.geoformer_forward(O.make_weights(), dict(data), None, O.default_geo_config(), RO.make_homography_fn(), None, feats)
    assert len(ref['b_ids']) > 40 and sorted(set(ref['b_ids'].tolist())) == [0, 1], len(ref['b_ids'])
    assert tuple(out['hw0_i'].tolist()) == (64, 80) and tuple(out['hw1_i'].tolist()) == (64, 80)
    for k in ('b_ids', 'i_ids', 'j_ids', 'm_bids'):
        np.testing.assert_array_equal(out[k].cpu().numpy(), ref[k].numpy())
    for k in ('mkpts0_c', 'mkpts1_c', 'mkpts0_f', 'mkpts1_f'):
        np.testing.assert_allclose(out[k].detach().float().cpu().numpy(), np.asarray(ref[k]), rtol=1e-6, atol=1e-5)


# ------------------------------------------------------------------------------------------------------------------------------
# matcher level: fp16, image files of three sizes
# ------------------------------------------------------------------------------------------------------------------------------
SIZES = {'a': (200, 168), 'b': (280, 210), 'c': (240, 168)}          # (w, h) of the files -> resized to 160 x 184, 160 x 208, 160 x 224


def _write_images(root, sizes=SIZES):
    from PIL import Image
    rng = np.random.default_rng(11)
    paths = []
    for name, (w, h) in sizes.items():
        paths.append(os.path.join(root, name + '.png'))
        Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(paths[-1])
    return paths


def _matcher(**kw):
    from geoformer_amd import matcher as MT
    from geoformer_amd.weights import deterministic_init_
    m = MT.GeoFormerMatcher(imsize=160, match_threshold=0.0, precision='fp16', **kw)
    deterministic_init_(m.model)
    m.model.fine_matching.thr = 0.0
    return m


def _assert_results_equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w) and len(w[0]) > 4
        for x, y in zip(g, w):
            assert np.asarray(x).shape == np.asarray(y).shape and np.array_equal(x, y)


def test_match_many_padded_runs_unequal_pairs_in_one_model_call(tmp_path):
    a, b, c = _write_images(str(tmp_path))
    # every pair has the largest image on one side, so no sample is padded on both sides: at this matcher's threshold 0 a sample with
    # padding on both sides can match padding with padding (see CASES above; not with any threshold above 1 / (L S))
    pairs = [(a, c), (c, b), (b, c)]
    m = _matcher(no_match_upscale=True)
    assert [m.resized_shape(p) for p in (a, b, c)] == [(160, 184), (160, 208), (160, 224)]
    calls = []
    inner = m.model.match_features
    m.model.match_features = lambda f0, f1, **kw: calls.append((len(f0), kw)) or inner(f0, f1, **kw)
    got = m.match_many(pairs, batch=4, pad=True, max_waste=4.0)
    assert calls == [(3, {'pad': True})] and (m.store.extractions, len(m.store)) == (3, 3)
    # each pair's tuple: the model's padded call on the same batch, split by m_bids
    recs0, recs1 = [m.extract(p[0]) for p in pairs], [m.extract(p[1]) for p in pairs]
    assert m.store.extractions == 3
    with torch.no_grad():
        data = inner([r.features for r in recs0], [r.features for r in recs1], pad=True)
    assert sorted(set(data['m_bids'].tolist())) == [0, 1, 2]
    _assert_results_equal(got, m._results(data, recs0, recs1))
    assert len(got[0]) == 5 and all(np.array_equal(g[4], np.array(r0.scale + r1.scale)) for g, r0, r1 in zip(got, recs0, recs1))
    # keypoints scaled back to the original images stay inside them.  A fine keypoint is its coarse cell's corner (0 .. size - 8 in the
    # resized image) plus a window offset of -2 .. 2 fine pixels = -4 .. 4 resized pixels, with or without padding: it is below size - 4
    # exactly when the cell is one of the image's own, and it may be up to 4 resized pixels left of / above the origin
    m.no_match_upscale = False
    up = m.match_many(pairs, batch=4, pad=True, max_waste=4.0)
    wh = {p: SIZES[os.path.basename(p)[0]] for p in (a, b, c)}
    for (p0, p1), res, r0, r1 in zip(pairs, up, recs0, recs1):
        assert len(res) == 4 and len(res[1]) > 4
        for kp, p, r in ((res[1], p0, r0), (res[2], p1, r1)):
            size, scale = np.array(wh[p], dtype=np.float64), np.array(r.scale)
            assert (kp < size).all() and (kp <= size - 4 * scale + 1e-3).all() and (kp >= -4 * scale - 1e-3).all(), (kp.min(0), kp.max(0), size)
    # a tight waste bound: three shapes, nothing shares a batch - the plain path's numbers
    calls.clear()
    m.no_match_upscale = True
    alone = m.match_many(pairs, batch=4, pad=True, max_waste=1.0)
    assert [n for n, _ in calls] == [1, 1, 1]
    _assert_results_equal(alone, m.match_many(pairs, batch=4))


def test_match_many_padded_on_equal_sizes_gives_the_unpadded_bits(tmp_path):
    paths = _write_images(str(tmp_path), {'a': (200, 168), 'b': (200, 168), 'c': (200, 168)})
    pairs = [(paths[0], paths[1]), (paths[0], paths[2]), (paths[1], paths[2])]
    m = _matcher(no_match_upscale=True)
    want = m.match_many(pairs, batch=2)
    _assert_results_equal(m.match_many(pairs, batch=2, pad=True, max_waste=1.5), want)
    assert m.store.extractions == 3
