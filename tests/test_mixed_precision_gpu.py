"""The 'bf16_fp16' precision mode on the GPU: bf16 backbone maps, fp16 matching path.  The two kernels that read the backbone's maps
convert while they move the data (gf_pos_encode, gf_fine_gather); the conversion is torch's `x.float().to(out)` for every input
bit pattern (round to nearest even, no clamp: beyond fp16's range -> inf, below its subnormal spacing -> rounded like any other
value), so every check here is an equality, not a tolerance:
  1. gf_pos_encode over all 65536 input patterns, both directions, through its three code paths;
  2. gf_fine_gather bf16 maps -> fp16 windows against F.unfold, row kernel and general kernel, all 65536 patterns through the row kernel;
  3. the mode's forward_features on bf16 maps == the fp16 mode's on the same maps converted to fp16 (maps that fp16 holds exactly);
  4. the mode's forward from images == bf16 backbone -> .to(fp16) -> fp16 matching path, eagerly and replayed from a captured graph;
  5. GeoFormerMatcher(precision='bf16_fp16') on image files."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_inputs as GI

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F16, BF16 = torch.float16, torch.bfloat16
OUT_KEYS = ('b_ids', 'i_ids', 'j_ids', 'm_bids', 'mkpts0_c', 'mkpts1_c', 'mkpts0_f', 'mkpts1_f', 'mconf', 'conf_matrix',
            'dect_conf_matrix', 'fine_matrix')


def all_patterns(dtype, numel):
    """numel elements of a 16-bit float type running through all 65536 bit patterns (again from 0 when numel > 65536)."""
    assert numel >= 65536
    bits = (torch.arange(numel, dtype=torch.int32, device=DEV) % 65536).to(torch.int16)      # wraps to the signed pattern
    return bits.view(dtype)


def same_values(got, want):
    """Equal as values (so -0 == +0), NaNs in the same places."""
    assert got.dtype == want.dtype and got.shape == want.shape
    gn, wn = torch.isnan(got), torch.isnan(want)
    if not torch.equal(gn, wn):
        return False
    z = torch.zeros((), dtype=got.dtype, device=got.device)
    return bool((torch.where(gn, z, got) == torch.where(wn, z, want)).all())


def same_bits(got, want):
    assert got.dtype == want.dtype and got.element_size() == 2
    return got.shape == want.shape and torch.equal(got.contiguous().view(torch.int16), want.contiguous().view(torch.int16))


# ------------------------------------------------------------------ 1. gf_pos_encode
# layout -> (N, C, H, W): the smallest awkward shape of each code path that holds all 65536 patterns
PE_SHAPES = {
    'nhwc_vec': (1, 16, 64, 64),       # dense channels-last, C = 8 k: 8 channels per lane (exactly 65536 elements)
    'nhwc_scalar': (1, 12, 74, 74),    # channels-last, C = 12: the scalar path
    'nchw': (47, 40, 5, 7),            # NCHW, H W = 35 and C = 40: the LDS transpose with ragged 32 x 32 tiles in both directions
}


def _pe_input(layout, dtype):
    N, C, H, W = PE_SHAPES[layout]
    flat = all_patterns(dtype, N * C * H * W)
    if layout == 'nchw':
        return flat.view(N, C, H, W)
    return flat.view(N, H, W, C).permute(0, 3, 1, 2)       # channels-last memory seen as [N, C, H, W]


def _pe_table(layout, kind):
    N, C, H, W = PE_SHAPES[layout]
    if kind == 'zero':
        return torch.zeros(H, W, C, device=DEV)
    g = torch.Generator(device='cpu').manual_seed(20 + len(layout))
    # magnitudes from 2^-30 to 2^17: sums that round into fp16's subnormals, its normal range and past 65504
    t = torch.randn(H, W, C, generator=g) * torch.exp2(torch.randint(-30, 18, (H, W, C), generator=g).float())
    return t.to(DEV)


@pytest.mark.parametrize('table', ['zero', 'random'])
@pytest.mark.parametrize('layout', list(PE_SHAPES))
@pytest.mark.parametrize('src,dst', [(BF16, F16), (F16, BF16)], ids=['bf16_to_fp16', 'fp16_to_bf16'])
def test_pos_encode_converting_every_pattern(src, dst, layout, table):
    from geoformer_amd import ops
    N, C, H, W = PE_SHAPES[layout]
    x, pe = _pe_input(layout, src), _pe_table(layout, table)
    assert (x.stride(1) == 1) == (layout != 'nchw') and (layout != 'nchw' or x.stride(3) == 1)
    out = ops.pos_encode(x, pe, dst)
    want = (x.float().permute(0, 2, 3, 1) + pe).reshape(N, H * W, C).to(dst)
    assert out.dtype == dst and tuple(out.shape) == (N, H * W, C)
    assert same_values(out, want)
    if table == 'zero':
        # the conversion alone: what it does at the ends of fp16's range is part of the contract
        assert int(torch.isinf(want).sum()) > int(torch.isinf(x).sum()) or src == F16      # finite bf16 above 65504 -> inf, no clamp
        assert same_values(out, x.permute(0, 2, 3, 1).reshape(N, H * W, C).float().to(dst))


# ------------------------------------------------------------------ 2. gf_fine_gather
def unfold_windows(feat, b, cells, dtype, window=5, stride=4):
    """FinePreprocess's own formulation (fine_preprocess.py:41-56): F.unfold of the fp32 maps, gather by (b, cell), rounded to dtype
    -> [M, window^2, C]."""
    N, C = feat.shape[:2]
    u = F.unfold(feat.float().contiguous(), kernel_size=(window, window), stride=stride, padding=window // 2)      # [N, C ww, L]
    u = u.view(N, C, window * window, -1).permute(0, 3, 2, 1)                                                      # [N, L, ww, C]
    return u[b, cells].to(dtype)


def _gather_case(src, dst, C, CC, channels_last, seed):
    """N = 2, fine maps 16 x 24 against 16 x 20 (4 x 6 and 4 x 5 coarse cells), M = 7 with the four corner cells of both grids
    (zero padding on two sides at once) and a repeated cell; values far outside fp16's range and below its resolution included."""
    g = torch.Generator().manual_seed(seed)

    def maps(h, w):
        t = torch.randn(2, C, h, w, generator=g)
        t = t * torch.exp2(torch.randint(-32, 20, t.shape, generator=g).float())       # 2^-32 .. 2^19: both ends of fp16's range
        t[0, 0, 0, 0], t[1, C - 1, h - 1, w - 1], t[0, 1, 0, 1] = float('inf'), float('-inf'), -0.0
        t = t.to(src).to(DEV)
        return t.contiguous(memory_format=torch.channels_last) if channels_last else t.contiguous()
    f0, f1 = maps(16, 24), maps(16, 20)
    c0 = torch.randn(2, 24, CC, generator=g).to(dst).to(DEV)
    c1 = torch.randn(2, 20, CC, generator=g).to(dst).to(DEV)
    b = torch.tensor([0, 1, 0, 1, 1, 0, 1], device=DEV)
    i = torch.tensor([0, 5, 18, 23, 9, 14, 9], device=DEV)          # corners of the 4 x 6 grid: 0, 5, 18, 23; cell 9 of sample 1 twice
    j = torch.tensor([19, 15, 4, 0, 7, 11, 7], device=DEV)          # corners of the 4 x 5 grid: 0, 4, 15, 19
    return f0, f1, c0, c1, b, i, j


def _gather(f0, f1, c0, c1, b, i, j, dst):
    from geoformer_amd import ops
    return ops.fine_gather(f0, f1, c0, c1, b, i, j, 6, 5, 4, 5, dst)


@pytest.mark.parametrize('src,dst', [(BF16, F16), (F16, BF16)], ids=['bf16_to_fp16', 'fp16_to_bf16'])
def test_fine_gather_converting_rows(src, dst):
    """C = 128 / CC = 256 channels-last: the one-wave-per-window kernel in its converting form, against F.unfold bit for bit, and
    against the general kernel (the same maps as a non-channels-last copy) bit for bit."""
    f0, f1, c0, c1, b, i, j = _gather_case(src, dst, 128, 256, True, 41)
    assert f0.stride(1) == 1 and f1.stride(1) == 1
    win, ccat = _gather(f0, f1, c0, c1, b, i, j, dst)
    M = len(b)
    assert win.dtype == dst and tuple(win.shape) == (2 * M, 25, 128) and tuple(ccat.shape) == (2 * M, 256)
    assert same_bits(win[:M], unfold_windows(f0, b, i, dst)) and same_bits(win[M:], unfold_windows(f1, b, j, dst))
    assert same_bits(ccat[:M], c0[b, i]) and same_bits(ccat[M:], c1[b, j])
    if src == BF16:
        assert bool(torch.isinf(win).sum() > torch.isinf(f0).sum())             # finite values beyond 65504 arrived as inf: no clamp
    assert bool((win[0, :2] == 0).all()) and bool((win[0, 12] != 0).any())      # corner cell: padded rows are zeros, the centre is not
    g0, g1 = f0.contiguous(), f1.contiguous()
    assert g0.stride(1) != 1
    win2, ccat2 = _gather(g0, g1, c0, c1, b, i, j, dst)
    assert same_bits(win, win2) and same_bits(ccat, ccat2)


def test_fine_gather_converting_general_kernel():
    """C = 12 NCHW maps: no 16-byte pieces, the general kernel converts element by element."""
    f0, f1, c0, c1, b, i, j = _gather_case(BF16, F16, 12, 24, False, 43)
    win, ccat = _gather(f0, f1, c0, c1, b, i, j, F16)
    M = len(b)
    assert same_bits(win[:M], unfold_windows(f0, b, i, F16)) and same_bits(win[M:], unfold_windows(f1, b, j, F16))
    assert same_bits(ccat[:M], c0[b, i]) and same_bits(ccat[M:], c1[b, j])


@pytest.mark.parametrize('src,dst', [(BF16, F16), (F16, BF16)], ids=['bf16_to_fp16', 'fp16_to_bf16'])
def test_fine_gather_rows_convert_every_pattern(src, dst):
    """All 65536 input patterns through the row kernel's in-register conversion: a 16 x 32 x 128 channels-last map holds each once.
    The 5 x 5 windows (stride 4) of its 4 x 8 cells reach rows 0..14 and columns 0..30 only, so the patterns are laid out three
    times: in order, in reverse order (the last row and column become the first) and rolled by half the map in both directions
    (for the two corners that the reversal maps onto each other)."""
    from geoformer_amd import ops

    def layouts(flat):
        a = flat.view(16, 32, 128)
        rolled = a.roll((8, 16), (0, 1))
        return (torch.stack([a, flat.flip(0).view(16, 32, 128)]).permute(0, 3, 1, 2),        # image 0: samples 0 and 1
                torch.stack([rolled, rolled]).permute(0, 3, 1, 2))                            # image 1
    f0, f1 = layouts(all_patterns(src, 65536))
    assert f0.stride(1) == 1 and f1.stride(1) == 1
    g = torch.Generator().manual_seed(47)
    c = torch.randn(2, 32, 256, generator=g).to(dst).to(DEV)
    cells = torch.arange(32, device=DEV).repeat(2)
    b = torch.arange(2, device=DEV).repeat_interleave(32)
    win, _ = ops.fine_gather(f0, f1, c, c, b, cells, cells, 8, 8, 4, 5, dst)
    assert same_values(win[:64], unfold_windows(f0, b, cells, dst)) and same_values(win[64:], unfold_windows(f1, b, cells, dst))
    seen = torch.zeros(65536, dtype=torch.bool, device=DEV)
    for o in layouts(torch.arange(65536, device=DEV)):
        seen[F.unfold(o.float().contiguous(), 5, stride=4, padding=2).long().flatten()] = True
    assert bool(seen.all())


# ------------------------------------------------------------------ 3. the mode == the fp16 mode on converted maps
def _exact_in_fp16(maps):
    """bf16 maps with the few values fp16 cannot hold exactly zeroed (those below its normal range, 2^-14); asserts they were few and
    that the result survives bf16 -> fp16 -> bf16 unchanged: a condition on the inputs, not a tolerance on the outputs."""
    out, small, total = [], 0, 0
    for t in maps:
        t = t.to(DEV).to(BF16)
        tiny = (t != 0) & (t.abs().float() < 2.0 ** -14)
        small, total = small + int(tiny.sum()), total + t.numel()
        t = torch.where(tiny, torch.zeros((), dtype=BF16, device=DEV), t)
        assert same_bits(t.to(F16).to(BF16), t)
        out.append(t)
    assert small < 1e-3 * total, (small, total)
    return out


def _forward_case(name):
    if name == 'hpatches_unequal':         # 480 x 640 against 480 x 608, N = 1, the thresholds of the outcome test
        (c0, f0), (c1, f1), _ = GI.hpatches_like_features(0, 1)
        return {'image0': torch.zeros(1, 1, 480, 640), 'image1': torch.zeros(1, 1, 480, 608)}, (c0, f0, c1, f1), 0.2, 0.1
    case = GI.g10_cases()['g10b_e2e_planted_n2']
    (c0, f0), (c1, f1) = case['feats']
    return case['data'], (c0, f0, c1, f1), case['coarse_thr'], case['fine_thr']


@pytest.mark.parametrize('name', ['hpatches_unequal', 'planted_n2'])
def test_mode_equals_fp16_mode_on_converted_maps(name):
    from test_e2e_gpu import build, to_dev
    data, maps, thr, fthr = _forward_case(name)
    maps = _exact_in_fp16(maps)
    if name == 'hpatches_unequal':         # channels-last like the backbone's output: the vector / row kernels; the other case: NCHW
        maps = [t.contiguous(memory_format=torch.channels_last) for t in maps]
    mixed, half = build(thr, fthr, 'bf16_fp16'), build(thr, fthr, 'fp16')
    assert (mixed.compute_dtype, mixed.backbone_dtype) == (F16, BF16)
    with torch.no_grad():
        got = mixed.forward_features(to_dev(data), *maps)
        ref = half.forward_features(to_dev(data), *(t.to(F16) for t in maps))
    assert len(ref['b_ids']) > 20 and len(ref['mconf']) > 10, name
    for k in OUT_KEYS:
        assert got[k].dtype == ref[k].dtype and torch.equal(got[k], ref[k]), (name, k)
    for k, t in got['_feat_dev'].items():
        assert t.dtype == F16, (name, k, t.dtype)


# ------------------------------------------------------------------ 4. from images
def test_forward_from_images_eager_and_graphed():
    """Unequal shapes at batch 1 (160 x 160 against 160 x 128: two backbone calls): the mode's forward == the bf16 mode's backbone,
    its four maps converted to fp16, the fp16 mode's matching path - bit for bit; the backbone's maps stay bf16; graph replay == eager."""
    from geoformer_amd import miopen
    from test_e2e_gpu import build
    miopen.use_shipped_find_db()
    i0, i1 = (t.to(DEV) for t in GI.textured_pair(160, 160, 960))
    i1 = i1[..., :128].contiguous()
    mixed, whole, half = build(0.0, 0.0, 'bf16_fp16'), build(0.0, 0.0, 'bf16'), build(0.0, 0.0, 'fp16')
    with torch.no_grad():
        eager = mixed({'image0': i0, 'image1': i1})
        (c0, f0), (c1, f1) = whole._backbone(i0), whole._backbone(i1)
        assert {t.dtype for t in (c0, f0, c1, f1)} == {BF16}
        for im, want in ((i0, (c0, f0)), (i1, (c1, f1))):          # the eager mixed path itself: its own backbone hands over the same bf16 maps
            own = mixed._backbone(im)
            assert [t.dtype for t in own] == [BF16] * 2 and all(torch.equal(a, b) for a, b in zip(own, want))
        ref = half.forward_features({'image0': i0, 'image1': i1}, *(t.to(F16) for t in (c0, f0, c1, f1)))
        assert len(ref['b_ids']) > 5 and len(ref['mconf']) > 0
        for k in OUT_KEYS:
            assert torch.equal(eager[k], ref[k]), k
        assert all(t.dtype == F16 for t in eager['_feat_dev'].values())
        mixed.enable_graphs()
        for _ in range(2):                                         # capture + replay, then a replay alone
            graphed = mixed({'image0': i0, 'image1': i1})
            assert len(mixed._graphs) == 1
            feats = graphed['_backbone_feats']
            assert [t.dtype for t in feats] == [BF16] * 4
            for t, want in zip(feats, (c0, f0, c1, f1)):
                assert torch.equal(t, want)
            for k in OUT_KEYS:
                assert torch.equal(graphed[k], eager[k]), k
        mixed.enable_graphs(False)


# ------------------------------------------------------------------ 5. matcher
def test_matcher_in_the_mode(tmp_path):
    from PIL import Image
    from geoformer_amd import matcher as MT
    from geoformer_amd.weights import deterministic_init_
    rng = np.random.default_rng(5)
    w, h = 200, 168
    paths = [os.path.join(str(tmp_path), f'{k}.ppm') for k in (1, 2)]
    for p in paths:
        Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(p)
    m = MT.GeoFormerMatcher(imsize=160, match_threshold=0.0, precision='bf16_fp16')
    deterministic_init_(m.model)
    m.model.fine_matching.thr = 0.0
    assert (m.model.precision, m.model.compute_dtype, m.model.backbone_dtype) == ('bf16_fp16', F16, BF16)
    assert {p.dtype for p in m.model.backbone.parameters()} == {BF16}
    res = m.match_pairs(*paths)
    assert len(res) == 4
    matches, k1, k2, scores = res
    assert len(matches) > 0 and matches.shape[1] == 4 and len(k1) == len(k2) == len(scores) == len(matches)
    assert np.isfinite(matches).all() and np.isfinite(scores).all() and scores.min() >= 0 and scores.max() <= 1
    # a fine keypoint is its coarse cell's centre moved by at most 2 fine pixels = 4 pixels of the resized image (184 x 160 here)
    reach = 4 * max(w / 184, h / 160)
    for k in (k1, k2):
        assert k[:, 0].min() >= -reach and k[:, 0].max() <= w + reach and k[:, 1].min() >= -reach and k[:, 1].max() <= h + reach
