"""The one pos_encode kernel and the one fine_gather kernel pair behind their three map sources (batch tensor, address table, record
table), on inputs that only the shared code paths see: strided and cropped views through the tensor entries, more samples than a grid
dimension holds, and record tables whose entries take different paths in one launch.  Every comparison is on bits (torch.equal) against a
torch formula.

Every map is a view into a larger allocation whose other elements are 77 (or random and non-zero): a read outside a view shows up as a
wrong value, not as a silent zero."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
MARGIN = 64                     # elements of 77 in front of and behind every strided map (keeps 32-byte alignment for every dtype)


def _pe_formula(x, pe, tout):
    return (x.float() + pe.permute(2, 0, 1)).to(tout).flatten(2).transpose(1, 2)


# ------------------------------------------------------------------------------------------------------------------------------
# A. pos_encode, tensor entry, strided views: every second sample of a parent, cropped in both directions
# ------------------------------------------------------------------------------------------------------------------------------
PE_PARENTS = {                     # name -> (parent shape in memory order, channels-last?)
    'nhwc_vector': ((4, 6, 9, 16), True),      # C % 8 == 0, strides multiples of 8, the view's base a multiple of 32 bytes: 8 channels per lane
    'nhwc_c20': ((4, 6, 9, 20), True),         # C % 8 != 0: one element per lane
    'nchw': ((4, 40, 6, 9), False),            # the LDS transpose with a row stride (9) that is not the view's width (5)
}


@pytest.mark.parametrize('tin,tout', [(F16, F16), (BF16, F16), (F32, F32)], ids=lambda t: str(t).split('.')[-1])
@pytest.mark.parametrize('parent', list(PE_PARENTS))
def test_pos_encode_tensor_entry_reads_a_strided_cropped_view(parent, tin, tout):
    from geoformer_amd import ops
    shape, channels_last = PE_PARENTS[parent]
    buf = torch.full(shape, 77.0, dtype=tin, device=DEV)
    x = (buf.permute(0, 3, 1, 2) if channels_last else buf)[1::2, :, 1:4, 2:7]
    N, C, H, W = x.shape
    assert (N, H, W) == (2, 3, 5) and (x.stride(1) == 1) == channels_last
    if parent == 'nhwc_vector':
        assert x.data_ptr() % 32 == 0
    g = torch.Generator().manual_seed(3)
    x.copy_((torch.randn(N, C, H, W, generator=g) * 3).to(tin))
    pe = torch.randn(H, W, C, generator=g).to(DEV)
    got = ops.pos_encode(x, pe, tout)
    assert got.shape == (N, H * W, C) and got.dtype == tout
    assert torch.equal(got, _pe_formula(x, pe, tout))


# ------------------------------------------------------------------------------------------------------------------------------
# B. fine_gather, tensor entry, cropped views: memory continues behind every edge of the extent
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', [40, 39])
@pytest.mark.parametrize('form,dtype', [('rows', F16), ('general', F32)], ids=lambda t: str(t).split('.')[-1])
def test_fine_gather_tensor_entry_reads_cropped_views(form, dtype, M):
    """Side 0: the 16 x 20 view [4:20, 8:28] of a [2,128,20,28] parent, 4 x 5 coarse cells; side 1: the 12 x 16 view [4:16, 8:24], 3 x 4 cells;
    stride 4, window 5, CC = 256.  Every (sample, cell of side 0) with j = i % 12; M = 39: one match dropped, 2M % 4 != 0."""
    from geoformer_amd import ops
    g = torch.Generator().manual_seed(11)
    parents = []
    for _ in range(2):
        p = (torch.randn(2, 20, 28, 128, generator=g) * 3).to(dtype).to(DEV)          # random and non-zero: a tap read outside a view is seen
        parents.append(p.permute(0, 3, 1, 2) if form == 'rows' else p.permute(0, 3, 1, 2).contiguous())
    f0, f1 = parents[0][:, :, 4:20, 8:28], parents[1][:, :, 4:16, 8:24]
    assert f0.shape == (2, 128, 16, 20) and f1.shape == (2, 128, 12, 16) and (f0.stride(1) == 1) == (form == 'rows')
    c0 = torch.randn(2, 20, 256, generator=g).to(dtype).to(DEV)
    c1 = torch.randn(2, 12, 256, generator=g).to(dtype).to(DEV)
    b = [n for n in range(2) for _ in range(20)]
    i = [c for _ in range(2) for c in range(20)]
    if M == 39:
        del b[17], i[17]
    assert len(b) == M
    b, i = torch.tensor(b, device=DEV), torch.tensor(i, device=DEV)
    j = i % 12
    win, ccat = ops.fine_gather(f0, f1, c0, c1, b, i, j, 5, 4, 4, 5, dtype)
    assert win.shape == (2 * M, 25, 128) and ccat.shape == (2 * M, 256) and win.dtype == dtype
    unf0 = torch.nn.functional.unfold(f0.contiguous().float(), kernel_size=5, stride=4, padding=2).view(2, 128, 25, 20)
    unf1 = torch.nn.functional.unfold(f1.contiguous().float(), kernel_size=5, stride=4, padding=2).view(2, 128, 25, 12)
    assert torch.equal(win[:M], unf0[b, :, :, i].permute(0, 2, 1).to(dtype))
    assert torch.equal(win[M:], unf1[b, :, :, j].permute(0, 2, 1).to(dtype))
    assert torch.equal(ccat[:M], c0[b, i]) and torch.equal(ccat[M:], c1[b, j])
    # a corner cell: window rows and columns 0, 1 are F.unfold's padding - in memory, the parent's rows 2, 3 and columns 6, 7
    w = win[:M][(b == 1) & (i == 0)][0].view(5, 5, 128)
    assert bool((w[:2] == 0).all()) and bool((w[:, :2] == 0).all()) and bool((w[2:, 2:] != 0).any())


# ------------------------------------------------------------------------------------------------------------------------------
# C. pos_encode, tensor entry, more samples than a grid dimension holds
# ------------------------------------------------------------------------------------------------------------------------------
def test_pos_encode_tensor_entry_takes_more_than_65535_samples():
    from geoformer_amd import ops
    g = torch.Generator().manual_seed(5)
    N = 65537
    x = torch.randn(N, 1, 1, 8, generator=g).to(F16).to(DEV).permute(0, 3, 1, 2)
    pe = torch.randn(1, 1, 8, generator=g).to(DEV)
    got = ops.pos_encode(x, pe, F16)
    assert got.shape == (N, 1, 8)
    assert torch.equal(got, _pe_formula(x, pe, F16))


# ------------------------------------------------------------------------------------------------------------------------------
# D. one record table whose entries differ in eligibility for the 16-byte paths
# ------------------------------------------------------------------------------------------------------------------------------
FG_EXT0, FG_EXT1 = [(4, 5), (3, 5), (4, 3)], [(3, 4), (2, 4), (3, 2)]       # coarse extents on canvases of 4 x 5 and 3 x 4 cells
MIXED = [(0, 1), (4, 1), (0, 2)]            # (elements added to the row stride, pixel stride in units of C) of maps 0, 1, 2


def _strided_map(c, h, w, seed, row_pad, pix):
    """A channels-last fp16 [c,h,w] map with pixel stride pix * c and row stride w * pix * c + row_pad, inside a 77-filled allocation."""
    sw = pix * c
    sh = w * sw + row_pad
    flat = torch.full((MARGIN + h * sh + MARGIN,), 77.0, dtype=F16, device=DEV)
    m = flat.as_strided((c, h, w), (1, sh, sw), MARGIN)
    m.copy_((torch.randn(c, h, w, generator=torch.Generator().manual_seed(seed)) * 3).to(F16))
    assert m.data_ptr() % 32 == 0
    return m


def _mixed_maps(extents, scale, seed):
    maps = [_strided_map(128, scale * h, scale * w, seed + k, *MIXED[k]) for k, (h, w) in enumerate(extents)]
    assert [(m.stride(1) % 8, m.stride(2) % 8) for m in maps] == [(0, 0), (4, 0), (0, 0)] and maps[2].stride(2) == 256
    return maps


def _pad_stack(maps, H, W):
    """Dense channels-last copies of the maps, zero-padded at the right and bottom to H x W and stacked."""
    out = torch.zeros(len(maps), H, W, maps[0].shape[0], dtype=maps[0].dtype, device=DEV).permute(0, 3, 1, 2)
    for n, m in enumerate(maps):
        out[n, :, :m.shape[1], :m.shape[2]] = m
    return out


def test_pos_encode_ragged_table_of_mixed_eligibility():
    from geoformer_amd import ops
    maps = _mixed_maps(FG_EXT0, 1, 40)
    pe = torch.randn(4, 5, 128, generator=torch.Generator().manual_seed(6)).to(DEV)
    mask = torch.full((3, 4, 5), 9, dtype=torch.uint8, device=DEV)
    got = ops.pos_encode(ops.RaggedMapBatch(maps), pe, F16, mask_out=mask)
    assert torch.equal(got, _pe_formula(_pad_stack(maps, 4, 5), pe, F16))
    hs, ws = (torch.tensor(v, device=DEV)[:, None, None] for v in zip(*FG_EXT0))
    want = (torch.arange(4, device=DEV)[None, :, None] < hs) & (torch.arange(5, device=DEV)[None, None, :] < ws)
    assert torch.equal(mask, want.to(torch.uint8))


def test_fine_gather_ragged_tables_of_mixed_eligibility():
    from geoformer_amd import ops
    maps0, maps1 = _mixed_maps(FG_EXT0, 4, 50), _mixed_maps(FG_EXT1, 4, 60)
    g = torch.Generator().manual_seed(7)
    c0 = torch.randn(3, 20, 256, generator=g).to(F16).to(DEV)
    c1 = torch.randn(3, 12, 256, generator=g).to(F16).to(DEV)
    b, i, j = [], [], []
    for n in range(3):                                 # every own cell of every sample on side 0, j cycling through the sample's own cells on side 1
        ci = [y * 5 + x for y in range(FG_EXT0[n][0]) for x in range(FG_EXT0[n][1])]
        cj = [y * 4 + x for y in range(FG_EXT1[n][0]) for x in range(FG_EXT1[n][1])]
        b += [n] * len(ci)
        i += ci
        j += [cj[k % len(cj)] for k in range(len(ci))]
    M = len(b)
    assert M == 47
    b, i, j = (torch.tensor(v, device=DEV) for v in (b, i, j))
    win, ccat = ops.fine_gather(ops.RaggedMapBatch(maps0), ops.RaggedMapBatch(maps1), c0, c1, b, i, j, 5, 4, 4, 5, F16)
    p0, p1 = _pad_stack(maps0, 16, 20), _pad_stack(maps1, 12, 16)
    unf0 = torch.nn.functional.unfold(p0.float(), kernel_size=5, stride=4, padding=2).view(3, 128, 25, 20)
    unf1 = torch.nn.functional.unfold(p1.float(), kernel_size=5, stride=4, padding=2).view(3, 128, 25, 12)
    assert win.shape == (2 * M, 25, 128) and win.dtype == F16
    assert torch.equal(win[:M], unf0[b, :, :, i].permute(0, 2, 1).to(F16))
    assert torch.equal(win[M:], unf1[b, :, :, j].permute(0, 2, 1).to(F16))
    assert torch.equal(ccat[:M], c0[b, i]) and torch.equal(ccat[M:], c1[b, j])
