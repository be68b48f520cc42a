"""K3 with a row-address table as its A operand (ops.linear_rows) and the fine-level entry built on it (ops.fine_rows,
FinePreprocess.forward without the window copy).  Every comparison is on bits (torch.equal) against the copying path on the same inputs:
ops.linear on the gathered rows, ops.fine_gather plus ops.linear.

Rows and maps are views into larger allocations filled with 77 or with random non-zero values: a read beside a named row shows up as a
wrong value, not as a silent zero."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------------------------------------
# A. the engine: linear_rows against linear on the gathered copy
# ------------------------------------------------------------------------------------------------------------------------------
def _table(M, K, dtype, seed):
    """40 source rows of K elements with a row stride of K + 8 inside a 77-filled buffer; a table of M entries that repeats rows (M > 40
    always does, smaller M by construction) and holds a block of nine zero addresses (M > 1).  -> (int64 table, the gathered copy, the
    buffer itself: the table only names its rows, the caller keeps it alive)."""
    g = torch.Generator().manual_seed(seed)
    R, ld = 40, K + 8
    buf = torch.full((R, ld), 77.0, dtype=dtype, device=DEV)
    buf[:, :K] = torch.randn(R, K, generator=g).to(dtype).to(DEV)
    idx = torch.randint(0, R, (M,), generator=g)
    if M > 2:
        idx[M - 1] = idx[0]                                   # a repeated row, whatever the draw
    zero = torch.zeros(M, dtype=torch.bool)
    if M > 1:
        zero[M // 3:M // 3 + 9] = True
    assert buf.data_ptr() % 16 == 0 and (ld * 2) % 16 == 0
    table = (buf.data_ptr() + idx * (ld * 2)).masked_fill(zero, 0).to(DEV)
    gathered = buf[idx.to(DEV), :K].masked_fill(zero.to(DEV)[:, None], 0).contiguous()
    return table, gathered, buf


@pytest.mark.parametrize('N', [128, 512])
@pytest.mark.parametrize('K', [128, 256])
@pytest.mark.parametrize('M', [1, 127, 128, 300])
@pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])
def test_linear_rows_matches_linear_on_the_gathered_copy(dtype, M, K, N):
    from geoformer_amd import ops
    table, gathered, _keep = _table(M, K, dtype, 1000 + M + K + N)
    g = torch.Generator().manual_seed(7)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    got = ops.linear_rows(table, w, bias=bias)
    assert got.shape == (M, N) and got.dtype == dtype
    assert torch.equal(got, ops.linear(gathered, w, bias=bias))
    # 25-row groups (the fine windows): M = 127 and 300 are no multiples of 128, M = 127 none of 25 either
    rg = torch.randn((M + 24) // 25, N, generator=g).to(dtype).to(DEV)
    got = ops.linear_rows(table, w, rowgroup_bias=rg, rowgroup_rows=25)
    assert torch.equal(got, ops.linear(gathered, w, rowgroup_bias=rg, rowgroup_rows=25))


@pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])
def test_linear_rows_zero_address_is_a_row_of_zeros_and_epilogues_follow_linear(dtype):
    from geoformer_amd import ops
    g = torch.Generator().manual_seed(9)
    w = (torch.randn(128, 128, generator=g) / 11.0).to(dtype).to(DEV)
    bias = torch.randn(128, generator=g).to(DEV)
    got = ops.linear_rows(torch.zeros(1, dtype=torch.int64, device=DEV), w, bias=bias)
    assert torch.equal(got, bias.to(dtype)[None])
    table, gathered, _keep = _table(130, 128, dtype, 5)
    ln = (torch.randn(128, generator=g).to(DEV), torch.randn(128, generator=g).to(DEV))
    res = torch.randn(130, 128, generator=g).to(dtype).to(DEV)
    for kw in ({'epilogue': ops.EPI_RELU}, {'epilogue': ops.EPI_TANH}, {'epilogue': ops.EPI_LN, 'ln': ln},
               {'epilogue': ops.EPI_LN_RES, 'ln': ln, 'residual': res}):
        assert torch.equal(ops.linear_rows(table, w, bias=bias, **kw), ops.linear(gathered, w, bias=bias, **kw)), kw


def test_linear_rows_argument_errors():
    from geoformer_amd import ops, _lib
    t = torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.GeoFormerHipError, match='16-bit'):
        ops.linear_rows(t, torch.zeros(128, 128, device=DEV))
    w = torch.zeros(128, 128, dtype=F16, device=DEV)
    with pytest.raises(_lib.GeoFormerHipError, match='16-byte aligned'):
        ops.linear_rows(t, w, row_align=8)
    h = _lib.lib()
    assert h.gf_linear_rows(None, 16, None, 0, 0, 128, w.data_ptr(), None, None, 0, 0, None, None, 1e-5, None, 0, None, 0, w.data_ptr(), 128, 1, 4, 128, None) == -1
    assert b'null pointer' in h.gf_last_error()


# ------------------------------------------------------------------------------------------------------------------------------
# B. the fine-level entry: FinePreprocess.forward against fine_gather + linear, three map sources
# ------------------------------------------------------------------------------------------------------------------------------
HC, WC, STRIDE, WIN = 8, 12, 4, 5                      # coarse grid 8 x 12, fine maps 32 x 48, 5 x 5 windows
EXT = [(8, 12), (6, 10)]                               # ragged source: the samples' own coarse extents on the 8 x 12 canvas


def _matches(M, ext):
    """M matches (b, i, j) over two samples, match k in sample k % 2.  Per sample, first the special cells - where the sample's own extent
    is smaller than the canvas, the canvas cells just below and right of it (window taps outside the extent with memory behind them:
    zeros), then the four corners, a cell on each border and an interior cell of its OWN extent - then random own cells.  Cells are
    counted on the canvas.  M = 1: sample 0's top left corner."""
    g = torch.Generator().manual_seed(M)
    b, i, j = [], [], []
    for k in range(M):
        n = k % 2
        h, w = ext[n]
        special = [(h, w // 2)] * (h < HC) + [(h // 2, w)] * (w < WC)
        special += [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1), (h // 2, w // 2)]
        yi, xi = special[k // 2] if k // 2 < len(special) else (int(torch.randint(0, h, (1,), generator=g)), int(torch.randint(0, w, (1,), generator=g)))
        yj, xj = special[(k // 2 + 3) % len(special)] if k // 2 < len(special) else (int(torch.randint(0, h, (1,), generator=g)), int(torch.randint(0, w, (1,), generator=g)))
        b.append(n)
        i.append(yi * WC + xi)
        j.append(yj * WC + xj)
    return tuple(torch.tensor(v, device=DEV) for v in (b, i, j))


def _fine_maps(source, dtype, seed):
    """Two channels-last fine maps per side as `source` hands them over, each a crop of a larger random (non-zero) parent."""
    from geoformer_amd import ops
    g = torch.Generator().manual_seed(seed)
    H, W = HC * STRIDE, WC * STRIDE
    sides = []
    for _ in range(2):
        parent = (torch.randn(2, H + 8, W + 8, 128, generator=g) * 3).to(dtype).to(DEV).permute(0, 3, 1, 2)
        full = parent[:, :, 4:4 + H, 8:8 + W]
        if source == 'tensor':
            sides.append(full)
        elif source == 'table':
            sides.append(ops.MapBatch([full[0], full[1]]))
        else:
            sides.append(ops.RaggedMapBatch([full[n, :, :h * STRIDE, :w * STRIDE] for n, (h, w) in enumerate(EXT)], canvas=(H, W)))
    return sides


def _preprocess(dtype):
    from geoformer_amd.model.modules import FinePreprocess
    from geoformer_amd.model.cvpr_ds_config import get_default_cfg
    torch.manual_seed(3)
    return FinePreprocess(get_default_cfg()).to(DEV).eval()


def _parent_path(fp, f0, f1, c0, c1, b, i, j, dtype):
    """FinePreprocess.forward as it was before the row tables: the copies, then three plain GEMMs."""
    from geoformer_amd import ops
    w = fp.weights(dtype)
    win, ccat = ops.fine_gather(f0, f1, c0, c1, b, i, j, WC, WC, STRIDE, WIN, dtype)
    ctx = ops.linear(ops.linear(ccat, w['dw'], bias=w['db']), w['mw_ctx'], bias=w['mb'])
    out = ops.linear(win, w['mw_win'], rowgroup_bias=ctx, rowgroup_rows=WIN * WIN)
    M = b.shape[0]
    return out[:M], out[M:], win


def _count_calls(monkeypatch, name):
    from geoformer_amd import ops
    calls, real = [], getattr(ops, name)

    def wrapped(*a, **k):
        calls.append(name)
        return real(*a, **k)
    monkeypatch.setattr(ops, name, wrapped)
    return calls


def _run_forward(fp, f0, f1, c0, c1, b, i, j):
    data = {'hw0_f': torch.tensor([HC * STRIDE, WC * STRIDE]), 'hw0_c': torch.tensor([HC, WC]), 'hw1_c': torch.tensor([HC, WC]),
            'b_ids': b, 'i_ids': i, 'j_ids': j}
    with torch.no_grad():
        return fp(f0, f1, c0, c1, data)


@pytest.mark.parametrize('M', [1, 7, 150])
@pytest.mark.parametrize('source', ['tensor', 'table', 'ragged'])
@pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])
def test_fine_preprocess_reads_the_rows_in_place(dtype, source, M, monkeypatch):
    fp = _preprocess(dtype)
    f0, f1 = _fine_maps(source, dtype, 21)
    g = torch.Generator().manual_seed(22)
    c0, c1 = (torch.randn(2, HC * WC, 256, generator=g).to(dtype).to(DEV) for _ in range(2))
    b, i, j = _matches(M, EXT if source == 'ragged' else [(HC, WC)] * 2)
    want0, want1, win = _parent_path(fp, f0, f1, c0, c1, b, i, j, dtype)
    assert bool((win[0, 0] == 0).all())                                      # match 0 sits on a corner: its first tap is padding
    if source == 'ragged' and M > 1:
        below = win[1].view(5, 5, 128)                                       # match 1: sample 1, the canvas cell just below its own extent
        assert bool((below[2:] == 0).all()) and bool((below[:2] != 0).any())
    gathers, tables = _count_calls(monkeypatch, 'fine_gather'), _count_calls(monkeypatch, 'fine_rows')
    got0, got1 = _run_forward(fp, f0, f1, c0, c1, b, i, j)
    assert not gathers and tables == ['fine_rows']
    assert got0.shape == (M, 25, 128) and got0.dtype == dtype
    assert torch.equal(got0, want0) and torch.equal(got1, want1)


def test_fine_preprocess_bf16_maps_fp16_windows_keep_the_gather(monkeypatch):
    """The bf16-backbone / fp16-matching mode converts while it gathers: nothing to name, the copying path stays."""
    fp = _preprocess(F16)
    f0, f1 = _fine_maps('tensor', BF16, 31)
    g = torch.Generator().manual_seed(32)
    c0, c1 = (torch.randn(2, HC * WC, 256, generator=g).to(F16).to(DEV) for _ in range(2))
    b, i, j = _matches(7, [(HC, WC)] * 2)
    want0, want1, _ = _parent_path(fp, f0, f1, c0, c1, b, i, j, F16)
    gathers, tables = _count_calls(monkeypatch, 'fine_gather'), _count_calls(monkeypatch, 'fine_rows')
    got0, got1 = _run_forward(fp, f0, f1, c0, c1, b, i, j)
    assert gathers == ['fine_gather'] and not tables
    assert torch.equal(got0, want0) and torch.equal(got1, want1)


def test_fine_rows_names_every_tap_and_coarse_row():
    """The tables themselves: reading the named rows back gives fine_gather's windows and coarse rows, zeros where the address is 0."""
    from geoformer_amd import ops
    f0, f1 = _fine_maps('ragged', F16, 41)
    g = torch.Generator().manual_seed(42)
    c0, c1 = (torch.randn(2, HC * WC, 256, generator=g).to(F16).to(DEV) for _ in range(2))
    b, i, j = _matches(150, EXT)
    win, ccat = ops.fine_gather(f0, f1, c0, c1, b, i, j, WC, WC, STRIDE, WIN, F16)
    win_rows, c_rows = ops.fine_rows(f0, f1, c0, c1, b, i, j, WC, WC, STRIDE, WIN)
    assert win_rows.shape == (300, 25) and c_rows.shape == (300,) and int((win_rows == 0).sum()) > 0
    assert torch.equal((win_rows == 0), (win == 0).all(-1))
    eye = torch.eye(128, dtype=F16, device=DEV)              # the identity as weights: the product IS the gathered rows
    assert torch.equal(ops.linear_rows(win_rows, eye), win)
    assert torch.equal(ops.linear_rows(c_rows, torch.eye(256, dtype=F16, device=DEV)), ccat)


# ------------------------------------------------------------------------------------------------------------------------------
# C. GeoTransformer's self layer: k | v projected at the inlier tokens only, against the projection of every token
# ------------------------------------------------------------------------------------------------------------------------------
def _self_layer_case(L, dtype, seed):
    """One 'self' layer on N = 2 pairs (four images) with key counts 0, 1, 37 and L; the token lists hold distinct tokens below the count
    and garbage (negative, huge) behind it."""
    from geoformer_amd.model.modules import GeoTransformer
    torch.manual_seed(seed)
    gt = GeoTransformer({'nhead': 4}, ['self'], 256, linear=False).to(DEV).eval()
    g = torch.Generator().manual_seed(seed + 1)
    both = torch.randn(4, L, 256, generator=g).to(dtype).to(DEV)
    counts = [0, 1, 37, L]
    idx = torch.empty(4, L, dtype=torch.int32)
    for n, c in enumerate(counts):
        idx[n, :c] = torch.randperm(L, generator=g)[:c].to(torch.int32)
        idx[n, c:] = torch.tensor([-7, 0x7FFFFFF0, L, -(1 << 31)], dtype=torch.int64).to(torch.int32).repeat(L)[:L - c]
    idx = idx.to(DEV)
    nidx = torch.tensor(counts, dtype=torch.int32, device=DEV)
    geo = {'nidx': nidx.view(2, 2).t().contiguous(), 'idx_both': idx, 'nidx_both': nidx, 'idx0': idx[:2], 'idx1': idx[2:]}
    return gt, both, geo


def _self_layer(gt, both, geo):
    with torch.no_grad():
        f0, f1 = gt(both[:2], both[2:], geo, both=both)
    return torch.cat([f0, f1], 0)


@pytest.mark.parametrize('L', [96, 256])
@pytest.mark.parametrize('dtype', [F16, BF16], ids=['f16', 'bf16'])
def test_geo_self_layer_projects_keys_at_the_inlier_tokens_only(dtype, L, monkeypatch):
    gt, both, geo = _self_layer_case(L, dtype, 50 + L)
    gt.kv_at_inliers = False
    want = _self_layer(gt, both, geo)                       # q | k | v of every token in one GEMM, K4 gathers by the list
    gt.kv_at_inliers = True
    tables = _count_calls(monkeypatch, 'linear_rows')
    got = _self_layer(gt, both, geo)
    assert tables == ['linear_rows']
    assert torch.equal(got, want)
    assert torch.equal(got[0], both[0]) and not torch.equal(got[3], both[3])          # no keys: the image keeps its features


def test_geo_self_layer_replays_from_a_captured_graph():
    gt, both, geo = _self_layer_case(96, F16, 70)
    g = torch.Generator().manual_seed(71)
    geo['idx_both'] = torch.stack([torch.randperm(96, generator=g) for _ in range(4)]).to(torch.int32).to(DEV)     # valid under any count
    x = both.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _self_layer(gt, x, geo)                             # first use outside the capture: workspaces, the cached identity list
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = _self_layer(gt, x, geo)
    for k in range(2):
        x.copy_(both.roll(k + 1, 1))
        geo['nidx_both'].copy_(geo['nidx_both'].roll(1))    # the counts live on the device: a replay follows them
        graph.replay()
        torch.cuda.synchronize()
        gt.kv_at_inliers = False
        want = _self_layer(gt, x, geo)                      # eagerly, k | v of every token
        gt.kv_at_inliers = True
        assert torch.equal(out, want)


def test_identity_list_first_made_inside_a_capture_is_not_kept():
    """The cached token list must never be a tensor of some graph's memory pool: a first call inside a capture gets its own list."""
    from geoformer_amd.model.modules import GeoTransformer
    gt = GeoTransformer({'nhead': 4}, ['self'], 256, linear=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        inside = gt._identity(4, 96, torch.device(DEV, torch.cuda.current_device()))
    assert not gt._ident
    graph.replay()
    torch.cuda.synchronize()
    want = torch.arange(96, dtype=torch.int32, device=DEV).expand(4, 96)
    assert inside.stride(0) == 0 and torch.equal(inside, want)
    kept = gt._identity(4, 96, torch.device(DEV, torch.cuda.current_device()))
    assert len(gt._ident) == 1 and torch.equal(kept, want) and kept.data_ptr() != inside.data_ptr()
