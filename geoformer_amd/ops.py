"""Thin torch-tensor front end of the C ABI: pointer plumbing, workspace caching, stream passing.

Every function enqueues on torch's current stream and returns device tensors; data-dependent
counts stay on the device (`counts` tensors) until a caller needs their value.
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import GF_BF16, GF_F16, GF_F32, check

_DTYPES = {torch.float32: GF_F32, torch.float16: GF_F16, torch.bfloat16: GF_BF16}


def _dt(t):
    try:
        return _DTYPES[t.dtype]
    except KeyError:
        raise TypeError(f'geoformer_amd kernels take float32, float16 or bfloat16 tensors, got {t.dtype}') from None


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_raw_device = getattr(torch._C, '_cuda_getDevice', None)


def _stream_handle(device=None):
    """torch's current HIP stream (of `device`, default: the current device) as an integer handle.  Through the two C-level getters when
    this torch build has them: torch.cuda.current_stream() costs ~8 us of Python per call - a millisecond per batch-1 pair at 113 launches."""
    if _raw_stream is not None and _raw_device is not None:
        idx = _raw_device() if device is None else (device.index if isinstance(device, torch.device) else device)
        if isinstance(idx, int):
            return _raw_stream(idx)
    return torch.cuda.current_stream(device).cuda_stream


def _stream():
    return ctypes.c_void_p(_stream_handle())


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.GeoFormerHipError('geoformer_amd ops need CUDA(HIP) tensors; there is no CPU path')


class _Workspaces:
    """One growing byte buffer per (device, tag, stream)."""

    def __init__(self):
        self.bufs = {}

    def get(self, tag, nbytes, device):
        key = (device, tag, _stream_handle(device))
        b = self.bufs.get(key)
        if b is None or b.numel() < nbytes:
            b = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
            self.bufs[key] = b
        return b


_ws = _Workspaces()


def _contig(t):
    return t if t.is_contiguous() else t.contiguous()


def match_only_supported(f0, f1, masked=False, force_one=False):
    """Is the match-only mode of K1 (conf_matrix not materialised) built for these operands?"""
    return bool(_lib.lib().gf_dual_softmax_match_only_supported(_dt(f0), f0.shape[1], f1.shape[1], f0.shape[2], int(masked), int(bool(force_one))))


def dual_softmax_conf_at(f0, f1, temperature, b, i, j):
    """Single entries conf[b, i, j] (fp32 [P]) recomputed bit-identically to the matrix gf_dual_softmax_match writes, from the same
    features and the statistics its last call on this device and stream left in the workspace (match-only mode's way to a few
    values).  The workspace is stamped by that call with (N, L, S, C, temperature, the two feature pointers): when the stamp
    does not belong to THESE arguments - another pair of feature tensors was matched since (GeoFormer.forward runs two
    CoarseMatching passes on one workspace), the shape changed - or an index is out of range, the entry comes back NaN.  The stamp also
    carries a fingerprint of the features' CONTENT (64 sampled 8-byte words, 512 bytes in all): a new tensor that the caching allocator
    placed at a freed tensor's address does not pass for it.  It is a SAMPLED check: an in-place edit of the stamped tensors that misses
    the sampled words (one masked row, say) still passes - after editing the features in place, call dual_softmax_match again before
    asking for entries.  The features must be contiguous (the very tensors the match call got): a copy made here
    would never carry the stamped pointers."""
    _need_cuda(f0, f1)
    if not (f0.is_contiguous() and f1.is_contiguous()):
        raise ValueError('dual_softmax_conf_at: pass the contiguous feature tensors gf_dual_softmax_match was called with')
    N, L, C = f0.shape
    S = f1.shape[1]
    b, i, j = (_contig(t.to(device=f0.device, dtype=torch.int64)) for t in (b, i, j))
    out = torch.empty(b.numel(), dtype=torch.float32, device=f0.device)
    L_ = _lib.lib()
    ws = _ws.get('k1', L_.gf_dual_softmax_workspace_bytes(N, L, S), f0.device)
    check(L_.gf_dual_softmax_conf_at(_p(f0), _p(f1), _dt(f0), N, L, S, C, float(temperature), _p(b), _p(i), _p(j), b.numel(), _p(out),
                                     _p(ws), ws.numel(), _stream()), 'gf_dual_softmax_conf_at')
    return out


def dual_softmax_match(f0, f1, temperature, thr, hw0_c, hw1_c, scale, mask0=None, mask1=None, scale0=None,
                       scale1=None, force_one=False, materialize=True):
    """K1.  f0 [N,L,C], f1 [N,S,C] -> dict(conf [N,L,S] fp32, b_ids/i_ids/j_ids int64 [cap], mconf [cap],
    mkpts0_c/mkpts1_c [cap,2], counts int32 [1+N]) - all on the device, match arrays at capacity.
    materialize=False: match-only mode (conf_matrix is None; everything else bit-identical), where the library is built for it
    (match_only_supported) - otherwise the matrix is materialised as usual."""
    _need_cuda(f0, f1)
    f0, f1 = _contig(f0), _contig(f1)
    N, L, C = f0.shape
    S = f1.shape[1]
    dev = f0.device
    cap = N * min(L, S) + (N if force_one else 0)
    match_only = not materialize and match_only_supported(f0, f1, mask0 is not None, force_one)
    conf = None if match_only else torch.empty(N, L, S, dtype=torch.float32, device=dev)
    ids = torch.empty(3, cap, dtype=torch.int64, device=dev)
    mconf = torch.empty(cap, dtype=torch.float32, device=dev)
    mk = torch.empty(2, cap, 2, dtype=torch.float32, device=dev)
    counts = torch.empty(1 + N, dtype=torch.int32, device=dev)
    m0 = m1 = None
    if mask0 is not None:
        m0 = _contig(mask0.reshape(N, L).to(torch.uint8))
        m1 = _contig(mask1.reshape(N, S).to(torch.uint8))
    s0 = None if scale0 is None else _contig(scale0.to(device=dev, dtype=torch.float32))
    s1 = None if scale1 is None else _contig(scale1.to(device=dev, dtype=torch.float32))
    L_ = _lib.lib()
    nbytes = L_.gf_dual_softmax_workspace_bytes(N, L, S)
    ws = _ws.get('k1', nbytes, dev)
    check(L_.gf_dual_softmax_match(_p(f0), _p(f1), _dt(f0), N, L, S, C, _p(m0), _p(m1), float(temperature), float(thr),
                                   int(bool(force_one)), int(hw0_c[1]), int(hw1_c[1]), float(scale), _p(s0), _p(s1),
                                   _p(conf), _p(ids[0]), _p(ids[1]), _p(ids[2]), _p(mconf), _p(mk[0]), _p(mk[1]),
                                   _p(counts), _p(ws), ws.numel(), _stream()), 'gf_dual_softmax_match')
    return {'conf_matrix': conf, 'b_ids': ids[0], 'i_ids': ids[1], 'j_ids': ids[2], 'mconf': mconf,
            'mkpts0_c': mk[0], 'mkpts1_c': mk[1], 'counts': counts}


class _MapTable:
    """What MapBatch and RaggedMapBatch share: the list of maps, the tensor-like `.shape` / `.dtype` / `.device`, the maps' addresses with
    their common alignment, and the device table the kernels read - one row of int64 words per map, which the subclass's _rows() gives."""

    def __init__(self, maps, shape):
        self.maps = maps
        self.shape = torch.Size(shape)
        self.dtype, self.device = maps[0].dtype, maps[0].device
        self.addresses = [m.data_ptr() for m in maps]
        low = 256                                           # the largest power of two (bytes, capped) dividing every address
        for a in self.addresses:
            low = min(low, a & -a) if a else low
        self.align = int(low)
        self._tables = {}

    def __len__(self):
        return len(self.maps)

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def table(self):
        """The N rows as an int64 device tensor, for launches on the CURRENT stream.  No device synchronisation: the rows are
        written into a pinned host tensor and copied asynchronously on the current stream (torch's pinned-memory allocator holds the
        host block back until that copy has run).  Kept per stream by this object, so it lives as long as the batch does and at least
        until the launches that read it have been enqueued; freed afterwards, the caching allocator's stream order keeps the block from
        being handed out to work that runs before them."""
        key = _stream_handle(self.device)
        t = self._tables.get(key)
        if t is None:
            host = torch.tensor(self._rows(), dtype=torch.int64).pin_memory()
            with torch.cuda.device(self.device):
                t = self._tables[key] = host.to(self.device, non_blocking=True)
        return t


class MapBatch(_MapTable):
    """A batch of N feature maps that lie in SEPARATE allocations: a list of [C,H,W] device tensors of one shape, dtype, device and
    stride triple (entries may repeat: one query map against N candidates), read where they lie by the address-table entries
    gf_pos_encode_ptrs / gf_fine_gather_ptrs - `pos_encode` and `fine_gather` below take it in place of the [N,C,H,W] tensor.
    Behaves like that tensor for `.shape`, `.dtype` and `.device`, and nothing more: the two ops are the only readers.
    `table()`: the N addresses as an int64 [N] device tensor.
    Raises ValueError when the maps differ in shape, dtype, device or strides."""

    def __init__(self, maps):
        maps = list(maps)
        if not maps:
            raise ValueError('MapBatch: no maps')
        m0 = maps[0]
        if m0.dim() != 3:
            raise ValueError(f'MapBatch: maps are [C,H,W] tensors, got {tuple(m0.shape)}')
        for m in maps[1:]:
            if m.shape != m0.shape or m.dtype != m0.dtype or m.device != m0.device or m.stride() != m0.stride():
                raise ValueError(f'MapBatch: the maps of a batch must agree in shape, dtype, device and strides: {tuple(m0.shape)} {m0.dtype} '
                                 f'{m0.device} strides {m0.stride()} against {tuple(m.shape)} {m.dtype} {m.device} strides {m.stride()}')
        super().__init__(maps, (len(maps),) + tuple(m0.shape))
        self.map_stride = tuple(m0.stride())                # (sc, sh, sw), elements

    def _rows(self):
        return self.addresses


class RaggedMapBatch(_MapTable):
    """A batch of N feature maps of UNEQUAL extents: a list of [C,h_k,w_k] device tensors of one C, dtype, device and layout kind (all
    channels-last with stride 1 on C, or all contiguous), laid at the top left of a common canvas (default: the per-axis maximum of
    the extents; entries may repeat).  Read where they lie by gf_pos_encode_ragged / gf_fine_gather_ragged through a device table of
    gf_map_record (base, strides, extent): canvas positions outside a map's own extent read as zero - the bits of the tensor path on
    the maps zero-padded at the right and bottom and stacked.  `.shape` is (N, C, H, W) of the CANVAS; otherwise like MapBatch.
    `table()`: the N records as an int64 [N,5] device tensor.
    Raises ValueError on mixed C, dtype, device or layout kind, on an empty list and on a canvas smaller than an extent."""

    def __init__(self, maps, canvas=None):
        maps = list(maps)
        if not maps:
            raise ValueError('RaggedMapBatch: no maps')
        m0 = maps[0]
        kinds = set()
        for m in maps:
            if m.dim() != 3:
                raise ValueError(f'RaggedMapBatch: maps are [C,h,w] tensors, got {tuple(m.shape)}')
            if m.shape[0] != m0.shape[0] or m.dtype != m0.dtype or m.device != m0.device:
                raise ValueError(f'RaggedMapBatch: the maps of a batch must agree in C, dtype and device: {tuple(m0.shape)} {m0.dtype} {m0.device} '
                                 f'against {tuple(m.shape)} {m.dtype} {m.device}')
            kind = {'nhwc'} if m.stride(0) == 1 else set()
            if m.is_contiguous():
                kind.add('nchw')                       # a map with C == 1 (or h == w == 1) is both
            if not kind:
                raise ValueError(f'RaggedMapBatch: a map must be channels-last (stride 1 on C) or contiguous, got strides {m.stride()}')
            kinds.add(frozenset(kind))
        common = frozenset.intersection(*kinds)
        if not common:
            raise ValueError('RaggedMapBatch: the maps of a batch must share one layout kind: all channels-last or all contiguous')
        hmax, wmax = max(m.shape[1] for m in maps), max(m.shape[2] for m in maps)
        H, W = (hmax, wmax) if canvas is None else (int(canvas[0]), int(canvas[1]))
        if H < hmax or W < wmax:
            raise ValueError(f'RaggedMapBatch: canvas {H} x {W} is smaller than the largest extents {hmax} x {wmax}')
        super().__init__(maps, (len(maps), m0.shape[0], H, W))
        self.layout = 'nhwc' if 'nhwc' in common else 'nchw'
        self.extents = [(int(m.shape[1]), int(m.shape[2])) for m in maps]

    def records(self):
        """The N gf_map_record entries as rows of five int64 words: base, sc, sh, sw, h | (w << 32)."""
        return [[a, *m.stride(), h | (w << 32)] for a, m, (h, w) in zip(self.addresses, self.maps, self.extents)]

    _rows = records


def pos_encode(x, pe_hwc, out_dtype, out=None, mask_out=None):
    """a1.  x [N,C,H,W] (any strides; fp32, fp16 or bf16), pe_hwc fp32 [H,W,C] on the device -> [N, H*W, C] of out_dtype (into `out`
    if given).  Any input / output dtype pair, bf16 -> fp16 and fp16 -> bf16 included: bit-equal to (x.float() + pe).to(out_dtype).
    x may be a MapBatch (N maps in separate allocations, read in place through gf_pos_encode_ptrs): the bits of the tensor path on
    torch.stack of the maps.  x may be a RaggedMapBatch (maps of unequal extents on one canvas, gf_pos_encode_ragged): H, W are the
    canvas's, the bits are those of the tensor path on the maps zero-padded and stacked, and mask_out (optional, a contiguous uint8 or
    bool [N,H,W] device tensor) is written by the same launch with the padding mask: true inside each map's own extent."""
    _need_cuda(pe_hwc)
    ragged, table = isinstance(x, RaggedMapBatch), isinstance(x, MapBatch)
    N, C, H, W = x.shape
    if out is None:
        out = torch.empty(N, H * W, C, dtype=out_dtype, device=x.device)
    elif out.shape != (N, H * W, C) or out.dtype != out_dtype or not out.is_contiguous():
        raise ValueError('out must be a contiguous [N, H*W, C] tensor of out_dtype')
    if mask_out is not None and not ragged:
        raise ValueError('pos_encode: mask_out is written for a RaggedMapBatch only (other inputs have no padding)')
    _need_cuda(*(x.maps if ragged or table else (x,)), mask_out)
    if ragged and (tuple(pe_hwc.shape) != (H, W, C) or pe_hwc.dtype != torch.float32 or not pe_hwc.is_contiguous()):
        raise ValueError(f'pos_encode: the table must be a contiguous fp32 [{H},{W},{C}] tensor (the canvas), got {tuple(pe_hwc.shape)}')
    if mask_out is not None and (mask_out.shape != (N, H, W) or mask_out.dtype not in (torch.uint8, torch.bool) or not mask_out.is_contiguous()):
        raise ValueError('mask_out must be a contiguous uint8 or bool [N, H, W] tensor')
    L_, rest = _lib.lib(), (_p(pe_hwc), _p(out), _DTYPES[out_dtype], N, C, H, W)
    if ragged:
        check(L_.gf_pos_encode_ragged(_p(x.table()), _dt(x), x.align, *rest, _p(mask_out), _stream()), 'gf_pos_encode_ragged')
    elif table:
        check(L_.gf_pos_encode_ptrs(_p(x.table()), _dt(x), *x.map_stride, x.align, *rest, _stream()), 'gf_pos_encode_ptrs')
    else:
        check(L_.gf_pos_encode(_p(x), _dt(x), *x.stride(), *rest, _stream()), 'gf_pos_encode')
    return out


def image_gray_resize(src_u8, wt, ht, out=None, normalised=True, reciprocal=False):
    """Image preprocessing in one launch: decoded uint8 image -> gray -> resize to (wt, ht) -> [1,1,ht,wt] fp32 in [0,1]
    (normalised=False: the resized gray image itself, [ht,wt] uint8).  Bit-identical to matcher.cv2_resize_linear_u8(
    cv2_gray_u8(src), wt, ht) and to that image / 255.0 in torch: the correctly rounded quotient, as torch divides on the CPU, or
    with reciprocal=True the product with fp32(1 / 255), as torch's device kernel computes `t / 255.0` (it turns a Python-scalar
    divisor into a multiplication; last-bit differences for 126 of the 256 byte values) - the bits of matcher's host path on a GPU.
    src_u8: CUDA uint8 [H,W,3] (RGB) or [H,W] (already gray), pixels contiguous, any row stride (a crop needs no copy).
    out: optional destination holding ht*wt contiguous elements of the result's dtype, e.g. one [1,ht,wt] slice of an
    [N,1,ht,wt] batch: images of different source sizes are assembled into a batch without a cat."""
    _need_cuda(src_u8, out)
    if src_u8.dtype != torch.uint8 or src_u8.dim() not in (2, 3) or (src_u8.dim() == 3 and src_u8.shape[2] != 3):
        raise ValueError(f'image_gray_resize: src_u8 must be a uint8 [H,W,3] or [H,W] tensor, got {src_u8.dtype} {tuple(src_u8.shape)}')
    ch = 3 if src_u8.dim() == 3 else 1
    hs, ws = src_u8.shape[:2]
    wt, ht = int(wt), int(ht)
    if hs < 1 or ws < 1 or (ch == 3 and src_u8.stride(2) != 1) or (ws > 1 and src_u8.stride(1) != ch) or (hs > 1 and src_u8.stride(0) < ws * ch):
        raise ValueError('image_gray_resize: the pixels of a source row must be contiguous (row stride >= W * channels)')
    dtype = torch.float32 if normalised else torch.uint8
    if out is None:
        out = torch.empty(ht, wt, dtype=dtype, device=src_u8.device)
    elif out.dtype != dtype or out.numel() != ht * wt or not out.is_contiguous() or out.device != src_u8.device:
        raise ValueError(f'image_gray_resize: out must hold {ht} x {wt} contiguous {dtype} elements on {src_u8.device}')
    stride = src_u8.stride(0) if hs > 1 else ws * ch
    kind = _lib.GF_IMAGE_U8 if not normalised else _lib.GF_IMAGE_F32_NORMALISED_RCP if reciprocal else _lib.GF_IMAGE_F32_NORMALISED
    check(_lib.lib().gf_image_gray_resize(_p(src_u8), ch, hs, ws, stride, _p(out), kind,
                                          ht, wt, ctypes.c_void_p(_stream_handle(src_u8.device))), 'gf_image_gray_resize')
    return out.view(1, 1, ht, wt) if normalised else out.view(ht, wt)


def image_warp_resize(src_u8, M, wt, ht, out=None, normalised=True, reciprocal=False, warp_size=None, brightness_contrast=None):
    """One image of a homography training pair in one launch: decoded uint8 image -> gray -> cv2.warpPerspective(gray, M, warp_size)
    -> resize to (wt, ht) -> optional brightness / contrast -> [1,1,ht,wt] fp32 in [0,1] (normalised=False: [ht,wt] uint8).  No warped
    image is materialised.  Bit-identical to matcher.cv2_resize_linear_u8(homo_data.cv2_warp_perspective_u8(cv2_gray_u8(src), M, *warp_size),
    wt, ht), then homo_data.brightness_contrast_u8, then the division of image_gray_resize (`reciprocal` as there).
    M: the FORWARD 3x3 matrix (source -> warped image, what cv2.warpPerspective takes), anything numpy reads as 3x3; it is inverted
    here in fp64 and the inverse travels in the launch arguments.  A singular or non-finite M is a ValueError.
    warp_size: (w, h) of the warped image the resize reads, default the source's size (HomoDataset.py:96).
    brightness_contrast: None or (alpha, beta): v -> clip(trunc(fp32(v) * alpha + beta * 255), 0, 255) on the resized uint8 value.
    M = identity at the source's size is image_gray_resize with the brightness / contrast step (image 0 of a pair).
    src_u8, out: as image_gray_resize."""
    import numpy as np
    _need_cuda(src_u8, out)
    if src_u8.dtype != torch.uint8 or src_u8.dim() not in (2, 3) or (src_u8.dim() == 3 and src_u8.shape[2] != 3):
        raise ValueError(f'image_warp_resize: src_u8 must be a uint8 [H,W,3] or [H,W] tensor, got {src_u8.dtype} {tuple(src_u8.shape)}')
    ch = 3 if src_u8.dim() == 3 else 1
    hs, ws = src_u8.shape[:2]
    wt, ht = int(wt), int(ht)
    ww, hw = (ws, hs) if warp_size is None else (int(warp_size[0]), int(warp_size[1]))
    if min(wt, ht, ww, hw) < 1:
        raise ValueError(f'image_warp_resize: sizes must be positive, got target {wt} x {ht}, warp {ww} x {hw}')
    if hs < 1 or ws < 1 or (ch == 3 and src_u8.stride(2) != 1) or (ws > 1 and src_u8.stride(1) != ch) or (hs > 1 and src_u8.stride(0) < ws * ch):
        raise ValueError('image_warp_resize: the pixels of a source row must be contiguous (row stride >= W * channels)')
    M = np.asarray(M.detach().cpu().numpy() if torch.is_tensor(M) else M, dtype=np.float64)
    if M.shape != (3, 3) or not np.isfinite(M).all():
        raise ValueError('image_warp_resize: M must be a finite 3x3 matrix')
    try:
        minv = np.linalg.inv(M)
    except np.linalg.LinAlgError:
        minv = None
    if minv is None or not np.isfinite(minv).all():
        raise ValueError('image_warp_resize: M is singular')
    dtype = torch.float32 if normalised else torch.uint8
    if out is None:
        out = torch.empty(ht, wt, dtype=dtype, device=src_u8.device)
    elif out.dtype != dtype or out.numel() != ht * wt or not out.is_contiguous() or out.device != src_u8.device:
        raise ValueError(f'image_warp_resize: out must hold {ht} x {wt} contiguous {dtype} elements on {src_u8.device}')
    stride = src_u8.stride(0) if hs > 1 else ws * ch
    kind = _lib.GF_IMAGE_U8 if not normalised else _lib.GF_IMAGE_F32_NORMALISED_RCP if reciprocal else _lib.GF_IMAGE_F32_NORMALISED
    bc = None
    if brightness_contrast is not None:
        alpha, beta = (float(v) for v in brightness_contrast)
        if not (np.isfinite(alpha) and np.isfinite(beta)):
            raise ValueError('image_warp_resize: brightness_contrast must be two finite numbers')
        bc = (ctypes.c_float * 2)(alpha, beta)
    check(_lib.lib().gf_image_warp_resize(_p(src_u8), ch, hs, ws, stride, (ctypes.c_double * 9)(*minv.reshape(-1)), hw, ww, _p(out), kind,
                                          ht, wt, bc, ctypes.c_void_p(_stream_handle(src_u8.device))), 'gf_image_warp_resize')
    return out.view(1, 1, ht, wt) if normalised else out.view(ht, wt)


ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2


def _nhwc(t):
    if t.dim() != 4 or not t.is_contiguous(memory_format=torch.channels_last):
        raise ValueError('expected a channels_last [N,C,H,W] tensor')
    return t


def bias_act_(x, bias=None, residual=None, act=ACT_NONE, slope=0.01):
    """Backbone glue, in place: x <- act(x + bias[c] + residual) on channels_last [N,C,H,W] tensors."""
    _need_cuda(x)
    _nhwc(x)
    if residual is not None and (_nhwc(residual).shape != x.shape or residual.dtype != x.dtype):
        raise ValueError('residual must match x')
    N, C, H, W = x.shape
    check(_lib.lib().gf_bias_act_nhwc(_p(x), _p(bias), _p(residual), _p(x), N * H * W, C, int(act), float(slope), _dt(x),
                                      _stream()), 'gf_bias_act_nhwc')
    return x


def upsample_add_(hi, lo):
    """Backbone glue, in place: hi <- hi + bilinear(lo -> hi's size, align_corners=True); channels_last."""
    _need_cuda(hi, lo)
    _nhwc(hi), _nhwc(lo)
    N, C, H, W = hi.shape
    if lo.shape[:2] != (N, C) or lo.dtype != hi.dtype:
        raise ValueError('lo must have the batch, channels and dtype of hi')
    check(_lib.lib().gf_upsample_add_nhwc(_p(lo), _p(hi), _p(hi), N, lo.shape[2], lo.shape[3], H, W, C, _dt(hi),
                                          _stream()), 'gf_upsample_add_nhwc')
    return hi


def upsample_bilinear_backward(dhi, h, w):
    """Training: the gradient of F.interpolate(lo, size=(H, W), mode='bilinear', align_corners=True) with respect to lo [N, C, h, w], given
    dhi [N, C, H, W] channels_last (fp32 / fp16 / bf16, C % 4 == 0); a gather, bit-reproducible."""
    _need_cuda(dhi)
    _nhwc(dhi)
    N, C, H, W = dhi.shape
    dlo = torch.empty(N, C, int(h), int(w), dtype=dhi.dtype, device=dhi.device, memory_format=torch.channels_last)
    check(_lib.lib().gf_upsample_bilinear_backward_nhwc(_p(dhi), _p(dlo), N, int(h), int(w), H, W, C, _dt(dhi), _stream()),
          'gf_upsample_bilinear_backward_nhwc')
    return dlo


def conv1x1_upsample_add(x, weight, lo):
    """Backbone glue: 1x1 convolution of channels_last x [N,Cin,H,W] with weight [Cout,Cin(,1,1)] plus the bilinear
    (align_corners=True) upsampling of channels_last lo [N,Cout,h,w], in one K3 launch -> channels_last [N,Cout,H,W]."""
    _need_cuda(x, weight, lo)
    _nhwc(x), _nhwc(lo)
    N, Cin, H, W = x.shape
    Cout = weight.shape[0]
    w2 = _contig(weight.reshape(Cout, Cin))
    if lo.shape[:2] != (N, Cout) or lo.dtype != x.dtype or w2.dtype != x.dtype:
        raise ValueError('lo must be [N, Cout, h, w] of the dtype of x and weight')
    out = torch.empty(N, Cout, H, W, dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    check(_lib.lib().gf_conv1x1_upsample_add_nhwc(_p(x), _p(w2), _p(lo), _p(out), N, lo.shape[2], lo.shape[3], H, W, Cin, Cout,
                                                  _dt(x), _stream()), 'gf_conv1x1_upsample_add_nhwc')
    return out


def conv1x1(x, weight, stride=1):
    """Backbone glue: 1x1 convolution (no bias) of channels_last x [N,Cin,H,W] with weight [Cout,Cin(,1,1)], stride 1 or 2 ->
    channels_last [N,Cout,H/stride,W/stride]; one K3 launch on the (strided) pixel rows (gf_conv1x1_nhwc)."""
    _need_cuda(x, weight)
    _nhwc(x)
    N, Cin, H, W = x.shape
    Cout = weight.shape[0]
    w2 = _contig(weight.reshape(Cout, Cin))
    if w2.dtype != x.dtype:
        raise ValueError('weight must have the dtype of x')
    out = torch.empty(N, Cout, H // stride, W // stride, dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    check(_lib.lib().gf_conv1x1_nhwc(_p(x), _p(w2), _p(out), N, H, W, Cin, Cout, int(stride), _dt(x), _stream()), 'gf_conv1x1_nhwc')
    return out


def stem_conv7x7(image, weight, shift, dtype=torch.float16):
    """Backbone stem: image [N,1,H,W] (fp32 or `dtype`, contiguous), weight fp32 [128,1,7,7] (BN folded), shift fp32 [128]
    -> relu(conv 7x7 / stride 2 / pad 3 + shift), `dtype` (fp16 / bf16) channels_last [N,128,Ho,Wo]."""
    _need_cuda(image, weight, shift)
    N, one, H, W = image.shape
    if one != 1 or not image.is_contiguous():
        raise ValueError('stem_conv7x7 needs a contiguous [N,1,H,W] image')
    C = weight.shape[0]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.empty(N, C, Ho, Wo, dtype=dtype, device=image.device, memory_format=torch.channels_last)
    check(_lib.lib().gf_stem_conv7x7_dt(_p(image), _dt(image), _p(weight), _p(shift), _p(out), _DTYPES[dtype], N, H, W, C, _stream()),
          'gf_stem_conv7x7_dt')
    return out


def _rows(t):
    """[..., C] tensor whose last dim is contiguous -> (tensor, row stride in elements)."""
    if t.stride(-1) != 1:
        t = t.contiguous()
    return t, t.stride(-2)


def linear_attention(q, k, v, nhead, q_mask=None, kv_mask=None, eps=1e-6):
    """K2.  q [N,L,C], k,v [N,S,C] (row-strided views allowed) -> [N,L,C]."""
    _need_cuda(q, k, v)
    N, L, C = q.shape
    S = k.shape[1]
    D = C // nhead
    q, ldq = _rows(q)
    k, ldk = _rows(k)
    v, ldv = _rows(v)
    for t, ld, n in ((q, ldq, L), (k, ldk, S), (v, ldv, S)):
        if t.stride(0) != ld * n:
            raise ValueError('linear_attention needs batch stride == rows * row stride')
    out = torch.empty(N, L, C, dtype=q.dtype, device=q.device)
    qm = None if q_mask is None else _contig(q_mask.reshape(N, L).to(torch.uint8))
    km = None if kv_mask is None else _contig(kv_mask.reshape(N, S).to(torch.uint8))
    L_ = _lib.lib()
    nbytes = L_.gf_linear_attention_workspace_bytes(N, S, nhead, D)
    ws = _ws.get('k2', nbytes, q.device)
    check(L_.gf_linear_attention(_p(q), _p(k), _p(v), _dt(q), N, L, S, nhead, D, ldq, ldk, ldv, _p(qm), _p(km),
                                 float(eps), _p(out), _p(ws), ws.numel(), _stream()), 'gf_linear_attention')
    return out


RANSAC_ITERS = 1024
RANSAC_SEED = 0x5EED
RANSAC_LM_ITERS = 10            # Levenberg-Marquardt steps behind the refit: what cv2.findHomography(..., cv2.RANSAC, ...) appends


def ransac_homography(mkpts0_c, mkpts1_c, counts, N, scale, scale0=None, scale1=None, thr=8.0, iters=RANSAC_ITERS,
                      seed=RANSAC_SEED, integer_keypoints=True, min_points=9, lm_iters=RANSAC_LM_ITERS):
    """Device RANSAC on the first-pass coarse matches.  Returns dict(kp0, kp1 fp32 [cap,2], M fp64 [N,3,3],
    M_f32, Minv_f32 [N,3,3], valid int32 [N], keep uint8 [cap])."""
    _need_cuda(mkpts0_c, mkpts1_c, counts)
    dev = mkpts0_c.device
    cap = mkpts0_c.shape[0]
    kp = torch.empty(2, max(cap, 1), 2, dtype=torch.float32, device=dev)
    M = torch.empty(N, 3, 3, dtype=torch.float64, device=dev)
    Mf = torch.empty(2, N, 3, 3, dtype=torch.float32, device=dev)
    valid = torch.empty(N, dtype=torch.int32, device=dev)
    keep = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
    s0 = None if scale0 is None else _contig(scale0.to(device=dev, dtype=torch.float32))
    s1 = None if scale1 is None else _contig(scale1.to(device=dev, dtype=torch.float32))
    L_ = _lib.lib()
    nbytes = L_.gf_ransac_workspace_bytes(N, iters)
    ws = _ws.get('ransac', nbytes, dev)
    check(L_.gf_ransac_homography_v2(_p(mkpts0_c), _p(mkpts1_c), _p(counts), N, max(cap, 1), float(scale), _p(s0), _p(s1),
                                     float(thr), int(iters), int(seed), int(min_points), int(bool(integer_keypoints)), _p(kp[0]), _p(kp[1]),
                                     _p(M), _p(Mf[0]), _p(Mf[1]), _p(valid), _p(keep), _p(ws), ws.numel(), _stream(), int(lm_iters)),
          'gf_ransac_homography_v2')
    return {'kp0': kp[0], 'kp1': kp[1], 'M': M, 'M_f32': Mf[0], 'Minv_f32': Mf[1], 'valid': valid, 'keep': keep}


POSE_RANSAC_ITERS = 1024        # fixed, not adaptive (OpenCV's own cap is 1000); a positive multiple of 32


def _intrinsics(K, N, dev):
    return _contig(K.to(device=dev, dtype=torch.float32).reshape(N, 9))


def _intrinsics_rows(K, rows, dev):
    """K [rows,3,3], or one [3,3] for all -> a fresh contiguous fp32 [rows,9]."""
    Kt = torch.as_tensor(K, dtype=torch.float32, device=dev)
    return _contig((Kt.reshape(1, 9).expand(rows, 9) if Kt.numel() == 9 else Kt.reshape(rows, 9)).clone())


def _scores_offsets(what, scores, offsets, M, N, dev):
    """The row filter's scores (None without scores or rows) and the int32 [N+1] offsets of the N problems of a match list."""
    sc = None if scores is None or M == 0 else _contig(scores.float())
    off = _contig(offsets.to(device=dev, dtype=torch.int32))
    if off.numel() != N + 1:
        raise ValueError(f'{what}: offsets has {off.numel()} entries for N = {N}')
    return sc, off


def ransac_essential(mkpts0, mkpts1, counts, N, K0, K1, pixel_thr=0.5, iters=POSE_RANSAC_ITERS, seed=RANSAC_SEED):
    """Device essential-matrix RANSAC + pose recovery (metrics.py:72-98 without its cv2 host round trip).  mkpts0/mkpts1 fp32 [M,2] pixel
    keypoints sorted by pair, counts int32 [1+N] on the device, K0/K1 [N,3,3].  Returns dict(E fp64 [N,3,3] of Frobenius norm 1,
    R fp64 [N,3,3], t fp64 [N,3] unit, valid int32 [N], n_inliers int32 [N], inliers uint8 [M], hypothesis int32 [N,2])."""
    _need_cuda(mkpts0, mkpts1, counts)
    dev = mkpts0.device
    cap = mkpts0.shape[0]
    m0 = _contig(mkpts0.float()) if cap else torch.zeros(1, 2, dtype=torch.float32, device=dev)
    m1 = _contig(mkpts1.float()) if cap else torch.zeros(1, 2, dtype=torch.float32, device=dev)
    k0, k1 = _intrinsics(K0, N, dev), _intrinsics(K1, N, dev)
    E = torch.empty(N, 3, 3, dtype=torch.float64, device=dev)
    R = torch.empty(N, 3, 3, dtype=torch.float64, device=dev)
    t = torch.empty(N, 3, dtype=torch.float64, device=dev)
    valid = torch.empty(N, dtype=torch.int32, device=dev)
    nin = torch.empty(N, dtype=torch.int32, device=dev)
    best = torch.empty(N, 2, dtype=torch.int32, device=dev)
    inl = torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev)
    L_ = _lib.lib()
    ws = _ws.get('pose', L_.gf_pose_workspace_bytes(N, max(int(iters), 1)), dev)
    check(L_.gf_pose_essential_ransac(_p(m0), _p(m1), _p(counts), N, max(cap, 1), _p(k0), _p(k1), float(pixel_thr), int(iters), int(seed),
                                      _p(E), _p(R), _p(t), _p(valid), _p(nin), _p(best), _p(inl), _p(ws), ws.numel(), _stream()),
          'gf_pose_essential_ransac')
    return {'E': E, 'R': R, 't': t, 'valid': valid, 'n_inliers': nin, 'inliers': inl[:cap], 'hypothesis': best}


FUND_RANSAC_ITERS = 512         # fixed, not adaptive; a positive multiple of 64.  An all-inlier sample of 7 at 50 % outliers: 98 % of the pairs


def ransac_fundamental(matches, scores, offsets, N, pixel_thr=1.0, sc_thres=0.25, iters=FUND_RANSAC_ITERS, seed=RANSAC_SEED, refit=0):
    """Device fundamental-matrix RANSAC for the N pairs of a match list (csrc/fund_solver.h): two-view verification without intrinsics.
    matches fp32 [M,4] pixel rows (x0, y0, x1, y1) sorted by pair, scores fp32 [M] or None, offsets int32 [N+1] on the device.  A row takes
    part iff it is finite and (with scores) scores >= sc_thres.  Returns dict(F fp64 [N,3,3] of Frobenius norm 1 (x1^T F x0 = 0), valid
    int32 [N], n_inliers int32 [N], inliers uint8 [M], hypothesis int32 [N,2]).
    refit = R in 1 .. 8: the winner is refitted on its inliers up to R times (normalised eight-point fit, rank 2 enforced, inliers selected
    again; a candidate with fewer inliers is never taken - the `refit` rule of csrc/fund_solver.h, one more launch); F, n_inliers and
    inliers are then the refined model's, hypothesis still names the seven-point model that seeded it, and the dict gains rounds int32 [N],
    the refits accepted per pair (0: the pair's outputs are the seven-point winner's bits)."""
    _need_cuda(matches, offsets)
    dev = matches.device
    M = matches.shape[0]
    m = _contig(matches.float().reshape(M, 4)) if M else torch.zeros(1, 4, dtype=torch.float32, device=dev)
    sc, off = _scores_offsets('ransac_fundamental', scores, offsets, M, N, dev)
    F = torch.empty(N, 3, 3, dtype=torch.float64, device=dev)
    valid = torch.empty(N, dtype=torch.int32, device=dev)
    nin = torch.empty(N, dtype=torch.int32, device=dev)
    best = torch.empty(N, 2, dtype=torch.int32, device=dev)
    inl = torch.zeros(max(M, 1), dtype=torch.uint8, device=dev)
    L_ = _lib.lib()
    if refit:
        rounds = torch.empty(N, dtype=torch.int32, device=dev)
        ws = _ws.get('fundamental_lo', L_.gf_fundamental_lo_workspace_bytes(N, M, max(int(iters), 1)), dev)
        check(L_.gf_fundamental_ransac_lo(_p(m), _p(sc), _p(off), N, M, float(sc_thres), float(pixel_thr), int(iters), int(seed), _p(F), _p(valid),
                                          _p(nin), _p(best), _p(inl), int(refit), _p(rounds), _p(ws), ws.numel(), _stream()),
              'gf_fundamental_ransac_lo')
        return {'F': F, 'valid': valid, 'n_inliers': nin, 'inliers': inl[:M], 'hypothesis': best, 'rounds': rounds}
    ws = _ws.get('fundamental', L_.gf_fundamental_workspace_bytes(N, M, max(int(iters), 1)), dev)
    check(L_.gf_fundamental_ransac(_p(m), _p(sc), _p(off), N, M, float(sc_thres), float(pixel_thr), int(iters), int(seed), _p(F), _p(valid),
                                   _p(nin), _p(best), _p(inl), _p(ws), ws.numel(), _stream()),
          'gf_fundamental_ransac')
    return {'F': F, 'valid': valid, 'n_inliers': nin, 'inliers': inl[:M], 'hypothesis': best}


REL_RANSAC_ITERS = 512          # fixed, not adaptive; a positive multiple of 64.  An all-inlier sample of 5 at 50 % outliers: 1 - 1e-7 of the pairs


def ransac_relative_pose(matches, scores, offsets, N, K0, K1, pixel_thr=1.0, sc_thres=0.25, iters=REL_RANSAC_ITERS, seed=RANSAC_SEED, refit=0):
    """Device essential-matrix RANSAC with pose recovery for the N pairs of a match list (csrc/rel_solver.h): two-view verification with
    known intrinsics.  matches fp32 [M,4] pixel rows (x0, y0, x1, y1) sorted by pair, scores fp32 [M] or None, offsets int32 [N+1] on the
    device, K0 / K1 [N,3,3] (or [3,3] for all).  A row takes part iff it is finite and (with scores) scores >= sc_thres; a pair is estimated
    iff 5 rows take part and its focal lengths are finite and positive.  Five-point hypotheses, squared Sampson distance in normalised
    coordinates below (pixel_thr / mean focal)^2.  Returns dict(E fp64 [N,3,3] of Frobenius norm 1, R fp64 [N,3,3], t fp64 [N,3] unit with
    x1 ~ R x0 + t, valid int32 [N], n_inliers int32 [N], n_cheiral int32 [N], inliers uint8 [M], hypothesis int32 [N,2]).
    refit = R in 1 .. 8: the pose is refitted on its inliers up to R times (three Gauss-Newton steps on the signed Sampson residual over
    (R, unit t), inliers selected again; a candidate with fewer inliers is never taken - step 7 of csrc/rel_solver.h, one more launch);
    E = [t]x R, R, t, n_inliers and inliers are then the refined model's, hypothesis still names the five-point model that seeded it, and
    the dict gains rounds int32 [N], the refits accepted per pair (0: the pair's outputs are the five-point winner's bits)."""
    _need_cuda(matches, offsets)
    dev = matches.device
    M = matches.shape[0]
    m = _contig(matches.float().reshape(M, 4)) if M else torch.zeros(1, 4, dtype=torch.float32, device=dev)
    sc, off = _scores_offsets('ransac_relative_pose', scores, offsets, M, N, dev)
    rows = max(N, 1)                # (N <= 0 is the entry point's error to report: it gets real pointers)
    ks = [_intrinsics_rows(K, rows, dev) for K in (K0, K1)]
    E = torch.empty(rows, 3, 3, dtype=torch.float64, device=dev)
    R = torch.empty(rows, 3, 3, dtype=torch.float64, device=dev)
    t = torch.empty(rows, 3, dtype=torch.float64, device=dev)
    valid = torch.empty(rows, dtype=torch.int32, device=dev)
    nin = torch.empty(rows, dtype=torch.int32, device=dev)
    nch = torch.empty(rows, dtype=torch.int32, device=dev)
    best = torch.empty(rows, 2, dtype=torch.int32, device=dev)
    inl = torch.zeros(max(M, 1), dtype=torch.uint8, device=dev)
    out = {'E': E, 'R': R, 't': t, 'valid': valid, 'n_inliers': nin, 'n_cheiral': nch, 'inliers': inl[:M], 'hypothesis': best}
    L_ = _lib.lib()
    if refit:
        rounds = torch.empty(rows, dtype=torch.int32, device=dev)
        ws = _ws.get('relpose_lo', L_.gf_relpose_lo_workspace_bytes(N, M, max(int(iters), 1)), dev)
        check(L_.gf_relpose_ransac_lo(_p(m), _p(sc), _p(off), N, M, _p(ks[0]), _p(ks[1]), float(sc_thres), float(pixel_thr), int(iters), int(seed),
                                      _p(E), _p(R), _p(t), _p(valid), _p(nin), _p(nch), _p(best), _p(inl), int(refit), _p(rounds), _p(ws),
                                      ws.numel(), _stream()),
              'gf_relpose_ransac_lo')
        out['rounds'] = rounds
        return out
    ws = _ws.get('relpose', L_.gf_relpose_workspace_bytes(N, M, max(int(iters), 1)), dev)
    check(L_.gf_relpose_ransac(_p(m), _p(sc), _p(off), N, M, _p(ks[0]), _p(ks[1]), float(sc_thres), float(pixel_thr), int(iters), int(seed), _p(E),
                               _p(R), _p(t), _p(valid), _p(nin), _p(nch), _p(best), _p(inl), _p(ws), ws.numel(), _stream()),
          'gf_relpose_ransac')
    return out


ABS_RANSAC_ITERS = 512          # fixed, not adaptive; a positive multiple of 64.  An all-inlier sample of 3 at 70 % outliers: 1 - 1e-6 of the queries


def ransac_absolute_pose(p2d, p3d, scores, offsets, N, K, pixel_thr=12.0, sc_thres=0.25, iters=ABS_RANSAC_ITERS, seed=RANSAC_SEED, refit=0):
    """Device absolute-pose RANSAC for the N queries of a 2-D - 3-D correspondence list (csrc/abs_solver.h): localisation.
    p2d fp32 [M,2] query pixels and p3d fp32 [M,3] world points, sorted by query, scores fp32 [M] or None, offsets int32 [N+1] on the
    device, K [N,3,3] (or [3,3] for all).  A row takes part iff it is finite and (with scores) scores >= sc_thres.  P3P hypotheses,
    inliers by reprojection error below pixel_thr.  Returns dict(R fp64 [N,3,3], t fp64 [N,3] with x_cam = R X + t, valid int32 [N],
    n_inliers int32 [N], inliers uint8 [M], hypothesis int32 [N,2], rounds int32 [N]).
    refit = R in 1 .. 8: the winner is refitted on its inliers up to R times (three Gauss-Newton steps on the reprojection error, inliers
    selected again; a candidate with fewer inliers is never taken - the `refit` rule of csrc/abs_solver.h, one more launch); rounds
    counts the refits accepted per query (0: the query's outputs are the P3P winner's bits)."""
    _need_cuda(p2d, p3d, offsets)
    dev = p2d.device
    M = p2d.shape[0]
    a = _contig(p2d.float().reshape(M, 2)) if M else torch.zeros(1, 2, dtype=torch.float32, device=dev)
    b = _contig(p3d.float().reshape(M, 3)) if M else torch.zeros(1, 3, dtype=torch.float32, device=dev)
    if p3d.shape[0] != M:
        raise ValueError(f'ransac_absolute_pose: {M} 2-D points but {p3d.shape[0]} 3-D points')
    sc, off = _scores_offsets('ransac_absolute_pose', scores, offsets, M, N, dev)
    rows = max(N, 1)                # (N <= 0 is the entry point's error to report: it gets real pointers)
    k = _intrinsics_rows(K, rows, dev)
    R = torch.empty(rows, 3, 3, dtype=torch.float64, device=dev)
    t = torch.empty(rows, 3, dtype=torch.float64, device=dev)
    valid = torch.empty(rows, dtype=torch.int32, device=dev)
    nin = torch.empty(rows, dtype=torch.int32, device=dev)
    best = torch.empty(rows, 2, dtype=torch.int32, device=dev)
    rounds = torch.empty(rows, dtype=torch.int32, device=dev)
    inl = torch.zeros(max(M, 1), dtype=torch.uint8, device=dev)
    L_ = _lib.lib()
    ws = _ws.get('abspose', L_.gf_abspose_workspace_bytes(N, M, max(int(iters), 1)), dev)
    check(L_.gf_abspose_ransac(_p(a), _p(b), _p(sc), _p(off), N, M, _p(k), float(sc_thres), float(pixel_thr), int(iters), int(seed), int(refit),
                               _p(R), _p(t), _p(valid), _p(nin), _p(best), _p(rounds), _p(inl), _p(ws), ws.numel(), _stream()),
          'gf_abspose_ransac')
    return {'R': R, 't': t, 'valid': valid, 'n_inliers': nin, 'inliers': inl[:M], 'hypothesis': best, 'rounds': rounds}


def xyz_map_table(maps, device):
    """The device table of gf_xyz_lookup for a list of fp32 [H, W, 3] device tensors (None: a pair without a map) -> int64 [P, 2] tensor
    (the address, then h | w << 32).  The caller keeps the maps alive until the lookup has run."""
    rec = []
    for m in maps:
        if m is None:
            rec.append((0, 0))
            continue
        if m.dtype != torch.float32 or m.dim() != 3 or m.shape[2] != 3 or not m.is_contiguous() or not m.is_cuda:
            raise ValueError('xyz_map_table: a map must be a contiguous fp32 [H, W, 3] tensor on the device')
        rec.append((m.data_ptr(), int(m.shape[0]) | (int(m.shape[1]) << 32)))
    return torch.tensor(rec, dtype=torch.int64).reshape(-1, 2).to(device)


def xyz_lookup(table, pair_offsets, pts, pts_stride=None):
    """3-D points of database keypoints (csrc/abs_solver.h: as_xyz_sample): table from xyz_map_table (P records), pair_offsets int32
    [P+1] on the device, pts fp32 [M,2] (x, y) - or any fp32 tensor whose row i starts pts_stride floats after row i - 1, as the
    columns 2:4 of a match list.  Returns fp32 [M,3]; NaN where the keypoint is outside its map, next to a pixel without a 3-D point,
    or in no pair."""
    _need_cuda(table, pair_offsets, pts)
    dev = pts.device
    M, P = pts.shape[0], table.shape[0]
    out = torch.empty(M, 3, dtype=torch.float32, device=dev)
    if M == 0 or P == 0:
        return out.fill_(float('nan'))
    if pts.dtype != torch.float32 or pts.stride(-1) != 1:
        raise ValueError('xyz_lookup: pts must be fp32 with unit stride along a row')
    stride = int(pts.stride(0)) if pts_stride is None else int(pts_stride)
    off = _contig(pair_offsets.to(device=dev, dtype=torch.int32))
    if off.numel() != P + 1:
        raise ValueError(f'xyz_lookup: pair_offsets has {off.numel()} entries for {P} maps')
    check(_lib.lib().gf_xyz_lookup(_p(table), P, _p(off), _p(pts), stride, M, _p(out), _stream()), 'gf_xyz_lookup')
    return out


CM_ST_OK, CM_ST_NONFINITE, CM_ST_NO_PREIMAGE, CM_ST_ARGS = 0, 1, 2, 3      # camera_spec.h CM_ST_*: the status byte of a point


def camera_table(records, device):
    """The device table of undistort_points / distort_points for a list of canonical camera records (fx, fy, cx, cy, k1, k2, p1, p2;
    csrc/camera_spec.h, matcher.canonical_camera makes them) -> fp64 [C, 8] tensor."""
    recs = [tuple(float(v) for v in r) for r in records]
    if any(len(r) != 8 for r in recs):
        raise ValueError('camera_table: a canonical record has 8 values: fx, fy, cx, cy, k1, k2, p1, p2')
    return torch.tensor(recs, dtype=torch.float64).reshape(-1, 8).to(device)


def _camera_points(entry, pts, seg_offsets, seg_camera, cameras, pts_stride, out, want_status, flags):
    _need_cuda(pts, seg_offsets, seg_camera, cameras)
    dev = pts.device
    P, S, C = pts.shape[0], seg_camera.numel(), cameras.shape[0]
    if out is None:
        out = torch.empty(P, 2, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (P, 2) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f'{entry}: out must be a contiguous fp32 [{P}, 2] tensor on the device of pts')
    status = torch.empty(P, dtype=torch.uint8, device=dev) if want_status else None
    if pts.dtype != torch.float32 or (P and pts.stride(-1) != 1):
        raise ValueError(f'{entry}: pts must be fp32 with unit stride along a row')
    if cameras.dtype != torch.float64 or cameras.dim() != 2 or cameras.shape[1] != 8 or not cameras.is_contiguous():
        raise ValueError(f'{entry}: cameras must be a contiguous fp64 [C, 8] tensor (ops.camera_table)')
    stride = (int(pts.stride(0)) if P else 2) if pts_stride is None else int(pts_stride)
    off = _contig(seg_offsets.to(device=dev, dtype=torch.int32))
    cam = _contig(seg_camera.to(device=dev, dtype=torch.int32))
    if off.numel() != S + 1:
        raise ValueError(f'{entry}: seg_offsets has {off.numel()} entries for {S} segments')
    own = flags is None
    if own:
        flags = torch.zeros(2, dtype=torch.int32, device=dev)
    check(getattr(_lib.lib(), entry)(_p(pts), stride, P, _p(off), _p(cam), S, _p(cameras), C, _p(out), _p(status), _p(flags), _stream()), entry)
    if own and P:
        raise_camera_flags(entry, flags.cpu())
    return out, status


def raise_camera_flags(what, flags):
    """flags: the two flag words of gf_undistort_points / gf_distort_points on the host."""
    if int(flags[0]):
        raise ValueError(f'{what}: seg_offsets is not an ascending list from 0 to the number of points')
    if int(flags[1]):
        raise ValueError(f'{what}: a segment names a camera outside the table')


def undistort_points(pts, seg_offsets, seg_camera, cameras, pts_stride=None, out=None, flags=None):
    """Pixels of real cameras -> pixels of an ideal pinhole camera with the same fx, fy, cx, cy (csrc/camera_spec.h), one launch.  pts
    fp32 [P, 2] (x, y) - or any fp32 tensor whose row i starts pts_stride floats after row i - 1, as the columns 0:2 or 2:4 of a match
    block, read in place; seg_offsets int32 [S+1] and seg_camera int32 [S] on the device cut the rows into segments of one camera each;
    cameras from camera_table.  Returns (out fp32 [P, 2], status uint8 [P]): status 0 fine, 1 non-finite input, 2 no pre-image found (the
    pixel lies beyond the model's range), 3 the row has no segment or camera; on status != 0 the row of out is NaN - the stages downstream
    drop such rows.  A camera without distortion passes the input bits through.
    Offsets that do not ascend from 0 to P and a camera index outside the table raise ValueError after one device-to-host read of two
    flag words; nothing wraps.  flags = an int32 [2] device tensor of zeros: no read here, the caller looks at it (raise_camera_flags)
    with a read of its own."""
    return _camera_points('gf_undistort_points', pts, seg_offsets, seg_camera, cameras, pts_stride, out, True, flags)


def distort_points(pts, seg_offsets, seg_camera, cameras, pts_stride=None, out=None, flags=None):
    """The inverse of undistort_points in closed form: pixels of the ideal pinhole camera -> pixels of the real image, for drawing matches
    on the images and for round trips.  Same arguments; returns out fp32 [P, 2] (NaN for a non-finite row)."""
    return _camera_points('gf_distort_points', pts, seg_offsets, seg_camera, cameras, pts_stride, out, False, flags)[0]


def epipolar_errors(mkpts0, mkpts1, m_bids, T_0to1, K0, K1):
    """Squared symmetric epipolar distance of every match under E = [t]x R of its pair's T_0to1 (metrics.py:30-69), fp32 [M]."""
    _need_cuda(mkpts0, mkpts1, m_bids, T_0to1)
    dev = mkpts0.device
    M, N = mkpts0.shape[0], T_0to1.shape[0]
    out = torch.empty(M, dtype=torch.float32, device=dev)
    T = _contig(T_0to1.to(device=dev, dtype=torch.float32).reshape(N, 16))
    check(_lib.lib().gf_epipolar_errors(_p(_contig(mkpts0.float())), _p(_contig(mkpts1.float())), _p(_contig(m_bids.to(torch.int64))), M, _p(T),
                                        _p(_intrinsics(K0, N, dev)), _p(_intrinsics(K1, N, dev)), N, _p(out), _stream()),
          'gf_epipolar_errors')
    return out


def window_geometry(H_f32, valid, grid_hw, img_hw, key_grid_w, scale=8, window_size=5, window_scale=None,
                    debug=False):
    """a8.  H_f32 [N,3,3] maps the query grid (grid_hw cells) into the image of size img_hw (pixels).
    -> win int32 [N, L, ws*ws] (+ kps int32 [N,L,ww,2], warped fp32 [N,L,2] when debug)."""
    _need_cuda(H_f32)
    N = H_f32.shape[0]
    hq, wq = grid_hw
    L = hq * wq
    ww = window_size * window_size
    dev = H_f32.device
    win = torch.empty(N, L, ww, dtype=torch.int32, device=dev)
    kps = torch.empty(N, L, ww, 2, dtype=torch.int32, device=dev) if debug else None
    warped = torch.empty(N, L, 2, dtype=torch.float32, device=dev) if debug else None
    wsc = None if window_scale is None else _contig(window_scale.to(device=dev, dtype=torch.float32))
    Hc = _contig(H_f32.reshape(N, 9).float())
    check(_lib.lib().gf_window_geometry(_p(Hc), _p(valid), N, hq, wq, int(img_hw[0]), int(img_hw[1]), int(key_grid_w),
                                        int(scale), int(window_size), _p(wsc), _p(win), _p(kps), _p(warped), _stream()),
          'gf_window_geometry')
    return (win, kps, warped) if debug else win


def inlier_index(kp0, kp1, keep, counts, N, L, S, w0, w1, scale=8):
    """a7.  -> dict(map0 uint8 [N,L], map1 [N,S], idx0 int32 [N,L], idx1 [N,S], nidx int32 [N,2])."""
    dev = kp0.device
    map0 = torch.empty(N, L, dtype=torch.uint8, device=dev)
    map1 = torch.empty(N, S, dtype=torch.uint8, device=dev)
    idx0 = torch.empty(N, L, dtype=torch.int32, device=dev)
    idx1 = torch.empty(N, S, dtype=torch.int32, device=dev)
    nidx = torch.empty(N, 2, dtype=torch.int32, device=dev)
    check(_lib.lib().gf_inlier_index(_p(kp0), _p(kp1), _p(keep), _p(counts), N, L, S, int(w0), int(w1), int(scale),
                                     _p(map0), _p(map1), _p(idx0), _p(idx1), _p(nidx), _stream()), 'gf_inlier_index')
    return {'map0': map0, 'map1': map1, 'idx0': idx0, 'idx1': idx1, 'nidx': nidx}


def self_attention_gathered(q, kmap, vmap, idx, nkeys, nhead=4):
    """K4.  q, kmap, vmap [N,L,256]; idx int32 [N,>=L]; nkeys int32 view with one entry per sample (any stride) -> [N,L,256].
    Row-strided views are taken as they are when the library can move their rows as 16-byte pieces (16-bit modes: a 16-byte aligned
    base and a row stride that is a multiple of 8 elements - e.g. the halves of a [N, L, 512] k|v projection); any other view is
    copied to a contiguous tensor first."""
    _need_cuda(q, kmap, vmap, idx, nkeys)
    N, L, C = q.shape

    def rows16(t):
        t, ld = _rows(t)
        if t.element_size() == 2 and (t.data_ptr() % 16 != 0 or ld % 8 != 0):
            t = t.contiguous()
            ld = t.shape[-1]
        return t, ld
    q, ldq = rows16(q)
    kmap, ldk = rows16(kmap)
    vmap, ldv = rows16(vmap)
    for t, ld in ((q, ldq), (kmap, ldk), (vmap, ldv)):
        if t.stride(0) != ld * L:
            raise ValueError('self_attention_gathered needs batch stride == L * row stride')
    out = torch.empty(N, L, C, dtype=q.dtype, device=q.device)
    L_ = _lib.lib()
    nbytes = L_.gf_self_attention_workspace_bytes(N, L, _dt(q))
    ws = _ws.get('k4', nbytes, q.device)
    check(L_.gf_self_attention_gathered(_p(q), _p(kmap), _p(vmap), _dt(q), N, L, nhead, C // nhead, ldq, ldk, ldv,
                                        _p(idx), idx.stride(0), _p(nkeys), nkeys.stride(0) if nkeys.dim() else 1,
                                        _p(out), _p(ws), ws.numel(), _stream()), 'gf_self_attention_gathered')
    return out


def window_cross_attention(q, kmap, vmap, win, valid=None, nhead=4, hw_q=None, hw_k=None):
    """K5.  q [N,L,256]; kmap, vmap [N,S,256]; win int32 [N,L,25] -> [N,L,256].  With the map shapes hw_q = (hq, wq),
    hw_k = (hk, wk) (L = hq*wq, S = hk*wk) the 16-bit modes run the tiled form (key / value rows of a query tile's windows
    staged in LDS once)."""
    _need_cuda(q, kmap, vmap, win)
    N, L, C = q.shape
    S = kmap.shape[1]
    q, ldq = _rows(q)
    kmap, ldk = _rows(kmap)
    vmap, ldv = _rows(vmap)
    if q.stride(0) != ldq * L or kmap.stride(0) != ldk * S or vmap.stride(0) != ldv * S:
        raise ValueError('window_cross_attention needs batch stride == rows * row stride')
    out = torch.empty(N, L, C, dtype=q.dtype, device=q.device)
    if hw_q is not None and hw_k is not None and ldq % 8 == 0 and ldk % 8 == 0 and ldv % 8 == 0:
        if hw_q[0] * hw_q[1] != L or hw_k[0] * hw_k[1] != S:
            raise ValueError('window_cross_attention: map shapes do not match the token counts')
        check(_lib.lib().gf_window_cross_attention_tiled(_p(q), _p(kmap), _p(vmap), _dt(q), N, hw_q[0], hw_q[1], hw_k[0],
                                                         hw_k[1], nhead, C // nhead, ldq, ldk, ldv, _p(win), win.shape[-1],
                                                         _p(valid), _p(out), _stream()), 'gf_window_cross_attention_tiled')
        return out
    check(_lib.lib().gf_window_cross_attention(_p(q), _p(kmap), _p(vmap), _dt(q), N, L, S, nhead, C // nhead, ldq, ldk,
                                               ldv, _p(win), win.shape[-1], _p(valid), _p(out), _stream()),
          'gf_window_cross_attention')
    return out


def window_inverse_index(win, S):
    """The inverse of the window table win int32 [N, L, WW] (cell of the other image per window position, < 0 = masked) for the gather form
    of K5's backward: (entries int32 [N*L*WW] = l*WW + k sorted - stably - by global cell n*S + cell, masked positions last;
    offsets int32 [N*S + 1]).  torch ops only, no host synchronisation; one sort of N*L*WW keys."""
    N, L, WW = win.shape
    base = (torch.arange(N, device=win.device, dtype=torch.int64) * S)[:, None, None]
    key = torch.where(win >= 0, win.to(torch.int64) + base, N * S).reshape(-1)
    key, order = torch.sort(key, stable=True)
    entries = (order % (L * WW)).to(torch.int32)
    counts = torch.bincount(key, minlength=N * S + 1)[:N * S]
    offsets = torch.zeros(N * S + 1, dtype=torch.int32, device=win.device)
    offsets[1:] = counts.cumsum(0).to(torch.int32)
    return entries, offsets


def window_cross_attention_backward_gather(q, kmap, vmap, dout, win, index, nhead=4):
    """(dq [N,L,256], dk, dv [N,S,256], all of q's dtype) of window_cross_attention given dout [N,L,256], the cell sums gathered along
    `index` = window_inverse_index(win, S): no atomics, bit-reproducible."""
    _need_cuda(q, kmap, vmap, dout, win)
    N, L, C = q.shape
    S = kmap.shape[1]
    q, ldq = _rows(q)
    kmap, ldk = _rows(kmap)
    vmap, ldv = _rows(vmap)
    if q.stride(0) != ldq * L or kmap.stride(0) != ldk * S or vmap.stride(0) != ldv * S:
        raise ValueError('window_cross_attention_backward needs batch stride == rows * row stride')
    dout = _contig(dout)
    entries, offsets = index
    dq = torch.empty(N, L, C, dtype=q.dtype, device=q.device)
    dkv = torch.empty(2, N, S, C, dtype=q.dtype, device=q.device)
    L_ = _lib.lib()
    ws = _ws.get('k5bwd', L_.gf_window_cross_attention_backward_workspace_bytes(N, L, win.shape[-1]), q.device)
    check(L_.gf_window_cross_attention_backward_gather(_p(q), _p(kmap), _p(vmap), _p(dout), _dt(q), N, L, S, nhead, C // nhead, ldq, ldk, ldv,
                                                       _p(win), win.shape[-1], _p(entries), _p(offsets), _p(dq), _p(dkv[0]), _p(dkv[1]),
                                                       _p(ws), ws.numel(), _stream()), 'gf_window_cross_attention_backward_gather')
    return dq, dkv[0], dkv[1]


def window_cross_attention_backward(q, kmap, vmap, dout, win, nhead=4):
    """(dq [N,L,256] of q's dtype, dk, dv fp32 [N,S,256]) of window_cross_attention given dout [N,L,256]."""
    _need_cuda(q, kmap, vmap, dout, win)
    N, L, C = q.shape
    S = kmap.shape[1]
    q, ldq = _rows(q)
    kmap, ldk = _rows(kmap)
    vmap, ldv = _rows(vmap)
    if q.stride(0) != ldq * L or kmap.stride(0) != ldk * S or vmap.stride(0) != ldv * S:
        raise ValueError('window_cross_attention_backward needs batch stride == rows * row stride')
    dout = _contig(dout)
    dq = torch.empty(N, L, C, dtype=q.dtype, device=q.device)
    dkv = torch.zeros(2, N, S, C, dtype=torch.float32, device=q.device)
    check(_lib.lib().gf_window_cross_attention_backward(_p(q), _p(kmap), _p(vmap), _p(dout), _dt(q), N, L, S, nhead, C // nhead, ldq, ldk, ldv,
                                                        _p(win), win.shape[-1], _p(dq), _p(dkv[0]), _p(dkv[1]), _stream()),
          'gf_window_cross_attention_backward')
    return dq, dkv[0], dkv[1]


def fine_gather(feat_f0, feat_f1, feat_c0, feat_c1, b_ids, i_ids, j_ids, w0c, w1c, stride, window, out_dtype):
    """K7.  feat_f* [N,Cf,H,W] any strides, both of one dtype (fp32, fp16 or bf16; it need not be out_dtype); feat_c* [N,L,CC]
    contiguous of out_dtype; ids int64 [M] (M > 0) -> (win [2M, W*W, Cf], ccat [2M, CC]), both of out_dtype.  The window values
    are feat.float().to(out_dtype) bit for bit (bf16 maps -> fp16 windows: the 'bf16_fp16' mode; no clamp: beyond fp16's range -> inf).
    feat_f0 / feat_f1 may be MapBatches (both, or neither): the maps are read in place through gf_fine_gather_ptrs, same bits.
    Or RaggedMapBatches (both, or neither; gf_fine_gather_ragged): w0c / w1c are the canvases' widths in coarse cells, a tap outside a
    map's own extent is zero, the bits are those of the tensor path on the maps zero-padded and stacked."""
    kind0, kind1 = (RaggedMapBatch if isinstance(f, RaggedMapBatch) else MapBatch if isinstance(f, MapBatch) else None for f in (feat_f0, feat_f1))
    if kind0 is not kind1:
        raise TypeError('fine_gather: feat_f0 and feat_f1 must both be tensors, both be MapBatches or both be RaggedMapBatches')
    if kind0 is not None:
        _need_cuda(*feat_f0.maps, *feat_f1.maps, feat_c0, feat_c1, b_ids)
        if len(feat_f0) != len(feat_f1):
            raise ValueError(f'fine_gather: {len(feat_f0)} maps on side 0, {len(feat_f1)} on side 1')
    else:
        _need_cuda(feat_f0, feat_f1, feat_c0, feat_c1, b_ids)
    M = b_ids.shape[0]
    Cf = feat_f0.shape[1]
    CC = feat_c0.shape[-1]
    dev = feat_f0.device
    win = torch.empty(2 * M, window * window, Cf, dtype=out_dtype, device=dev)
    ccat = torch.empty(2 * M, CC, dtype=out_dtype, device=dev)
    fc0, fc1 = _contig(feat_c0), _contig(feat_c1)
    if fc0.dtype != out_dtype or fc1.dtype != out_dtype or feat_f0.dtype != feat_f1.dtype:
        raise TypeError('fine_gather: coarse features must already be in out_dtype; fine maps must share a dtype')
    ids = [_contig(t) for t in (b_ids, i_ids, j_ids)]
    L_ = _lib.lib()
    rest = (Cf, _p(fc0), _p(fc1), _DTYPES[out_dtype], fc0.shape[1], fc1.shape[1], CC, *map(_p, ids), M, int(w0c), int(w1c), int(stride),
            int(window), _p(win), _p(ccat), _stream())
    if kind0 is RaggedMapBatch:
        check(L_.gf_fine_gather_ragged(_p(feat_f0.table()), _p(feat_f1.table()), len(feat_f0), _dt(feat_f0), min(feat_f0.align, feat_f1.align),
                                       *rest), 'gf_fine_gather_ragged')
        return win, ccat
    # the two entries with strides and extent common to all samples: those of one map (MapBatch: [C,H,W]) or of the batch tensor
    strides = [feat.map_stride if kind0 is MapBatch else feat.stride() for feat in (feat_f0, feat_f1)]
    s0, s1 = ((ctypes.c_long * len(st))(*st) for st in strides)
    geom = (ctypes.cast(s0, ctypes.c_void_p), ctypes.cast(s1, ctypes.c_void_p), *feat_f0.shape[2:], *feat_f1.shape[2:])
    if kind0 is MapBatch:
        check(L_.gf_fine_gather_ptrs(_p(feat_f0.table()), _p(feat_f1.table()), len(feat_f0), _dt(feat_f0), min(feat_f0.align, feat_f1.align),
                                     *geom, *rest), 'gf_fine_gather_ptrs')
    else:
        check(L_.gf_fine_gather(_p(feat_f0), _p(feat_f1), _dt(feat_f0), *geom, *rest), 'gf_fine_gather')
    return win, ccat


def _map_kind(feat_f0, feat_f1, what):
    kind0, kind1 = (RaggedMapBatch if isinstance(f, RaggedMapBatch) else MapBatch if isinstance(f, MapBatch) else None for f in (feat_f0, feat_f1))
    if kind0 is not kind1:
        raise TypeError(f'{what}: feat_f0 and feat_f1 must both be tensors, both be MapBatches or both be RaggedMapBatches')
    return kind0


def fine_rows_supported(feat_f0, feat_f1, dtype):
    """Can `fine_rows` name the window rows of these maps for a `linear_rows` in `dtype`?  16-bit maps of that very dtype (nothing to
    convert) whose channel rows are contiguous and 16-byte aligned: channels-last, every other stride a multiple of 8 elements.  Decided
    from what the host knows (dtypes, strides, addresses): no device synchronisation."""
    kind = _map_kind(feat_f0, feat_f1, 'fine_rows')
    if dtype not in (torch.float16, torch.bfloat16) or feat_f0.dtype != dtype or feat_f1.dtype != dtype or feat_f0.shape[1] % 64:
        return False
    for f in (feat_f0, feat_f1):
        if kind is None:
            ok = f.data_ptr() % 16 == 0 and f.stride(1) == 1 and all(s % 8 == 0 for s in (f.stride(0), f.stride(2), f.stride(3)))
        elif kind is MapBatch:
            ok = f.align >= 16 and f.map_stride[0] == 1 and f.map_stride[1] % 8 == 0 and f.map_stride[2] % 8 == 0
        else:
            ok = f.align >= 16 and all(m.stride(0) == 1 and m.stride(1) % 8 == 0 and m.stride(2) % 8 == 0 for m in f.maps)
        if not ok:
            return False
    return True


def fine_rows(feat_f0, feat_f1, feat_c0, feat_c1, b_ids, i_ids, j_ids, w0c, w1c, stride, window, supported=None):
    """The K7 gather as address tables for `linear_rows` (gf_fine_rows and its siblings; `fine_rows_supported` says when): the arguments of
    `fine_gather` -> (win_rows int64 [2M, W*W], coarse_rows int64 [2M]): the address of every window tap's channel row in the fine maps
    (0 where fine_gather writes zeros) and of the coarse feature rows.  feat_c* must be contiguous and, like the maps, outlive the
    launches that read the tables.  supported: `fine_rows_supported`'s answer for these maps, where the caller has asked already."""
    kind = _map_kind(feat_f0, feat_f1, 'fine_rows')
    if not (fine_rows_supported(feat_f0, feat_f1, feat_f0.dtype) if supported is None else supported):
        raise ValueError('fine_rows: the maps need 16-bit, contiguous, 16-byte aligned channel rows (fine_rows_supported)')
    if not (feat_c0.is_contiguous() and feat_c1.is_contiguous()) or feat_c0.element_size() != 2 or feat_c1.element_size() != 2:
        raise ValueError('fine_rows: the coarse features must be contiguous 16-bit tensors')
    if kind is not None and len(feat_f0) != len(feat_f1):
        raise ValueError(f'fine_rows: {len(feat_f0)} maps on side 0, {len(feat_f1)} on side 1')
    _need_cuda(*(feat_f0.maps + feat_f1.maps if kind is not None else (feat_f0, feat_f1)), feat_c0, feat_c1, b_ids)
    M = b_ids.shape[0]
    dev = feat_f0.device
    win_rows = torch.empty(2 * M, window * window, dtype=torch.int64, device=dev)
    c_rows = torch.empty(2 * M, dtype=torch.int64, device=dev)
    ids = [_contig(t) for t in (b_ids, i_ids, j_ids)]
    L_ = _lib.lib()
    rest = (_p(feat_c0), _p(feat_c1), feat_c0.shape[1], feat_c1.shape[1], feat_c0.shape[-1], *map(_p, ids), M, int(w0c), int(w1c), int(stride),
            int(window), _p(win_rows), _p(c_rows), _stream())
    if kind is RaggedMapBatch:
        check(L_.gf_fine_rows_ragged(_p(feat_f0.table()), _p(feat_f1.table()), len(feat_f0), min(feat_f0.align, feat_f1.align), *rest),
              'gf_fine_rows_ragged')
        return win_rows, c_rows
    strides = [feat.map_stride if kind is MapBatch else feat.stride() for feat in (feat_f0, feat_f1)]
    s0, s1 = ((ctypes.c_long * len(st))(*st) for st in strides)
    geom = (ctypes.cast(s0, ctypes.c_void_p), ctypes.cast(s1, ctypes.c_void_p), *feat_f0.shape[2:], *feat_f1.shape[2:])
    if kind is MapBatch:
        check(L_.gf_fine_rows_ptrs(_p(feat_f0.table()), _p(feat_f1.table()), len(feat_f0), min(feat_f0.align, feat_f1.align), *geom, *rest),
              'gf_fine_rows_ptrs')
    else:
        check(L_.gf_fine_rows(_p(feat_f0), _p(feat_f1), *geom, *rest), 'gf_fine_rows')
    return win_rows, c_rows


def fine_match(f0, f1, temperature, thr, b_ids, mkpts0_c, mkpts1_c, coarse_scale, c2f_scale, fine_scale, scale0=None,
               scale1=None):
    """K8.  f0, f1 [M,25,C] (M > 0) -> dict(fine_matrix [M,25,25], mkpts0_f/mkpts1_f [M,2] (first count rows
    valid), mconf [M], m_bids int64 [M], count int32 [1])."""
    _need_cuda(f0, f1)
    f0, f1 = _contig(f0), _contig(f1)
    M, WW, C = f0.shape
    dev = f0.device
    fm = torch.empty(M, WW, WW, dtype=torch.float32, device=dev)
    mk = torch.empty(2, M, 2, dtype=torch.float32, device=dev)
    mconf = torch.empty(M, dtype=torch.float32, device=dev)
    mb = torch.empty(M, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    s0 = None if scale0 is None else _contig(scale0.to(device=dev, dtype=torch.float32))
    s1 = None if scale1 is None else _contig(scale1.to(device=dev, dtype=torch.float32))
    L_ = _lib.lib()
    nbytes = L_.gf_fine_match_workspace_bytes(M)
    ws = _ws.get('k8', nbytes, dev)
    check(L_.gf_fine_match(_p(f0), _p(f1), _dt(f0), M, WW, C, float(temperature), float(thr), _p(_contig(b_ids)),
                           _p(_contig(mkpts0_c)), _p(_contig(mkpts1_c)), float(coarse_scale), float(c2f_scale),
                           float(fine_scale), _p(s0), _p(s1), _p(fm), _p(mk[0]), _p(mk[1]), _p(mconf), _p(mb), _p(count),
                           _p(ws), ws.numel(), _stream()), 'gf_fine_match')
    return {'fine_matrix': fm, 'mkpts0_f': mk[0], 'mkpts1_f': mk[1], 'mconf': mconf, 'm_bids': mb, 'count': count}


EPI_NONE, EPI_RELU, EPI_TANH, EPI_LN, EPI_LN_RES = 0, 1, 2, 3, 4


def _rows2d(t):
    """[..., K] -> (tensor viewed as rows, row stride); last dim contiguous and rows uniformly strided."""
    if t.stride(-1) != 1:
        t = t.contiguous()
    lead = t.shape[:-1]
    ld = t.stride(-2) if t.dim() > 1 else t.shape[-1]
    # every leading dim must collapse onto one row stride
    expect = ld
    for size, stride in zip(reversed(lead), reversed(t.stride()[:-1])):
        if size != 1 and stride != expect:
            t = t.contiguous()
            ld = t.shape[-1]
            break
        expect *= size
    return t, ld


def linear(a1, w, a2=None, bias=None, rowgroup_bias=None, rowgroup_rows=0, epilogue=EPI_NONE, ln=None, eps=1e-5,
           residual=None, row_flag=None, flag_rows=0, out=None):
    """K3.  out[..., n] = epi([a1|a2] @ w.T + bias + rowgroup_bias); see include/geoformer_hip.h (gf_linear).
    ln = (gamma fp32 [N], beta fp32 [N]) for the LayerNorm epilogues."""
    _need_cuda(a1, w)
    a1, lda1 = _rows2d(a1)
    k1 = a1.shape[-1]
    k2, lda2 = 0, 0
    if a2 is not None:
        a2, lda2 = _rows2d(a2)
        k2 = a2.shape[-1]
    N = w.shape[0]
    M = a1.numel() // k1
    if out is None:
        out = torch.empty(*a1.shape[:-1], N, dtype=a1.dtype, device=a1.device)
    elif out.shape != (*a1.shape[:-1], N) or out.dtype != a1.dtype or not out.is_contiguous():
        raise ValueError('out must be a contiguous tensor of the result shape and dtype')
    res, ldres = (None, 0) if residual is None else _rows2d(residual)
    g, b = (None, None) if ln is None else ln
    check(_lib.lib().gf_linear(_p(a1), lda1, k1, _p(a2), lda2, k2, _p(w), _p(bias), _p(rowgroup_bias), int(rowgroup_rows),
                               int(epilogue), _p(g), _p(b), float(eps), _p(res), ldres, _p(row_flag), int(flag_rows), _p(out),
                               N, _dt(a1), M, N, _stream()), 'gf_linear')
    return out


def index_rows(x, idx):
    """The row table of a token list (gf_index_rows): x [N, L, C] with contiguous rows and batch stride L * row stride, idx int32 [N, >= L]
    -> int64 [N, L], entry (n, j) the address of x[n, clamp(idx[n, j], 0, L - 1)].  x must outlive the launches that read the table."""
    _need_cuda(x, idx)
    N, L, _ = x.shape
    ld = x.stride(1)
    if x.stride(2) != 1 or x.stride(0) != ld * L or idx.dtype != torch.int32 or idx.shape[0] != N or idx.shape[1] < L or idx.stride(1) != 1:
        raise ValueError('index_rows: x needs batch stride == L * row stride, idx int32 [N, >= L] with contiguous rows')
    rows = torch.empty(N, L, dtype=torch.int64, device=x.device)
    check(_lib.lib().gf_index_rows(_p(x), ld * x.element_size(), _p(idx), idx.stride(0), N, L, _p(rows), _stream()), 'gf_index_rows')
    return rows


def linear_rows(rows, w, row_align=16, bias=None, rowgroup_bias=None, rowgroup_rows=0, epilogue=EPI_NONE, ln=None, eps=1e-5,
                residual=None, row_flag=None, flag_rows=0, out=None, group_count=None):
    """K3 on gathered rows without the gather (gf_linear_rows): `rows` is a contiguous int64 device tensor [...] of row addresses - each
    names w.shape[1] contiguous elements of w's dtype (fp16 or bf16), 16-byte aligned; 0 names a row of zeros - and the result
    [..., N] has the bits of `linear` on those rows copied into a tensor.  row_align: the caller's promise - a power of two (bytes)
    that divides every non-zero address, at least 16; the table lies in device memory and is not inspected, the value selects nothing
    (a caller who cannot promise 16 gets an error instead of misaligned loads).  The rows must stay allocated and unchanged until the launch has run.  Other arguments as in `linear`.
    group_count: int32 device view with one entry per rows[g] (rows [G, R]: G groups of R rows; any stride): only the first
    group_count[g] rows of group g are wanted - a 128-row tile without a wanted row is skipped and its output rows stay unwritten."""
    _need_cuda(rows, w)
    if rows.dtype != torch.int64 or not rows.is_contiguous():
        raise ValueError('linear_rows: rows must be a contiguous int64 tensor of addresses')
    if w.dim() != 2 or not w.is_contiguous():
        raise ValueError('linear_rows: w must be a contiguous [N, K] tensor')
    N, k = w.shape
    M = rows.numel()
    if out is None:
        out = torch.empty(*rows.shape, N, dtype=w.dtype, device=w.device)
    elif out.shape != (*rows.shape, N) or out.dtype != w.dtype or not out.is_contiguous():
        raise ValueError('out must be a contiguous tensor of the result shape and dtype')
    res, ldres = (None, 0) if residual is None else _rows2d(residual)
    g, b = (None, None) if ln is None else ln
    gstride = grows = 0
    if group_count is not None:
        if rows.dim() != 2 or group_count.dtype != torch.int32 or group_count.numel() != rows.shape[0]:
            raise ValueError('linear_rows: group_count needs rows [G, R] and one int32 count per group')
        grows, gstride = rows.shape[1], (group_count.stride(0) if group_count.dim() else 1)
    check(_lib.lib().gf_linear_rows(_p(rows), int(row_align), _p(group_count), gstride, grows, k, _p(w), _p(bias), _p(rowgroup_bias), int(rowgroup_rows), int(epilogue),
                                    _p(g), _p(b), float(eps), _p(res), ldres, _p(row_flag), int(flag_rows), _p(out), N, _dt(w), M, N,
                                    _stream()), 'gf_linear_rows')
    return out


# ---------------------------------------------------------------------------------------------
# training: fused dual-softmax focal loss (forward + backward in HIP, nothing L x S is materialised)
# ---------------------------------------------------------------------------------------------
class CoarseFocalLoss(torch.autograd.Function):
    """sum_k -alpha (1 - p_k)^gamma log p_k * w_k over the positives k = (b, i, j), p = the dual-softmax confidence
    of (f0, f1) at temperature `temperature` (loftr_loss.py:246-270 on coarse_matching.py:113-125).  Returns
    (loss_sum, p [P]); gradients flow to f0 and f1 only."""

    @staticmethod
    def forward(ctx, f0, f1, pos_b, pos_i, pos_j, temperature, alpha, gamma, weight, mask0=None, mask1=None):
        _need_cuda(f0, f1, pos_b)
        N, L, C = f0.shape
        S = f1.shape[1]
        P = pos_b.numel()
        ctx_dtype = f0.dtype                       # the gradients go back in the caller's dtype
        if f0.dtype == torch.bfloat16:           # the mixed-bf16 training step: the kernels take fp16 operands (same 16-bit
            f0, f1 = f0.to(torch.float16), f1.to(torch.float16)       # storage, 3 more mantissa bits; features are O(1))
        f0c, f1c = _contig(f0), _contig(f1)
        if f0c.dtype not in (torch.float32, torch.float16) or f1c.dtype != f0c.dtype:
            raise ValueError('f0/f1 must both be fp32, fp16 or bf16')
        L_ = _lib.lib()
        ws = torch.empty(L_.gf_coarse_loss_workspace_bytes(N, L, S), dtype=torch.uint8, device=f0.device)
        conf = torch.empty(P, dtype=torch.float32, device=f0.device)
        loss, grad = torch.empty_like(conf), torch.empty_like(conf)
        pb, pi, pj = _contig(pos_b.long()), _contig(pos_i.long()), _contig(pos_j.long())
        w = None if weight is None else _contig(weight.float())
        m0 = None if mask0 is None else _contig(mask0.reshape(N, L).to(torch.uint8))
        m1 = None if mask1 is None else _contig(mask1.reshape(N, S).to(torch.uint8))
        ctx.masks = (m0, m1)
        check(L_.gf_coarse_loss_forward(_p(f0c), _p(f1c), _dt(f0c), N, L, S, C, _p(m0), _p(m1), float(temperature), _p(pb), _p(pi), _p(pj), P, _p(w),
                                        float(alpha), float(gamma), _p(conf), _p(loss), _p(grad), _p(ws), ws.numel(), _stream()),
              'gf_coarse_loss_forward')
        ctx.save_for_backward(pb, pi, pj, grad, ws)
        ctx.meta = (N, L, S, C, float(temperature), ctx_dtype)
        ctx.mark_non_differentiable(conf)
        return loss.sum(), conf

    @staticmethod
    def backward(ctx, g_loss, _g_conf):
        pb, pi, pj, grad, ws = ctx.saved_tensors
        N, L, S, C, temperature, dtype = ctx.meta
        d0 = torch.empty(N, L, C, dtype=torch.float32, device=grad.device)
        d1 = torch.empty(N, S, C, dtype=torch.float32, device=grad.device)
        m0, m1 = ctx.masks
        gl = _contig(g_loss.detach().reshape(1).to(device=grad.device, dtype=torch.float32))   # stays on the device: no host sync
        check(_lib.lib().gf_coarse_loss_backward(N, L, S, C, _p(m0), _p(m1), temperature, _p(pb), _p(pi), _p(pj), pb.numel(), _p(grad),
                                                 1.0, _p(gl), _p(d0), _p(d1), _p(ws), ws.numel(), _stream()),
              'gf_coarse_loss_backward')
        return d0.to(dtype), d1.to(dtype), None, None, None, None, None, None, None, None, None


def coarse_focal_loss(f0, f1, pos_b, pos_i, pos_j, temperature, alpha=0.25, gamma=2.0, weight=None, mask0=None, mask1=None):
    return CoarseFocalLoss.apply(f0, f1, pos_b, pos_i, pos_j, temperature, alpha, gamma, weight, mask0, mask1)


# ---------------------------------------------------------------------------------------------
# training: backward of the K3 chain (linear, LayerNorm, activation) - see csrc/k_train.hip
# ---------------------------------------------------------------------------------------------
def linear_wgrad(dy, x, out=None, accumulate=False):
    """dW [cout, cin] fp32 (+)= dy^T x over all leading dimensions; dy [..., cout], x [..., cin] 16-bit (row-strided views allowed).
    `out` may be a column block of a wider gradient (row stride > cin): the two halves of torch.cat([x, m]) write theirs."""
    _need_cuda(dy, x)
    dy, lddy = _rows2d(dy)
    x, ldx = _rows2d(x)
    cout, cin = dy.shape[-1], x.shape[-1]
    T = dy.numel() // cout
    if out is None:
        out = torch.empty(cout, cin, dtype=torch.float32, device=dy.device)
    L_ = _lib.lib()
    ws = _ws.get('wgrad', L_.gf_linear_wgrad_workspace_bytes(T, cout, cin), dy.device)
    check(L_.gf_linear_wgrad(_p(dy), lddy, _p(x), ldx, _dt(dy), T, cout, cin, _p(out), out.stride(0), int(bool(accumulate)), _p(ws), ws.numel(),
                             _stream()), 'gf_linear_wgrad')
    return out


def layernorm_forward(y, gamma, beta, eps=1e-5):
    """(LayerNorm(y) in y's 16-bit dtype, stats fp32 [T, 2] = (mean, rstd)); gamma, beta fp32."""
    _need_cuda(y, gamma)
    y = _contig(y)
    C = y.shape[-1]
    T = y.numel() // C
    out = torch.empty_like(y)
    stats = torch.empty(T, 2, dtype=torch.float32, device=y.device)
    check(_lib.lib().gf_layernorm_forward(_p(y), _dt(y), T, C, _p(gamma), _p(beta), float(eps), _p(out), _p(stats), _stream()),
          'gf_layernorm_forward')
    return out, stats


def layernorm_backward(dout, y, stats, gamma):
    """(dy in y's dtype, dgamma fp32 [C], dbeta fp32 [C])."""
    _need_cuda(dout, y)
    dout, y = _contig(dout), _contig(y)
    C = y.shape[-1]
    T = y.numel() // C
    dy = torch.empty_like(y)
    dg = torch.empty(2, C, dtype=torch.float32, device=y.device)
    L_ = _lib.lib()
    ws = _ws.get('lnbwd', L_.gf_layernorm_backward_workspace_bytes(C), y.device)
    check(L_.gf_layernorm_backward(_p(dout), _p(y), _p(stats), _dt(y), T, C, _p(gamma), _p(dy), _p(dg[0]), _p(dg[1]), 0, _p(ws), ws.numel(),
                                   _stream()), 'gf_layernorm_backward')
    return dy, dg[0], dg[1]


def activation_backward(dh, h, kind):
    """dz = dh * act'(z) from the activation's output h (kind 'relu' | 'tanh'); 16-bit tensors."""
    _need_cuda(dh, h)
    dh, h = _contig(dh), _contig(h)
    dz = torch.empty_like(h)
    check(_lib.lib().gf_activation_backward(_p(dh), _p(h), _p(dz), h.numel(), {'relu': 0, 'tanh': 1}[kind], _dt(h), _stream()),
          'gf_activation_backward')
    return dz


def linear_attention_backward(q, k, v, dout, nhead, q_mask=None, kv_mask=None, eps=1e-6):
    """(dq [N,L,C], dk, dv [N,S,C]) of K2's linear attention given dout [N,L,C]; q [N,L,C], k, v [N,S,C] (row-strided views allowed),
    heads of 32 channels, 16-bit tensors."""
    _need_cuda(q, k, v, dout)
    N, L, C = q.shape
    S = k.shape[1]
    D = C // nhead
    q, ldq = _rows(q)
    k, ldk = _rows(k)
    v, ldv = _rows(v)
    dout, ldo = _rows(dout)
    for t, ld, n in ((q, ldq, L), (dout, ldo, L), (k, ldk, S), (v, ldv, S)):
        if t.stride(0) != ld * n:
            raise ValueError('linear_attention_backward needs batch stride == rows * row stride')
    dq = torch.empty(N, L, C, dtype=q.dtype, device=q.device)
    dkv = torch.empty(2, N, S, C, dtype=q.dtype, device=q.device)
    qm = None if q_mask is None else _contig(q_mask.reshape(N, L).to(torch.uint8))
    km = None if kv_mask is None else _contig(kv_mask.reshape(N, S).to(torch.uint8))
    L_ = _lib.lib()
    ws = _ws.get('k2bwd', L_.gf_linear_attention_backward_workspace_bytes(N, L, S, nhead), q.device)
    check(L_.gf_linear_attention_backward(_p(q), _p(k), _p(v), _p(dout), _dt(q), N, L, S, nhead, D, ldq, ldk, ldv, ldo, _p(qm), _p(km), float(eps),
                                          _p(dq), _p(dkv[0]), _p(dkv[1]), _p(ws), ws.numel(), _stream()), 'gf_linear_attention_backward')
    return dq, dkv[0], dkv[1]


def _rows16(t, rows):
    """A [N, rows, C] 16-bit tensor as the training attention kernels take it: last dim contiguous, 16-byte aligned rows with a stride
    that is a multiple of 8 elements, batch stride = rows x row stride; anything else is copied."""
    if (t.stride(-1) != 1 or t.data_ptr() % 16 or t.stride(-2) % 8 or t.stride(-2) < t.shape[-1] or
            (t.shape[0] > 1 and t.stride(0) != rows * t.stride(-2))):
        t = t.contiguous()
    return t, t.stride(-2)


def full_attention_train_forward(q, k, v, nhead):
    """K4 (training): softmax(q k^T / sqrt(D)) v of FullAttention (geo_attention.py:72-101, no masks) on q [N,L,256], k, v [N,S,256] 16-bit
    tensors with 4 heads of 64 -> (out [N,L,256], lse fp32 [N,4,L] = base-2 log-sum-exp of the scaled logits, kept for the backward)."""
    _need_cuda(q, k, v)
    N, L, C = q.shape
    S = k.shape[1]
    D = C // nhead
    q, ldq = _rows16(q, L)
    k, ldk = _rows16(k, S)
    v, ldv = _rows16(v, S)
    out = torch.empty(N, L, C, dtype=q.dtype, device=q.device)
    lse = torch.empty(N, nhead, L, dtype=torch.float32, device=q.device)
    check(_lib.lib().gf_full_attention_train_forward(_p(q), _p(k), _p(v), _dt(q), N, L, S, nhead, D, ldq, ldk, ldv, 1.0 / D ** 0.5, _p(out), C,
                                                     _p(lse), _stream()), 'gf_full_attention_train_forward')
    return out, lse


def full_attention_backward(q, k, v, out, dout, lse, nhead):
    """(dq [N,L,256], dk, dv [N,S,256]) of full_attention_train_forward given its out / lse and dout [N,L,256]."""
    _need_cuda(q, k, v, out, dout, lse)
    N, L, C = q.shape
    S = k.shape[1]
    D = C // nhead
    q, ldq = _rows16(q, L)
    k, ldk = _rows16(k, S)
    v, ldv = _rows16(v, S)
    out, ldo = _rows16(out, L)
    dout, lddo = _rows16(dout, L)
    dq = torch.empty(N, L, C, dtype=q.dtype, device=q.device)
    dkv = torch.empty(2, N, S, C, dtype=q.dtype, device=q.device)
    L_ = _lib.lib()
    ws = _ws.get('k4bwd', L_.gf_full_attention_backward_workspace_bytes(N, L, nhead), q.device)
    check(L_.gf_full_attention_backward(_p(q), _p(k), _p(v), _p(out), _p(dout), _p(_contig(lse)), _dt(q), N, L, S, nhead, D, ldq, ldk, ldv, ldo, lddo,
                                        1.0 / D ** 0.5, _p(dq), _p(dkv[0]), _p(dkv[1]), _p(ws), ws.numel(), _stream()),
          'gf_full_attention_backward')
    return dq, dkv[0], dkv[1]


def window_linear_attention_backward(q, k, v, dout, eps=1e-6):
    """(dq, dk, dv) [Nw, Lw, 128] of the fine level's window linear attention (8 heads of 16, Lw <= 32, no masks) given dout."""
    _need_cuda(q, k, v, dout)
    q, k, v, dout = _contig(q), _contig(k), _contig(v), _contig(dout)
    Nw, Lw, C = q.shape
    if C != 128 or Lw > 32 or k.shape != q.shape or v.shape != q.shape or dout.shape != q.shape:
        raise ValueError('window_linear_attention_backward: [Nw, Lw <= 32, 128] tensors of one shape')
    d = torch.empty(3, Nw, Lw, C, dtype=q.dtype, device=q.device)
    if Nw:
        check(_lib.lib().gf_window_linear_attention_backward(_p(q), _p(k), _p(v), _p(dout), _dt(q), Nw, Lw, float(eps), _p(d[0]), _p(d[1]),
                                                             _p(d[2]), _stream()), 'gf_window_linear_attention_backward')
    return d[0], d[1], d[2]


def fine_match_backward(f0, f1, temperature, dconf):
    """(df0, df1) [M,25,C] of K8's fine_matrix given dconf fp32 [M,25,25]; f0, f1 [M,25,C] (M > 0) of one dtype."""
    _need_cuda(f0, f1, dconf)
    f0, f1, dconf = _contig(f0), _contig(f1), _contig(dconf.float())
    M, WW, C = f0.shape
    df = torch.empty(2, M, WW, C, dtype=f0.dtype, device=f0.device)
    check(_lib.lib().gf_fine_match_backward(_p(f0), _p(f1), _dt(f0), M, WW, C, float(temperature), _p(dconf), _p(df[0]), _p(df[1]), _stream()),
          'gf_fine_match_backward')
    return df[0], df[1]


# ---------------------------------------------------------------------------------------------
# keypoint consolidation for SfM (csrc/k_keypoints.hip over csrc/keypoint_spec.h)
# ---------------------------------------------------------------------------------------------
KP_FLAG_COORD_RANGE, KP_FLAG_IMAGE_RANGE = 1, 2        # keypoint_spec.h KP_FLAG_*: bits of counts[0]


def consolidate_keypoints(matches, scores, pair_offsets, pair_images, n_images, sc_thres=0.25, psize=48.0, dthres=4.0, unique=True):
    """Pair matches -> one keypoint list per image and every match as a pair of keypoint indices, on the device: the reference's
    process_matches_and_keypoints_exporth5 / matches_to_keypoint_ids (score filter, quantize_keypoints or compute_keypoints, the uniqueness
    filter), bit for bit.  Device tensors: matches [M,4] (x0, y0, x1, y1; cast to fp32 first, as the reference stores them), scores [M],
    pair_offsets [P+1] (ascending, first 0, last M), pair_images [P,2] (image index of each side; a pair listed twice contributes twice).
    Returns (keypoints fp32 [K,2] image-major, kp_offsets int32 [n_images+1], ids int32 [M',2] per-image keypoint indices in row order,
    ids_offsets int32 [P+1]).  psize <= 0 or dthres <= 0: the exact mode (equal coordinates share a keypoint; no filter, as in the reference).
    Rows with a score below sc_thres, a NaN score or a non-finite coordinate are dropped (the reference would carry NaN through its
    dictionaries).  Supported: n_images <= 524288; quantised mode: psize > 2 and |coordinates| <= 2^22 - a larger coordinate or an image
    index outside [0, n_images) raises after the call's one device-to-host read (the output sizes and the status word), nothing wraps.
    Between the kernels, the order-preserving plumbing is torch's: one stable sort by group key and three scans."""
    _need_cuda(matches, scores, pair_offsets, pair_images)
    dev = matches.device
    M, P, n_images = int(matches.shape[0]), int(pair_images.shape[0]), int(n_images)
    if matches.shape != (M, 4) or scores.shape != (M,) or pair_offsets.shape != (P + 1,) or pair_images.shape != (P, 2):
        raise ValueError('consolidate_keypoints: matches [M,4], scores [M], pair_offsets [P+1], pair_images [P,2]')
    m, sc = _contig(matches.to(torch.float32)), _contig(scores.to(torch.float32))
    off, pim = _contig(pair_offsets.to(torch.int32)), _contig(pair_images.to(torch.int32))
    psize, dthres = float(psize), float(dthres)
    quant = psize > 0 and dthres > 0
    N = 2 * M
    L_ = _lib.lib()

    def i32(*shape):
        return torch.empty(*shape, dtype=torch.int32, device=dev)
    counts = i32(8)
    keys = torch.empty(N, dtype=torch.int64, device=dev)
    keys2 = None if quant else torch.empty(N, dtype=torch.int64, device=dev)
    pts = torch.empty(N, 2, dtype=torch.float32, device=dev)
    pseg, seg_begin = i32(N), i32(N)
    check(L_.gf_keypoint_keys(_p(m), _p(sc), _p(off), _p(pim), P, M, n_images, float(sc_thres), psize, dthres, _p(keys), _p(keys2), _p(pts),
                              _p(pseg), _p(seg_begin), _p(counts), _stream()), 'gf_keypoint_keys')
    if M == 0:
        return (torch.zeros(0, 2, dtype=torch.float32, device=dev), torch.zeros(n_images + 1, dtype=torch.int32, device=dev),
                torch.zeros(0, 2, dtype=torch.int32, device=dev), torch.zeros(P + 1, dtype=torch.int32, device=dev))
    if n_images < 1:
        raise ValueError('consolidate_keypoints: rows but no images')
    # grouping: a stable sort keeps arrival order inside a group (exact mode: least significant key first)
    if quant:
        order = torch.sort(keys, stable=True).indices
    else:
        o2 = torch.sort(keys2, stable=True).indices
        order = o2[torch.sort(keys[o2], stable=True).indices]
    head = i32(N)
    check(L_.gf_keypoint_heads(_p(keys), _p(keys2), _p(order), M, _p(head), _stream()), 'gf_keypoint_heads')
    group_scan = torch.cumsum(head, 0, dtype=torch.int32)
    ws = _ws.get('keypoints', L_.gf_keypoint_workspace_bytes(M), dev)
    owner, slot, creator = i32(N), i32(N), i32(N)
    cxy = torch.empty(N, 2, dtype=torch.float32, device=dev)
    check(L_.gf_keypoint_walk(_p(keys), _p(order), _p(head), _p(group_scan), _p(pts), _p(seg_begin), M, psize, dthres, _p(owner), _p(slot),
                              _p(creator), _p(cxy), _p(counts), _p(ws), ws.numel(), _stream()), 'gf_keypoint_walk')
    # keypoint ranks: a creator's id is its rank among its image's creators in arrival order.  Arrival order is segment (pair, side) major and a
    # segment lies in one image, so: scan the creator flags, count per segment, order the segments by image (stably), scan again - 2 P numbers.
    creator_scan = torch.cumsum(creator, 0, dtype=torch.int32)
    cx = torch.cat([creator_scan.new_zeros(1), creator_scan]).long()
    o64 = off.long()
    n = o64[1:] - o64[:-1]
    seg_b = torch.stack([2 * o64[:-1], 2 * o64[:-1] + n], 1).reshape(-1)
    seg_e = torch.stack([2 * o64[:-1] + n, 2 * o64[1:]], 1).reshape(-1)
    seg_cnt = cx[seg_e] - cx[seg_b]
    simg = pim.reshape(-1).long().clamp(0, n_images - 1)            # (a pair with an index out of range has no creators; the status word reports it)
    so = torch.sort(simg, stable=True).indices
    csum = torch.cat([seg_cnt.new_zeros(1), torch.cumsum(seg_cnt[so], 0)])
    seg_base = torch.empty_like(seg_cnt)
    seg_base[so] = csum[:-1]
    seg_adj = (seg_base - cx[seg_b]).to(torch.int32)
    kp_offsets = csum[torch.searchsorted(simg[so], torch.arange(n_images + 1, device=dev))].to(torch.int32)
    keep = i32(M)
    check(L_.gf_keypoint_filter(_p(sc), _p(off), P, M, _p(owner), _p(slot), int(bool(unique) and quant), _p(keep), _p(ws), ws.numel(), _stream()),
          'gf_keypoint_filter')
    keep_scan = torch.cumsum(keep, 0, dtype=torch.int32)
    keypoints = torch.empty(N, 2, dtype=torch.float32, device=dev)
    ids = i32(M, 2)
    ids_offsets = i32(P + 1)
    check(L_.gf_keypoint_emit(_p(creator), _p(creator_scan), _p(pseg), _p(seg_adj), _p(cxy), _p(keep), _p(keep_scan), _p(off), _p(pim), P, M,
                              _p(owner), _p(kp_offsets), _p(keypoints), _p(ids), _p(ids_offsets), _p(counts), _stream()), 'gf_keypoint_emit')
    c = counts.cpu()                                                # the one device-to-host read: status bits, K, M'
    flags, K, rows = int(c[0]), int(c[4]), int(c[5])
    if flags & KP_FLAG_IMAGE_RANGE:
        raise _lib.GeoFormerHipError(f'consolidate_keypoints: pair_images holds an index outside [0, {n_images})')
    if flags & KP_FLAG_COORD_RANGE:
        raise _lib.GeoFormerHipError('consolidate_keypoints: a coordinate lies outside the supported +-2^22 of the quantised mode')
    return keypoints[:K], kp_offsets, ids[:rows], ids_offsets


# ---------------------------------------------------------------------------------------------
# tracks and their triangulation from known poses (csrc/k_triangulate.hip over csrc/tri_solver.h)
# ---------------------------------------------------------------------------------------------
TR_FLAG_EDGE_RANGE = 1          # tri_solver.h TR_FLAG_*: bits of gf_track_link's status word


def build_tracks(ids, id_off, pair_images, kp_off, n_nodes=None):
    """The tracks of a keypoint match graph on the device (csrc/tri_solver.h, steps 1 and 2).  Device tensors: ids int32 [E,2] (per-image
    keypoint indices of every match row), id_off int32 [P+1] (the rows of pair p), pair_images int32 [P,2], kp_off int32 [n_images+1] (the
    prefix sum of the per-image keypoint counts) - what consolidate_keypoints returns.  Keypoint k of image i is node kp_off[i] + k; a
    track is a connected component with at least two nodes.  Returns (track_off int32 [T+1], obs_image int32 [N_obs], obs_kp int32
    [N_obs], obs_node int32 [N_obs]): tracks in ascending order of their smallest node, observations ascending (image-major).
    gf_track_link (lock-free union-find, one thread per row) and gf_track_flatten; the track list between them and the triangulation is
    torch's - a stable sort of the nodes by root and scans - with one device-to-host read (the sizes and the status word; one more for
    kp_off[-1] unless n_nodes, the number of keypoints, is given).  A row naming an image or a keypoint that does not exist raises after
    that read; nothing wraps."""
    _need_cuda(ids, id_off, pair_images, kp_off)
    dev = kp_off.device
    E, P, n_images = int(ids.shape[0]), int(pair_images.shape[0]), int(kp_off.numel()) - 1
    if ids.shape != (E, 2) or id_off.shape != (P + 1,) or pair_images.shape != (P, 2) or n_images < 0:
        raise ValueError('build_tracks: ids [E,2], id_off [P+1], pair_images [P,2], kp_off [n_images+1]')
    ids_, ido, pim, kpo = (_contig(x.to(torch.int32)) for x in (ids, id_off, pair_images, kp_off))
    n_nodes = int(kpo[-1]) if n_nodes is None else int(n_nodes)     # (a caller that holds the number of keypoints saves this read)
    L_ = _lib.lib()
    parent = torch.empty(max(n_nodes, 1), dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    check(L_.gf_track_link(_p(ids_), _p(ido), _p(pim), P, E, _p(kpo), n_images, n_nodes, _p(parent), _p(status), _stream()), 'gf_track_link')
    check(L_.gf_track_flatten(_p(parent), n_nodes, _stream()), 'gf_track_flatten')
    parent = parent[:n_nodes]
    empty = torch.zeros(0, dtype=torch.int32, device=dev)
    if n_nodes == 0:
        if int(status[0]) & TR_FLAG_EDGE_RANGE:
            raise _lib.GeoFormerHipError('build_tracks: a match row names an image or a keypoint that does not exist')
        return torch.zeros(1, dtype=torch.int32, device=dev), empty, empty.clone(), empty.clone()
    # nodes by root (stable: ascending inside a component; roots ascend with the component's smallest node), then segment lengths
    root, order = torch.sort(parent, stable=True)
    head = torch.ones(n_nodes, dtype=torch.int64, device=dev)
    head[1:] = (root[1:] != root[:-1]).long()
    seg = torch.cumsum(head, 0) - 1
    cnt = torch.zeros(n_nodes, dtype=torch.int64, device=dev).scatter_add_(0, seg, torch.ones_like(seg))
    keep_obs = cnt[seg] >= 2
    keep_trk = cnt >= 2
    sizes = torch.stack([keep_trk.sum(), keep_obs.sum(), status[0].long()]).cpu()          # the one device-to-host read
    T, n_obs, flags = int(sizes[0]), int(sizes[1]), int(sizes[2])
    if flags & TR_FLAG_EDGE_RANGE:
        raise _lib.GeoFormerHipError('build_tracks: a match row names an image or a keypoint that does not exist')
    obs_node = order[torch.sort((~keep_obs).to(torch.int8), stable=True).indices[:n_obs]].to(torch.int32)
    lens = cnt[torch.sort((~keep_trk).to(torch.int8), stable=True).indices[:T]]
    track_off = torch.cat([lens.new_zeros(1), torch.cumsum(lens, 0)]).to(torch.int32)
    obs_image = (torch.searchsorted(kpo.long(), obs_node.long(), right=True) - 1).clamp_(0, max(n_images - 1, 0)).to(torch.int32)
    obs_kp = obs_node - kpo[obs_image.long()]
    return track_off, obs_image, obs_kp, obs_node


def triangulate_tracks(track_off, obs_image, obs_uv, K, R, t, pixel_thr=4.0, min_angle_deg=1.5, min_obs=2, refit=0, seed=RANSAC_SEED):
    """One 3-D point per track from known camera poses, on the device (csrc/tri_solver.h, steps 3 - 9).  track_off int32 [T+1] and
    obs_image int32 [N_obs] as build_tracks returns them, obs_uv fp32 [N_obs,2] pixels, K [n_images,3,3] (fp32), R [n_images,3,3] and
    t [n_images,3] (fp64, x_cam = R X + t; NaN: an image without a pose, its observations take no part).  Hypotheses: the two-view
    midpoint of every pair of a track's observations up to length 11, 64 drawn pairs above; a pair whose rays meet at less than
    min_angle_deg has no solution (the threshold goes to the device as its cosine, computed here once); inliers by reprojection error
    below pixel_thr; most inliers win, then the smallest hypothesis.  A track is valid iff no image occurs twice in it (conflict) and its
    winner has at least min_obs (>= 2) inliers.  refit = R in 1 .. 8: up to R refits of the point on its inliers (three Gauss-Newton steps,
    inliers selected again, never fewer than before).  Returns dict(X fp64 [T,3] (zeros where not valid), valid, conflict, n_inliers,
    hypothesis, rounds int32 [T], err2 fp64 [T] (mean squared reprojection error of the inliers), inliers uint8 [N_obs]).  No host
    synchronisation; bit-identical from run to run."""
    _need_cuda(track_off, obs_image, obs_uv)
    dev = track_off.device
    T, n_obs = int(track_off.numel()) - 1, int(obs_image.numel())
    if T < 0 or obs_uv.shape != (n_obs, 2):
        raise ValueError('triangulate_tracks: track_off [T+1], obs_image [N_obs], obs_uv [N_obs,2]')
    Kt = _contig(torch.as_tensor(K, dtype=torch.float32, device=dev).reshape(-1, 9))
    Rt = _contig(torch.as_tensor(R, dtype=torch.float64, device=dev).reshape(-1, 9))
    tt = _contig(torch.as_tensor(t, dtype=torch.float64, device=dev).reshape(-1, 3))
    n_images = int(Kt.shape[0])
    if Rt.shape[0] != n_images or tt.shape[0] != n_images:
        raise ValueError(f'triangulate_tracks: {n_images} K but {Rt.shape[0]} R and {tt.shape[0]} t')
    toff, oimg, ouv = _contig(track_off.to(torch.int32)), _contig(obs_image.to(torch.int32)), _contig(obs_uv.to(torch.float32))
    rows = max(T, 1)
    X = torch.zeros(rows, 3, dtype=torch.float64, device=dev)
    err2 = torch.zeros(rows, dtype=torch.float64, device=dev)
    valid, conflict, nin, hyp, rounds = (torch.zeros(rows, dtype=torch.int32, device=dev) for _ in range(5))
    inl = torch.zeros(max(n_obs, 1), dtype=torch.uint8, device=dev)
    L_ = _lib.lib()
    ws = _ws.get('triangulate', L_.gf_triangulate_workspace_bytes(T, n_images), dev)
    cos_min = math.cos(math.radians(float(min_angle_deg)))
    check(L_.gf_triangulate(_p(toff), T, n_obs, _p(oimg), _p(ouv), _p(Kt), _p(Rt), _p(tt), n_images, float(pixel_thr), cos_min, int(min_obs),
                            int(refit), int(seed), _p(X), _p(valid), _p(conflict), _p(nin), _p(hyp), _p(rounds), _p(err2), _p(inl), _p(ws),
                            ws.numel(), _stream()), 'gf_triangulate')
    return {'X': X[:T], 'valid': valid[:T], 'conflict': conflict[:T], 'n_inliers': nin[:T], 'hypothesis': hyp[:T], 'rounds': rounds[:T],
            'err2': err2[:T], 'inliers': inl[:n_obs]}


# ---------------------------------------------------------------------------------------------
# bundle adjustment: poses and points refined jointly (csrc/k_bundle.hip over csrc/ba_spec.h)
# ---------------------------------------------------------------------------------------------
BA_MAX_FREE = 128               # ba_spec.h: the reduced camera system is dense, at most 768 x 768
BA_MAX_ITERS = 64
BA_PCG_MAX_FREE = 65536         # ba_pcg_spec.h: solver='pcg' never stores the reduced camera system
BA_PCG_MAX_ITERS = 256
BA_FLAG_STEP_FAILED, BA_FLAG_POINT_HELD, BA_FLAG_FREE_NO_POSE = 1, 2, 4     # bits of the status word


def bundle_adjust(obs_off, obs_image, obs_uv, K, R, t, X, free, thr=4.0, iters=16, host=None, solver='dense', cg_iters=64, cg_tol=1e-6):
    """Camera poses and 3-D points refined jointly on the device (csrc/ba_spec.h): Levenberg-Marquardt on the truncated squared
    reprojection error, the points eliminated by the Schur complement, the reduced camera system solved by a dense Cholesky.  Device
    tensors: obs_off int32 [T+1], obs_image int32 [N_obs], obs_uv fp32 [N_obs,2] (the observations of every point, as TriangulatedTracks
    holds them), K [n_images,3,3] fp32, R [n_images,3,3] and t [n_images,3] fp64 (x_cam = R X + t; NaN: an image without a pose, it takes
    no part and keeps its bits), X fp64 [T,3], free bool [n_images] (the cameras that move; every other one is fixed).  host: dict(obs_off,
    obs_image, free) - numpy copies of the three small tables, which the entry point checks before it enqueues; without it they are read
    back from the device here.  More than 128 free cameras is a ValueError.  The image-major index of the observations is torch's stable
    sort.  Returns dict(R, t, X, inliers uint8 [N_obs] (takes part at the final state), n_inliers int32 [T], cost fp64 [iters+1] (never
    increases), accepted int32 [iters], lam fp64 [iters+1], status int32 [1] (BA_FLAG_* bits)).  All iterations are enqueued at once, the
    decision to accept a step is taken on the device; no host synchronisation; bit-identical from run to run and to the host build.
    solver='pcg' (csrc/ba_pcg_spec.h): the reduced camera system is solved by matrix-free preconditioned conjugate gradients instead (block
    Jacobi: the per-camera 6 x 6 blocks; at most cg_iters (1 .. 256) CG iterations per LM iteration, stopped once <r, M^-1 r> has fallen to
    cg_tol^2 (0 <= cg_tol < 1) of its start; running out of iterations is no failure, the cost test judges the step).  It takes up to
    BA_PCG_MAX_FREE (65536) free cameras, its workspace is O(N_obs + T + F), and the result gains cg_used int32 [iters] and cg_res fp64
    [iters] (the CG iterations of every LM iteration and the last <r, M^-1 r> over its start)."""
    import numpy as np
    if solver not in ('dense', 'pcg'):
        raise ValueError(f"bundle_adjust: solver must be 'dense' or 'pcg', not {solver!r}")
    pcg = solver == 'pcg'
    if pcg and not 1 <= int(cg_iters) <= BA_PCG_MAX_ITERS:
        raise ValueError(f'bundle_adjust: cg_iters must be 1 .. {BA_PCG_MAX_ITERS}')
    if pcg and not 0.0 <= float(cg_tol) < 1.0:
        raise ValueError('bundle_adjust: cg_tol must be in [0, 1)')
    _need_cuda(obs_off, obs_image, obs_uv)
    dev = obs_off.device
    T, n_obs = int(obs_off.numel()) - 1, int(obs_image.numel())
    if T < 1 or n_obs < 1 or obs_uv.shape != (n_obs, 2):
        raise ValueError('bundle_adjust: obs_off [T+1], obs_image [N_obs], obs_uv [N_obs,2] with at least one point and one observation')
    Kt = _contig(torch.as_tensor(K, dtype=torch.float32, device=dev).reshape(-1, 9))
    Rt = _contig(torch.as_tensor(R, dtype=torch.float64, device=dev).reshape(-1, 9))
    tt = _contig(torch.as_tensor(t, dtype=torch.float64, device=dev).reshape(-1, 3))
    Xt = _contig(torch.as_tensor(X, dtype=torch.float64, device=dev).reshape(-1, 3))
    n_images = int(Kt.shape[0])
    if Rt.shape[0] != n_images or tt.shape[0] != n_images or Xt.shape[0] != T or n_images < 1:
        raise ValueError(f'bundle_adjust: {n_images} K but {Rt.shape[0]} R and {tt.shape[0]} t; {T} points but {Xt.shape[0]} X')
    if not 1 <= int(iters) <= BA_MAX_ITERS:
        raise ValueError(f'bundle_adjust: iters must be 1 .. {BA_MAX_ITERS}')
    if not (float(thr) > 0 and math.isfinite(float(thr))):
        raise ValueError('bundle_adjust: thr must be positive and finite')
    free_d = torch.as_tensor(free, device=dev).reshape(-1) != 0
    if host is None:
        host = {'obs_off': obs_off.cpu().numpy(), 'obs_image': obs_image.cpu().numpy(), 'free': free_d.cpu().numpy()}
    free_h = np.asarray(host['free']).reshape(-1) != 0
    if free_h.size != n_images:
        raise ValueError(f'bundle_adjust: {n_images} images but {free_h.size} free flags')
    F = int(free_h.sum())
    if pcg and F > BA_PCG_MAX_FREE:
        raise ValueError(f'bundle_adjust: {F} free cameras, the limit of solver=\'pcg\' is {BA_PCG_MAX_FREE}: fix more images')
    if not pcg and F > BA_MAX_FREE:
        raise ValueError(f'bundle_adjust: {F} free cameras, the limit is {BA_MAX_FREE} (the reduced camera system is solved densely): fix more images')
    ooh, oop = _host_i32(host['obs_off'])
    oih, oip = _host_i32(host['obs_image'])
    if ooh.size != T + 1 or oih.size != n_obs:
        raise ValueError('bundle_adjust: the host copies differ in size from the device tables')
    if n_obs and (oih.min() < 0 or oih.max() >= n_images):
        raise ValueError('bundle_adjust: an observation names an image outside [0, n_images)')
    # the image-major index: a stable sort of the observations by image, here on the host copy and there on the device - the same order
    ioh, iop = _host_i32(np.argsort(oih, kind='stable'))
    ifh, ifp = _host_i32(np.concatenate([[0], np.cumsum(np.bincount(oih, minlength=n_images))]))
    cfh, cfp = _host_i32(np.where(free_h, np.cumsum(free_h) - 1, -1))
    toff, oimg, ouv = _i32(obs_off, dev), _i32(obs_image, dev), _contig(obs_uv.to(torch.float32))
    img_obs = torch.sort(oimg, stable=True).indices.to(torch.int32)
    img_off = torch.cat([toff.new_zeros(1), torch.cumsum(torch.bincount(oimg.long(), minlength=n_images), 0).to(torch.int32)])
    cam_free = torch.where(free_d, torch.cumsum(free_d.to(torch.int32), 0, dtype=torch.int32) - 1, torch.full_like(img_off[:n_images], -1))
    cam_free = _contig(cam_free.to(torch.int32))
    Ro, to, Xo = torch.empty_like(Rt), torch.empty_like(tt), torch.empty_like(Xt)
    inl = torch.zeros(n_obs, dtype=torch.uint8, device=dev)
    nin = torch.zeros(T, dtype=torch.int32, device=dev)
    cost = torch.zeros(int(iters) + 1, dtype=torch.float64, device=dev)
    lam = torch.zeros(int(iters) + 1, dtype=torch.float64, device=dev)
    acc = torch.zeros(int(iters), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    L_ = _lib.lib()
    if pcg:
        cg_used = torch.zeros(int(iters), dtype=torch.int32, device=dev)
        cg_res = torch.zeros(int(iters), dtype=torch.float64, device=dev)
        ws = _ws.get('bundle_adjust_pcg', L_.gf_bundle_pcg_workspace_bytes(T, n_obs, n_images, F), dev)
        check(L_.gf_bundle_adjust_pcg(oop, oip, ifp, iop, cfp, _p(toff), T, n_obs, _p(oimg), _p(ouv), _p(img_off), _p(img_obs), _p(cam_free), n_images,
                                      F, _p(Kt), _p(Rt), _p(tt), _p(Xt), float(thr), int(iters), int(cg_iters), float(cg_tol), _p(Ro), _p(to), _p(Xo),
                                      _p(inl), _p(nin), _p(cost), _p(acc), _p(lam), _p(status), _p(cg_used), _p(cg_res), _p(ws), ws.numel(),
                                      _stream()), 'gf_bundle_adjust_pcg')
        return {'R': Ro.view(n_images, 3, 3), 't': to, 'X': Xo, 'inliers': inl, 'n_inliers': nin, 'cost': cost, 'accepted': acc, 'lam': lam,
                'status': status, 'cg_used': cg_used, 'cg_res': cg_res}
    ws = _ws.get('bundle_adjust', L_.gf_bundle_workspace_bytes(T, n_obs, n_images, F), dev)
    check(L_.gf_bundle_adjust(oop, oip, ifp, iop, cfp, _p(toff), T, n_obs, _p(oimg), _p(ouv), _p(img_off), _p(img_obs), _p(cam_free), n_images, F,
                              _p(Kt), _p(Rt), _p(tt), _p(Xt), float(thr), int(iters), _p(Ro), _p(to), _p(Xo), _p(inl), _p(nin), _p(cost), _p(acc),
                              _p(lam), _p(status), _p(ws), ws.numel(), _stream()), 'gf_bundle_adjust')
    return {'R': Ro.view(n_images, 3, 3), 't': to, 'X': Xo, 'inliers': inl, 'n_inliers': nin, 'cost': cost, 'accepted': acc, 'lam': lam,
            'status': status}


# ---------------------------------------------------------------------------------------------
# sparse localisation: covisibility clusters, unique 2-D - 3-D rows, the winning cluster (csrc/k_covis.hip over csrc/covis_spec.h)
# ---------------------------------------------------------------------------------------------
CV_MAX_LIST = 1024              # covis_spec.h: the longest database list of one query
CV_PAIR_WORDS = 8
_CV_FLAGS = ((1, 'an image that does not exist'), (2, 'a keypoint its image does not have, or a row outside ids'),
             (4, 'a point that does not exist'), (8, 'a list position outside its list'))


def _cv_raise(what, flags):
    if flags:
        raise _lib.GeoFormerHipError(f'{what}: the tables name ' + '; '.join(t for b, t in _CV_FLAGS if flags & b))


def _host_i32(a):
    """a small int32 table as a contiguous numpy array and its address (the *_host arguments: read before anything is enqueued)"""
    import numpy as np
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, ctypes.c_void_p(a.ctypes.data)


def _i32(t, dev):
    return _contig(t.to(device=dev, dtype=torch.int32))


def covis_clusters(kp_off, point_of_keypoint, obs_offsets, obs_image, list_off, list_img, sorted_img, sorted_pos, host, enable=True, status=None):
    """Covisibility clusters of every query's database list on the device (csrc/covis_spec.h, steps 2 and 3).  Device tensors: kp_off int32
    [n_images+1], point_of_keypoint int32 [n_nodes] (flat; -1: none), obs_offsets int32 [T+1] and obs_image int32 [N_obs] of the points,
    list_off int32 [Q+1] and list_img int32 [L] (every query's database images in order of first appearance), sorted_img / sorted_pos int32
    [L] (each list sorted by image id, with the positions).  host: dict(list_off, list_img) - numpy copies of the two small tables, which
    the entry point checks before it enqueues (a list above 1024 entries, an image that does not exist: GeoFormerHipError).  Two positions
    are linked iff a point has an observation in both images; a cluster is a connected component on the list alone.  Returns (cluster int32
    [L]: the cluster number of every position, numbered in ascending order of a cluster's smallest position; n_clusters int32 [Q]; status
    int32 [1]: bits set on the device for tables that name what does not exist - the caller reads it with its sizes).  enable=False: every
    position has cluster 0.  One launch, one workgroup per query, no host synchronisation; the same bytes in every run."""
    _need_cuda(kp_off, point_of_keypoint, obs_offsets, obs_image, list_off, list_img, sorted_img, sorted_pos)
    dev = kp_off.device
    Q, Lt = int(list_off.numel()) - 1, int(list_img.numel())
    n_images, n_nodes, T, n_obs = int(kp_off.numel()) - 1, int(point_of_keypoint.numel()), int(obs_offsets.numel()) - 1, int(obs_image.numel())
    if Q < 0 or n_images < 0 or T < 0 or sorted_img.numel() != Lt or sorted_pos.numel() != Lt:
        raise ValueError('covis_clusters: kp_off [n_images+1], obs_offsets [T+1], list_off [Q+1], list_img / sorted_img / sorted_pos [L]')
    loh, lop = _host_i32(host['list_off'])
    lih, lip = _host_i32(host['list_img'])
    if loh.size != Q + 1 or lih.size != Lt:
        raise ValueError('covis_clusters: the host copies differ in size from the device tables')
    cluster = torch.zeros(max(Lt, 1), dtype=torch.int32, device=dev)
    ncl = torch.zeros(max(Q, 1), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev) if status is None else status
    check(_lib.lib().gf_covis_cluster(_p(_i32(kp_off, dev)), n_images, _p(_i32(point_of_keypoint, dev)), n_nodes, _p(_i32(obs_offsets, dev)), T,
                                      _p(_i32(obs_image, dev)), n_obs, lop, lip, _p(_i32(list_off, dev)), _p(_i32(list_img, dev)),
                                      _p(_i32(sorted_img, dev)), _p(_i32(sorted_pos, dev)), Q, Lt, int(bool(enable)), _p(cluster), _p(ncl),
                                      _p(status), _stream()), 'gf_covis_cluster')
    return cluster[:Lt], ncl[:Q], status


def sparse_rows(pairs, pair_row_off, ids, kp_off, point_of_keypoint, n_points, list_off, cluster, n_clusters, host, dedup=False, status=None,
                keypoints=None, points=None):
    """The 2-D - 3-D rows of sparse localisation on the device, in problem order (csrc/covis_spec.h, steps 4 - 6).  Device tensors: pairs
    int32 [C,8] (the contributing pairs in pair order: query index, query image, database image, first and end row in ids, the query's
    column of ids, the database image's position in its query's list, 0), pair_row_off int32 [C+1] (the prefix sum of their row counts),
    ids int32 [E,2], kp_off, point_of_keypoint (flat), list_off int32 [Q+1], and cluster / n_clusters as covis_clusters returns them.
    n_points: T.  host: dict(pairs) - the numpy copy the entry point checks before it enqueues.  gf_sparse_rows writes per original row the
    query keypoint's node, the point, the problem (query-major, then cluster number) and keep (the database keypoint has a point); the
    stable order by problem and, with dedup, the first occurrence of every (query keypoint, point) inside a problem are torch's stable
    sorts and scans.  One device-to-host read (N problems, M rows, the status words; tables that name what does not exist raise after it).
    Returns dict(row_kp, row_pt, row_prob int32 [M0], keep uint8 [M0], first_of int32 [M0] (the original row that stands for a row: itself
    without dedup; -1 for a row without a point), slot int32 [M0] (the RANSAC row of first_of; -1), sel int64 [M] (the original rows of
    the RANSAC rows), prob_off int32 [N+1], prob_base int32 [Q+1], N, M, and - with keypoints fp32 [n_nodes,2] and points fp32 [T,3] -
    p2d fp32 [M,2] and p3d fp32 [M,3])."""
    _need_cuda(pairs, pair_row_off, ids, kp_off, point_of_keypoint, list_off, cluster, n_clusters)
    dev = kp_off.device
    C, E, Q = int(pairs.shape[0]), int(ids.shape[0]), int(list_off.numel()) - 1
    n_images, n_nodes, Lt = int(kp_off.numel()) - 1, int(point_of_keypoint.numel()), int(cluster.numel())
    if pairs.shape != (C, CV_PAIR_WORDS) or pair_row_off.numel() != C + 1 or ids.shape != (E, 2) or n_clusters.numel() != Q:
        raise ValueError('sparse_rows: pairs [C,8], pair_row_off [C+1], ids [E,2], n_clusters [Q]')
    ph, php = _host_i32(host['pairs'])
    if ph.size != C * CV_PAIR_WORDS:
        raise ValueError('sparse_rows: the host copy of pairs differs in size from the device table')
    M0 = int((ph.reshape(-1, CV_PAIR_WORDS)[:, 4].astype('int64') - ph.reshape(-1, CV_PAIR_WORDS)[:, 3]).sum()) if C else 0
    if M0 >= 2 ** 31:
        raise _lib.GeoFormerHipError('sparse_rows: 2^31 rows or more')
    prob_base = torch.zeros(Q + 1, dtype=torch.int32, device=dev)
    prob_base[1:] = torch.cumsum(n_clusters.to(torch.int64), 0).to(torch.int32)
    rows = max(M0, 1)
    row_kp, row_pt, row_prob = (torch.full((rows,), -1, dtype=torch.int32, device=dev) for _ in range(3))
    keep = torch.zeros(rows, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev) if status is None else status
    check(_lib.lib().gf_sparse_rows(php, _p(_i32(pairs, dev)), _p(_i32(pair_row_off, dev)), C, M0, _p(_i32(ids, dev)), E, _p(_i32(kp_off, dev)),
                                    n_images, _p(_i32(point_of_keypoint, dev)), n_nodes, int(n_points), _p(_i32(list_off, dev)),
                                    _p(_i32(cluster, dev)), Lt, _p(prob_base), Q, _p(row_kp), _p(row_pt), _p(row_prob), _p(keep), _p(status),
                                    _stream()), 'gf_sparse_rows')
    row_kp, row_pt, row_prob, keep = row_kp[:M0], row_pt[:M0], row_prob[:M0], keep[:M0]
    kept = keep.bool()
    # kept rows first, in (problem, original row) order: a stable sort by problem with the dropped rows behind every problem
    big = torch.iinfo(torch.int32).max
    order = torch.sort(torch.where(kept, row_prob, torch.full_like(row_prob, big)), stable=True).indices       # [M0] original rows
    ar = torch.arange(M0, dtype=torch.int64, device=dev)
    first_of = torch.where(kept, ar, torch.full_like(ar, -1))
    if dedup and M0:
        # runs of equal (problem, keypoint, point): three stable sorts, least significant key first; a run's head is its earliest row
        perm = ar
        for key in (row_pt, row_kp, torch.where(kept, row_prob, torch.full_like(row_prob, big))):
            perm = perm[torch.sort(key[perm], stable=True).indices]
        a, b, c = row_prob[perm], row_kp[perm], row_pt[perm]
        head = torch.ones(M0, dtype=torch.bool, device=dev)
        head[1:] = (a[1:] != a[:-1]) | (b[1:] != b[:-1]) | (c[1:] != c[:-1])
        head_at = torch.cummax(torch.where(head, ar, torch.zeros_like(ar)), 0).values
        first = torch.empty_like(ar)
        first[perm] = perm[head_at]
        first_of = torch.where(kept, first, first_of)
    rep = kept & (first_of == ar)                                      # the rows RANSAC sees
    rep_sorted = rep[order]
    pos = torch.cumsum(rep_sorted.to(torch.int64), 0) - 1
    slot_of_row = torch.full((M0,), -1, dtype=torch.int64, device=dev)
    slot_of_row[order] = torch.where(rep_sorted, pos, torch.full_like(pos, -1))
    slot = torch.where(kept, slot_of_row[first_of.clamp(min=0)], torch.full_like(ar, -1)) if M0 else slot_of_row
    n_prob = prob_base[-1:].to(torch.int64)
    sizes = torch.cat([n_prob, rep.sum().reshape(1), status.to(torch.int64)]).cpu()          # the one device-to-host read
    N, M = int(sizes[0]), int(sizes[1])
    _cv_raise('sparse_rows', int(sizes[2]))
    sel = order[torch.sort((~rep_sorted).to(torch.int8), stable=True).indices[:M]]        # (M is known: no second read for a mask's size)
    per_prob = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    if M:
        per_prob.scatter_add_(0, row_prob[sel].to(torch.int64) + 1, torch.ones(M, dtype=torch.int64, device=dev))
    out = {'row_kp': row_kp, 'row_pt': row_pt, 'row_prob': row_prob, 'keep': keep, 'first_of': first_of.to(torch.int32), 'slot': slot.to(torch.int32),
           'sel': sel, 'prob_off': torch.cumsum(per_prob, 0).to(torch.int32), 'prob_base': prob_base, 'N': N, 'M': M}
    if keypoints is not None and points is not None:
        out['p2d'] = keypoints[row_kp[sel].long()] if M else keypoints.new_zeros(0, 2)
        out['p3d'] = points[row_pt[sel].long()] if M else points.new_zeros(0, 3)
    return out


def select_cluster(prob_base, rs, row_prob, slot, min_inliers=12):
    """The winning cluster of every query and the masks on the original rows, on the device (csrc/covis_spec.h, steps 8 and 9).  prob_base
    int32 [Q+1], rs: what ransac_absolute_pose returned for the N = prob_base[-1] problems, row_prob / slot int32 [M0] as sparse_rows
    returns them.  The winner of a query is its valid problem with the most inliers, then the lowest cluster number.  Returns dict(winner
    int32 [Q] (cluster number; -1), localized int32 [Q] (a winner with at least min_inliers inliers), R fp64 [Q,3,3], t fp64 [Q,3],
    n_inliers, rounds int32 [Q] (the winner's; zeros without one), cluster_inliers int32 [N] (the inliers of every problem; 0 where
    RANSAC found no model), mask uint8 [M0] (a row of a winning problem: the inlier byte of its slot; 0 otherwise)).  No host
    synchronisation."""
    _need_cuda(prob_base, row_prob, slot, rs['valid'])
    dev = prob_base.device
    Q, M0 = int(prob_base.numel()) - 1, int(row_prob.numel())
    N, M = int(rs['valid'].numel()), int(rs['inliers'].numel())
    qrows = max(Q, 1)
    winner, localized, nin, rounds = (torch.zeros(qrows, dtype=torch.int32, device=dev) for _ in range(4))
    Rq = torch.zeros(qrows, 3, 3, dtype=torch.float64, device=dev)
    tq = torch.zeros(qrows, 3, dtype=torch.float64, device=dev)
    is_win = torch.zeros(max(N, 1), dtype=torch.uint8, device=dev)
    mask = torch.zeros(max(M0, 1), dtype=torch.uint8, device=dev)
    check(_lib.lib().gf_covis_select(_p(_i32(prob_base, dev)), Q, N, _p(_i32(rs['valid'], dev)), _p(_i32(rs['n_inliers'], dev)), _p(_contig(rs['R'])),
                                     _p(_contig(rs['t'])), _p(_i32(rs['rounds'], dev)), _p(_contig(rs['inliers'])), M, _p(_i32(row_prob, dev)),
                                     _p(_i32(slot, dev)), M0, int(min_inliers), _p(winner), _p(localized), _p(Rq), _p(tq), _p(nin), _p(rounds),
                                     _p(is_win), _p(mask), _stream()), 'gf_covis_select')
    return {'winner': winner[:Q], 'localized': localized[:Q], 'R': Rq[:Q], 't': tq[:Q], 'n_inliers': nin[:Q], 'rounds': rounds[:Q],
            'cluster_inliers': torch.where(rs['valid'] == 1, rs['n_inliers'], torch.zeros_like(rs['n_inliers'])), 'mask': mask[:M0]}
