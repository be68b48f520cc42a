"""Caller-side counterpart of the reference's inference / evaluation wrappers:

  * `resize_im`, `load_gray_scale_tensor`   eval_tool/immatch/utils/data_io.py:16-26, :48-62
  * `GeoFormerMatcher`                      inference.py:12-99 and eval_tool/immatch/modules/geoformer.py:12-99
                                            (same constructor arguments, `match_pairs` return convention)
  * `cal_error_auc`, `cal_reproj_dists`, `eval_hpatches`
                                            eval_tool/immatch/utils/hpatches_helper.py:13-34, :94-317

OpenCV and torchvision are not available offline: images are read with PIL, converted to gray and resized as UINT8
images by a restatement of OpenCV's published 8-bit paths (`cv2_gray_u8`: the 14-bit fixed-point BGR->gray of
cv2.imread(..., IMREAD_GRAYSCALE); `cv2_resize_linear_u8`: cv2.resize's default INTER_LINEAR for 8-bit images, 11-bit
fixed-point coefficients, half-pixel centres, round-half-up) - byte work, bit for bit; OpenCV itself is absent from the
build container, so the restatement is pinned by hand-derived vectors (tests/test_matcher_cpu.py), not by OpenCV's own
output.  The homography of the HPatches metric is estimated from the fine matches by the device RANSAC
(`ops.ransac_homography(..., thr=ransac_thres, integer_keypoints=False, min_points=4)`).
"""
import collections
import glob
import math
import os
import threading
import time
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import ops
from .model.cvpr_ds_config import get_default_cfg
from .model.full_model import PRECISIONS, GeoFormer, ImageFeatures
from .model.geo_config import get_cfg_model


def resize_im(wo, ho, imsize=None, dfactor=1, value_to_scale=max, aspan=False):
    """Target size: scale so that value_to_scale(w, h) == imsize when it exceeds it (or always with
    aspan), then floor both sides to multiples of dfactor.  Returns (wt, ht, (wo/wt, ho/ht))."""
    wt, ht = wo, ho
    if imsize and imsize > 0 and (aspan or value_to_scale(wo, ho) > imsize):
        s = imsize / value_to_scale(wo, ho)
        ht, wt = int(round(ho * s)), int(round(wo * s))
    wt, ht = int(wt // dfactor * dfactor), int(ht // dfactor * dfactor)
    return wt, ht, (wo / wt, ho / ht)


def cv2_gray_u8(rgb):
    """[H,W,3] uint8 RGB -> [H,W] uint8 as cv2.imread(path, cv2.IMREAD_GRAYSCALE) converts a colour file (data_io.py:50):
    (R*4899 + G*9617 + B*1868 + 2^13) >> 14 (OpenCV imgcodecs' icvCvt_BGR2Gray_8u_C3C1R, 14-bit coefficients)."""
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    return ((r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14).astype(np.uint8)


def _cv_round(x):
    """cvRound: round half to even (lrint) - what saturate_cast<short>(float) does."""
    return np.rint(x)


def _linear_coeffs(ssize, dsize, clamp_index):
    """Source index and the two 11-bit weights of every destination position (imgproc/resize.cpp, resize generic path:
    fx = (float)((dx + 0.5) * scale - 0.5); sx = floor(fx); fx -= sx; weights saturate_cast<short>({1 - fx, fx} * 2048)).
    Horizontally an out-of-range sx is clamped together with fx = 0; vertically the ROW indices are clamped instead."""
    scale = float(ssize) / float(dsize)
    d = np.arange(dsize, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if clamp_index:
        lo, hi = s < 0, s >= ssize - 1
        f = np.where(lo | hi, np.float32(0), f)
        s = np.where(lo, 0, np.where(hi, ssize - 1, s))
    w1 = np.clip(_cv_round(f * np.float32(2048)), -32768, 32767).astype(np.int64)
    w0 = np.clip(_cv_round((np.float32(1) - f) * np.float32(2048)), -32768, 32767).astype(np.int64)
    return s, w0, w1


def cv2_resize_linear_u8(src, wt, ht):
    """cv2.resize(src, (wt, ht)) for a single-channel uint8 image with the default INTER_LINEAR (data_io.py:53), OpenCV's
    fixed-point path: horizontal pass into 19-bit integers (pixel x 11-bit weight), vertical pass
    dst = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2  (VResizeLinear<uchar, int, short>).  An exact 2x
    decimation in both directions is INTER_AREA instead (resize.cpp: 'INTER_LINEAR && is_area_fast && iscale == 2'):
    (a + b + c + d + 2) >> 2."""
    src = np.ascontiguousarray(src, dtype=np.uint8)
    hs, ws = src.shape
    if (ws, hs) == (wt, ht):
        return src.copy()
    if ws == 2 * wt and hs == 2 * ht:
        t = src.astype(np.int64)
        return ((t[0::2, 0::2] + t[0::2, 1::2] + t[1::2, 0::2] + t[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    sx, a0, a1 = _linear_coeffs(ws, wt, clamp_index=True)
    sy, b0, b1 = _linear_coeffs(hs, ht, clamp_index=False)
    t = src.astype(np.int64)
    rows = t[:, sx] * a0[None, :] + t[:, np.minimum(sx + 1, ws - 1)] * a1[None, :]            # [hs, wt]
    r0, r1 = rows[np.clip(sy, 0, hs - 1)], rows[np.clip(sy + 1, 0, hs - 1)]                  # [ht, wt]
    out = (((b0[:, None] * (r0 >> 4)) >> 16) + ((b1[:, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def load_image_u8(im_path):
    """The decoder half of `load_gray_image`: uint8 [H,W,3] RGB that still needs the fixed-point gray conversion
    (`cv2_gray_u8` on the host, or the device kernel behind `ops.image_gray_resize`), or uint8 [H,W] that is final already
    (the JPEG luma plane, mode 'L' files).
    PNG / PPM / BMP colour files (HPatches is PPM): OpenCV decodes BGR and applies its fixed-point BGR2GRAY - `cv2_gray_u8`,
    byte for byte.  JPEG (the FIRE / ISC evaluation images): OpenCV hands IMREAD_GRAYSCALE to libjpeg as
    out_color_space = JCS_GRAYSCALE, i.e. the decoder emits the Y plane of the file's YCbCr data itself and no RGB image ever
    exists; PIL's `draft('L', ...)` configures libjpeg the same way, so that path is used for JPEG files (bit-equal to the Y
    channel of a YCbCr decode: tests/test_matcher_cpu.py).  Limits: a CMYK / RGB-encoded (Adobe) JPEG falls back to the
    formula on the decoded RGB, and libjpeg-turbo vs libjpeg IDCT differences between the two installations are not ours to pin."""
    from PIL import Image
    im = Image.open(im_path)
    if im.format in ('JPEG', 'MPO') and im.mode in ('RGB', 'L'):
        im.draft('L', im.size)                                       # libjpeg JCS_GRAYSCALE, what OpenCV asks for
        if im.mode == 'L':
            return np.array(im, dtype=np.uint8)
    if im.mode in ('RGB', 'RGBA', 'P', 'CMYK', 'YCbCr'):
        return np.array(im.convert('RGB'), dtype=np.uint8)
    return np.array(im.convert('L'), dtype=np.uint8)


def load_gray_image(im_path):
    """[H,W] uint8 like cv2.imread(im_path, cv2.IMREAD_GRAYSCALE) (data_io.py:50): `load_image_u8` + `cv2_gray_u8` where the
    decoder returned colour."""
    im = load_image_u8(im_path)
    return cv2_gray_u8(im) if im.ndim == 3 else im


class _Staging:
    """Pinned host buffers for the uploads of preprocess='device', one per (device, slot), grown on demand and reused: no
    per-image pin_memory() allocation.  A pair uploads two images before anything synchronises, so each image of a pair has its
    own slot; an event recorded behind every copy is waited for before the slot's bytes are overwritten (it has long
    completed in a matching loop, whose result download synchronises the stream)."""

    def __init__(self):
        self.slots = {}

    def upload(self, im, device, slot=0):
        """numpy uint8 image -> device tensor of the same shape, copied asynchronously on the current stream."""
        device = torch.device(device)
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        key = (device.index, slot)
        buf, ev = self.slots.get(key, (None, None))
        if ev is not None:
            ev.synchronize()
        if buf is None or buf.numel() < im.size:
            buf = torch.empty(max(im.size, 1 << 20), dtype=torch.uint8).pin_memory()
            ev = torch.cuda.Event()
            self.slots[key] = (buf, ev)
        host = buf[:im.size].view(im.shape)
        host.numpy()[...] = im
        with torch.cuda.device(device):
            dev = host.to(device, non_blocking=True)
            ev.record()
        return dev


_staging = _Staging()
PREPROCESS = ('host', 'device')


def load_gray_scale_tensor(im_path, device, imsize=None, dfactor=8, value_to_scale=min, aspan=False, preprocess='host', slot=0):
    """[1,1,H,W] float in [0,1] + (wo/wt, ho/ht); H, W multiples of dfactor (load_gray_scale_tensor_cv, data_io.py:48-62:
    gray uint8 image -> cv2.resize on the uint8 image -> to_tensor).
    preprocess='host': gray conversion and resize in numpy, the fp32 image is uploaded.  preprocess='device': the decoded
    uint8 bytes go to the device through the pinned staging buffer `slot` and one kernel (ops.image_gray_resize) does gray,
    resize and the division - the same bits; callers that upload several images before they synchronise give each its own slot."""
    if preprocess not in PREPROCESS:
        raise ValueError(f'preprocess must be one of {PREPROCESS}, got {preprocess!r}')
    if preprocess == 'device':
        if torch.device(device).type != 'cuda':
            raise ValueError(f"preprocess='device' runs on the GPU: it needs a cuda device, got device={device!r} (use preprocess='host')")
        im = load_image_u8(im_path)
        ho, wo = im.shape[:2]
        wt, ht, scale = resize_im(wo, ho, imsize=imsize, dfactor=dfactor, value_to_scale=value_to_scale, aspan=aspan)
        with torch.cuda.device(device):
            return ops.image_gray_resize(_staging.upload(im, device, slot), wt, ht, reciprocal=True), scale       # the host path's `/ 255.0` on a GPU
    im = load_gray_image(im_path)
    ho, wo = im.shape
    wt, ht, scale = resize_im(wo, ho, imsize=imsize, dfactor=dfactor, value_to_scale=value_to_scale, aspan=aspan)
    im = cv2_resize_linear_u8(im, wt, ht)
    t = torch.from_numpy(im).to(device=device, dtype=torch.float32)[None, None]
    return t / 255.0, scale


# ---------------------------------------------------------------------------------------------
# features once, matches many times: the per-image half of a match, kept by key
# ---------------------------------------------------------------------------------------------
class StoredImage(NamedTuple):
    """One extracted image: the backbone's maps (GeoFormer.extract_features) and the resize ratios load_im returned with it."""
    features: ImageFeatures
    scale: Tuple[float, float]       # (wo / wt, ho / ht)

    @property
    def nbytes(self):
        return self.features.nbytes


class FeatureStore:
    """key -> record with least-recently-used eviction under an optional byte budget (max_bytes=None: unbounded).  The matcher's
    keys are (path, preprocessing signature).  `extractions` counts the records made (misses), `hits` the lookups served from
    the store.  A lock guards lookup, insert and evict: the HPatches loop may feed the GPU from two host pipelines; the extraction
    itself runs outside the lock (two threads missing the same key both extract, the first insert wins, both count)."""

    def __init__(self, max_bytes: Optional[int] = None):
        if max_bytes is not None and max_bytes < 0:
            raise ValueError('max_bytes must be None (unbounded) or >= 0')
        self.max_bytes = max_bytes
        self.extractions = self.hits = self.evictions = 0
        self.nbytes = 0
        self._items = collections.OrderedDict()     # key -> (record, nbytes), least recently used first
        self._lock = threading.Lock()

    def __len__(self):
        return len(self._items)

    def __contains__(self, key):
        return key in self._items

    def keys(self):
        """Least recently used first."""
        return list(self._items)

    def get(self, key):
        with self._lock:
            item = self._items.get(key)
            if item is None:
                return None
            self._items.move_to_end(key)
            self.hits += 1
            return item[0]

    def put(self, key, record, nbytes=None):
        """Inserts `record` as the most recently used entry (an entry already under `key` is kept and returned instead), then evicts
        from the least recently used end until the budget holds again.  The new entry itself stays, whatever its size."""
        nbytes = int(record.nbytes if nbytes is None else nbytes)
        with self._lock:
            self.extractions += 1
            if key in self._items:
                self._items.move_to_end(key)
                return self._items[key][0]
            self._items[key] = (record, nbytes)
            self.nbytes += nbytes
            while self.max_bytes is not None and self.nbytes > self.max_bytes and len(self._items) > 1:
                # An evicted record may still be read by launches that are enqueued but have not run.  That is safe: extraction and
                # matching are enqueued on the current stream, and the caching allocator hands a freed block to later work on the
                # same stream only - work that runs after those launches.  (Callers also hold the records of the batch in flight.)
                _, (_, freed) = self._items.popitem(last=False)
                self.nbytes -= freed
                self.evictions += 1
            return record

    def get_or_extract(self, key, extract):
        rec = self.get(key)
        return rec if rec is not None else self.put(key, extract())

    def clear(self):
        with self._lock:
            self._items.clear()
            self.nbytes = 0


def group_pairs(shapes, batch):
    """shapes[k] = any hashable description of pair k's (shape0, shape1).  -> list of index lists, each of one shape group and at most
    `batch` long: groups in order of first appearance, a group's pairs in input order, its last batch possibly short."""
    if batch < 1:
        raise ValueError('batch must be >= 1')
    groups = collections.OrderedDict()
    for k, sh in enumerate(shapes):
        groups.setdefault(sh, []).append(k)
    return [idx[s:s + batch] for idx in groups.values() for s in range(0, len(idx), batch)]


# match_many(pad=True): see group_pairs_padded.  The best of {1.1, 1.25, 1.5, 2} in profiles/padded_batch.txt (tools/padded_batch_probe.py: 120 pairs
# over 8 sizes, 1420.7 pairs/s against 1412.0 .. 1414.3 for the others and 1270.0 unpadded) - a lead inside that run's spread, and the candidate that
# changes a pair's matches least
DEFAULT_PAD_WASTE = 1.1


def group_pairs_padded(shapes, batch, max_waste):
    """shapes[k] = ((h0, w0), (h1, w1)): pair k's two map (or image) shapes.  -> list of index lists for padded batches: every index
    once, at most `batch` per list, a list's indices in input order.  Pairs are ordered by the area of their two shapes (ties: input
    order) and batches filled greedily in that order; a batch is closed when it is full, or when adding the next pair would push, on
    either side, count x canvas area (the canvas: the per-axis maximum over the batch) above max_waste x the sum of the pairs' own
    areas - the matching path's work grows with the canvas, so max_waste bounds the work spent on padding.  max_waste = 1 batches
    equal shapes only; one shape throughout gives group_pairs' batches."""
    if batch < 1:
        raise ValueError('batch must be >= 1')
    if not max_waste >= 1:
        raise ValueError('max_waste must be >= 1 (canvas area over own area)')
    shapes = [tuple((int(h), int(w)) for h, w in sh) for sh in shapes]
    order = sorted(range(len(shapes)), key=lambda k: (sum(h * w for h, w in shapes[k]), k))
    out, cur = [], []
    canvas, own = [(0, 0), (0, 0)], [0, 0]
    for k in order:
        new_canvas = [(max(c[0], s[0]), max(c[1], s[1])) for c, s in zip(canvas, shapes[k])]
        new_own = [o + s[0] * s[1] for o, s in zip(own, shapes[k])]
        fits = len(cur) < batch and all((len(cur) + 1) * c[0] * c[1] <= max_waste * o for c, o in zip(new_canvas, new_own))
        if cur and not fits:
            out.append(sorted(cur))
            cur = []
            new_canvas, new_own = list(shapes[k]), [s[0] * s[1] for s in shapes[k]]
        cur.append(k)
        canvas, own = new_canvas, new_own
    if cur:
        out.append(sorted(cur))
    return out


def read_pair_list(list_path):
    """Two image paths per line (whitespace separated; blank lines and lines starting with '#' are skipped); a relative path is
    relative to the directory of the list file."""
    base = os.path.dirname(os.path.abspath(list_path))
    pairs = []
    with open(list_path) as f:
        for no, line in enumerate(f, 1):
            parts = line.split()
            if not parts or parts[0].startswith('#'):
                continue
            if len(parts) != 2:
                raise ValueError(f'{list_path}:{no}: expected two image paths, got {len(parts)} fields')
            pairs.append(tuple(p if os.path.isabs(p) else os.path.normpath(os.path.join(base, p)) for p in parts))
    return pairs


IMAGE_EXTENSIONS = ('.png', '.jpg', '.jpeg', '.ppm', '.pgm', '.bmp', '.tif', '.tiff')


def all_pairs(image_dir):
    """Every pair (i < j) of the image files directly under `image_dir`, sorted by name."""
    names = sorted(n for n in os.listdir(image_dir) if n.lower().endswith(IMAGE_EXTENSIONS))
    paths = [os.path.join(image_dir, n) for n in names]
    return [(paths[i], paths[j]) for i in range(len(paths)) for j in range(i + 1, len(paths))]


class GeoFormerMatcher:
    def __init__(self, imsize, match_threshold, no_match_upscale=False, ckpt=None, device='cuda', precision='fp32',
                 miopen_search=False, preprocess='host', cache_bytes=None):
        """precision / miopen_search / preprocess are additions: 'fp16' is the fast mode ('bf16', 'bf16_fp16': GeoFormer.set_precision);
        miopen_search=True lets MIOpen search its convolution algorithms once per new image shape (seconds each, ~25 % faster
        backbone afterwards: 6.8 -> 5.2 ms per 480x640 pair) - worth it when a dataset repeats a few shapes; preprocess='device'
        moves gray conversion, resize and normalisation of the decoded images from numpy to one kernel per image
        (load_gray_scale_tensor), same bits.  cache_bytes: byte budget of the feature store behind extract / match_many (None: unbounded)."""
        self.store = FeatureStore(cache_bytes)
        if preprocess not in PREPROCESS:
            raise ValueError(f'preprocess must be one of {PREPROCESS}, got {preprocess!r}')
        if preprocess == 'device' and torch.device(device).type != 'cuda':
            raise ValueError(f"preprocess='device' runs on the GPU: it needs a cuda device, got device={device!r} (use preprocess='host')")
        self.preprocess = preprocess
        from . import miopen
        miopen.use_shipped_find_db()              # no-op if the caller configured MIOpen already
        if miopen_search:
            torch.backends.cudnn.benchmark = True
        self.device, self.imsize = device, imsize
        self.match_threshold, self.no_match_upscale = match_threshold, no_match_upscale
        conf = get_default_cfg()
        conf['match_coarse']['thr'] = match_threshold
        gcfg = get_cfg_model()
        gcfg['coarse_thr'] = match_threshold
        gcfg['precision'] = precision
        self.model = GeoFormer(conf, gcfg)
        self.ckpt_name = 'random'
        if ckpt is not None:
            sd = torch.load(ckpt, map_location='cpu')
            sd = sd.get('state_dict', sd)
            self.model.load_state_dict(sd, strict=False)
            self.ckpt_name = os.path.splitext(os.path.basename(ckpt))[0]
        self.model = self.model.eval().to(device)
        self.name = f'GeoFormer_{self.ckpt_name}' + ('_noms' if no_match_upscale else '')

    def load_im(self, im_path, slot=0):
        return load_gray_scale_tensor(im_path, self.device, imsize=self.imsize, dfactor=8, value_to_scale=min,
                                      preprocess=self.preprocess, slot=slot)

    def match_inputs_(self, gray1, gray2):
        with torch.no_grad():
            batch = self.model({'image0': gray1, 'image1': gray2})
        kpts1, kpts2 = batch['mkpts0_f'].cpu().numpy(), batch['mkpts1_f'].cpu().numpy()
        scores = batch['mconf'].cpu().numpy()
        return np.concatenate([kpts1, kpts2], axis=1), kpts1, kpts2, scores

    def match_pairs(self, im1_path, im2_path):
        gray1, sc1 = self.load_im(im1_path, slot=0)
        gray2, sc2 = self.load_im(im2_path, slot=1)        # its own staging buffer: the first upload may still be in flight
        upscale = np.array([sc1 + sc2])
        matches, kpts1, kpts2, scores = self.match_inputs_(gray1, gray2)
        if self.no_match_upscale:
            return matches, kpts1, kpts2, scores, upscale.squeeze(0)
        return upscale * matches, sc1 * kpts1, sc2 * kpts2, scores

    __call__ = match_pairs

    # -- features once, matches many times (GeoFormer.extract_features / match_features behind a FeatureStore)
    def _store_key(self, im_path):
        return (im_path, (self.imsize, self.preprocess, self.model.precision, str(self.model.backbone_dtype)))

    def resized_shape(self, im_path):
        """(H, W) of the tensor load_im makes of the file, from the file's header alone."""
        from PIL import Image
        with Image.open(im_path) as im:
            wo, ho = im.size
        wt, ht, _ = resize_im(wo, ho, imsize=self.imsize, dfactor=8, value_to_scale=min)
        return ht, wt

    def extract(self, im_path, slot=0) -> StoredImage:
        """The image's feature record (maps + resize ratios) through the store: loaded (preprocess = host or device, as match_pairs
        loads it) and run through the backbone on a miss, the kept record on a hit."""
        def make():
            gray, scale = self.load_im(im_path, slot=slot)
            with torch.no_grad():
                return StoredImage(self.model.extract_features(gray)[0], scale)
        return self.store.get_or_extract(self._store_key(im_path), make)

    def _results(self, data, recs0, recs1):
        """The model's batch output -> one match_pairs-style tuple per pair, split by m_bids."""
        k0, k1 = data['mkpts0_f'].cpu().numpy(), data['mkpts1_f'].cpu().numpy()
        scores, bids = data['mconf'].cpu().numpy(), data['m_bids'].cpu().numpy()
        out = []
        for n, (r0, r1) in enumerate(zip(recs0, recs1)):
            sel = bids == n
            kpts1, kpts2, sc = k0[sel], k1[sel], scores[sel]
            matches = np.concatenate([kpts1, kpts2], axis=1)
            upscale = np.array([r0.scale + r1.scale])
            if self.no_match_upscale:
                out.append((matches, kpts1, kpts2, sc, upscale.squeeze(0)))
            else:
                out.append((upscale * matches, r0.scale * kpts1, r1.scale * kpts2, sc))
        return out

    def match_features(self, rec0: StoredImage, rec1: StoredImage):
        """match_pairs from two kept records: same return convention (no_match_upscale included)."""
        with torch.no_grad():
            data = self.model.match_features([rec0.features], [rec1.features])
        return self._results(data, [rec0], [rec1])[0]

    def match_pairs_cached(self, im1_path, im2_path):
        """match_pairs with both images going through the store (an image that recurs is extracted once)."""
        return self.match_features(self.extract(im1_path, slot=0), self.extract(im2_path, slot=1))

    def match_many(self, pairs, batch=8, pad=False, max_waste=None):
        """[(path0, path1), ...] -> one match_pairs-style tuple per pair, in the order of `pairs`.  Pairs are grouped by their two
        resized shapes and run `batch` at a time through GeoFormer.match_features; every image is extracted once (once per stay in the
        store, under a byte budget).  A pair's numbers are those of the model on ITS BATCH - as with any batched `forward`, the device
        RANSAC draws its samples per position in the batch - so they equal match_pairs' exactly for batches of one pair.
        pad=True: pairs of UNEQUAL shapes share a batch (group_pairs_padded with max_waste, default DEFAULT_PAD_WASTE): the kept maps
        are matched on a common canvas with padding masks (GeoFormer.match_features(pad=True)); the backbone never sees padding and
        each record's own resize ratios still scale its keypoints (the maps share the canvas's origin).  A list of one shape gives
        the bits of pad=False."""
        pairs = [tuple(p) for p in pairs]
        shape = {}
        for p in pairs:
            for path in p:
                if path not in shape:
                    shape[path] = self.resized_shape(path)
        results = [None] * len(pairs)
        pair_shapes = [(shape[a], shape[b]) for a, b in pairs]
        groups = (group_pairs_padded(pair_shapes, batch, DEFAULT_PAD_WASTE if max_waste is None else max_waste) if pad
                  else group_pairs(pair_shapes, batch))
        for idx in groups:
            recs0 = [self.extract(pairs[k][0], slot=0) for k in idx]       # held here: eviction cannot free a map of the batch in flight
            recs1 = [self.extract(pairs[k][1], slot=1) for k in idx]
            with torch.no_grad():
                data = self.model.match_features([r.features for r in recs0], [r.features for r in recs1], pad=pad)
            for k, res in zip(idx, self._results(data, recs0, recs1)):
                results[k] = res
        return results


# ---------------------------------------------------------------------------------------------
# keypoints and match ids for SfM from pair matches (process_matches_and_keypoints_exporth5 of localize_sfm_helper.py, on the device)
# ---------------------------------------------------------------------------------------------
class ConsolidatedMatches(NamedTuple):
    names: list              # image paths in order of first appearance in the pair list
    keypoints: list          # per image: [K_i, 2] float32
    pair_images: np.ndarray  # [P, 2] int32: indices into names
    matches: list            # per pair: [n_p, 2] int32 keypoint indices (into keypoints[pair_images[p, 0]], keypoints[pair_images[p, 1]])


def consolidate_matches(pairs, results, sc_thres=0.25, qt_psize=48, qt_dthres=4, qt_unique=True, device='cuda', keep=None):
    """[(path0, path1), ...] and the tuples match_many returned for them (either return convention: element 0 is the [n, 4] matches,
    element 3 the scores) -> ConsolidatedMatches: what COLMAP-style triangulation and localisation consume - one keypoint list per image
    and every match as two keypoint indices.  The reference's process_matches_and_keypoints_exporth5 with its defaults: matches scoring
    below sc_thres are dropped, keypoints of an image closer than qt_dthres inside one qt_psize cell are merged into their running midpoint
    (a detector-free matcher never returns the same sub-pixel point twice: without merging every track has length two), and with qt_unique
    a keypoint keeps only its best match per pair.  qt_psize <= 0 or qt_dthres <= 0: keypoints are merged only where coordinates are equal.
    Matches are taken as float32 (match_many's upscaled float64 is cast first; the reference stores float32 keypoints anyway).  One upload,
    ops.consolidate_keypoints on the device, bit-identical to the serial rule (csrc/keypoint_spec.h).  A pair without surviving rows gives
    [0, 2]; a pair listed twice contributes twice, as in the reference.
    keep: one boolean mask per pair (verify_matches(...).masks): only the rows it marks enter - the result is that of the same call on lists
    with the other rows removed beforehand."""
    pairs = [tuple(p) for p in pairs]
    if len(pairs) != len(results):
        raise ValueError(f'consolidate_matches: {len(pairs)} pairs but {len(results)} results')
    if keep is not None and len(keep) != len(pairs):
        raise ValueError(f'consolidate_matches: {len(pairs)} pairs but {len(keep)} masks')
    index = {}
    pair_images = np.array([[index.setdefault(path, len(index)) for path in p] for p in pairs], np.int32).reshape(-1, 2)
    ms = [np.asarray(r[0], dtype=np.float32).reshape(-1, 4) for r in results]
    ss = [np.asarray(r[3], dtype=np.float32).reshape(-1) for r in results]
    if any(len(m) != len(s) for m, s in zip(ms, ss)):
        raise ValueError('consolidate_matches: a result whose matches and scores differ in length')
    if keep is not None:
        ks = [np.asarray(k, dtype=bool).reshape(-1) for k in keep]
        if any(len(k) != len(m) for k, m in zip(ks, ms)):
            raise ValueError('consolidate_matches: a mask whose length is not its pair\'s number of matches')
        ms, ss = [m[k] for m, k in zip(ms, ks)], [x[k] for x, k in zip(ss, ks)]
    offsets = np.concatenate([[0], np.cumsum([len(m) for m in ms])]).astype(np.int32)
    M, P = int(offsets[-1]), len(pairs)
    # one upload: the four arrays as one block of 32-bit words
    block = np.concatenate([a.reshape(-1).view(np.int32) for a in (*ms, *ss, offsets, pair_images)])
    with torch.cuda.device(device):
        d = torch.from_numpy(block).to(device)
        matches = d[:4 * M].view(torch.float32).view(M, 4)
        scores = d[4 * M:5 * M].view(torch.float32)
        off = d[5 * M:5 * M + P + 1]
        pim = d[5 * M + P + 1:].view(P, 2)
        kp, kpo, ids, ido = ops.consolidate_keypoints(matches, scores, off, pim, len(index), sc_thres, qt_psize, qt_dthres, qt_unique)
        kp, kpo, ids, ido = kp.cpu().numpy(), kpo.cpu().numpy(), ids.cpu().numpy(), ido.cpu().numpy()
    return ConsolidatedMatches(list(index), [kp[kpo[i]:kpo[i + 1]].copy() for i in range(len(index))], pair_images,
                               [ids[ido[q]:ido[q + 1]].copy() for q in range(P)])


# ---------------------------------------------------------------------------------------------
# two-view geometric verification without intrinsics: a fundamental-matrix RANSAC per pair, all pairs in one call on the device
# ---------------------------------------------------------------------------------------------
class VerifiedMatches(NamedTuple):
    F: np.ndarray            # [P, 3, 3] float64, x1^T F x0 = 0 in pixels, Frobenius norm 1 (zeros where RANSAC found no model)
    n_inliers: np.ndarray    # [P] int32
    verified: np.ndarray     # [P] bool: a model was found and it has at least min_inliers inliers
    masks: list              # per pair: [n_p] bool, the inliers of a verified pair; all False otherwise
    rounds: np.ndarray       # [P] int32: refits on the inliers accepted per pair (zeros without refit)


def verify_matches(pairs, results, thr=1.0, min_inliers=15, sc_thres=0.25, iters=None, device='cuda', refit=0):
    """Geometric verification of the matches of every pair, for image sets without poses or intrinsics: a detector-free matcher returns
    confident-looking matches for pairs that show different scenes, and a track should only see matches that one epipolar geometry
    explains.  Per pair a fundamental-matrix RANSAC (ops.ransac_fundamental: rows scoring below sc_thres or not finite take no part,
    seven-point hypotheses, squared Sampson distance below thr^2 pixels; the rule is csrc/fund_solver.h) - one upload, three launches for
    all pairs, one read back.  verified[p] = a model was found and n_inliers[p] >= min_inliers.  refit = R in 1 .. 8: one more launch
    refits every winner on its inliers up to R times (normalised eight-point fit, rank 2, inliers selected again; never fewer inliers
    than before); F, n_inliers, verified and masks are then the refined model's and rounds counts the accepted refits.  No
    planar-degeneracy test: the F of a planar scene is valid but arbitrary, its inlier set is still the plane's.  pairs / results as
    consolidate_matches takes them."""
    if len(pairs) != len(results):
        raise ValueError(f'verify_matches: {len(pairs)} pairs but {len(results)} results')
    P = len(results)
    ms = [np.asarray(r[0], dtype=np.float32).reshape(-1, 4) for r in results]
    ss = [np.asarray(r[3], dtype=np.float32).reshape(-1) for r in results]
    if any(len(m) != len(x) for m, x in zip(ms, ss)):
        raise ValueError('verify_matches: a result whose matches and scores differ in length')
    if P == 0:
        return VerifiedMatches(np.zeros((0, 3, 3)), np.zeros(0, np.int32), np.zeros(0, bool), [], np.zeros(0, np.int32))
    offsets = np.concatenate([[0], np.cumsum([len(m) for m in ms])]).astype(np.int32)
    M = int(offsets[-1])
    block = np.concatenate([a.reshape(-1).view(np.int32) for a in (*ms, *ss, offsets)])
    with torch.cuda.device(device):
        d = torch.from_numpy(block).to(device)
        rs = ops.ransac_fundamental(d[:4 * M].view(torch.float32).view(M, 4), d[4 * M:5 * M].view(torch.float32), d[5 * M:], P, pixel_thr=thr,
                                    sc_thres=sc_thres, iters=ops.FUND_RANSAC_ITERS if iters is None else iters, refit=refit)
        if not refit:
            rs['rounds'] = torch.zeros(P, dtype=torch.int32, device=rs['valid'].device)
        out = torch.cat([rs[k].reshape(-1).view(torch.uint8) for k in ('F', 'valid', 'n_inliers', 'rounds', 'inliers')]).cpu().numpy()
    F = out[:72 * P].view(np.float64).reshape(P, 3, 3).copy()
    valid = out[72 * P:76 * P].view(np.int32)
    nin = out[76 * P:80 * P].view(np.int32).copy()
    rounds = out[80 * P:84 * P].view(np.int32).copy()
    inl = out[84 * P:].astype(bool)
    verified = (valid == 1) & (nin >= min_inliers)
    masks = [inl[offsets[p]:offsets[p + 1]].copy() if verified[p] else np.zeros(len(ms[p]), bool) for p in range(P)]
    return VerifiedMatches(F, nin, verified, masks, rounds)


# ---------------------------------------------------------------------------------------------
# calibrated two-view verification: an essential-matrix RANSAC with pose recovery per pair, all pairs in one call on the device
# ---------------------------------------------------------------------------------------------
class RelativePoses(NamedTuple):
    E: np.ndarray            # [P, 3, 3] float64, x1^T E x0 = 0 in normalised coordinates, Frobenius norm 1 (zeros where no pose was found)
    R: np.ndarray            # [P, 3, 3] float64, x1 ~ R x0 + t
    t: np.ndarray            # [P, 3] float64, unit length (the scale of a relative pose is not observable)
    n_inliers: np.ndarray    # [P] int32
    verified: np.ndarray     # [P] bool: a pose was found and it has at least min_inliers inliers
    masks: list              # per pair: [n_p] bool, the inliers of a verified pair; all False otherwise
    rounds: np.ndarray       # [P] int32: refits on the inliers accepted per pair (zeros without refit)


def relative_poses(pairs, results, intrinsics, thr=1.0, min_inliers=15, sc_thres=0.25, iters=None, device='cuda', refit=0):
    """The relative pose of every pair from its matches, for image sets with known intrinsics: where K is known a fundamental matrix is
    the wrong model - two degrees of freedom too many, and no R, t.  Per pair an essential-matrix RANSAC with pose recovery
    (ops.ransac_relative_pose: rows scoring below sc_thres or not finite take no part, five-point hypotheses on normalised coordinates,
    squared Sampson distance below (thr / mean focal length)^2, the pose by the inliers' cheirality votes; the rule is
    csrc/rel_solver.h) - one upload, four launches for all pairs, one read back.  intrinsics[path]: 3 x 3 K of the image, in the pixels of
    the matches (what localize_queries takes and undistort_results returns); a pair whose image has no entry is a ValueError.
    verified[p] = a pose was found and n_inliers[p] >= min_inliers; verified and masks mean what they mean in VerifiedMatches, so
    consolidate_matches(..., keep=rp.masks) works unchanged.  refit = R in 1 .. 8: one more launch refits every pose on its inliers up to
    R times (Gauss-Newton on the Sampson residual over R and unit t, inliers selected again; never fewer inliers than before); E, R, t,
    n_inliers, verified and masks are then the refined model's and rounds counts the accepted refits.  On a purely planar scene the
    essential matrix has a twin solution and either may be returned; there is no homography model test.  pairs / results as
    consolidate_matches takes them."""
    pairs = [tuple(p) for p in pairs]
    if len(pairs) != len(results):
        raise ValueError(f'relative_poses: {len(pairs)} pairs but {len(results)} results')
    for p in pairs:
        for path in p:
            if path not in intrinsics:
                raise ValueError(f'relative_poses: no intrinsics for {path!r}')
    P = len(results)
    ms = [np.asarray(r[0], dtype=np.float32).reshape(-1, 4) for r in results]
    ss = [np.asarray(r[3], dtype=np.float32).reshape(-1) for r in results]
    if any(len(m) != len(x) for m, x in zip(ms, ss)):
        raise ValueError('relative_poses: a result whose matches and scores differ in length')
    if P == 0:
        return RelativePoses(np.zeros((0, 3, 3)), np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros(0, bool), [],
                             np.zeros(0, np.int32))
    Ks = np.stack([np.stack([np.asarray(intrinsics[path], dtype=np.float32).reshape(9) for path in p]) for p in pairs])      # [P, 2, 9]
    offsets = np.concatenate([[0], np.cumsum([len(m) for m in ms])]).astype(np.int32)
    M = int(offsets[-1])
    block = np.concatenate([a.reshape(-1).view(np.int32) for a in (*ms, *ss, offsets, Ks[:, 0], Ks[:, 1])])
    with torch.cuda.device(device):
        d = torch.from_numpy(block).to(device)
        k = d[5 * M + P + 1:].view(torch.float32)
        rs = ops.ransac_relative_pose(d[:4 * M].view(torch.float32).view(M, 4), d[4 * M:5 * M].view(torch.float32), d[5 * M:5 * M + P + 1], P,
                                      k[:9 * P].view(P, 3, 3), k[9 * P:].view(P, 3, 3), pixel_thr=thr, sc_thres=sc_thres,
                                      iters=ops.REL_RANSAC_ITERS if iters is None else iters, refit=refit)
        if not refit:
            rs['rounds'] = torch.zeros(P, dtype=torch.int32, device=rs['valid'].device)
        out = torch.cat([rs[q].reshape(-1).view(torch.uint8) for q in ('E', 'R', 't', 'valid', 'n_inliers', 'rounds', 'inliers')]).cpu().numpy()
    E = out[:72 * P].view(np.float64).reshape(P, 3, 3).copy()
    R = out[72 * P:144 * P].view(np.float64).reshape(P, 3, 3).copy()
    t = out[144 * P:168 * P].view(np.float64).reshape(P, 3).copy()
    valid = out[168 * P:172 * P].view(np.int32)
    nin = out[172 * P:176 * P].view(np.int32).copy()
    rounds = out[176 * P:180 * P].view(np.int32).copy()
    inl = out[180 * P:].astype(bool)
    verified = (valid == 1) & (nin >= min_inliers)
    masks = [inl[offsets[p]:offsets[p + 1]].copy() if verified[p] else np.zeros(len(ms[p]), bool) for p in range(P)]
    return RelativePoses(E, R, t, nin, verified, masks, rounds)


# ---------------------------------------------------------------------------------------------
# localisation: a camera pose per query from its matches against database images with known 3-D points, all queries in one call
# ---------------------------------------------------------------------------------------------
class LocalizedQueries(NamedTuple):
    names: list              # the queries, in order of first appearance in the pair list
    R: np.ndarray            # [Q, 3, 3] float64, x_cam = R X + t in world units (zeros where RANSAC found no model)
    t: np.ndarray            # [Q, 3] float64
    n_inliers: np.ndarray    # [Q] int32
    localized: np.ndarray    # [Q] bool: a model was found and it has at least min_inliers inliers
    masks: list              # per PAIR: [n_p] bool, the inliers of a localised query's pair; all False otherwise
    rounds: np.ndarray       # [Q] int32: refits on the inliers accepted per query (zeros without refit)
    # localize_queries_sparse with covis_cluster or dedup (None otherwise):
    n_clusters: Optional[np.ndarray] = None   # [Q] int32: covisibility clusters of the query's database images (1 with clustering off, 0: no image)
    cluster: Optional[np.ndarray] = None      # [Q] int32: the number of the winning cluster, -1 if there is none
    db_names: Optional[list] = None           # per query: its database images, in order of first appearance in the pair list
    db_cluster: Optional[list] = None         # per query: int32 array, the cluster of each entry of db_names
    cluster_inliers: Optional[list] = None    # per query: int32 [C_q], the inliers of each cluster's pose (0: RANSAC found no model)


def localize_queries(pairs, results, intrinsics, xyz_maps, thr=12.0, min_inliers=12, sc_thres=0.25, iters=None, device='cuda', refit=0):
    """Camera poses of query images from their matches against database images whose pixels have known 3-D points - the step the
    reference's eval_aachen / eval_robotcar / eval_inloc leave to hloc and pycolmap.  pairs: (query, database) paths, results: what
    match_many returned for them (matches [n, 4] = query x, y, database x, y; scores).  intrinsics[query]: 3 x 3 K of the query in the
    coordinates of its matches.  xyz_maps[database]: float32 [H, W, 3] array (NaN: no 3-D point) or the path of a .npy holding one, in
    the coordinates of the database keypoints; each map is uploaded once.  Every database keypoint gets its 3-D point by bilinear lookup
    (ops.xyz_lookup), all pairs of a query form one problem in pair order, and one absolute-pose RANSAC per query follows
    (ops.ransac_absolute_pose: P3P hypotheses, reprojection error below thr pixels; the rule is csrc/abs_solver.h) - one upload, the
    lookup, three launches (four with refit) for all queries, one read back.  localized[q] = a model was found and n_inliers[q] >=
    min_inliers.  No covisibility clustering; no distortion parameters here: undistort_results removes lens distortion from the matches
    beforehand."""
    if len(pairs) != len(results):
        raise ValueError(f'localize_queries: {len(pairs)} pairs but {len(results)} results')
    P = len(results)
    ms = [np.asarray(r[0], dtype=np.float32).reshape(-1, 4) for r in results]
    ss = [np.asarray(r[3], dtype=np.float32).reshape(-1) for r in results]
    if any(len(m) != len(x) for m, x in zip(ms, ss)):
        raise ValueError('localize_queries: a result whose matches and scores differ in length')
    names, qidx = [], {}
    for q, _ in pairs:
        if q not in qidx:
            qidx[q] = len(names)
            names.append(q)
    Q = len(names)
    if P == 0:
        return LocalizedQueries([], np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros(0, bool), [], np.zeros(0, np.int32))
    missing = [q for q in names if q not in intrinsics] + [d for _, d in pairs if d not in xyz_maps]
    if missing:
        raise ValueError(f'localize_queries: no intrinsics / 3-D map for {missing[0]!r}')
    order = sorted(range(P), key=lambda p: qidx[pairs[p][0]])          # stable: a query's pairs stay in pair order
    pair_off = np.concatenate([[0], np.cumsum([len(ms[p]) for p in order])]).astype(np.int32)
    per_query = np.bincount([qidx[pairs[p][0]] for p in order], weights=[len(ms[p]) for p in order], minlength=Q)
    query_off = np.concatenate([[0], np.cumsum(per_query)]).astype(np.int32)
    M = int(pair_off[-1])
    Ks = np.stack([np.asarray(intrinsics[q], dtype=np.float32).reshape(9) for q in names])
    rows = np.concatenate([ms[p] for p in order]) if M else np.zeros((0, 4), np.float32)
    with torch.cuda.device(device):
        dmaps = {}
        for _, dname in pairs:
            if dname not in dmaps:
                m = xyz_maps[dname]
                m = np.load(m) if isinstance(m, (str, os.PathLike)) else np.asarray(m)
                if m.ndim != 3 or m.shape[2] != 3:
                    raise ValueError(f'localize_queries: the 3-D map of {dname!r} has shape {m.shape}, expected [H, W, 3]')
                dmaps[dname] = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).to(device)
        table = np.array([[dmaps[pairs[p][1]].data_ptr(), dmaps[pairs[p][1]].shape[0] | (dmaps[pairs[p][1]].shape[1] << 32)] for p in order],
                         dtype=np.int64)
        # one upload: the table first (64-bit words), then everything else as 32-bit words
        block = np.concatenate([a.reshape(-1).view(np.int32) for a in
                                (table, np.ascontiguousarray(rows[:, :2]), np.ascontiguousarray(rows[:, 2:]), *[ss[p] for p in order],
                                 pair_off, query_off, Ks)])
        d = torch.from_numpy(block).to(device)
        o = 4 * P
        tab = d[:o].view(torch.int64).view(P, 2)
        p2d = d[o:o + 2 * M].view(torch.float32).view(M, 2)
        pdb = d[o + 2 * M:o + 4 * M].view(torch.float32).view(M, 2)
        sc = d[o + 4 * M:o + 5 * M].view(torch.float32)
        poff = d[o + 5 * M:o + 5 * M + P + 1]
        qoff = d[o + 5 * M + P + 1:o + 5 * M + P + Q + 2]
        Kd = d[o + 5 * M + P + Q + 2:].view(torch.float32).view(Q, 9)
        p3d = ops.xyz_lookup(tab, poff, pdb)
        rs = ops.ransac_absolute_pose(p2d, p3d, sc, qoff, Q, Kd, pixel_thr=thr, sc_thres=sc_thres,
                                      iters=ops.ABS_RANSAC_ITERS if iters is None else iters, refit=refit)
        out = torch.cat([rs[k].reshape(-1).view(torch.uint8) for k in ('R', 't', 'valid', 'n_inliers', 'rounds', 'inliers')]).cpu().numpy()
        del dmaps
    R = out[:72 * Q].view(np.float64).reshape(Q, 3, 3).copy()
    t = out[72 * Q:96 * Q].view(np.float64).reshape(Q, 3).copy()
    valid = out[96 * Q:100 * Q].view(np.int32)
    nin = out[100 * Q:104 * Q].view(np.int32).copy()
    rounds = out[104 * Q:108 * Q].view(np.int32).copy()
    inl = out[108 * Q:].astype(bool)
    localized = (valid == 1) & (nin >= min_inliers)
    masks = [None] * P
    for k, p in enumerate(order):
        masks[p] = inl[pair_off[k]:pair_off[k + 1]].copy() if localized[qidx[pairs[p][0]]] else np.zeros(len(ms[p]), bool)
    return LocalizedQueries(names, R, t, nin, localized, masks, rounds)


def rotation_to_quaternion(R):
    """(qw, qx, qy, qz) of a rotation matrix, qw >= 0 - the convention of the localisation benchmarks' submission files."""
    R = np.asarray(R, dtype=np.float64)
    k = np.array([[R[0, 0] - R[1, 1] - R[2, 2], 0, 0, 0],
                  [R[0, 1] + R[1, 0], R[1, 1] - R[0, 0] - R[2, 2], 0, 0],
                  [R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], R[2, 2] - R[0, 0] - R[1, 1], 0],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    w, v = np.linalg.eigh(k)                                          # the eigenvector of the largest eigenvalue: (x, y, z, w)
    q = v[[3, 0, 1, 2], np.argmax(w)]
    return q if q[0] >= 0 else -q


def read_intrinsics(path):
    """One line per query: `path fx fy cx cy` (blank lines and '#' lines are skipped; a relative path is relative to the file) ->
    {path: 3 x 3 K}."""
    base = os.path.dirname(os.path.abspath(path))
    out = {}
    with open(path) as f:
        for no, line in enumerate(f, 1):
            parts = line.split()
            if not parts or parts[0].startswith('#'):
                continue
            if len(parts) != 5:
                raise ValueError(f'{path}:{no}: expected `path fx fy cx cy`, got {len(parts)} fields')
            fx, fy, cx, cy = (float(v) for v in parts[1:])
            name = parts[0] if os.path.isabs(parts[0]) else os.path.normpath(os.path.join(base, parts[0]))
            out[name] = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    return out


def write_intrinsics(path, intrinsics, names=None):
    """The inverse of read_intrinsics: one line `name fx fy cx cy` per entry of `names` (default: every key), names as they are."""
    with open(path, 'w') as f:
        for name in (intrinsics if names is None else names):
            K = np.asarray(intrinsics[name], dtype=np.float64)
            f.write(' '.join([name] + [repr(float(v)) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2])]) + '\n')


# ---------------------------------------------------------------------------------------------
# lens distortion: the match coordinates of real cameras are undistorted once, on the device, before any geometry runs
# ---------------------------------------------------------------------------------------------
CAMERA_MODELS = {'SIMPLE_PINHOLE': 3, 'PINHOLE': 4, 'SIMPLE_RADIAL': 4, 'RADIAL': 5, 'OPENCV': 8}     # COLMAP's names -> number of parameters


class Camera(NamedTuple):
    model: str               # a key of CAMERA_MODELS
    width: int
    height: int
    params: tuple            # COLMAP's order: f | fx fy, then cx cy, then the model's distortion terms


def canonical_camera(camera):
    """The canonical record (fx, fy, cx, cy, k1, k2, p1, p2) of csrc/camera_spec.h for a Camera of any supported model."""
    model, p = camera.model, tuple(float(v) for v in camera.params)
    if model not in CAMERA_MODELS:
        raise ValueError(f'camera model {model!r} is not supported (supported: {", ".join(CAMERA_MODELS)})')
    if len(p) != CAMERA_MODELS[model]:
        raise ValueError(f'{model} takes {CAMERA_MODELS[model]} parameters, got {len(p)}')
    if model in ('PINHOLE', 'OPENCV'):
        return p + (0.0,) * (8 - len(p))
    return (p[0], p[0], p[1], p[2]) + p[3:] + (0.0,) * (7 - len(p))


def read_cameras(path):
    """hloc's query-list lines: `path MODEL W H params...` with COLMAP's model names and parameter order (SIMPLE_PINHOLE f cx cy; PINHOLE
    fx fy cx cy; SIMPLE_RADIAL f cx cy k; RADIAL f cx cy k1 k2; OPENCV fx fy cx cy k1 k2 p1 p2).  Blank lines and '#' lines are skipped; a
    relative path is relative to the file -> {path: Camera}.  An unknown model, a wrong number of parameters, a value that is not finite
    or a focal length that is not positive is a ValueError naming file and line."""
    base = os.path.dirname(os.path.abspath(path))
    out = {}
    with open(path) as f:
        for no, line in enumerate(f, 1):
            parts = line.split()
            if not parts or parts[0].startswith('#'):
                continue
            if len(parts) < 4:
                raise ValueError(f'{path}:{no}: expected `path MODEL W H params...`, got {len(parts)} fields')
            model = parts[1]
            if model not in CAMERA_MODELS:
                raise ValueError(f'{path}:{no}: unknown camera model {model!r} (supported: {", ".join(CAMERA_MODELS)})')
            if len(parts) - 4 != CAMERA_MODELS[model]:
                raise ValueError(f'{path}:{no}: {model} takes {CAMERA_MODELS[model]} parameters, got {len(parts) - 4}')
            try:
                w, h = int(parts[2]), int(parts[3])
                params = tuple(float(v) for v in parts[4:])
            except ValueError:
                raise ValueError(f'{path}:{no}: W and H must be integers and the parameters numbers') from None
            if not all(math.isfinite(v) for v in params):
                raise ValueError(f'{path}:{no}: a parameter that is not finite')
            if not all(v > 0 for v in params[:2 if model in ('PINHOLE', 'OPENCV') else 1]):
                raise ValueError(f'{path}:{no}: a focal length that is not positive')
            name = parts[0] if os.path.isabs(parts[0]) else os.path.normpath(os.path.join(base, parts[0]))
            out[name] = Camera(model, w, h, params)
    return out


def write_cameras(path, cameras):
    """The inverse of read_cameras: one line per camera; a name under the file's directory is written relative to it."""
    base = os.path.dirname(os.path.abspath(path))
    with open(path, 'w') as f:
        for name, cam in cameras.items():
            canonical_camera(cam)                                          # (the model and its parameter count)
            full = os.path.abspath(name)
            shown = os.path.relpath(full, base) if full.startswith(base + os.sep) else full
            f.write(' '.join([shown, cam.model, str(int(cam.width)), str(int(cam.height))] + [repr(float(v)) for v in cam.params]) + '\n')


def pinhole_of(cameras):
    """{name: Camera} -> {name: 3 x 3 K}: the intrinsics that hold for undistorted coordinates (what read_intrinsics returns)."""
    out = {}
    for name, cam in cameras.items():
        fx, fy, cx, cy = canonical_camera(cam)[:4]
        out[name] = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    return out


class UndistortedResults(list):
    """The list undistort_results returns, with n_failed int32 [P] (rows of a pair with a side that has no pre-image) and status (per
    pair: uint8 [n_p, 2], the status byte of each side of each row: 0 fine, 1 non-finite input, 2 no pre-image)."""
    n_failed = None
    status = None


def _original_pixel_rows(results):
    """[n, 4] float32 matches in the pixels of the original images for either return convention of match_many: the four-element tuple
    holds them, the five-element one (no_match_upscale) holds resized coordinates and, as element 4, the factors that scale them back."""
    return [np.ascontiguousarray((np.asarray(r[0], dtype=np.float64).reshape(-1, 4) * np.asarray(r[4], dtype=np.float64).reshape(1, 4)
                                  if len(r) > 4 else np.asarray(r[0])).astype(np.float32).reshape(-1, 4)) for r in results]


def undistort_results(pairs, results, cameras, device='cuda'):
    """[(path0, path1), ...], the tuples match_many returned for them (either return convention) and {path: Camera} -> (results',
    intrinsics): the same tuples with every coordinate replaced by the pixel of an ideal pinhole camera with the same fx, fy, cx, cy, and
    {path: 3 x 3 K} of those cameras (pinhole_of) - what verify_matches, consolidate_matches, localize_queries, triangulate, refine and
    localize_queries_sparse take, unchanged.  The rule is csrc/camera_spec.h (COLMAP's SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL,
    OPENCV; a guarded Newton iteration in fp64): one upload of all rows, one launch per side (ops.undistort_points reads the two sides of
    the [M, 4] block in place), one read back.  Scores are untouched; matches, kpts1 and kpts2 come back as float32.  A row with a side
    that has no pre-image (the pixel lies beyond the model's range) or a non-finite coordinate is NaN on that side: the stages downstream
    drop such rows.  results'.n_failed counts them per pair, results'.status holds the status bytes.
    Camera parameters refer to the original image, so the coordinates of a no_match_upscale tuple are first scaled back by its element 4;
    the tuple returned for it holds original-image coordinates and ones as element 4.
    Every image of `pairs` needs an entry in `cameras`, else ValueError.  Thresholds downstream are then in ideal-pinhole pixels, which
    are stretched towards the corners under barrel distortion."""
    pairs = [tuple(p) for p in pairs]
    if len(pairs) != len(results):
        raise ValueError(f'undistort_results: {len(pairs)} pairs but {len(results)} results')
    index = {}
    pim = np.array([[index.setdefault(path, len(index)) for path in p] for p in pairs], np.int32).reshape(-1, 2)
    missing = [n for n in index if n not in cameras]
    if missing:
        raise ValueError(f'undistort_results: no camera for {missing[0]!r}')
    names = list(index)
    intrinsics = pinhole_of({n: cameras[n] for n in names})
    ms = _original_pixel_rows(results)
    P = len(pairs)
    offsets = np.concatenate([[0], np.cumsum([len(m) for m in ms])]).astype(np.int32)
    M = int(offsets[-1])
    out = UndistortedResults()
    if M:
        table = np.array([canonical_camera(cameras[n]) for n in names], dtype=np.float64)
        C = len(names)
        # one upload: the camera table first (64-bit words), then everything else as 32-bit words
        block = np.concatenate([a.reshape(-1).view(np.int32) for a in (table, *ms, offsets, np.ascontiguousarray(pim[:, 0]),
                                                                       np.ascontiguousarray(pim[:, 1]))])
        with torch.cuda.device(device):
            d = torch.from_numpy(block).to(device)
            o = 16 * C
            tab = d[:o].view(torch.float64).view(C, 8)
            rows = d[o:o + 4 * M].view(torch.float32).view(M, 4)
            off = d[o + 4 * M:o + 4 * M + P + 1]
            cam = d[o + 4 * M + P + 1:].view(2, P)
            res = torch.empty(2, M, 2, dtype=torch.float32, device=d.device)
            flags = torch.zeros(2, dtype=torch.int32, device=d.device)
            st = [ops.undistort_points(rows[:, 2 * s:2 * s + 2], off, cam[s], tab, out=res[s], flags=flags)[1] for s in (0, 1)]
            back = torch.cat([res.view(-1).view(torch.uint8), flags.view(torch.uint8), *st]).cpu().numpy()      # the one read back
        ops.raise_camera_flags('undistort_results', back[16 * M:16 * M + 8].view(np.int32))
        xy = back[:16 * M].view(np.float32).reshape(2, M, 2)
        status = back[16 * M + 8:].reshape(2, M)
    else:
        xy, status = np.zeros((2, 0, 2), np.float32), np.zeros((2, 0), np.uint8)
    out.status, failed = [], []
    for p, r in enumerate(results):
        b, e = int(offsets[p]), int(offsets[p + 1])
        k0, k1 = xy[0, b:e].copy(), xy[1, b:e].copy()
        m = np.concatenate([k0, k1], axis=1)
        out.append((m, k0, k1, r[3], np.ones(4)) if len(r) > 4 else (m, k0, k1, r[3]))
        s = np.ascontiguousarray(status[:, b:e].T)
        out.status.append(s)
        failed.append(int((s == ops.CM_ST_NO_PREIMAGE).any(axis=1).sum()))
    out.n_failed = np.array(failed, np.int32)
    return out, intrinsics


def undistort_points(points, camera, device='cuda'):
    """[n, 2] pixels of one Camera -> (float32 [n, 2] pixels of the ideal pinhole camera with its fx, fy, cx, cy, uint8 [n] status as in
    undistort_results) - for the point lists of estimate_relative_pose and estimate_absolute_pose, with K = pinhole_of's."""
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float32).reshape(-1, 2))
    n = len(pts)
    if n == 0:
        canonical_camera(camera)
        return np.zeros((0, 2), np.float32), np.zeros(0, np.uint8)
    with torch.cuda.device(device):
        tab = ops.camera_table([canonical_camera(camera)], device)
        seg = torch.tensor([0, n, 0], dtype=torch.int32).to(device)
        out, st = ops.undistort_points(torch.from_numpy(pts).to(device), seg[:2], seg[2:], tab)
        return out.cpu().numpy(), st.cpu().numpy()


def write_consolidated(out_dir, cm: ConsolidatedMatches):
    """names.txt (one image path per line, line i = image i), keypoints.npz (k00000, ...: [K_i, 2] float32 per image) and matches.npz
    (pairs [P, 2] int32 image indices; m00000, ...: [n_p, 2] int32 keypoint indices per pair)."""
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, 'names.txt'), 'w') as f:
        f.writelines(n + '\n' for n in cm.names)
    np.savez(os.path.join(out_dir, 'keypoints.npz'), **{f'k{i:05d}': k for i, k in enumerate(cm.keypoints)})
    np.savez(os.path.join(out_dir, 'matches.npz'), pairs=cm.pair_images, **{f'm{q:05d}': m for q, m in enumerate(cm.matches)})


def read_consolidated(in_dir) -> ConsolidatedMatches:
    """The inverse of write_consolidated: names.txt, keypoints.npz and matches.npz under in_dir -> ConsolidatedMatches."""
    with open(os.path.join(in_dir, 'names.txt')) as f:
        names = [line.rstrip('\n') for line in f if line.rstrip('\n')]
    with np.load(os.path.join(in_dir, 'keypoints.npz')) as kz:
        keypoints = [np.asarray(kz[f'k{i:05d}'], dtype=np.float32).reshape(-1, 2) for i in range(len(names))]
    with np.load(os.path.join(in_dir, 'matches.npz')) as mz:
        pair_images = np.asarray(mz['pairs'], dtype=np.int32).reshape(-1, 2)
        matches = [np.asarray(mz[f'm{q:05d}'], dtype=np.int32).reshape(-1, 2) for q in range(len(pair_images))]
    return ConsolidatedMatches(names, keypoints, pair_images, matches)


def quaternion_to_rotation(q):
    """The rotation matrix of (qw, qx, qy, qz), normalised first: the inverse of rotation_to_quaternion."""
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def read_poses(path):
    """One line per image: `path qw qx qy qz tx ty tz` with x_cam = R X + t, the format `localize --out` writes (blank lines and '#' lines
    are skipped; a relative path is relative to the file) -> {path: (R 3 x 3, t [3])}."""
    base = os.path.dirname(os.path.abspath(path))
    out = {}
    with open(path) as f:
        for no, line in enumerate(f, 1):
            parts = line.split()
            if not parts or parts[0].startswith('#'):
                continue
            if len(parts) != 8:
                raise ValueError(f'{path}:{no}: expected `path qw qx qy qz tx ty tz`, got {len(parts)} fields')
            v = np.array([float(x) for x in parts[1:]])
            if not np.all(np.isfinite(v)) or not np.linalg.norm(v[:4]) > 0:
                raise ValueError(f'{path}:{no}: the pose is not finite or its quaternion is zero')
            name = parts[0] if os.path.isabs(parts[0]) else os.path.normpath(os.path.join(base, parts[0]))
            out[name] = (quaternion_to_rotation(v[:4]), v[4:].copy())
    return out


# ---------------------------------------------------------------------------------------------
# triangulation of the database images from their known poses (hloc's triangulation / COLMAP's point_triangulator in
# localize_sfm_helper.py:reconstruct_database_pairs), and localisation against the triangulated points
# ---------------------------------------------------------------------------------------------
class TriangulatedTracks(NamedTuple):
    points: np.ndarray       # [T_valid, 3] float64: the triangulated 3-D points, in world units
    errors: np.ndarray       # [T_valid] float64: root of the mean squared reprojection error of a point's inliers, in pixels
    obs_offsets: np.ndarray  # [T_valid + 1] int32: the inlier observations of point k are obs_offsets[k] : obs_offsets[k + 1]
    obs_image: np.ndarray    # [N] int32: index into the ConsolidatedMatches' names
    obs_keypoint: np.ndarray  # [N] int32: index into that image's keypoints
    point_of_keypoint: list  # per image: [K_i] int32, the point a keypoint is an inlier observation of; -1: none
    n_tracks: int            # connected components of the match graph with at least two keypoints
    n_conflict: int          # of them: tracks in which an image occurs twice (not triangulated)
    n_rejected: int          # of them: tracks without a conflict that ended without a point (no solution, or fewer than min_obs inliers)


def triangulate(cm: ConsolidatedMatches, intrinsics, poses, thr=4.0, min_angle=1.5, min_obs=2, refit=2, device='cuda') -> TriangulatedTracks:
    """3-D points for the tracks of a ConsolidatedMatches from known camera poses, on the device.  intrinsics[name]: 3 x 3 K in the
    coordinates of the keypoints; poses[name] = (R, t) with x_cam = R X + t (what localize_queries returns and read_poses reads).  Images
    without an entry in poses take no part.  A track is a connected component of the graph whose nodes are keypoints and whose edges are
    matches (ops.build_tracks); a track with the same image twice is a conflict and is left out; every other track gets the best two-view
    midpoint among its observation pairs (rays meeting at min_angle degrees or more; inliers: reprojection error below thr pixels), refitted
    on its inliers up to `refit` times (ops.triangulate_tracks; the rule is csrc/tri_solver.h), and is kept with at least min_obs
    inliers.  refit defaults to 2 here (0 in ops): a two-ray midpoint alone is a poor point for a long track.  Before the upload the world
    origin is moved to the centre of the bounding box of the camera centres (fp64), and the points are moved back afterwards.  One upload,
    one read back.  No bundle adjustment, no re-triangulation or merging of tracks, no splitting of conflict tracks; no distortion
    here: undistort_results removes it from the matches before they are consolidated."""
    n, kp_off, K, R, t, origin, ids, id_off, kps, pim = _triangulation_inputs(cm, intrinsics, poses)
    n_nodes, P, E = int(kp_off[-1]), len(cm.matches), len(ids)
    empty = _assemble_tracks(n, kp_off, 0, *([np.zeros(0)] * 4), np.zeros(1, np.int32), *([np.zeros(0, np.int32)] * 2), np.zeros(0, bool), origin)
    if n_nodes == 0 or E == 0:
        return empty
    # one upload: the fp64 words first, then everything else as 32-bit words
    block = np.concatenate([a.reshape(-1).view(np.int32) for a in (np.ascontiguousarray(R), np.ascontiguousarray(t), K, kps, ids, id_off, pim, kp_off)])
    with torch.cuda.device(device):
        d = torch.from_numpy(block).to(device)
        o = 0

        def take(words, dtype, *shape):
            nonlocal o
            v = d[o:o + words].view(dtype).view(*shape)
            o += words
            return v
        Rd, td = take(18 * n, torch.float64, n, 9), take(6 * n, torch.float64, n, 3)
        Kd, kpd = take(9 * n, torch.float32, n, 9), take(2 * n_nodes, torch.float32, n_nodes, 2)
        idd, iod, pimd, kpod = take(2 * E, torch.int32, E, 2), take(P + 1, torch.int32, P + 1), take(2 * P, torch.int32, P, 2), take(n + 1, torch.int32, n + 1)
        track_off, obs_image, obs_kp, obs_node = ops.build_tracks(idd, iod, pimd, kpod, n_nodes=n_nodes)
        T = int(track_off.numel()) - 1
        if T == 0:
            return empty
        rs = ops.triangulate_tracks(track_off, obs_image, kpd[obs_node.long()], Kd, Rd, td, pixel_thr=thr, min_angle_deg=min_angle, min_obs=min_obs,
                                    refit=refit)
        out = torch.cat([x.reshape(-1).view(torch.uint8) for x in (rs['X'], rs['err2'], rs['valid'], rs['conflict'], track_off, obs_image, obs_kp,
                                                                   rs['inliers'])]).cpu().numpy()
    N = int(obs_image.numel())
    return _assemble_tracks(n, kp_off, T, out[:24 * T].view(np.float64).reshape(T, 3), out[24 * T:32 * T].view(np.float64),
                            out[32 * T:36 * T].view(np.int32), out[36 * T:40 * T].view(np.int32), out[40 * T:44 * T + 4].view(np.int32),
                            out[44 * T + 4:44 * T + 4 + 4 * N].view(np.int32), out[44 * T + 4 + 4 * N:44 * T + 4 + 8 * N].view(np.int32),
                            out[44 * T + 4 + 8 * N:], origin)


def _triangulation_inputs(cm, intrinsics, poses):
    """What triangulate uploads: (n images, kp_off int32 [n+1], K fp32 [n,9], R fp64 [n,9] and t fp64 [n,3] with NaN for an image without
    a pose and t moved to the new origin, origin [3], ids int32 [E,2], id_off int32 [P+1], keypoints fp32 [n_nodes,2], pair_images)."""
    n = len(cm.names)
    counts = np.array([len(k) for k in cm.keypoints], np.int64)
    kp_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    K, R, t = np.zeros((n, 9), np.float32), np.full((n, 9), np.nan), np.full((n, 3), np.nan)
    K[:, [0, 4, 8]] = 1.0
    for i, name in enumerate(cm.names):
        if name not in poses:
            continue
        if name not in intrinsics:
            raise ValueError(f'triangulate: no intrinsics for {name!r}')
        K[i] = np.asarray(intrinsics[name], dtype=np.float32).reshape(9)
        R[i] = np.asarray(poses[name][0], dtype=np.float64).reshape(9)
        t[i] = np.asarray(poses[name][1], dtype=np.float64).reshape(3)
    posed = np.isfinite(R).all(1) & np.isfinite(t).all(1)
    origin = np.zeros(3)
    if posed.any():
        centres = -np.einsum('nji,nj->ni', R[posed].reshape(-1, 3, 3), t[posed])
        origin = 0.5 * (centres.min(0) + centres.max(0))
        t[posed] = t[posed] + np.einsum('nij,j->ni', R[posed].reshape(-1, 3, 3), origin)        # x_cam = R (X' + origin) + t
    ids = np.concatenate([np.asarray(m, np.int32).reshape(-1, 2) for m in cm.matches]) if len(cm.matches) else np.zeros((0, 2), np.int32)
    id_off = np.concatenate([[0], np.cumsum([len(m) for m in cm.matches])]).astype(np.int32)
    kps = np.concatenate([np.asarray(k, np.float32).reshape(-1, 2) for k in cm.keypoints]) if n else np.zeros((0, 2), np.float32)
    return n, kp_off, K, R, t, origin, ids, id_off, kps, np.asarray(cm.pair_images, np.int32).reshape(-1, 2)


def _assemble_tracks(n, kp_off, T, X, err2, valid, conflict, toff, oimg, okp, inl, origin) -> TriangulatedTracks:
    """The per-track and per-observation outputs of ops.triangulate_tracks -> TriangulatedTracks (points moved back by origin)."""
    valid, conflict, inl = np.asarray(valid) == 1, np.asarray(conflict) == 1, np.asarray(inl).astype(bool)
    nv = int(valid.sum())
    track_of_obs = np.repeat(np.arange(T), np.diff(toff))
    point_of_track = np.full(T, -1, np.int64)
    point_of_track[valid] = np.arange(nv)
    keep = inl & valid[track_of_obs]
    per_point = np.bincount(point_of_track[track_of_obs[keep]], minlength=nv)
    pok = np.full(int(kp_off[-1]), -1, np.int32)
    pok[kp_off[oimg[keep]] + okp[keep]] = point_of_track[track_of_obs[keep]]
    return TriangulatedTracks(np.asarray(X, np.float64).reshape(T, 3)[valid] + origin, np.sqrt(np.asarray(err2, np.float64)[valid]),
                              np.concatenate([[0], np.cumsum(per_point)]).astype(np.int32), oimg[keep].astype(np.int32), okp[keep].astype(np.int32),
                              [pok[kp_off[i]:kp_off[i + 1]].copy() for i in range(n)], int(T), int(conflict.sum()),
                              int(T - conflict.sum() - nv))


# ---------------------------------------------------------------------------------------------
# bundle adjustment: the database poses and the triangulated points refined jointly (ops.bundle_adjust; the rule is csrc/ba_spec.h)
# ---------------------------------------------------------------------------------------------
class RefinedStructure(NamedTuple):
    poses: dict              # name -> (R 3 x 3, t [3]) with x_cam = R X + t: every entry of the input, the free ones refined
    tracks: TriangulatedTracks  # the points refined; only observations that are inliers at the final state, points with at least min_obs
    cost: np.ndarray         # [stages * iters + stages] float64: the truncated cost before the first and after every iteration, per stage
    accepted: np.ndarray     # [stages * iters] int32: 1 where the iteration's step was taken
    n_free: int              # cameras that were free to move
    cg_used: Optional[np.ndarray] = None  # solver='pcg': [stages * iters] int32, the CG iterations of every iteration; None for 'dense'


def _refine_inputs(cm, tt, intrinsics, poses, fixed):
    """What refine uploads: dict(K fp32 [n,9], R / t fp64 with NaN for an image without a pose and t moved to the new origin, origin [3], X
    fp64 [T,3] moved likewise, obs_off, obs_image int32, uv fp32 [N,2], free bool [n]).  Free: a pose, not named in fixed, and at least one
    observation."""
    n, kp_off, K, R, t, origin = _triangulation_inputs(cm, intrinsics, poses)[:6]
    unknown = [f for f in fixed if f not in cm.names]
    if unknown:
        raise ValueError(f'refine: fixed names {unknown[0]!r}, which is not an image of the keypoints')
    obs_image = np.ascontiguousarray(tt.obs_image, np.int32)
    obs_kp = np.asarray(tt.obs_keypoint, np.int64)
    if len(obs_image) and (obs_image.min() < 0 or obs_image.max() >= n):
        raise ValueError('refine: the tracks name an image the keypoints do not have')
    kps = np.concatenate([np.asarray(k, np.float32).reshape(-1, 2) for k in cm.keypoints]) if n else np.zeros((0, 2), np.float32)
    counts = np.diff(kp_off)
    if len(obs_image) and (obs_kp.min() < 0 or (obs_kp >= counts[obs_image]).any()):
        raise ValueError('refine: the tracks name a keypoint its image does not have')
    posed = np.isfinite(R).all(1) & np.isfinite(t).all(1)
    fixed = set(fixed)
    free = posed & np.array([name not in fixed for name in cm.names], bool) & (np.bincount(obs_image, minlength=n) > 0)
    return dict(n=n, kp_off=kp_off, K=K, R=R, t=t, origin=origin, X=np.asarray(tt.points, np.float64).reshape(-1, 3) - origin,
                obs_off=np.ascontiguousarray(tt.obs_offsets, np.int32), obs_image=obs_image, obs_kp=obs_kp.astype(np.int32),
                uv=np.ascontiguousarray(kps[kp_off[obs_image].astype(np.int64) + obs_kp]), free=free, posed=posed)


def _refine_device(a, thrs, iters, device, solver='dense', cg_iters=64, cg_tol=1e-6):
    """One upload, one ops.bundle_adjust per threshold (each from the state the one before left, all on the device, all with the same
    solver), one read back -> dict(R [n,9], t [n,3], X [T,3], inliers uint8 [N], cost, accepted; with solver='pcg' also cg_used) in numpy."""
    n, T, N = a['n'], len(a['X']), len(a['obs_image'])
    block = np.concatenate([x.reshape(-1).view(np.int32) for x in (np.ascontiguousarray(a['R']), np.ascontiguousarray(a['t']),
                                                                   np.ascontiguousarray(a['X']), a['K'], a['uv'], a['obs_off'], a['obs_image'],
                                                                   a['free'].astype(np.int32))])
    with torch.cuda.device(device):
        d = torch.from_numpy(block).to(device)
        o = 0

        def take(words, dtype, *shape):
            nonlocal o
            v = d[o:o + words].view(dtype).view(*shape)
            o += words
            return v
        R, t, X = take(18 * n, torch.float64, n, 9), take(6 * n, torch.float64, n, 3), take(6 * T, torch.float64, T, 3)
        K, uv = take(9 * n, torch.float32, n, 9), take(2 * N, torch.float32, N, 2)
        ooff, oimg, free = take(T + 1, torch.int32, T + 1), take(N, torch.int32, N), take(n, torch.int32, n)
        host = {'obs_off': a['obs_off'], 'obs_image': a['obs_image'], 'free': a['free']}
        costs, accs, used = [], [], []
        pcg = solver == 'pcg'
        kw = dict(solver=solver, cg_iters=cg_iters, cg_tol=cg_tol) if pcg else {}
        for thr in thrs:
            rs = ops.bundle_adjust(ooff, oimg, uv, K, R, t, X, free, thr=thr, iters=iters, host=host, **kw)
            R, t, X = rs['R'], rs['t'], rs['X']
            costs.append(rs['cost'])
            accs.append(rs['accepted'])
            used.append(rs['cg_used'] if pcg else rs['accepted'][:0])
        out = torch.cat([x.reshape(-1).view(torch.uint8) for x in (R, t, X, torch.cat(costs), torch.cat(accs), torch.cat(used),
                                                                   rs['inliers'])]).cpu().numpy()
    nc, na = len(thrs) * (iters + 1), len(thrs) * iters
    cut = np.cumsum([0, 72 * n, 24 * n, 24 * T, 8 * nc, 4 * na, 4 * na if pcg else 0])
    f64 = lambda k: out[cut[k]:cut[k + 1]].view(np.float64)
    r = dict(R=f64(0).reshape(n, 9), t=f64(1).reshape(n, 3), X=f64(2).reshape(T, 3), cost=f64(3).copy(),
             accepted=out[cut[4]:cut[5]].view(np.int32).copy(), inliers=out[cut[6]:].copy())
    if pcg:
        r['cg_used'] = out[cut[5]:cut[6]].view(np.int32).copy()
    return r


def _assemble_refined(cm, tt, poses, a, r, min_obs) -> RefinedStructure:
    """The outputs of the device (or of the host build: the CPU tests) -> RefinedStructure, in world coordinates."""
    n, T, origin = a['n'], len(a['X']), a['origin']
    inl = np.asarray(r['inliers']).astype(bool)
    point_of_obs = np.repeat(np.arange(T), np.diff(a['obs_off']))
    valid = np.bincount(point_of_obs[inl], minlength=T) >= min_obs
    keep = inl & valid[point_of_obs]
    nv = int(valid.sum())
    new_id = np.full(T, -1, np.int64)
    new_id[valid] = np.arange(nv)
    oimg, okp, pt = a['obs_image'][keep], a['obs_kp'][keep], new_id[point_of_obs[keep]]
    R, t, X = r['R'].reshape(n, 3, 3), r['t'], r['X']
    Y = np.einsum('nij,nj->ni', R[oimg], X[point_of_obs[keep]]) + t[oimg]
    K = a['K'].astype(np.float64)[oimg]
    e2 = (K[:, 0] * Y[:, 0] / Y[:, 2] + K[:, 2] - a['uv'][keep, 0]) ** 2 + (K[:, 4] * Y[:, 1] / Y[:, 2] + K[:, 5] - a['uv'][keep, 1]) ** 2
    per_point = np.bincount(pt, minlength=nv)
    err = np.sqrt(np.bincount(pt, weights=e2, minlength=nv) / np.maximum(per_point, 1))
    pok = np.full(int(a['kp_off'][-1]), -1, np.int32)
    pok[a['kp_off'][oimg] + okp] = pt
    tracks = TriangulatedTracks(X[valid] + origin, err, np.concatenate([[0], np.cumsum(per_point)]).astype(np.int32), oimg.astype(np.int32),
                                okp.astype(np.int32), [pok[a['kp_off'][i]:a['kp_off'][i + 1]].copy() for i in range(n)], tt.n_tracks,
                                tt.n_conflict, tt.n_rejected + int(T - nv))
    out = dict(poses)
    for i, name in enumerate(cm.names):
        if a['free'][i]:
            out[name] = (R[i].copy(), t[i] - R[i] @ origin)             # t' = t + R origin
    return RefinedStructure(out, tracks, np.asarray(r['cost']), np.asarray(r['accepted']), int(a['free'].sum()),
                            np.asarray(r['cg_used']) if 'cg_used' in r else None)


def refine(cm: ConsolidatedMatches, tt: TriangulatedTracks, intrinsics, poses, fixed=(), iters=16, thr=4.0, min_obs=2,
           device='cuda', solver='dense', cg_iters=64, cg_tol=1e-6) -> RefinedStructure:
    """Bundle adjustment on the device: the poses of the images of cm and the points of tt refined jointly, minimising the squared
    reprojection error of tt's observations truncated at thr pixels (ops.bundle_adjust; the rule is csrc/ba_spec.h: Levenberg-Marquardt,
    points eliminated by the Schur complement, dense Cholesky of the reduced camera system, `iters` iterations enqueued at once).  poses[name]
    = (R, t) as triangulate takes them; fixed: names of images whose poses are trusted and stay as they are.  An image is free when it has
    a pose, is not fixed and has an observation; more than 128 free images is a ValueError (ops.BA_MAX_FREE).  With fewer than two fixed
    images nothing but the damping holds the frame, and the result may drift by a small similarity: fix the images whose poses are
    trusted.  An observation takes part only while its error is below thr, so thr must exceed the reprojection error of the start or the
    observations never join: thr may be a sequence, e.g. (20, 8, 4) - one run per threshold, each from the state the one before left.
    Returns RefinedStructure: poses (a dict like the input), tracks (the layout of tt: only observations that are inliers at the final
    state, points with fewer than min_obs of them dropped, errors recomputed, point_of_keypoint rebuilt), cost, accepted, n_free.  The world
    origin is moved to the centre of the camera centres' bounding box before the upload and back afterwards, as in triangulate.  One upload,
    one read back.  solver='pcg' (csrc/ba_pcg_spec.h) solves the reduced camera system by matrix-free preconditioned conjugate gradients
    instead of the dense Cholesky: up to 65536 free images (ops.BA_PCG_MAX_FREE), at most cg_iters (1 .. 256) CG iterations per iteration,
    stopped at the relative tolerance cg_tol (in [0, 1)); every stage of a thr schedule uses the same solver, and the result's cg_used is
    the log of CG iterations (None for 'dense').  The preconditioner is block Jacobi and the tolerance is fixed.  No intrinsics or
    distortion refinement, no robust loss other than the truncation, no re-triangulation inside the loop: call triangulate again with the
    refined poses to win observations back."""
    if solver not in ('dense', 'pcg'):
        raise ValueError(f"refine: solver must be 'dense' or 'pcg', not {solver!r}")
    pcg = solver == 'pcg'
    if pcg and not 1 <= int(cg_iters) <= ops.BA_PCG_MAX_ITERS:
        raise ValueError(f'refine: cg_iters must be 1 .. {ops.BA_PCG_MAX_ITERS}')
    if pcg and not 0.0 <= float(cg_tol) < 1.0:
        raise ValueError('refine: cg_tol must be in [0, 1)')
    thrs = tuple(float(x) for x in (thr if isinstance(thr, (tuple, list, np.ndarray)) else (thr,)))
    if not thrs or not all(x > 0 and np.isfinite(x) for x in thrs):
        raise ValueError('refine: thr must be positive')
    if not 1 <= int(iters) <= ops.BA_MAX_ITERS:
        raise ValueError(f'refine: iters must be 1 .. {ops.BA_MAX_ITERS}')
    if min_obs < 2:
        raise ValueError('refine: min_obs must be at least 2')
    a = _refine_inputs(cm, tt, intrinsics, poses, fixed)
    if pcg and int(a['free'].sum()) > ops.BA_PCG_MAX_FREE:
        raise ValueError(f"refine: {int(a['free'].sum())} free images, the limit is {ops.BA_PCG_MAX_FREE} with solver='pcg': name more "
                         'images in fixed')
    if not pcg and int(a['free'].sum()) > ops.BA_MAX_FREE:
        raise ValueError(f"refine: {int(a['free'].sum())} free images, the limit is {ops.BA_MAX_FREE} (the reduced camera system is solved "
                         "densely): name more images in fixed, or pass solver='pcg'")
    if len(a['X']) == 0 or len(a['obs_image']) == 0:
        return RefinedStructure(dict(poses), tt, np.zeros(0), np.zeros(0, np.int32), int(a['free'].sum()), np.zeros(0, np.int32) if pcg else None)
    if pcg:
        return _assemble_refined(cm, tt, poses, a, _refine_device(a, thrs, int(iters), device, solver='pcg', cg_iters=int(cg_iters),
                                                                  cg_tol=float(cg_tol)), min_obs)
    return _assemble_refined(cm, tt, poses, a, _refine_device(a, thrs, int(iters), device), min_obs)


def write_poses(path, poses):
    """One line per image: `path qw qx qy qz tx ty tz` with x_cam = R X + t - what read_poses reads."""
    with open(path, 'w') as f:
        for name, (R, t) in poses.items():
            f.write(' '.join([name] + [repr(float(v)) for v in (*rotation_to_quaternion(R), *np.asarray(t, np.float64).reshape(3))]) + '\n')


def localize_queries_sparse(cm: ConsolidatedMatches, tt: TriangulatedTracks, queries, intrinsics, thr=12.0, min_inliers=12, iters=None, refit=0,
                            device='cuda', covis_cluster=False, dedup=False) -> LocalizedQueries:
    """Camera poses of query images against triangulated points: the sparse counterpart of localize_queries for datasets with database
    poses and no depth.  queries: image names of cm.  For every pair of cm that joins a query and an image with points (the query on either
    side), the rows are p2d = the query's keypoints, p3d = the point of the other image's keypoint (tt.point_of_keypoint; NaN where it has
    none, such a row takes no part).  All pairs of a query form one problem in pair order, then ops.ransac_absolute_pose as in
    localize_queries.  intrinsics[query]: 3 x 3 K.  masks: one per pair of cm ([n_p] bool; all False for a pair that joins no query to
    points).  With both flags off: indexing on the host and an existing op.
    covis_cluster (hloc's covisibility_clustering): the database images of a query are split into the connected components of the
    covisibility graph restricted to them (two images are linked iff they share a point of tt), one pose per component, and the component
    with the most inliers wins (then the lowest cluster number) - retrieval that returns two places that look alike no longer pools them.
    dedup: every (query keypoint, point) counts once per problem, however many database images show it; the mask of a repeated row is
    its first occurrence's.  With either flag the rows are built on the device (ops.covis_clusters, ops.sparse_rows, ops.select_cluster;
    the rule is csrc/covis_spec.h; one upload, pair-level bookkeeping on the host) and the result carries n_clusters, cluster, db_names,
    db_cluster and cluster_inliers.  At most 1024 database images per query."""
    names = list(dict.fromkeys(queries))
    Q = len(names)
    missing = [q for q in names if q not in intrinsics or q not in cm.names]
    if missing:
        raise ValueError(f'localize_queries_sparse: no intrinsics for, or no image named {missing[0]!r}')
    if covis_cluster or dedup:
        return _localize_sparse_device(cm, tt, names, intrinsics, thr, min_inliers, iters, refit, device, bool(covis_cluster), bool(dedup))
    p2d, p3d, query_off, pair_off, used, owner = _sparse_rows(cm, tt, names)
    masks = [np.zeros(len(m), bool) for m in cm.matches]
    M = len(p2d)
    if Q == 0 or M == 0:
        return LocalizedQueries(names, np.zeros((Q, 3, 3)), np.zeros((Q, 3)), np.zeros(Q, np.int32), np.zeros(Q, bool), masks, np.zeros(Q, np.int32))
    Ks = np.stack([np.asarray(intrinsics[q], dtype=np.float32).reshape(9) for q in names])
    block = np.concatenate([a.reshape(-1).view(np.int32) for a in (p2d, p3d, query_off, Ks)])
    with torch.cuda.device(device):
        d = torch.from_numpy(block).to(device)
        rs = ops.ransac_absolute_pose(d[:2 * M].view(torch.float32).view(M, 2), d[2 * M:5 * M].view(torch.float32).view(M, 3), None,
                                      d[5 * M:5 * M + Q + 1], Q, d[5 * M + Q + 1:].view(torch.float32).view(Q, 9), pixel_thr=thr,
                                      iters=ops.ABS_RANSAC_ITERS if iters is None else iters, refit=refit)
        out = torch.cat([rs[k].reshape(-1).view(torch.uint8) for k in ('R', 't', 'valid', 'n_inliers', 'rounds', 'inliers')]).cpu().numpy()
    R = out[:72 * Q].view(np.float64).reshape(Q, 3, 3).copy()
    t = out[72 * Q:96 * Q].view(np.float64).reshape(Q, 3).copy()
    valid = out[96 * Q:100 * Q].view(np.int32)
    nin = out[100 * Q:104 * Q].view(np.int32).copy()
    rounds = out[104 * Q:108 * Q].view(np.int32).copy()
    inl = out[108 * Q:].astype(bool)
    localized = (valid == 1) & (nin >= min_inliers)
    for pos, (p, q) in enumerate(zip(used, owner)):
        if localized[q]:
            masks[p] = inl[pair_off[pos]:pair_off[pos + 1]].copy()
    return LocalizedQueries(names, R, t, nin, localized, masks, rounds)


def _sparse_rows(cm, tt, names):
    """The 2-D - 3-D rows of localize_queries_sparse, sorted by query (a query's pairs in pair order): p2d fp32 [M,2], p3d fp32 [M,3] (NaN:
    the keypoint has no point), query_off int32 [Q+1], pair_off [n+1] (the rows of the n contributing pairs), and per contributing pair
    its index in cm and its query."""
    qidx = {q: k for k, q in enumerate(names)}
    image_q = np.array([qidx.get(nm, -1) for nm in cm.names], np.int64)
    has_pts = np.array([bool((p >= 0).any()) for p in tt.point_of_keypoint])
    rows2, rows3, owner, used = [], [], [], []
    for p in range(len(cm.matches)):
        i, j = (int(v) for v in cm.pair_images[p])
        m = np.asarray(cm.matches[p]).reshape(-1, 2)
        for qs, ds, a, b in ((i, j, 0, 1), (j, i, 1, 0)):
            if image_q[qs] >= 0 and image_q[ds] < 0 and has_pts[ds]:
                pt = tt.point_of_keypoint[ds][m[:, b]]
                x = np.full((len(m), 3), np.nan, np.float32)
                x[pt >= 0] = tt.points[pt[pt >= 0]]
                rows2.append(np.asarray(cm.keypoints[qs], np.float32).reshape(-1, 2)[m[:, a]]), rows3.append(x)
                owner.append(int(image_q[qs])), used.append(p)
                break
    order = sorted(range(len(used)), key=lambda k: owner[k])            # stable: a query's pairs stay in pair order
    lens = [len(rows2[k]) for k in order]
    pair_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    query_off = np.concatenate([[0], np.cumsum(np.bincount([owner[k] for k in order], weights=lens, minlength=len(names)))]).astype(np.int32)
    p2d = np.concatenate([rows2[k] for k in order]) if order else np.zeros((0, 2), np.float32)
    p3d = np.concatenate([rows3[k] for k in order]) if order else np.zeros((0, 3), np.float32)
    return p2d, p3d, query_off, pair_off, [used[k] for k in order], [owner[k] for k in order]


def _covis_tables(cm, tt, names):
    """The pair-level bookkeeping of the device path (csrc/covis_spec.h, step 1; O(pairs), after one count of tt.obs_image per image for
    "has a point"): which pairs contribute (the rule of _sparse_rows), every query's database list in order of first appearance, and each
    list sorted by image id.  -> dict(pairs int32 [C,8], pair_row_off
    int32 [C+1], used: the index in cm of each contributing pair, list_off int32 [Q+1], list_img, sorted_img, sorted_pos int32 [L])."""
    qidx = {q: k for k, q in enumerate(names)}
    image_q = [qidx.get(nm, -1) for nm in cm.names]
    has_pts = np.bincount(np.asarray(tt.obs_image, np.int64), minlength=len(cm.names)) > 0       # an image with a point has an observation
    id_off = np.concatenate([[0], np.cumsum([len(m) for m in cm.matches])]).astype(np.int64)
    if id_off[-1] >= 2 ** 31:
        raise ValueError('localize_queries_sparse: 2^31 match rows or more')
    lists, where, pairs, used = [[] for _ in names], [{} for _ in names], [], []
    for p in range(len(cm.matches)):
        i, j = (int(v) for v in cm.pair_images[p])
        for qs, ds, col in ((i, j, 0), (j, i, 1)):
            if image_q[qs] >= 0 and image_q[ds] < 0 and has_pts[ds]:
                q = image_q[qs]
                pos = where[q].setdefault(ds, len(lists[q]))
                if pos == len(lists[q]):
                    lists[q].append(ds)
                pairs.append((q, qs, ds, id_off[p], id_off[p + 1], col, pos, 0)), used.append(p)
                break
    longest = max([len(x) for x in lists], default=0)
    if longest > ops.CV_MAX_LIST:
        raise ValueError(f'localize_queries_sparse: a query with {longest} database images; at most {ops.CV_MAX_LIST}')
    pairs = np.array(pairs, np.int32).reshape(-1, ops.CV_PAIR_WORDS)
    flat = lambda xs: np.array([v for x in xs for v in x], np.int32)              # noqa: E731
    by_id = [sorted(range(len(x)), key=x.__getitem__) for x in lists]
    return {'pairs': pairs, 'pair_row_off': np.concatenate([[0], np.cumsum(pairs[:, 4].astype(np.int64) - pairs[:, 3])]).astype(np.int32),
            'used': used, 'list_off': np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32), 'list_img': flat(lists),
            'sorted_img': flat([[x[a] for a in o] for x, o in zip(lists, by_id)]), 'sorted_pos': flat(by_id)}


def _device_rows(cm, tt, names, intrinsics, tb, device, covis_cluster, dedup):
    """The device row path of localize_queries_sparse for the tables tb of _covis_tables: one upload, ops.covis_clusters, ops.sparse_rows
    (one read of the sizes) -> (K fp32 [Q,9], cluster, n_clusters, the dict of ops.sparse_rows with p2d and p3d), all on the device."""
    Q, C = len(names), len(tb['pairs'])
    kp_off = np.concatenate([[0], np.cumsum([len(k) for k in cm.keypoints])]).astype(np.int32)
    n_nodes, T = int(kp_off[-1]), len(tt.points)
    ids = np.concatenate([np.asarray(m, np.int32).reshape(-1, 2) for m in cm.matches])
    E = len(ids)
    Ks = np.stack([np.asarray(intrinsics[q], dtype=np.float32).reshape(9) for q in names])
    kps = np.concatenate([np.asarray(k, np.float32).reshape(-1, 2) for k in cm.keypoints])
    parts = (kp_off, np.concatenate(tt.point_of_keypoint).astype(np.int32), np.asarray(tt.obs_offsets, np.int32), np.asarray(tt.obs_image, np.int32),
             tb['pairs'], tb['pair_row_off'], ids, tb['list_off'], tb['list_img'], tb['sorted_img'], tb['sorted_pos'], Ks, kps,
             np.asarray(tt.points).astype(np.float32))                 # the points rounded once to fp32, as _sparse_rows does
    block = np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.int32) for a in parts])
    d = torch.from_numpy(block).to(device)                             # one upload
    o = 0

    def take(a, dtype=torch.int32, *shape):
        nonlocal o
        v = d[o:o + a.size].view(dtype)
        o += a.size
        return v.view(*shape) if shape else v
    kpo, pok, ooff, oimg = (take(a) for a in parts[:4])
    prs, pro, idd = take(parts[4], torch.int32, C, ops.CV_PAIR_WORDS), take(parts[5]), take(parts[6], torch.int32, E, 2)
    loff, limg, simg, spos = (take(a) for a in parts[7:11])
    Kd, kpd, ptd = take(Ks, torch.float32, Q, 9), take(kps, torch.float32, n_nodes, 2), take(parts[13], torch.float32, T, 3)
    cluster, ncl, status = ops.covis_clusters(kpo, pok, ooff, oimg, loff, limg, simg, spos, tb, enable=covis_cluster)
    rows = ops.sparse_rows(prs, pro, idd, kpo, pok, T, loff, cluster, ncl, tb, dedup=dedup, status=status, keypoints=kpd, points=ptd)
    return Kd, cluster, ncl, rows


def _localize_sparse_device(cm, tt, names, intrinsics, thr, min_inliers, iters, refit, device, covis_cluster, dedup):
    """localize_queries_sparse with covis_cluster or dedup: one upload, the cluster kernel, the row kernel with torch's sorts behind it, one
    read of the sizes, ops.ransac_absolute_pose over the problems, the selection kernel, one read back."""
    Q = len(names)
    tb = _covis_tables(cm, tt, names)
    Lt, used = len(tb['list_img']), tb['used']
    masks = [np.zeros(len(m), bool) for m in cm.matches]
    db_names = [[cm.names[i] for i in tb['list_img'][tb['list_off'][q]:tb['list_off'][q + 1]]] for q in range(Q)]
    zero = np.zeros(Q, np.int32)

    def result(R, t, nin, localized, rounds, ncl, win, cluster, cin):
        base = np.concatenate([[0], np.cumsum(ncl)])
        return LocalizedQueries(names, R, t, nin, localized, masks, rounds, ncl, win,
                                db_names, [cluster[tb['list_off'][q]:tb['list_off'][q + 1]].copy() for q in range(Q)],
                                [cin[base[q]:base[q + 1]].copy() for q in range(Q)])
    if Q == 0 or Lt == 0:                                              # no contributing pair: every list is empty, C_q = 0
        return result(np.zeros((Q, 3, 3)), np.zeros((Q, 3)), zero, np.zeros(Q, bool), zero.copy(), zero.copy(), np.full(Q, -1, np.int32),
                      np.zeros(0, np.int32), np.zeros(0, np.int32))
    with torch.cuda.device(device):
        Kd, cluster, ncl, rows = _device_rows(cm, tt, names, intrinsics, tb, device, covis_cluster, dedup)
        N, M = rows['N'], rows['M']
        if M == 0:
            ncl_h, cl_h = ncl.cpu().numpy(), cluster.cpu().numpy()
            return result(np.zeros((Q, 3, 3)), np.zeros((Q, 3)), zero, np.zeros(Q, bool), zero.copy(), ncl_h, np.full(Q, -1, np.int32), cl_h,
                          np.zeros(N, np.int32))
        query_of_prob = torch.repeat_interleave(torch.arange(Q, device=ncl.device), ncl.long(), output_size=N)
        rs = ops.ransac_absolute_pose(rows['p2d'], rows['p3d'], None, rows['prob_off'], N, Kd[query_of_prob], pixel_thr=thr,
                                      iters=ops.ABS_RANSAC_ITERS if iters is None else iters, refit=refit)
        sel = ops.select_cluster(rows['prob_base'], rs, rows['row_prob'], rows['slot'], min_inliers)
        out = torch.cat([x.reshape(-1).view(torch.uint8) for x in (sel['R'], sel['t'], sel['winner'], sel['localized'], sel['n_inliers'], sel['rounds'],
                                                                   ncl, cluster, sel['cluster_inliers'], sel['mask'])]).cpu().numpy()
    o = 0

    def read(count, dtype, *shape):
        nonlocal o
        v = out[o:o + count * np.dtype(dtype).itemsize].view(dtype).copy()
        o += count * np.dtype(dtype).itemsize
        return v.reshape(*shape) if shape else v
    R, t = read(9 * Q, np.float64, Q, 3, 3), read(3 * Q, np.float64, Q, 3)
    win, localized, nin, rounds, ncl_h = read(Q, np.int32), read(Q, np.int32).astype(bool), read(Q, np.int32), read(Q, np.int32), read(Q, np.int32)
    cl_h, cin, mask = read(Lt, np.int32), read(N, np.int32), out[o:].astype(bool)
    for c, p in enumerate(used):                                       # (a pair listed with a query contributes once; the masks of a query
        if localized[tb['pairs'][c, 0]]:                               #  that is not localised stay False, as with the flags off)
            masks[p] = mask[tb['pair_row_off'][c]:tb['pair_row_off'][c + 1]].copy()
    return result(R, t, nin, localized, rounds, ncl_h, win, cl_h, cin)


def read_triangulated(path) -> TriangulatedTracks:
    """What `triangulate --out FILE.npz` wrote -> TriangulatedTracks.  A file from before n_tracks, n_conflict and n_rejected were saved
    reads with -1 for the three counts."""
    with np.load(path) as z:
        kp_off = np.asarray(z['kp_offsets'], np.int64)
        pok = np.asarray(z['point_of_keypoint'], np.int32)
        counts = [int(z[k]) if k in z.files else -1 for k in ('n_tracks', 'n_conflict', 'n_rejected')]
        return TriangulatedTracks(np.asarray(z['points'], np.float64).reshape(-1, 3), np.asarray(z['errors'], np.float64),
                                  np.asarray(z['obs_offsets'], np.int32), np.asarray(z['obs_image'], np.int32), np.asarray(z['obs_keypoint'], np.int32),
                                  [pok[kp_off[i]:kp_off[i + 1]].copy() for i in range(len(kp_off) - 1)], *counts)


# ---------------------------------------------------------------------------------------------
# HPatches homography metric
# ---------------------------------------------------------------------------------------------
def cal_error_auc(errors, thresholds):
    """Area under the recall-vs-error curve up to each threshold, normalised by the threshold."""
    errors = np.asarray(errors, dtype=float)
    if errors.size == 0:
        return np.zeros(len(thresholds))
    n = errors.size
    err = np.concatenate([[0.0], np.sort(errors)])
    rec = np.arange(n + 1) / n
    out = []
    for t in thresholds:
        k = np.searchsorted(err, t)
        x = np.concatenate([err[:k], [t]])
        y = np.concatenate([rec[:k], [rec[k - 1]]])
        out.append(float(np.sum((y[1:] + y[:-1]) * 0.5 * np.diff(x))) / t)      # trapezoid rule
    return np.array(out, dtype=float)


def cal_reproj_dists(p1s, p2s, homography):
    p = np.concatenate([p1s, np.ones((len(p1s), 1))], axis=1) @ np.asarray(homography).T
    return np.sqrt(((p2s - p[:, :2] / p[:, 2:]) ** 2).sum(1))


def scale_homography(sw, sh):
    return np.array([[sw, 0, 0], [0, sh, 0], [0, 0, 1.0]])


def estimate_homography(matches, thr, device='cuda'):
    """RANSAC homography from [n,4] matches on the device; returns (H | None, inlier mask)."""
    if len(matches) < 4:
        return None, np.zeros(len(matches), bool)
    m = torch.as_tensor(matches, dtype=torch.float32, device=device)
    counts = torch.tensor([len(m), len(m)], dtype=torch.int32, device=device)
    rs = ops.ransac_homography(m[:, :2].contiguous(), m[:, 2:4].contiguous(), counts, 1, 1.0, thr=thr,
                               integer_keypoints=False, min_points=4)
    if int(rs['valid'][0]) == 0:
        return None, np.zeros(len(matches), bool)
    return rs['M'][0].cpu().numpy(), rs['keep'][:len(m)].cpu().numpy().astype(bool)


def estimate_relative_pose(matches, K0, K1, thr=0.5, device='cuda'):
    """Essential-matrix RANSAC + pose recovery from [n,4] pixel matches on the device (estimate_pose of the reference's metrics.py);
    returns (R, t, inlier mask) or None.  One pair per call, for the validation metrics; for the pairs of a match list - all in one
    call, with the row filter of consolidate_matches and an optional refit on the inliers - see relative_poses."""
    if len(matches) < 5:
        return None
    m = torch.as_tensor(np.asarray(matches), dtype=torch.float32, device=device)
    counts = torch.tensor([len(m), len(m)], dtype=torch.int32, device=device)
    k0 = torch.as_tensor(np.asarray(K0), dtype=torch.float32, device=device).reshape(1, 3, 3)
    k1 = torch.as_tensor(np.asarray(K1), dtype=torch.float32, device=device).reshape(1, 3, 3)
    rs = ops.ransac_essential(m[:, :2].contiguous(), m[:, 2:4].contiguous(), counts, 1, k0, k1, pixel_thr=thr)
    if int(rs['valid'][0]) == 0:
        return None
    return rs['R'][0].cpu().numpy(), rs['t'][0].cpu().numpy(), rs['inliers'].cpu().numpy().astype(bool)


def estimate_fundamental(matches, thr=1.0, device='cuda', refit=0):
    """Fundamental-matrix RANSAC from [n,4] pixel matches on the device (no intrinsics needed; csrc/fund_solver.h); returns
    (F with x1^T F x0 = 0 and Frobenius norm 1, inlier mask) or None.  refit: up to that many refits of the winner on its inliers (0 .. 8)."""
    if len(matches) < 7:
        return None
    m = torch.as_tensor(np.asarray(matches), dtype=torch.float32, device=device)
    offsets = torch.tensor([0, len(m)], dtype=torch.int32, device=device)
    rs = ops.ransac_fundamental(m[:, :4].contiguous(), None, offsets, 1, pixel_thr=thr, refit=refit)
    if int(rs['valid'][0]) == 0:
        return None
    return rs['F'][0].cpu().numpy(), rs['inliers'].cpu().numpy().astype(bool)


def estimate_absolute_pose(points2d, points3d, K, thr=12.0, refit=0, device='cuda', sample=0):
    """Absolute-pose (P3P) RANSAC from [n,2] pixels and their [n,3] world points on the device (csrc/abs_solver.h); returns (R, t with
    x_cam = R X + t, inlier mask) or None.  refit: up to that many Gauss-Newton refits of the winner on its inliers (0 .. 8).  sample: the
    problem index the hypotheses are drawn for (the draw of hypothesis t depends on (seed, problem, t)): the pose of problem q of a
    larger launch, as localize_queries makes it, is reproduced with sample=q."""
    if len(points2d) != len(points3d):
        raise ValueError(f'estimate_absolute_pose: {len(points2d)} 2-D points but {len(points3d)} 3-D points')
    if len(points2d) < 4:
        return None
    n, q = len(points2d), int(sample)
    a = torch.as_tensor(np.asarray(points2d), dtype=torch.float32, device=device).reshape(n, 2)
    b = torch.as_tensor(np.asarray(points3d), dtype=torch.float32, device=device).reshape(n, 3)
    offsets = torch.tensor([0] * (q + 1) + [n], dtype=torch.int32, device=device)
    rs = ops.ransac_absolute_pose(a, b, None, offsets, q + 1, torch.as_tensor(np.asarray(K), dtype=torch.float32).reshape(3, 3), pixel_thr=thr,
                                  refit=refit)
    if int(rs['valid'][q]) == 0:
        return None
    return rs['R'][q].cpu().numpy(), rs['t'][q].cpu().numpy(), rs['inliers'].cpu().numpy().astype(bool)


def corner_error(H_pred, H_gt, w, h):
    corners = np.array([[0, 0, 1], [0, h - 1, 1], [w - 1, 0, 1], [w - 1, h - 1, 1.0]])
    a = corners @ np.asarray(H_gt).T
    b = corners @ np.asarray(H_pred).T
    return float(np.mean(np.linalg.norm(a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:], axis=1)))


def hpatches_pairs(data_root, max_seqs: Optional[int] = None):
    """The protocol's pair list: every sequence (reverse lexical order, as hpatches_helper.eval_hpatches walks
    them), image 1 against images 2..6 -> [(sequence name, im1, im2, H_1_k path)]."""
    seqs = sorted(glob.glob(os.path.join(data_root, '*')))[::-1]
    if max_seqs:
        seqs = seqs[:max_seqs]
    return [(os.path.basename(seq), os.path.join(seq, '1.ppm'), os.path.join(seq, f'{k}.ppm'), os.path.join(seq, f'H_1_{k}'))
            for seq in seqs for k in range(2, 7)]


def eval_hpatches(matcher, data_root, ransac_thres=3, thres=(1, 3, 5, 10), scale_H=True, max_seqs: Optional[int] = None,
                  log=print, reuse_features=False):
    """Homography-estimation AUC over HPatches sequences (pairs 1 -> 2..6), the protocol of
    hpatches_helper.eval_hpatches with task='homography', h_solver='cv'.

    Pairs are independent: under torch.distributed (one process per GPU) the pair list is cut into contiguous
    per-rank blocks by `shard.run_sharded` and every rank ends up with the summaries of ALL pairs, so the metric
    is identical on every rank and to a single-process run.

    reuse_features: the pairs go through the matcher's feature store (`match_pairs_cached`), so image 1 of a sequence is extracted
    once instead of five times."""
    from PIL import Image
    from .shard import run_sharded

    def match_block(block):
        out = []
        for sname, im1, im2, hfile in block:
            H_gt = np.loadtxt(hfile)
            scale = np.ones(4)
            t0 = time.time()
            res = matcher.match_pairs_cached(im1, im2) if reuse_features else matcher(im1, im2)
            dt = time.time() - t0
            matches = res[0]
            if scale_H and len(res) > 4:       # matches stay in resized coordinates: move the GT homography there
                scale = res[4]
                H_gt = np.linalg.inv(scale_homography(scale[2], scale[3])) @ H_gt @ scale_homography(scale[0], scale[1])
            H_pred, _ = estimate_homography(matches, ransac_thres, matcher.device)
            if H_pred is None:
                d = float('nan')
            else:
                w, h = Image.open(im1).size
                d = corner_error(H_pred, H_gt, w / scale[0], h / scale[1])
            out.append((sname, d, len(matches), dt))
        return out
    rows = run_sharded(hpatches_pairs(data_root, max_seqs), match_block, batch=5)
    dists = {'a': [], 'i': [], 'v': []}
    for sname, d, _, _ in rows:
        dists['a'].append(d)
        dists[sname[0] if sname[0] in 'iv' else 'v'].append(d)
    out = {}
    for key, ds in dists.items():
        ds = np.asarray(ds, dtype=float)
        out['correct_' + key] = np.mean([[float(d <= t) for t in thres] for d in ds], axis=0) if len(ds) else np.zeros(len(thres))
        out['auc_' + key] = cal_error_auc(ds, thres)
    out.update(failed=int(sum(np.isnan(r[1]) for r in rows)), mean_matches=float(np.mean([r[2] for r in rows])) if rows else 0.0,
               match_time=float(np.mean([r[3] for r in rows])) if rows else 0.0, pairs=len(rows))
    log(f"Hest Correct: a={out['correct_a']} i={out['correct_i']} v={out['correct_v']}")
    log(f"Hest AUC: a={out['auc_a']} i={out['auc_i']} v={out['auc_v']}")
    return out


# ---------------------------------------------------------------------------------------------
# command line: the counterparts of `python inference.py` and `python eval_Hpatches.py`
#   python -m geoformer_amd.matcher match im1 im2 [--ckpt saved_ckpt/geoformer.ckpt] [--out matches.npz] [--preprocess device]
#   python -m geoformer_amd.matcher hpatches /path/to/hpatches-sequences-release [--ckpt ...] [--preprocess device] [--reuse-features]
#   python -m geoformer_amd.matcher pairs LIST | --all-pairs DIR  [--out DIR] [--batch B] [--cache-gb G] [--pad [--pad-waste R]]   (no reference counterpart)
#                                         [--keypoints DIR [--sc-thres S] [--qt-psize P] [--qt-dthres D] [--no-qt-unique]]   (process_matches_and_keypoints_exporth5)
#                                         [--verify [--verify-thr T] [--min-inliers K] [--verify-refit [R]]]   (two-view verification: fundamental-matrix RANSAC per pair)
#   python -m geoformer_amd.matcher localize LIST --xyz DIR --intrinsics FILE [--out FILE] [--thr T] [--min-inliers K] [--refit [R]]   (hloc's localize_sfm / localize_inloc)
#   python -m geoformer_amd.matcher triangulate KEYPOINTS_DIR --poses FILE --intrinsics FILE [--out FILE.npz] [--thr T] [--min-angle A] [--min-obs K] [--refit [R]]   (hloc's triangulation)
#   python -m geoformer_amd.matcher localize-sparse KEYPOINTS_DIR --points FILE.npz --queries FILE --intrinsics FILE [--covis-cluster] [--dedup] [--thr T] [--min-inliers K] [--refit [R]] [--out FILE]   (hloc's localize_sfm)
# ---------------------------------------------------------------------------------------------
def build_parser():
    """Defaults follow the reference per sub-command: `match` = inference.py:107 (imsize 640, matches scaled back to the
    original images); `hpatches` = eval_configs/geoformer.yml:7-11 with eval_Hpatches.py:96-100 (imsize 480, match
    threshold 0.2, no_match_upscale True -> the ground-truth homography is moved into resized coordinates, RANSAC
    threshold 3).  Under `python -m torch.distributed.run --nproc-per-node N -m geoformer_amd.matcher hpatches ...` the
    pair list is sharded over the N GPUs (shard.run_sharded).  `pairs` matches a list of pairs with every image's backbone pass run
    once (GeoFormerMatcher.match_many); its defaults are `match`'s."""
    import argparse
    ap = argparse.ArgumentParser(prog='python -m geoformer_amd.matcher')
    sub = ap.add_subparsers(dest='cmd', required=True)
    m = sub.add_parser('match', help='match one image pair (inference.py)')
    m.add_argument('im1'), m.add_argument('im2'), m.add_argument('--out', default=None)
    m.add_argument('--imsize', type=int, default=640)
    m.add_argument('--no-match-upscale', action='store_true')
    h = sub.add_parser('hpatches', help='homography AUC over HPatches sequences (eval_Hpatches.py)')
    h.add_argument('root'), h.add_argument('--max-seqs', type=int, default=None)
    h.add_argument('--ransac-thres', type=float, default=3.0)
    h.add_argument('--imsize', type=int, default=480)
    h.add_argument('--match-upscale', dest='no_match_upscale', action='store_false',
                   help='scale matches back to the original images instead of moving the GT homography (reference: off)')
    h.set_defaults(no_match_upscale=True)
    h.add_argument('--reuse-features', action='store_true',
                   help="keep each image's backbone features in the feature store: image 1 of a sequence is extracted once, not five times")
    q = sub.add_parser('pairs', help='match many pairs, extracting the features of every image once')
    q.add_argument('list', nargs='?', default=None, help='text file with two image paths per line (relative paths: relative to the file)')
    q.add_argument('--all-pairs', metavar='DIR', default=None, help='instead of a list: every pair of the images under DIR, sorted by name')
    q.add_argument('--out', default=None, help='directory for one .npz per pair (keys as `match --out`: matches, kpts1, kpts2, scores)')
    q.add_argument('--batch', type=int, default=8, help='pairs of equal shapes matched per model call')
    q.add_argument('--imsize', type=int, default=640)
    q.add_argument('--no-match-upscale', action='store_true')
    q.add_argument('--pad', action='store_true',
                   help='let pairs of unequal shapes share a batch: kept feature maps on a common canvas with padding masks')
    q.add_argument('--pad-waste', type=float, default=None, metavar='R',
                   help=f'with --pad: close a batch before its canvas area exceeds R times its pairs\' own area (default {DEFAULT_PAD_WASTE})')
    q.add_argument('--keypoints', metavar='DIR', default=None,
                   help='consolidate the matches for SfM: names.txt, keypoints.npz (one keypoint list per image) and matches.npz (every match as '
                        'two keypoint indices) under DIR')
    q.add_argument('--sc-thres', type=float, default=0.25, help='with --keypoints: matches scoring below this are dropped')
    q.add_argument('--qt-psize', type=float, default=48, help='with --keypoints: cell size of the keypoint quantisation (<= 0: merge equal points only)')
    q.add_argument('--qt-dthres', type=float, default=4, help='with --keypoints: keypoints of a cell closer than this are merged')
    q.add_argument('--no-qt-unique', dest='qt_unique', action='store_false',
                   help='with --keypoints: keep every match of a merged keypoint instead of its best one per pair')
    q.add_argument('--cameras', metavar='FILE', default=None,
                   help='one line per image: path MODEL W H params... (COLMAP\'s SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV; the '
                        'parameters refer to the original image).  The matches are undistorted on the device right after matching: every '
                        'coordinate written (--out, --keypoints, --verify) is then a pixel of the ideal pinhole camera with the same fx fy cx cy '
                        '(of the original image, also under --no-match-upscale), and --keypoints DIR also gets intrinsics.txt for `triangulate`, '
                        '`refine` and `localize-sparse`')
    q.add_argument('--verify', action='store_true',
                   help='verify every pair geometrically (fundamental-matrix RANSAC on the device, no intrinsics needed): each .npz of --out gains '
                        'F, inliers and verified; with --keypoints only the inliers of verified pairs are consolidated and two_view.npz is written')
    q.add_argument('--verify-thr', type=float, default=1.0, help='with --verify: inlier threshold, Sampson distance in pixels')
    q.add_argument('--min-inliers', type=int, default=15, help='with --verify: a pair with fewer inliers is not verified')
    q.add_argument('--verify-refit', type=int, nargs='?', const=4, default=0, metavar='R',
                   help='with --verify: refit every pair\'s model on its inliers up to R times (1 .. 8; the bare flag: 4) and select the inliers '
                        'again; each .npz of --out and two_view.npz gain refit_rounds')
    q.add_argument('--verify-pose', action='store_true',
                   help='verify every pair with known intrinsics (essential-matrix RANSAC with pose recovery on the device; needs --intrinsics or '
                        '--cameras, not with --verify; reuses --verify-thr, --min-inliers and --verify-refit): each .npz of --out gains E, R, t, '
                        'inliers and verified; with --keypoints only the inliers of verified pairs are consolidated and two_view.npz holds the poses')
    q.add_argument('--intrinsics', metavar='FILE', default=None, help='with --verify-pose: one line per image: path fx fy cx cy')
    loc = sub.add_parser('localize', help='camera poses of query images from their matches against database images with 3-D maps')
    loc.add_argument('list', help='text file with `query database` image paths per line (relative paths: relative to the file)')
    loc.add_argument('--xyz', metavar='DIR', required=True,
                     help="the 3-D map of a database image: DIR/<its path relative to the list>.npy, float32 [H, W, 3] in the coordinates of "
                          'its keypoints (the original image unless --no-match-upscale), NaN where a pixel has no 3-D point')
    cam = loc.add_mutually_exclusive_group(required=True)
    cam.add_argument('--intrinsics', metavar='FILE', default=None, help='one line per query: path fx fy cx cy')
    cam.add_argument('--cameras', metavar='FILE', default=None,
                     help='instead of --intrinsics: one line per image, queries and database images alike: path MODEL W H params... (as `pairs '
                          '--cameras`).  The matches are undistorted on the device right after matching; the 3-D maps are then looked up at '
                          'ideal-pinhole coordinates of the database images')
    loc.add_argument('--out', default=None, help='file with one line per localised query: path qw qx qy qz tx ty tz (x_cam = R X + t)')
    loc.add_argument('--thr', type=float, default=12.0, help='inlier threshold, reprojection error in pixels')
    loc.add_argument('--min-inliers', type=int, default=12, help='a query with fewer inliers is not localised')
    loc.add_argument('--sc-thres', type=float, default=0.25, help='matches scoring below this take no part')
    loc.add_argument('--refit', type=int, nargs='?', const=4, default=0, metavar='R',
                     help='refit every pose on its inliers up to R times (1 .. 8; the bare flag: 4) and select the inliers again')
    loc.add_argument('--batch', type=int, default=8, help='pairs of equal shapes matched per model call')
    loc.add_argument('--imsize', type=int, default=640)
    loc.add_argument('--no-match-upscale', action='store_true')
    loc.add_argument('--pad', action='store_true', help='let pairs of unequal shapes share a batch (as `pairs --pad`)')
    loc.add_argument('--pad-waste', type=float, default=None, metavar='R', help='with --pad: as `pairs --pad-waste`')
    tri = sub.add_parser('triangulate', help='3-D points for the tracks of a consolidated match directory from known camera poses')
    tri.add_argument('keypoints', metavar='KEYPOINTS_DIR', help='what `pairs --keypoints DIR` wrote: names.txt, keypoints.npz, matches.npz')
    tri.add_argument('--poses', metavar='FILE', required=True,
                     help='one line per database image: path qw qx qy qz tx ty tz (x_cam = R X + t; what `localize --out` writes); images '
                          'without a line take no part')
    tri.add_argument('--intrinsics', metavar='FILE', required=True, help='one line per image with a pose: path fx fy cx cy')
    tri.add_argument('--out', metavar='FILE.npz', default=None,
                     help='points, errors, obs_offsets, obs_image, obs_keypoint, point_of_keypoint (all images, concatenated in the order of '
                          'names.txt) and kp_offsets')
    tri.add_argument('--thr', type=float, default=4.0, help='inlier threshold, reprojection error in pixels')
    tri.add_argument('--min-angle', type=float, default=1.5, help='smallest triangulation angle of a hypothesis pair, in degrees')
    tri.add_argument('--min-obs', type=int, default=2, help='a track with fewer inlier observations gets no point (at least 2)')
    tri.add_argument('--refit', type=int, nargs='?', const=4, default=2, metavar='R',
                     help='refit every point on its inliers up to R times (0 .. 8; the bare flag: 4; default 2) and select the inliers again')
    tri.add_argument('--device', default='cuda')
    ls = sub.add_parser('localize-sparse', help='camera poses of query images against triangulated points, from the files of `pairs --keypoints` '
                                                'and `triangulate --out` (no model)')
    ls.add_argument('keypoints', metavar='KEYPOINTS_DIR', help='what `pairs --keypoints DIR` wrote, over database and query images')
    ls.add_argument('--points', metavar='FILE.npz', required=True, help='what `triangulate --out` wrote for the same KEYPOINTS_DIR')
    ls.add_argument('--queries', metavar='FILE', required=True, help='one query image name per line (as in names.txt, or relative to FILE)')
    ls.add_argument('--intrinsics', metavar='FILE', required=True, help='one line per query: path fx fy cx cy')
    ls.add_argument('--covis-cluster', action='store_true',
                    help="split every query's database images into covisibility clusters, one pose per cluster, the one with the most inliers wins")
    ls.add_argument('--dedup', action='store_true', help='count every (query keypoint, 3-D point) once per problem')
    ls.add_argument('--thr', type=float, default=12.0, help='inlier threshold, reprojection error in pixels')
    ls.add_argument('--min-inliers', type=int, default=12, help='a query with fewer inliers is not localised')
    ls.add_argument('--refit', type=int, nargs='?', const=4, default=0, metavar='R',
                    help='refit every pose on its inliers up to R times (1 .. 8; the bare flag: 4) and select the inliers again')
    ls.add_argument('--out', default=None, help='file with one line per localised query: path qw qx qy qz tx ty tz (x_cam = R X + t)')
    ls.add_argument('--device', default='cuda')
    rf = sub.add_parser('refine', help='bundle adjustment: refine the poses and the points of `triangulate --out` jointly (no model)')
    rf.add_argument('keypoints', metavar='KEYPOINTS_DIR', help='what `pairs --keypoints DIR` wrote')
    rf.add_argument('--points', metavar='PTS.npz', required=True, help='what `triangulate --out` wrote for the same KEYPOINTS_DIR')
    rf.add_argument('--poses', metavar='FILE', required=True, help='the poses the points were triangulated from: path qw qx qy qz tx ty tz')
    rf.add_argument('--intrinsics', metavar='FILE', required=True, help='one line per image with a pose: path fx fy cx cy')
    rf.add_argument('--fixed', metavar='FILE', default=None, help='one image name per line: poses that are trusted and do not move')
    rf.add_argument('--iters', type=int, default=16, help='Levenberg-Marquardt iterations per threshold (1 .. 64)')
    rf.add_argument('--thr', default='4.0', metavar='T[,T...]',
                    help='truncation of the reprojection error in pixels; several values, e.g. 20,8,4: one run per value, coarse to fine')
    rf.add_argument('--min-obs', type=int, default=2, help='a point with fewer inlier observations at the end is dropped (at least 2)')
    rf.add_argument('--out', metavar='PTS2.npz', required=True, help='the refined points, in the format of `triangulate --out`')
    rf.add_argument('--out-poses', metavar='FILE2', required=True, help='all poses, the free ones refined, in the format of --poses')
    rf.add_argument('--device', default='cuda')
    rf.add_argument('--solver', choices=('dense', 'pcg'), default='dense',
                    help='the reduced camera system: dense Cholesky (at most 128 free images) or matrix-free preconditioned conjugate '
                         'gradients (at most 65536)')
    rf.add_argument('--cg-iters', type=int, default=64, help='--solver pcg: the cap of CG iterations per iteration (1 .. 256)')
    rf.add_argument('--cg-tol', type=float, default=1e-6, help='--solver pcg: the relative tolerance at which CG stops, in [0, 1)')
    for p in (h, q, loc):
        p.add_argument('--cache-gb', type=float, default=None,
                       help='byte budget of the feature store in GB: least recently used images are dropped and extracted again when '
                            'needed (default: unbounded for `pairs`, 2 for `hpatches --reuse-features`)')
    for p in (m, h, q, loc):
        p.add_argument('--ckpt', default=None)
        p.add_argument('--match-threshold', type=float, default=0.2)
        p.add_argument('--precision', choices=PRECISIONS, default='fp16',
                       help="fp16 / bf16 = the fast modes (16-bit storage, fp32 accumulation; bf16 = BASELINE configs[1]'s wording); "
                            "bf16_fp16 = bf16 backbone, matching path in fp16 storage (the position-encoding and fine-window kernels "
                            "convert the backbone's maps as they read them; 260-pair outcome protocol against the fp32 oracle: dAUC@3 = -3.4e-4 +- 4.6e-4, "
                            "where fp16 has +3.4e-4 +- 4.4e-4 and bf16 -1.5e-3 +- 1.4e-3; profiles/mixed_precision_outcome_260.txt); fp32 = the reference's arithmetic")
        p.add_argument('--preprocess', choices=PREPROCESS, default='host',
                       help='where the decoded images are converted to gray, resized and normalised: numpy on the host, or one HIP kernel '
                            'per image on the device (bit-identical output)')
    return ap


def write_triangulated(path, tt: TriangulatedTracks):
    """What `triangulate --out` writes and read_triangulated reads: points, errors, obs_offsets, obs_image, obs_keypoint, point_of_keypoint
    (all images, concatenated in the order of names.txt), kp_offsets, and the counts n_tracks, n_conflict, n_rejected."""
    np.savez(path, points=tt.points, errors=tt.errors, obs_offsets=tt.obs_offsets, obs_image=tt.obs_image, obs_keypoint=tt.obs_keypoint,
             point_of_keypoint=np.concatenate(tt.point_of_keypoint) if tt.point_of_keypoint else np.zeros(0, np.int32),
             kp_offsets=np.concatenate([[0], np.cumsum([len(p) for p in tt.point_of_keypoint])]).astype(np.int32),
             n_tracks=np.int32(tt.n_tracks), n_conflict=np.int32(tt.n_conflict), n_rejected=np.int32(tt.n_rejected))


def run_localize_sparse(args):
    """The `localize-sparse` sub-command: the last link of the chain from the files the other sub-commands write.  A relative name in the
    queries and intrinsics files is looked up both as written and relative to its file, as run_triangulate does."""
    cm = read_consolidated(args.keypoints)
    tt = read_triangulated(args.points)
    if len(tt.point_of_keypoint) != len(cm.names) or any(len(p) != len(k) for p, k in zip(tt.point_of_keypoint, cm.keypoints)):
        raise SystemExit(f'localize-sparse: {args.points} was not written for the keypoints under {args.keypoints}')
    intr = read_intrinsics(args.intrinsics)
    base = os.path.dirname(os.path.abspath(args.intrinsics))
    for name in cm.names:
        full = name if os.path.isabs(name) else os.path.normpath(os.path.join(base, name))
        if name not in intr and full in intr:
            intr[name] = intr[full]
    qbase = os.path.dirname(os.path.abspath(args.queries))
    known = {(nm if os.path.isabs(nm) else os.path.normpath(os.path.join(qbase, nm))): nm for nm in cm.names}
    queries = []
    with open(args.queries) as f:
        for line in f:
            q = line.strip()
            if not q or q.startswith('#'):
                continue
            full = q if os.path.isabs(q) else os.path.normpath(os.path.join(qbase, q))
            queries.append(q if q in cm.names else known.get(full, q))
    lq = localize_queries_sparse(cm, tt, queries, intr, args.thr, args.min_inliers, refit=args.refit, device=args.device,
                                 covis_cluster=args.covis_cluster, dedup=args.dedup)
    if args.out:
        with open(args.out, 'w') as f:
            for k, name in enumerate(lq.names):
                if lq.localized[k]:
                    f.write(' '.join([name] + [repr(float(v)) for v in (*rotation_to_quaternion(lq.R[k]), *lq.t[k])]) + '\n')
    print(f'{int(lq.localized.sum())} of {len(lq.names)} queries localised against {len(tt.points)} points (thr {args.thr} px, at least '
          f'{args.min_inliers} inliers' + (', covisibility clusters' if args.covis_cluster else '') + (', unique rows' if args.dedup else '') + ')'
          + (f'; {int((lq.n_clusters > 1).sum())} queries with more than one cluster' if args.covis_cluster else '')
          + (f'; the refit on the inliers (up to {args.refit} rounds) changed {int((lq.rounds > 0).sum())} queries' if args.refit else '')
          + (f' -> {args.out}' if args.out else ''))
    return lq


def _named_tables(cm, *tables):
    """a relative name in a poses, intrinsics or names file is looked up both as written and relative to its file"""
    for table, path in tables:
        base = os.path.dirname(os.path.abspath(path))
        for name in cm.names:
            full = name if os.path.isabs(name) else os.path.normpath(os.path.join(base, name))
            if name not in table and full in table:
                table[name] = table[full]


def run_refine(args):
    """The `refine` sub-command: between `triangulate` and `localize-sparse` (or a second `triangulate`), from and to their files.  The
    poses file it writes names the images as names.txt does."""
    cm = read_consolidated(args.keypoints)
    tt = read_triangulated(args.points)
    if len(tt.point_of_keypoint) != len(cm.names) or any(len(p) != len(k) for p, k in zip(tt.point_of_keypoint, cm.keypoints)):
        raise SystemExit(f'refine: {args.points} was not written for the keypoints under {args.keypoints}')
    poses, intr = read_poses(args.poses), read_intrinsics(args.intrinsics)
    _named_tables(cm, (poses, args.poses), (intr, args.intrinsics))
    fixed = []
    if args.fixed:
        fbase = os.path.dirname(os.path.abspath(args.fixed))
        known = {(nm if os.path.isabs(nm) else os.path.normpath(os.path.join(fbase, nm))): nm for nm in cm.names}
        with open(args.fixed) as f:
            for line in f:
                q = line.strip()
                if q and not q.startswith('#'):
                    fixed.append(q if q in cm.names else known.get(q if os.path.isabs(q) else os.path.normpath(os.path.join(fbase, q)), q))
    rs = refine(cm, tt, intr, {nm: poses[nm] for nm in cm.names if nm in poses}, fixed, args.iters, args.thr, args.min_obs, device=args.device,
                solver=args.solver, cg_iters=args.cg_iters, cg_tol=args.cg_tol)
    write_triangulated(args.out, rs.tracks)
    write_poses(args.out_poses, rs.poses)
    print(f'{rs.n_free} free and {len(rs.poses) - rs.n_free} fixed images, {len(tt.points)} points, {len(tt.obs_image)} observations: cost '
          f'{float(rs.cost[0]) if len(rs.cost) else 0.0:.6g} -> {float(rs.cost[-1]) if len(rs.cost) else 0.0:.6g} in {int(rs.accepted.sum())} '
          f'accepted of {len(rs.accepted)} iterations (thr {",".join(repr(x) for x in args.thr)} px); {len(rs.tracks.points)} points and '
          f'{len(rs.tracks.obs_image)} observations kept, median reprojection error '
          f'{float(np.median(rs.tracks.errors)) if len(rs.tracks.errors) else 0.0:.3f} px -> {args.out}, {args.out_poses}')
    return rs


def run_triangulate(args):
    """The `triangulate` sub-command: names.txt lists the images as the pair list named them, so a relative name in the poses and
    intrinsics files is looked up both as written and relative to its file."""
    cm = read_consolidated(args.keypoints)
    poses, intr = read_poses(args.poses), read_intrinsics(args.intrinsics)
    for table, path in ((poses, args.poses), (intr, args.intrinsics)):
        base = os.path.dirname(os.path.abspath(path))
        for name in cm.names:
            full = name if os.path.isabs(name) else os.path.normpath(os.path.join(base, name))
            if name not in table and full in table:
                table[name] = table[full]
    tt = triangulate(cm, intr, poses, args.thr, args.min_angle, args.min_obs, args.refit, device=args.device)
    if args.out:
        write_triangulated(args.out, tt)
    print(f'{len(tt.points)} points from {tt.n_tracks} tracks of {sum(n in poses for n in cm.names)} posed images ({tt.n_conflict} with an image '
          f'twice, {tt.n_rejected} without a point; thr {args.thr} px, angle >= {args.min_angle} deg, at least {args.min_obs} observations, up '
          f'to {args.refit} refits); {len(tt.obs_image)} observations, median reprojection error '
          f'{float(np.median(tt.errors)) if len(tt.errors) else 0.0:.3f} px' + (f' -> {args.out}' if args.out else ''))
    return tt


def _cameras_for(path, pairs):
    """read_cameras(path) keyed by the image names of `pairs`: a name is looked up as the pair list has it, then as an absolute path."""
    cams = read_cameras(path)
    out = {}
    for name in {n for p in pairs for n in p}:
        full = os.path.abspath(name)
        if name not in cams and full not in cams:
            raise SystemExit(f'{path}: no camera for {name!r}')
        out[name] = cams[name] if name in cams else cams[full]
    return out


def _intrinsics_for(path, pairs):
    """read_intrinsics(path) keyed by the image names of `pairs`: a name is looked up as the pair list has it, then as an absolute path."""
    intr = read_intrinsics(path)
    out = {}
    for name in {n for p in pairs for n in p}:
        full = os.path.abspath(name)
        if name not in intr and full not in intr:
            raise SystemExit(f'{path}: no intrinsics for {name!r}')
        out[name] = intr[name] if name in intr else intr[full]
    return out


def main(argv=None):
    """`python -m geoformer_amd.matcher match|hpatches|pairs|localize|triangulate|refine|localize-sparse ...` (arguments: build_parser)."""
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.cmd == 'triangulate':                                       # no model: keypoints, matches and poses in, points out
        if args.min_obs < 2 or not 0 <= args.refit <= 8 or not args.thr > 0:
            ap.error('triangulate: need --min-obs >= 2, --refit 0 .. 8 and --thr > 0')
        run_triangulate(args)
        return
    if args.cmd == 'refine':                                            # no model: keypoints, points and poses in, points and poses out
        try:
            args.thr = tuple(float(x) for x in str(args.thr).split(','))
        except ValueError:
            ap.error('refine: --thr takes numbers separated by commas')
        if not 1 <= args.iters <= 64 or args.min_obs < 2 or not all(x > 0 for x in args.thr):
            ap.error('refine: need --iters 1 .. 64, --min-obs >= 2 and --thr > 0')
        if args.solver == 'pcg' and not (1 <= args.cg_iters <= 256 and 0.0 <= args.cg_tol < 1.0):
            ap.error('refine: need --cg-iters 1 .. 256 and 0 <= --cg-tol < 1')
        run_refine(args)
        return
    if args.cmd == 'localize-sparse':                                   # no model either: keypoints, matches and points in, poses out
        if not 0 <= args.refit <= 8 or not args.thr > 0:
            ap.error('localize-sparse: need --refit 0 .. 8 and --thr > 0')
        run_localize_sparse(args)
        return
    if args.cmd == 'pairs' and args.verify_pose:
        if args.verify:
            ap.error('pairs: --verify-pose may not be combined with --verify')
        if (args.intrinsics is None) == (args.cameras is None):
            ap.error('pairs: --verify-pose needs --intrinsics FILE or --cameras FILE (one of them)')
        if not 0 <= args.verify_refit <= 8 or not args.verify_thr > 0:
            ap.error('pairs: --verify-pose needs --verify-refit 0 .. 8 and --verify-thr > 0')
    world = int(os.environ.get('WORLD_SIZE', '1'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if world > 1:
        torch.cuda.set_device(local)
        torch.distributed.init_process_group('nccl', device_id=torch.device('cuda', local))
    if args.cmd == 'pairs' and (args.list is None) == (args.all_pairs is None):
        raise SystemExit('pairs: give either a pair list or --all-pairs DIR')
    cache_gb = getattr(args, 'cache_gb', None)
    if args.cmd == 'hpatches' and args.reuse_features and cache_gb is None:
        cache_gb = 2.0             # only image 1 of the current sequence is ever asked for again: no reason to keep the whole dataset
    matcher = GeoFormerMatcher(args.imsize, args.match_threshold, args.no_match_upscale, args.ckpt, device=f'cuda:{local}',
                               precision=args.precision, preprocess=args.preprocess,
                               cache_bytes=None if cache_gb is None else int(cache_gb * 2 ** 30))
    if args.cmd == 'pairs':
        pairs = read_pair_list(args.list) if args.list is not None else all_pairs(args.all_pairs)
        results = matcher.match_many(pairs, batch=args.batch, pad=args.pad, max_waste=args.pad_waste)
        intr = None
        if args.cameras:
            results, intr = undistort_results(pairs, results, _cameras_for(args.cameras, pairs), device=matcher.device)
            print(f'{args.cameras}: {sum(len(r[0]) for r in results)} matches undistorted, {int(results.n_failed.sum())} with a side beyond its '
                  f"camera model's range (dropped downstream)")
        vm = (verify_matches(pairs, results, args.verify_thr, args.min_inliers, args.sc_thres, device=matcher.device, refit=args.verify_refit)
              if args.verify else None)
        if args.verify_pose:
            vm = relative_poses(pairs, results, intr if intr is not None else _intrinsics_for(args.intrinsics, pairs), args.verify_thr, args.min_inliers, args.sc_thres, device=matcher.device, refit=args.verify_refit)
        refit = {} if vm is None or not args.verify_refit else {'refit_rounds': vm.rounds}
        model = {} if vm is None else {'E': vm.E, 'R': vm.R, 't': vm.t} if args.verify_pose else {'F': vm.F}
        if args.out:
            os.makedirs(args.out, exist_ok=True)
        for k, ((p0, p1), res) in enumerate(zip(pairs, results)):
            if args.out:
                stem = '_'.join(os.path.splitext(os.path.basename(p))[0] for p in (p0, p1))
                extra = {} if vm is None else {**{q: v[k] for q, v in model.items()}, 'inliers': vm.masks[k], 'verified': vm.verified[k],
                                               **{q: v[k] for q, v in refit.items()}}
                np.savez(os.path.join(args.out, f'{k:05d}_{stem}.npz'), matches=res[0], kpts1=res[1], kpts2=res[2], scores=res[3], **extra)
        if vm is not None:
            print(f'{int(vm.verified.sum())} of {len(pairs)} pairs verified (thr {args.verify_thr} px, at least {args.min_inliers} inliers), '
                  f'{sum(int(m.sum()) for m in vm.masks)} inlier matches'
                  + (f'; the refit on the inliers (up to {args.verify_refit} rounds) changed {int((vm.rounds > 0).sum())} pairs' if refit else ''))
        if args.keypoints:
            cm = consolidate_matches(pairs, results, args.sc_thres, args.qt_psize, args.qt_dthres, args.qt_unique, device=matcher.device,
                                     keep=None if vm is None else vm.masks)
            write_consolidated(args.keypoints, cm)
            if intr is not None:
                write_intrinsics(os.path.join(args.keypoints, 'intrinsics.txt'), intr, cm.names)
            if vm is not None:
                np.savez(os.path.join(args.keypoints, 'two_view.npz'), pairs=cm.pair_images, **model, n_inliers=vm.n_inliers, verified=vm.verified,
                         **refit)
            print(f'{len(cm.names)} images, {sum(len(k) for k in cm.keypoints)} keypoints, {sum(len(m) for m in cm.matches)} matches as keypoint '
                  f'indices -> {args.keypoints}')
        st = matcher.store
        print(f'{matcher.name}: {len(pairs)} pairs, {sum(len(r[0]) for r in results)} matches, {st.extractions} extractions, {st.hits} store hits')
    elif args.cmd == 'localize':
        pairs = read_pair_list(args.list)
        base = os.path.dirname(os.path.abspath(args.list))
        results = matcher.match_many(pairs, batch=args.batch, pad=args.pad, max_waste=args.pad_waste)
        xyz = {d: os.path.join(args.xyz, os.path.relpath(d, base) + '.npy') for _, d in pairs}
        if args.cameras:
            results, intr = undistort_results(pairs, results, _cameras_for(args.cameras, pairs), device=matcher.device)
        else:
            intr = read_intrinsics(args.intrinsics)
        lq = localize_queries(pairs, results, intr, xyz, args.thr, args.min_inliers, args.sc_thres,
                              device=matcher.device, refit=args.refit)
        if args.out:
            with open(args.out, 'w') as f:
                for k, name in enumerate(lq.names):
                    if lq.localized[k]:
                        f.write(' '.join([os.path.relpath(name, base)] + [repr(float(v)) for v in (*rotation_to_quaternion(lq.R[k]), *lq.t[k])]) + '\n')
        print(f'{int(lq.localized.sum())} of {len(lq.names)} queries localised (thr {args.thr} px, at least {args.min_inliers} inliers) from '
              f'{len(pairs)} pairs'
              + (f'; the refit on the inliers (up to {args.refit} rounds) changed {int((lq.rounds > 0).sum())} queries' if args.refit else ''))
    elif args.cmd == 'match':
        res = matcher(args.im1, args.im2)
        print(f'{matcher.name}: {len(res[0])} matches')
        if args.out:
            np.savez(args.out, matches=res[0], kpts1=res[1], kpts2=res[2], scores=res[3])
    else:
        quiet = int(os.environ.get('RANK', '0')) != 0
        out = eval_hpatches(matcher, args.root, ransac_thres=args.ransac_thres, max_seqs=args.max_seqs,
                            scale_H=matcher.no_match_upscale, log=(lambda s: None) if quiet else print, reuse_features=args.reuse_features)
        if not quiet and args.reuse_features:
            print(f'feature store: {matcher.store.extractions} extractions, {matcher.store.hits} hits')
        if not quiet:
            print({k: (v.tolist() if hasattr(v, 'tolist') else v) for k, v in out.items()})
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
