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

Also here: the feature store and the batching of pairs behind `match_many`, the single-problem `estimate_*` functions of the validation
metrics, and the command line (`python -m geoformer_amd.matcher ...`).  What becomes of the pair matches afterwards - consolidation,
verification, undistortion, localisation, triangulation, bundle adjustment and their file formats - is sfm.py; its names are imported
below, so `matcher.<name>` resolves for all of them.
"""
import collections
import glob
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
# the SfM library lives in sfm.py; its names stay reachable here (the command line below, the tests and the tools use them as matcher.<name>)
from .sfm import (CAMERA_MODELS, Camera, ConsolidatedMatches, LocalizedQueries, RefinedStructure, RelativePoses,  # noqa: F401
                  TriangulatedTracks, UndistortedResults, VerifiedMatches, _assemble_refined, _assemble_tracks, _covis_tables, _device_rows,
                  _localize_sparse_device, _original_pixel_rows, _refine_device, _refine_inputs, _sparse_rows, _triangulation_inputs,
                  canonical_camera, consolidate_matches, localize_queries, localize_queries_sparse, pinhole_of, quaternion_to_rotation,
                  read_cameras, read_consolidated, read_intrinsics, read_poses, read_triangulated, refine, relative_poses,
                  rotation_to_quaternion, triangulate, undistort_points, undistort_results, verify_matches, write_cameras,
                  write_consolidated, write_intrinsics, write_poses, write_triangulated)


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
