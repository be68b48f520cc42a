"""Homography training pairs from a directory of images: the counterpart of homodataset/HomoDataset.py (the dataset of
lightning/train_homo_geoformer.py) with the per-pixel work on the device.

For every sample the reference decodes the image to gray, draws a random perspective matrix, runs cv2.warpPerspective at full
resolution, resizes both images to the training size, applies photometric augmentation and moves the homography into resized
coordinates.  Here:

  * the geometry is restated in numpy fp64: `sample_homography` (utils/homography.py:352-386), `get_translation_mat`,
    `get_perspective_mat`, `scale_homography` (utils/preprocess_utils.py:23-52, :96-105), the target-size rule of `get_pair`
    (HomoDataset.py:98-109) and the rank slice (:40-45).  cv2.getPerspectiveTransform is the 8x8 solve, cv2.perspectiveTransform a
    homogeneous multiply.  The reference's quirks are kept as written: `get_perspective_mat` is CALLED with (ratio, width, height,
    trans) against a signature of (ratio, image_height, image_width, trans); the flip matrices use w / h, not w - 1 / h - 1; a
    singular matrix is drawn again; the two images are swapped with probability 0.5 and the homography inverted.  The reference
    rounds the matrix to fp32 on the way (torch .float()); here it stays fp64 until the batch tensors are written, and the
    inverses of the labels are taken in fp64 before that rounding.
  * the pictures: `preprocess='host'` runs the whole pipeline in numpy - `cv2_warp_perspective_u8`, a line-for-line restatement of
    csrc/warp_spec.h (OpenCV's 8-bit warpPerspective path; its one stated deviation from OpenCV is there), then
    matcher.cv2_resize_linear_u8 and `brightness_contrast_u8`; `preprocess='device'` uploads the decoded bytes through the pinned
    staging buffers of the matcher (one slot per image of the batch) and runs ONE launch per image of the pair
    (ops.image_warp_resize: gray, warp, resize, brightness / contrast, / 255) straight into the batch tensors.  The two give the
    same bits.  The swap is a choice of destination tensor, not a copy.
  * augmentation: the reference's aug_func is albumentations Compose(p=0.65) of OneOf([RandomBrightness(0.2, p=0.8),
    RandomContrast(0.3, p=0.6)], p=0.5) and OneOf([MotionBlur, GaussNoise], p=0.5).  The FIRST group is built, as a per-image
    (alpha, beta) with the reference's probabilities (pipeline 0.65, group 0.5, brightness : contrast = 0.8 : 0.6) and
    albumentations' uint8 look-up-table rule.  MotionBlur and GaussNoise are NOT built: they need a device random generator and a
    second pass over the image, and nothing available offline can pin them.
  * randomness: every draw of sample i in epoch e comes from one numpy.random.Generator keyed by (seed, e, i's position in the
    SORTED file list of the whole directory), so a sample is the same on every rank, worker and preprocess mode.  The distributions
    are the reference's; the stream is ours (the reference draws from the global `random` / `np.random` state in os.walk order).
  * `valid_mask_left` / `valid_mask_right` are NOT produced: nothing in the reference's training path reads them, and they need
    kornia's warp.  Negative pairs (`is_negs`) never occur in the reference either (its probability is 0.); the key is kept.
"""
import os

import numpy as np
import torch

from .. import matcher

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
EXTENSIONS = ('.jpg', '.ppm')
PATCH_RATIO, TRANSLATION = 0.8, 0.2              # HomoDataset.py:66-69 augmentation_params
P_PIPELINE, P_GROUP = 0.65, 0.5                  # alb.Compose(p=0.65), alb.OneOf(p=0.5)
W_BRIGHTNESS, W_CONTRAST = 0.8, 0.6              # OneOf weights: the transforms' own p
BRIGHTNESS_LIMIT, CONTRAST_LIMIT = 0.2, 0.3


# ---------------------------------------------------------------------------------------------
# pixels: csrc/warp_spec.h in numpy
# ---------------------------------------------------------------------------------------------
def warp_positions(minv, w, h):
    """ws_position for every destination pixel: (X, Y) int64 [h, w], the source position in 1/32 pixels."""
    m = np.asarray(minv, dtype=np.float64).reshape(9)
    x = np.arange(w, dtype=np.float64)[None, :]
    y = np.arange(h, dtype=np.float64)[:, None]
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        W = m[6] * x + m[7] * y + m[8]
        W = np.where(W != 0.0, 32.0 / W, 0.0)
        fX = (m[0] * x + m[1] * y + m[2]) * W
        fY = (m[3] * x + m[4] * y + m[5]) * W
        fX = np.where(fX < float(INT_MAX), fX, float(INT_MAX))          # std::min: a NaN lands on INT_MAX
        fX = np.where(float(INT_MIN) < fX, fX, float(INT_MIN))
        fY = np.where(fY < float(INT_MAX), fY, float(INT_MAX))
        fY = np.where(float(INT_MIN) < fY, fY, float(INT_MIN))
    return np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64)      # lrint: round half to even


def cv2_warp_perspective_u8(src, M, w, h):
    """cv2.warpPerspective(src, M, (w, h)) for a single-channel uint8 image with the defaults HomoDataset.py:96 uses (INTER_LINEAR,
    BORDER_CONSTANT 0, forward M): csrc/warp_spec.h line for line.  Minv = inv(M) in fp64; positions rounded to 1/32 pixel (half to
    even), negative positions floor; dst = ((32-ax)(32-ay) p00 + ax (32-ay) p01 + (32-ax) ay p10 + ax ay p11 + 512) >> 10 with a tap
    outside the source counting 0, each tap tested on its own."""
    src = np.ascontiguousarray(src, dtype=np.uint8)
    hs, ws = src.shape
    X, Y = warp_positions(np.linalg.inv(np.asarray(M, dtype=np.float64)), w, h)
    sx, ax, sy, ay = X >> 5, X & 31, Y >> 5, Y & 31
    t = src.astype(np.int64)

    def tap(cx, cy):
        inside = (cx >= 0) & (cx < ws) & (cy >= 0) & (cy < hs)
        return np.where(inside, t[np.clip(cy, 0, hs - 1), np.clip(cx, 0, ws - 1)], 0)
    bx, by = 32 - ax, 32 - ay
    out = (bx * by * tap(sx, sy) + ax * by * tap(sx + 1, sy) + bx * ay * tap(sx, sy + 1) + ax * ay * tap(sx + 1, sy + 1) + 512) >> 10
    return out.astype(np.uint8)


def brightness_contrast_u8(img, alpha, beta):
    """albumentations' uint8 look-up-table rule (RandomBrightness / RandomContrast): v -> clip(trunc(fp32(v) * alpha + beta * 255), 0, 255),
    every operation in fp32 (ws_brightness_contrast of csrc/warp_spec.h)."""
    a, b255 = np.float32(alpha), np.float32(beta) * np.float32(255)
    t = np.trunc(np.asarray(img).astype(np.float32) * a + b255)
    return np.clip(t, 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------
# geometry: utils/homography.py, utils/preprocess_utils.py in numpy fp64, draws from an explicit Generator
# ---------------------------------------------------------------------------------------------
def get_perspective_transform(src, dst):
    """cv2.getPerspectiveTransform: the 3x3 matrix (last entry 1) that maps four points onto four points, by the 8x8 solve."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    A, b = np.zeros((8, 8)), np.zeros(8)
    for k in range(4):
        (x, y), (u, v) = src[k], dst[k]
        A[k] = [x, y, 1, 0, 0, 0, -x * u, -y * u]
        A[k + 4] = [0, 0, 0, x, y, 1, -x * v, -y * v]
        b[k], b[k + 4] = u, v
    return np.append(np.linalg.solve(A, b), 1.0).reshape(3, 3)


def perspective_transform(pts, M):
    """cv2.perspectiveTransform: [n,2] points through the homography M (w == 0 gives 0, as OpenCV does)."""
    p = np.concatenate([np.asarray(pts, dtype=np.float64), np.ones((len(pts), 1))], axis=1) @ np.asarray(M, dtype=np.float64).T
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(p[:, 2:] != 0.0, p[:, :2] / p[:, 2:], 0.0)


def flip_matrices(h, w):
    """theta_flips of sample_homography: horizontal and vertical flip, with w / h where a pixel-exact flip would have w - 1 / h - 1."""
    return [np.array([[-1., 0., w], [0., 1., 0.], [0., 0., 1.]]), np.array([[1., 0., 0.], [0., -1., h], [0., 0., 1.]])]


def sample_homography(shape, rng):
    """utils/homography.py:352-386: the four corners of an (h, w) frame moved by integers from [-max(h,w)//3, max(h,w)//3) (with
    probability 0.2 from [-5, 5) instead); with probability 0.2 a flip REPLACES the matrix (0.6) or is applied first (0.4)."""
    h, w = shape
    corners = np.array([[0, 0], [0, h], [w, 0], [w, h]], dtype=np.float64)
    rg = max(h, w)
    warp = rng.integers(-rg // 3, rg // 3, size=(4, 2)).astype(np.float64)
    if rng.random() < 0.2:
        warp = rng.integers(-5, 5, size=(4, 2)).astype(np.float64)
    H = get_perspective_transform(corners, corners + warp)
    if rng.random() < 0.2:
        flip = flip_matrices(h, w)[int(rng.integers(0, 2))]
        H = flip if rng.random() < 0.6 else H @ flip
    return H


def get_translation_mat(image_height, image_width, trans, transformed_corners, rng):
    """utils/preprocess_utils.py:23-39."""
    left_top_min = np.min(transformed_corners, axis=0)
    right_bottom_min = np.min(np.array([image_width, image_height]) - transformed_corners, axis=0)
    trans_x_value = int(rng.uniform(0, trans) * image_width)
    trans_y_value = int(rng.uniform(0, trans) * image_height)
    if rng.uniform() > 0.5:            # translate x with respect to the left axis
        trans_x = trans_x_value if left_top_min[0] < 0 else -trans_x_value
    else:                              # ... the right axis
        trans_x = trans_x_value if right_bottom_min[0] > 0 else -trans_x_value
    if rng.uniform() > 0.5:            # translate y with respect to the top axis
        trans_y = trans_y_value if left_top_min[1] < 0 else -trans_y_value
    else:                              # ... the bottom axis
        trans_y = trans_y_value if right_bottom_min[1] > 0 else -trans_y_value
    T = np.eye(3)
    T[0, 2], T[1, 2] = trans_x, trans_y
    return T


def get_perspective_mat(patch_ratio, image_height, image_width, trans, rng):
    """utils/preprocess_utils.py:41-52, signature as there.  (HomoDataset.get_pair passes width for image_height and height for
    image_width; `HomoPairs` does the same.)"""
    patch_ratio = 1 - rng.random() * (1 - patch_ratio)
    pw, ph = int(patch_ratio * image_width), int(patch_ratio * image_height)
    patch_corners = np.array([[0, 0], [0, ph], [pw, ph], [pw, 0]], dtype=np.float64)
    H = sample_homography((image_height, image_width), rng)
    T = get_translation_mat(image_height, image_width, trans, perspective_transform(patch_corners, H), rng)
    return T @ H


def scale_homography(homo_matrix, src_height, src_width, dest_height, dest_width):
    """utils/preprocess_utils.py:96-105: the homography between the two images after both were resized."""
    S = np.diag([dest_width / src_width, dest_height / src_height, 1.0])
    return S @ np.asarray(homo_matrix, dtype=np.float64) @ np.linalg.inv(S)


def target_size(height, width, size, st):
    """(wt, ht) of get_pair (HomoDataset.py:98-109) for a source of height x width."""
    if st == 0:
        return (size[1], size[0]) if height > width else (size[0], size[1])
    if height > width:
        ht = size[0]
        return int((ht / height * width) // st * st), ht
    wt = size[1]
    return wt, int((wt / width * height) // st * st)


def list_images(img_dir):
    """Every .jpg / .ppm under img_dir (HomoDataset.py:28-37), SORTED: the reference takes os.walk order, sorting is our determinism."""
    out = []
    for cur, _, files in os.walk(img_dir):
        out += [os.path.join(cur, f) for f in files if f.endswith(EXTENSIONS)]
    return sorted(out)


def rank_slice(n, rank, world_size):
    """(start, end) of rank's share of n files (HomoDataset.py:40-45): len // world each, the remainder dropped."""
    if world_size is None:
        return 0, n
    bz = int(n // world_size)
    start = rank * bz
    return start, (start + bz if start + bz < n else n)


def sample_augment(rng):
    """One image's draw through aug_func: None, (1, beta) for RandomBrightness(0.2) or (alpha, 0) for RandomContrast(0.3)."""
    if not rng.random() < P_PIPELINE:
        return None
    if not rng.random() < P_GROUP:
        return None
    if rng.random() < W_BRIGHTNESS / (W_BRIGHTNESS + W_CONTRAST):
        return 1.0, float(np.float32(rng.uniform(-BRIGHTNESS_LIMIT, BRIGHTNESS_LIMIT)))
    return float(np.float32(1.0 + rng.uniform(-CONTRAST_LIMIT, CONTRAST_LIMIT))), 0.0


def sample_rng(seed, epoch, index):
    return np.random.default_rng([int(seed), int(epoch), int(index)])


class HomoPairs:
    def __init__(self, img_dir, size=(640, 480), st=32, rank=0, world_size=None, seed=0, device='cuda', preprocess='device', augment=True):
        """size, st, rank, world_size: HomoDataset's arguments (world_size is its `word_size`).  seed keys every draw; device is where
        the batch tensors live; preprocess 'device' (one HIP launch per image) or 'host' (numpy, same bits); augment=False switches
        the brightness / contrast draws off (they are still drawn, so the geometry of a sample does not depend on it)."""
        if preprocess not in matcher.PREPROCESS:
            raise ValueError(f'preprocess must be one of {matcher.PREPROCESS}, got {preprocess!r}')
        self.device = torch.device(device)
        if preprocess == 'device' and self.device.type != 'cuda':
            raise ValueError(f"preprocess='device' runs on the GPU: it needs a cuda device, got device={device!r} (use preprocess='host')")
        self.img_dir, self.size, self.st, self.seed = img_dir, tuple(size), int(st), int(seed)
        self.preprocess, self.augment = preprocess, bool(augment)
        files = list_images(img_dir)
        self.offset, end = rank_slice(len(files), rank, world_size)
        self.data = files[self.offset:end]
        self._hw = {}

    def __len__(self):
        return len(self.data)

    def source_hw(self, index):
        """(height, width) of file `index`, from its header."""
        if index not in self._hw:
            from PIL import Image
            with Image.open(self.data[index]) as im:
                self._hw[index] = (im.size[1], im.size[0])
        return self._hw[index]

    def target_hw(self, index):
        wt, ht = target_size(*self.source_hw(index), self.size, self.st)
        return ht, wt

    def sample(self, index, epoch=0):
        """Everything of sample `index` in `epoch` that is not a pixel: M (forward matrix at the source's resolution, fp64), the target
        size, the labels, the two (alpha, beta) draws and the swap."""
        height, width = self.source_hw(index)
        rng = sample_rng(self.seed, epoch, self.offset + index)
        while True:                                  # HomoDataset.py:89-95: draw again while the matrix cannot be inverted
            try:
                M = get_perspective_mat(PATCH_RATIO, width, height, TRANSLATION, rng)        # (width, height): as the reference calls it
                if np.isfinite(M).all() and np.isfinite(np.linalg.inv(M)).all():
                    break
            except np.linalg.LinAlgError:
                pass
        ht, wt = self.target_hw(index)
        aug_orig, aug_warp = sample_augment(rng), sample_augment(rng)
        if not self.augment:
            aug_orig = aug_warp = None
        swap = bool(rng.uniform(0, 1) < 0.5)
        H = scale_homography(M, height, width, ht, wt)
        H01 = np.linalg.inv(H) if swap else H
        name = os.path.split(self.data[index])[-1]
        return {'path': self.data[index], 'M': M, 'hw': (height, width), 'ht': ht, 'wt': wt, 'aug_orig': aug_orig, 'aug_warp': aug_warp,
                'swap': swap, 'H_0to1': H01.astype(np.float32), 'H_1to0': np.linalg.inv(H01).astype(np.float32),
                'pair_names': (name + '_0', name + '_1')}

    def pair_host(self, index, epoch=0):
        """The two uint8 [ht, wt] images of the sample BEFORE the swap (original, warped), all in numpy."""
        p = self.sample(index, epoch)
        gray = matcher.load_gray_image(p['path'])
        height, width = gray.shape
        out = []
        for im, aug in ((gray, p['aug_orig']), (cv2_warp_perspective_u8(gray, p['M'], width, height), p['aug_warp'])):
            im = matcher.cv2_resize_linear_u8(im, p['wt'], p['ht'])
            out.append(im if aug is None else brightness_contrast_u8(im, *aug))
        return out[0], out[1], p

    def batch(self, indices, epoch=0):
        """The dict HomoDataset.__getitem__ + the default collate give for these samples: image0, image1 [N,1,H,W] fp32 in [0,1],
        H_0to1, H_1to0 [N,3,3] fp32, pair_id int64 [N], is_negs bool [N] (tensors on `device`), dataset_name [N], pair_names (two
        lists of N names).  All samples must share one target shape (see `batches`)."""
        indices = [int(i) for i in indices]
        params = [self.sample(i, epoch) for i in indices]
        shapes = {(p['ht'], p['wt']) for p in params}
        if len(shapes) != 1:
            raise ValueError(f'HomoPairs.batch: samples {indices} have different target shapes {sorted(shapes)}; take index lists from batches()')
        (ht, wt), n, dev = next(iter(shapes)), len(indices), self.device
        images = [torch.empty(n, 1, ht, wt, dtype=torch.float32, device=dev) for _ in range(2)]
        for k, (i, p) in enumerate(zip(indices, params)):
            dst_orig, dst_warp = images[int(p['swap'])][k], images[1 - int(p['swap'])][k]            # the swap: which tensor gets which image
            if self.preprocess == 'device':
                from .. import ops
                with torch.cuda.device(dev):
                    d = matcher._staging.upload(matcher.load_image_u8(p['path']), dev, slot=k)
                    ops.image_warp_resize(d, np.eye(3), wt, ht, out=dst_orig, brightness_contrast=p['aug_orig'])
                    ops.image_warp_resize(d, p['M'], wt, ht, out=dst_warp, brightness_contrast=p['aug_warp'])
            else:
                orig, warped, _ = self.pair_host(i, epoch)
                dst_orig.copy_(torch.from_numpy(orig.astype(np.float32) / np.float32(255.0))[None])
                dst_warp.copy_(torch.from_numpy(warped.astype(np.float32) / np.float32(255.0))[None])
        return {'image0': images[0], 'image1': images[1],
                'H_0to1': torch.from_numpy(np.stack([p['H_0to1'] for p in params])).to(dev),
                'H_1to0': torch.from_numpy(np.stack([p['H_1to0'] for p in params])).to(dev),
                'is_negs': torch.zeros(n, dtype=torch.bool, device=dev), 'dataset_name': ['Oxford'] * n,
                'pair_id': torch.tensor(indices, dtype=torch.int64, device=dev),
                'pair_names': [[p['pair_names'][0] for p in params], [p['pair_names'][1] for p in params]]}

    def batches(self, batch_size, epoch=0, shuffle=True, drop_last=False):
        """Index lists of one target shape each, deterministic in (seed, epoch): the samples are walked in a seeded order (file order
        with shuffle=False), every shape fills its own bucket, a full bucket is yielded; the partial buckets follow unless drop_last."""
        order = np.arange(len(self.data))
        if shuffle:
            order = np.random.default_rng([self.seed, int(epoch), 2 ** 32 - 1, len(self.data)]).permutation(len(self.data))
        buckets = {}
        for i in order:
            b = buckets.setdefault(self.target_hw(int(i)), [])
            b.append(int(i))
            if len(b) == batch_size:
                yield list(b)
                b.clear()
        if not drop_last:
            for b in buckets.values():
                if b:
                    yield list(b)
