"""The homography-pair generator without a GPU (geoformer_amd/train/homo_data.py): the numpy restatement of csrc/warp_spec.h against
hand-derived vectors, exact fp64 bilinear sampling and the host build of the same header; the brightness / contrast rule; the
geometry restatements; determinism of HomoPairs; and that the labels describe the pictures."""
import os

import numpy as np
import pytest

import homo_cases as C
from geoformer_amd.train import homo_data as D

SRC = C.smooth_noisy()                       # [37, 53]


def warp(M, src=SRC):
    h, w = src.shape
    return D.cv2_warp_perspective_u8(src, M, w, h)


# ---------------------------------------------------------------------------------------------
# cv2_warp_perspective_u8: hand-derived vectors on a 37 x 53 image
# ---------------------------------------------------------------------------------------------
def test_identity_returns_the_source():
    assert np.array_equal(warp(C.M_IDENTITY), SRC)


def test_integer_translation_shifts_with_a_zero_border():
    want = np.zeros_like(SRC)
    want[:-2, 3:] = SRC[2:, :-3]            # dst(x, y) = src(x - 3, y + 2)
    assert np.array_equal(warp(C.M_SHIFT), want)


def test_half_pixel_translation_averages_neighbours_rounding_up():
    t = SRC.astype(np.int64)
    want = np.empty_like(t)
    want[:, 1:] = (t[:, :-1] + t[:, 1:] + 1) >> 1
    want[:, 0] = (t[:, 0] + 1) >> 1          # against the zero border
    assert np.array_equal(warp(C.M_HALF), want.astype(np.uint8))


def test_everything_outside_gives_zeros():
    assert not warp(C.M_OUTSIDE).any()


def test_horizon_inside_the_image():
    """Minv[7] = -0.05: W = 1 - 0.05 y is exactly 0 on row 20 and negative below.  W == 0 -> position (0, 0); no NaN-derived value."""
    h, w = SRC.shape
    minv = np.linalg.inv(C.M_HORIZON)
    assert np.array_equal(minv, C.MINV_HORIZON)
    Wd = minv[2, 0] * np.arange(w)[None, :] + minv[2, 1] * np.arange(h)[:, None] + minv[2, 2]
    assert (Wd[20] == 0).all() and (Wd[:20] > 0).all() and (Wd[21:] < 0).all()
    X, Y = D.warp_positions(minv, w, h)
    assert (X[20] == 0).all() and (Y[20] == 0).all()
    assert max(abs(X).max(), abs(Y).max()) < 2 ** 31 - 1           # no clamped (inf / NaN) position
    got = warp(C.M_HORIZON)
    assert (got[20] == SRC[0, 0]).all()
    assert np.array_equal(got[0], SRC[0])                           # row 0: W = 1, the identity
    assert not got[21:, 1:].any()                                   # below the horizon the source position is negative
    assert np.array_equal(got, C.host_warp(SRC, C.M_HORIZON, w, h))


def test_negative_positions_floor():
    """source x = 1.3 x - 4.3: destination column 3 reads at -0.4 -> X = -13, sx = -1 (floor; truncation would say 0), ax = 19."""
    h, w = SRC.shape
    X, _ = D.warp_positions(np.linalg.inv(C.M_NEGATIVE), w, h)
    assert X[0, 3] == -13 and (X[0, 3] >> 5, X[0, 3] & 31) == (-1, 19)
    got = warp(C.M_NEGATIVE)
    assert got[:, 3].any()                                          # the tap at column 0 counts, the one at -1 is the border
    assert np.array_equal(got, C.host_warp(SRC, C.M_NEGATIVE, w, h))


def test_against_exact_bilinear_sampling():
    """|u8 - exact| <= G/32 + 0.5 for pixels whose source position lies at least one pixel inside: G the image's largest neighbour
    difference; 1/64 pixel of position quantisation per axis times the slope, plus the final rounding."""
    h, w = SRC.shape
    t = SRC.astype(np.float64)
    G = max(np.abs(np.diff(t, axis=0)).max(), np.abs(np.diff(t, axis=1)).max())
    minv = np.linalg.inv(C.M_PERSPECTIVE)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    p = np.stack([x, y, np.ones_like(x)], -1) @ minv.T
    px, py = p[..., 0] / p[..., 2], p[..., 1] / p[..., 2]
    inside = (px >= 1) & (px <= w - 2) & (py >= 1) & (py <= h - 2)
    assert inside.sum() > 1000
    x0, y0 = np.floor(px[inside]).astype(int), np.floor(py[inside]).astype(int)
    fx, fy = px[inside] - x0, py[inside] - y0
    exact = (1 - fy) * ((1 - fx) * t[y0, x0] + fx * t[y0, x0 + 1]) + fy * ((1 - fx) * t[y0 + 1, x0] + fx * t[y0 + 1, x0 + 1])
    err = np.abs(warp(C.M_PERSPECTIVE).astype(np.float64)[inside] - exact).max()
    print(f'max error {err:.3f}, bound {G / 32 + 0.5:.3f}, {inside.sum()} of {h * w} pixels interior')
    assert err <= G / 32 + 0.5


def test_numpy_restatement_equals_the_host_build():
    h, w = SRC.shape
    for name, M in C.NAMED.items():
        assert np.array_equal(warp(M), C.host_warp(SRC, M, w, h)), name
    rng = np.random.default_rng(11)
    src = C.random_u8((h, w), 3)
    for k in range(20):
        M = D.get_perspective_mat(0.8, w, h, 0.2, rng)
        assert np.array_equal(D.cv2_warp_perspective_u8(src, M, w, h), C.host_warp(src, M, w, h)), k
    # another destination size than the source's
    assert np.array_equal(D.cv2_warp_perspective_u8(src, C.M_PERSPECTIVE, 41, 29), C.host_warp(src, C.M_PERSPECTIVE, 41, 29))


# ---------------------------------------------------------------------------------------------
# brightness / contrast
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alpha,beta', [(1, 0.2), (1, -0.2), (1.3, 0), (0.7, 0)])
def test_brightness_contrast_rule(alpha, beta):
    """All 256 values against the closed form: the exact product of the two fp32 numbers, rounded once to fp32 (an fp64 product of
    fp32 factors is exact), plus fp32(beta) * 255 rounded to fp32, truncated, clipped."""
    v = np.arange(256, dtype=np.uint8)
    a, b255 = float(np.float32(alpha)), float(np.float32(float(np.float32(beta)) * 255.0))
    want = np.array([min(255, max(0, int(np.float32(float(np.float32(k * a)) + b255)))) for k in range(256)], dtype=np.uint8)
    got = D.brightness_contrast_u8(v, alpha, beta)
    assert np.array_equal(got, want)
    assert np.array_equal(got, C.host_brightness_contrast(v, alpha, beta))
    if beta > 0:
        assert got[0] == 51 and got[204] == 255 and got[255] == 255 and got[203] == 254          # v + 51, the top clips
    elif beta < 0:
        assert got[0] == 0 and got[50] == 0 and got[52] == 1 and got[255] == 204                  # v - 51, the bottom clips
    elif alpha > 1:
        assert got[100] == 130 and got[196] == 254 and got[197] == 255 and got[255] == 255
    else:
        assert got[0] == 0 and got[100] == 70 and got[255] == 178


# ---------------------------------------------------------------------------------------------
# geometry restatements
# ---------------------------------------------------------------------------------------------
class Scripted:
    """A stand-in Generator that hands out scripted draws: walks sample_homography's branches without hunting for seeds."""

    def __init__(self, randoms=(), integers=(), uniforms=()):
        self.r, self.i, self.u = list(randoms), list(integers), list(uniforms)

    def random(self):
        return self.r.pop(0)

    def integers(self, lo, hi, size=None):
        v = np.asarray(self.i.pop(0))
        assert ((v >= lo) & (v < hi)).all() and (size is None or v.shape == tuple(size))
        return v

    def uniform(self, lo=0.0, hi=1.0):
        return lo + (hi - lo) * self.u.pop(0)


def test_get_perspective_transform_maps_the_corners():
    rng = np.random.default_rng(2)
    h, w = 480, 640
    corners = np.array([[0, 0], [0, h], [w, 0], [w, h]], dtype=np.float64)
    for _ in range(10):
        moved = corners + rng.integers(-max(h, w) // 3, max(h, w) // 3, size=(4, 2))
        M = D.get_perspective_transform(corners, moved)
        assert M[2, 2] == 1.0
        assert np.abs(D.perspective_transform(corners, M) - moved).max() < 1e-9


def test_sample_homography_branches():
    h, w = 30, 40
    corners = np.array([[0, 0], [0, h], [w, 0], [w, h]], dtype=np.float64)
    big = np.array([[3, -2], [5, 7], [-13, 1], [0, -9]])
    small = np.array([[1, -2], [4, -5], [0, 3], [-1, 2]])
    flip_x, flip_y = np.array([[-1., 0, w], [0, 1, 0], [0, 0, 1]]), np.array([[1., 0, 0], [0, -1, h], [0, 0, 1]])      # w and h, not w - 1 / h - 1
    M = D.sample_homography((h, w), Scripted(randoms=[0.5, 0.5], integers=[big]))                    # no small warp, no flip
    assert np.abs(D.perspective_transform(corners, M) - (corners + big)).max() < 1e-9
    M = D.sample_homography((h, w), Scripted(randoms=[0.1, 0.5], integers=[big, small]))              # the small warp replaces the large one
    assert np.abs(D.perspective_transform(corners, M) - (corners + small)).max() < 1e-9
    assert np.array_equal(D.sample_homography((h, w), Scripted(randoms=[0.5, 0.1, 0.59], integers=[big, 0])), flip_x)     # a flip replaces the matrix
    assert np.array_equal(D.sample_homography((h, w), Scripted(randoms=[0.5, 0.1, 0.59], integers=[big, 1])), flip_y)
    M = D.sample_homography((h, w), Scripted(randoms=[0.5, 0.19, 0.6], integers=[big, 1]))            # ... or is applied first
    assert np.allclose(M, D.get_perspective_transform(corners, corners + big) @ flip_y, rtol=0, atol=1e-12)
    # the draw range of the corners: [-max(h, w) // 3, max(h, w) // 3) with Python's floor division of the NEGATED value
    with pytest.raises(AssertionError):
        D.sample_homography((h, w), Scripted(randoms=[0.5, 0.5], integers=[np.full((4, 2), 13)]))
    D.sample_homography((h, w), Scripted(randoms=[0.5, 0.5], integers=[np.array([[-14, 12]] * 4)]))


def test_translation_and_perspective_mat():
    # get_translation_mat: both sign rules per axis
    tc = np.array([[-3., 4.], [10., 50.], [20., 8.], [5., 9.]])           # left_top_min = (-3, 4); right_bottom_min = (100 - 20, 60 - 50)
    T = D.get_translation_mat(60, 100, 0.2, tc, Scripted(uniforms=[0.5, 0.25, 0.9, 0.9]))     # x: left axis, min < 0 -> +10; y: top axis, min >= 0 -> -3
    assert np.array_equal(T, [[1, 0, 10], [0, 1, -3], [0, 0, 1]])
    T = D.get_translation_mat(60, 100, 0.2, tc, Scripted(uniforms=[0.5, 0.25, 0.1, 0.1]))     # right / bottom axis, both minima > 0 -> + +
    assert np.array_equal(T, [[1, 0, 10], [0, 1, 3], [0, 0, 1]])
    # get_perspective_mat = translation @ homography, the translation judged on the warped patch corners
    h, w = 30, 40
    big = np.array([[3, -2], [5, 7], [-13, 1], [0, -9]])
    M = D.get_perspective_mat(0.8, h, w, 0.2, Scripted(randoms=[0.5, 0.5, 0.5], integers=[big], uniforms=[0.5, 0.5, 0.9, 0.1]))
    Hm = D.sample_homography((h, w), Scripted(randoms=[0.5, 0.5], integers=[big]))
    ratio = 1 - 0.5 * (1 - 0.8)
    pc = np.array([[0, 0], [0, int(ratio * h)], [int(ratio * w), int(ratio * h)], [int(ratio * w), 0]], dtype=np.float64)
    T = D.get_translation_mat(h, w, 0.2, D.perspective_transform(pc, Hm), Scripted(uniforms=[0.5, 0.5, 0.9, 0.1]))
    assert np.array_equal(M, T @ Hm) and abs(T[0, 2]) == 4 and abs(T[1, 2]) == 3


def test_scale_homography_is_the_conjugation():
    rng = np.random.default_rng(4)
    M = D.get_perspective_mat(0.8, 640, 480, 0.2, rng)
    Hs = D.scale_homography(M, 480, 640, 352, 480)
    pts = rng.uniform(0, 400, size=(16, 2))
    s = np.array([480 / 640, 352 / 480])
    assert np.abs(D.perspective_transform(pts * s, Hs) - D.perspective_transform(pts, M) * s).max() < 1e-8
    S = np.diag([s[0], s[1], 1.0])
    assert np.allclose(Hs, S @ M @ np.diag([1 / s[0], 1 / s[1], 1.0]), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('hw,st,want', [((480, 640), 32, (480, 352)), ((640, 480), 32, (480, 640)), ((333, 500), 32, (480, 288)),
                                        ((500, 333), 32, (416, 640)), ((480, 640), 0, (640, 480)), ((640, 480), 0, (480, 640)),
                                        ((333, 500), 0, (640, 480)), ((500, 333), 0, (480, 640))])
def test_target_size_rule(hw, st, want):
    """get_pair :98-109 with size = (640, 480): st > 0 fixes the height of a portrait source to size[0] and the width of a landscape
    one to size[1], the other side follows the aspect ratio down to a multiple of st; st == 0 is size itself, transposed for portrait."""
    assert D.target_size(hw[0], hw[1], (640, 480), st) == want             # (wt, ht)


def test_rank_slice_drops_the_remainder():
    assert D.rank_slice(10, 0, None) == (0, 10)
    assert [D.rank_slice(10, r, 3) for r in range(3)] == [(0, 3), (3, 6), (6, 9)]          # file 9 is nobody's
    assert [D.rank_slice(9, r, 3) for r in range(3)] == [(0, 3), (3, 6), (6, 9)]
    assert D.rank_slice(2, 1, 2) == (1, 2)


# ---------------------------------------------------------------------------------------------
# HomoPairs on the host path
# ---------------------------------------------------------------------------------------------
SHAPES = [(96, 128), (128, 96), (96, 128), (120, 160), (128, 96), (96, 128), (80, 112)]


@pytest.fixture(scope='module')
def image_dir(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('homo'))
    return root, C.make_image_dir(root, SHAPES)


def pairs(root, **kw):
    kw = {'size': (96, 128), 'preprocess': 'host', 'device': 'cpu', **kw}
    return D.HomoPairs(root, **kw)


def test_file_list_is_sorted_and_rank_sliced(image_dir):
    root, paths = image_dir
    assert pairs(root).data == paths and len(paths) == 7
    a, b = pairs(root, rank=0, world_size=2), pairs(root, rank=1, world_size=2)
    assert a.data == paths[0:3] and b.data == paths[3:6]                                  # 7 // 2 each, the seventh dropped
    # a sample is keyed by its place in the whole sorted list: rank 1's first file draws what the unsliced dataset draws for file 3
    assert np.array_equal(b.sample(0)['M'], pairs(root).sample(3)['M'])
    assert b.sample(0)['pair_names'] == pairs(root).sample(3)['pair_names']


def test_get_perspective_mat_is_called_with_width_and_height_swapped(image_dir):
    root, _ = image_dir
    ds = pairs(root, seed=3)
    h, w = ds.source_hw(0)
    assert (h, w) == (96, 128)
    M = ds.sample(0, epoch=2)['M']
    assert np.array_equal(M, D.get_perspective_mat(0.8, w, h, 0.2, D.sample_rng(3, 2, 0)))          # (ratio, width, height, trans): the reference's call
    assert not np.array_equal(M, D.get_perspective_mat(0.8, h, w, 0.2, D.sample_rng(3, 2, 0)))


def test_samples_are_deterministic_and_epochs_differ(image_dir):
    root, paths = image_dir
    names = [os.path.basename(paths[i]) for i in (0, 2)]
    a, b = pairs(root, seed=1), pairs(root, seed=1)
    ba, bb = a.batch([0, 2], epoch=0), b.batch([0, 2], epoch=0)
    for k in ('image0', 'image1', 'H_0to1', 'H_1to0', 'pair_id', 'is_negs'):
        assert ba[k].equal(bb[k]), k
    assert ba['pair_names'] == bb['pair_names'] == [[n + '_0' for n in names], [n + '_1' for n in names]]
    assert ba['dataset_name'] == ['Oxford', 'Oxford'] and ba['image0'].shape == (2, 1, 96, 128) and ba['H_0to1'].shape == (2, 3, 3)
    assert np.array_equal(a.sample(0, 0)['M'], b.sample(0, 0)['M'])
    other = a.batch([0, 2], epoch=1)
    assert not np.array_equal(a.sample(0, 0)['M'], a.sample(0, 1)['M'])
    assert not other['H_0to1'].equal(ba['H_0to1']) and not other['image1'].equal(ba['image1'])
    assert not np.array_equal(pairs(root, seed=2).sample(0, 0)['M'], a.sample(0, 0)['M'])


def test_labels_are_inverse_of_each_other_after_the_swap(image_dir):
    root, _ = image_dir
    ds = pairs(root, seed=5)
    swaps = set()
    for i in range(len(ds)):
        for epoch in range(3):
            p = ds.sample(i, epoch)
            swaps.add(p['swap'])
            prod = p['H_0to1'].astype(np.float64) @ p['H_1to0'].astype(np.float64)
            assert np.abs(prod - np.eye(3)).max() < 1e-5, (i, epoch)
            H = D.scale_homography(p['M'], *p['hw'], p['ht'], p['wt'])
            want = np.linalg.inv(H) if p['swap'] else H
            assert np.array_equal(p['H_0to1'], want.astype(np.float32))
    assert swaps == {True, False}


def test_augmentation_draws_follow_the_reference_probabilities():
    rng = np.random.default_rng(0)
    draws = [D.sample_augment(rng) for _ in range(20000)]
    on = [d for d in draws if d is not None]
    assert abs(len(on) / len(draws) - 0.65 * 0.5) < 0.015
    bright = [d for d in on if d[0] == 1.0]
    assert abs(len(bright) / len(on) - 0.8 / 1.4) < 0.03
    assert all(abs(d[1]) <= 0.2 + 1e-6 for d in bright) and all(abs(d[0] - 1) <= 0.3 + 1e-6 and d[1] == 0.0 for d in on if d[0] != 1.0)


def test_batches_bucket_by_shape_deterministically(image_dir):
    root, _ = image_dir
    ds = pairs(root)
    shapes = [ds.target_hw(i) for i in range(len(ds))]
    assert set(shapes) == {(96, 128), (64, 128), (96, 64)}              # landscape: width 128, height by aspect; portrait: height 96
    for epoch in range(2):
        got = list(ds.batches(2, epoch))
        assert got == list(pairs(root).batches(2, epoch))
        assert sorted(i for b in got for i in b) == list(range(7))
        assert all(len({shapes[i] for i in b}) == 1 and len(b) <= 2 for b in got)
        assert all(len(b) == 2 for b in ds.batches(2, epoch, drop_last=True))
    assert list(ds.batches(2, 0)) != list(ds.batches(2, 1))
    assert [i for b in ds.batches(1, 0, shuffle=False) for i in b] == list(range(7))
    with pytest.raises(ValueError, match='different target shapes'):
        ds.batch([0, 1])


def centroid(img, cx, cy, r=10, background=20.0):
    """Intensity centroid above the background in the (2r + 1)^2 window around (cx, cy); None if the window leaves the frame."""
    h, w = img.shape
    x0, y0 = int(round(cx)) - r, int(round(cy)) - r
    if x0 < 0 or y0 < 0 or x0 + 2 * r + 1 > w or y0 + 2 * r + 1 > h:
        return None
    win = np.clip(img[y0:y0 + 2 * r + 1, x0:x0 + 2 * r + 1].astype(np.float64) - background, 0, None)
    if win.sum() < 1e-9:
        return None
    ys, xs = np.mgrid[0:2 * r + 1, 0:2 * r + 1]
    return np.array([x0 + (win * xs).sum() / win.sum(), y0 + (win * ys).sum() / win.sum()]), win.sum()


@pytest.mark.parametrize('seed,swap', [(1, True), (4, False)])
def test_labels_describe_the_pictures(tmp_path, seed, swap):
    """Three bright 9 x 9 blobs in a 96 x 128 PPM, resized to 64 x 96: the centroid of a blob in image1 lies within 1.5 px (the resize's
    half-pixel convention plus the centroid of a sheared blob) of H_0to1 applied to its centroid in image0.  Blobs that leave the
    frame are discarded; the seeds are chosen so that at least two stay, one with and one without the swap."""
    img = np.full((96, 128, 3), 20, dtype=np.uint8)
    centres = [(30, 28), (92, 36), (58, 70)]                            # (x, y)
    for cx, cy in centres:
        img[cy - 4:cy + 5, cx - 4:cx + 5] = 240
    C.write_ppm(str(tmp_path / 'blobs.ppm'), img)
    ds = D.HomoPairs(str(tmp_path), size=(96, 96), st=32, seed=seed, device='cpu', preprocess='host', augment=False)
    assert ds.target_hw(0) == (64, 96)
    b = ds.batch([0])
    p = ds.sample(0)
    assert p['swap'] == swap
    im0, im1 = (b[k][0, 0].numpy() * 255.0 for k in ('image0', 'image1'))
    H01 = b['H_0to1'][0].numpy().astype(np.float64)
    to_orig = b['H_1to0'][0].numpy().astype(np.float64) if p['swap'] else np.eye(3)     # resized original -> image0 (swapped: image1 IS the original)
    kept = 0
    for cx, cy in centres:
        c_res = np.array([[(cx + 0.5) * 96 / 128 - 0.5, (cy + 0.5) * 64 / 96 - 0.5]])      # the blob in the resized original
        guess0 = D.perspective_transform(c_res, to_orig)[0]
        c0 = centroid(im0, *guess0)
        if c0 is None:
            continue
        want = D.perspective_transform(c0[0][None], H01)[0]
        c1 = centroid(im1, *want)
        if c1 is None:
            continue
        d = np.linalg.norm(c1[0] - want)
        print(f'seed {seed} blob ({cx}, {cy}): image0 {c0[0]}, image1 {c1[0]}, predicted {want}, distance {d:.3f} px')
        assert c1[1] > 0.25 * c0[1], 'the window around the predicted position holds no blob'
        assert d < 1.5
        kept += 1
    assert kept >= 2
