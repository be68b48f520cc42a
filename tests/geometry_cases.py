"""Inputs and float64 references for the geometry stage (window_geometry, inlier_index, the RANSAC keypoint rescale and the model
validity rule).  Plain numpy / torch; nothing here imports the library under test.

Every kernel of this stage takes discrete decisions (a floor, an out-of-bounds test, a cell index), so a reference cannot be compared
"to a tolerance": an entry is either the same integer or it is not.  `window_reference` therefore evaluates the fp32-ROUNDED matrix in
float64 and returns, beside the integers, a per-entry `band`: the entries whose real coordinate lies so close to a decision boundary
that a correct fp32 evaluation may land on the other side.  Outside the band a kernel must reproduce the reference exactly.

The width of the band, `delta`, is derived from the fp32 round-off of the expression the kernel (and the reference implementation it
restates) evaluates - see `window_reference` - and is validated on the CPU against the fp32 oracle (tests/test_geometry_cases.py),
never tuned on the kernel."""
from fractions import Fraction

import numpy as np
import torch

U = 2.0 ** -24                      # unit round-off of fp32 (round to nearest)
W_GUARD = float(np.float32(1e-6))   # what an exactly-zero w is replaced by (fp32 constant)
DELTA_WILD = 0.25                   # a derived delta above this says nothing about the integer: only the contract is checked there
W_FLOOR_FACTOR = 2 * 4 * U          # |w| >= W_FLOOR_FACTOR * (|h6 x| + |h7 y| + |h8|) for `warped` / the integers to be compared
F32_SAFE = (1e-30, 1e38)            # magnitudes outside this range may flush or overflow in fp32: no bound is claimed there

SHAPES = [((80, 80), (640, 640)), ((60, 80), (480, 608))]     # (query grid, image that receives the windows)
WSCALES = [None, (1.25, 1.5), (1.2, 0.8)]                     # per-sample window scales: none, a dyadic pair, a non-dyadic pair
RESCALE_SCALES = [1.2, 0.8, 1.6, 2.0 / 3.0, 1.0 / 3.0, 1.1, 1.7]
BAND_SHARE_CAP = 0.01               # generic class: at most this share of entries in the band
HORIZON_COMPARABLE_MIN = 0.5        # horizon class: at least this share of entries outside the band


# ----------------------------------------------------------------------------------------------------------------- homographies
def _similarity(theta, zoom, tx, ty, cx=320.0, cy=320.0):
    c, s = np.cos(theta) * zoom, np.sin(theta) * zoom
    return np.array([[c, -s, cx - c * cx + s * cy + tx], [s, c, cy - s * cx - c * cy + ty], [0.0, 0.0, 1.0]])


def homographies(kind):
    """[(name, 3x3 float64)] of one class: 'exact', 'generic' or 'horizon'.  Deterministic (fixed seeds)."""
    if kind == 'exact':
        # every product, sum and quotient is an integer or a half-integer far below 2^24: exact in fp32 under any contraction.
        # With the integer-valued ones every window coordinate sits ON a decision boundary (an integer; 0, W or H for some).
        return [('identity', np.eye(3)),
                ('shift_8_16', np.array([[1., 0, 8], [0, 1, 16], [0, 0, 1]])),
                ('shift_-24_40', np.array([[1., 0, -24], [0, 1, 40], [0, 0, 1]])),
                ('shift_3_-7', np.array([[1., 0, 3], [0, 1, -7], [0, 0, 1]])),
                ('shift_frac', np.array([[1., 0, 3.25], [0, 1, -5.5], [0, 0, 1]])),
                ('rot90', np.array([[0., -1, 640], [1, 0, 0], [0, 0, 1]])),        # about (320, 320): x' = 640 - y reaches W exactly
                ('rot180', np.array([[-1., 0, 639], [0, -1, 639], [0, 0, 1]])),    # about the pixel centre (319.5, 319.5)
                ('rot180_edge', np.array([[-1., 0, 640], [0, -1, 480], [0, 0, 1]])),
                ('zoom2', np.array([[2., 0, 0], [0, 2, 0], [0, 0, 1]])),
                ('zoom_half', np.array([[0.5, 0, 0], [0, 0.5, 0], [0, 0, 1]])),
                ('zoom2_w2', np.array([[4., 0, 0], [0, 4, 0], [0, 0, 2]])),         # the same zoom through a division by w = 2
                ('shift_w_negative', np.array([[-1., 0, -8], [0, -1, -16], [0, 0, -1]]))]   # a shift by (8, 16) with w == -1
    if kind == 'generic':
        rng = np.random.default_rng(20240607)
        out = []
        zooms = np.r_[0.5, 2.6, np.exp(rng.uniform(np.log(0.5), np.log(2.6), 64))]   # both ends of the range, then random
        i = 0
        while len(out) < 28:
            z = zooms[i]; i += 1
            H = _similarity(rng.uniform(-0.5, 0.5), z, rng.uniform(-150, 150), rng.uniform(-150, 150))
            H[2, :2] = rng.uniform(-8e-4, 8e-4, 2)
            # the range condition of this class: w stays well away from 0 on the grid (a horizon near the grid belongs to the
            # 'horizon' class; it inflates delta and with it the band)
            corners = np.array([[0, 0, 1], [632, 0, 1], [0, 632, 1], [632, 632, 1.0]])
            if (corners @ H[2]).min() < 0.5:
                continue
            out.append((f'generic{len(out):02d}_z{z:.2f}', H))
        return out
    if kind == 'horizon':
        return [('w0_at_x256', np.array([[1., 0, 0], [0, 1, 0], [-1.0 / 256, 0, 1]])),   # exact in fp32: w == 0 exactly at x = 256
                ('w0_diag', np.array([[1.05, 0.02, 12.0], [-0.03, 0.97, -7.0], [-1.0 / 512, -1.0 / 512, 1]])),   # w == 0 on x + y = 512
                ('horizon_a', np.array([[0.9, -0.1, 30.0], [0.12, 1.1, -20.0], [-2.3e-3, 4.1e-4, 1]])),
                ('horizon_b', np.array([[1.2, 0.2, -50.0], [-0.15, 0.8, 60.0], [7.0e-4, -3.1e-3, 1]])),
                ('w_negative', np.array([[-1.1, 0.05, -20.0], [0.03, -0.9, -10.0], [-2.0e-4, -1.0e-4, -1]]))]    # w < 0 on the whole grid
    raise KeyError(kind)


# ----------------------------------------------------------------------------------------------------------------- windows
def _f32_exact(x):
    return x.astype(np.float32).astype(np.float64) == x


def window_reference(H32, grid_hw, img_hw, scale=8, window=5, wscale=None):
    """Float64 evaluation of the fp32-rounded matrix H32 [3,3] on the query grid `grid_hw` (cells of `scale` pixels), windows into
    an image of `img_hw` pixels whose coarse grid is img_w // scale wide.

    Returns a dict:
      warped [L,2] f64   the warped cell coordinates (after the w == 0 guard)
      w      [L]   f64   the homogeneous coordinate before the guard
      q      [L,ww,2]    the real window coordinates, x fastest: warped + (c - 2, r - 2) * scale * wscale
      kps    [L,ww,2] i64, mask [L,ww] bool, cell [L,ww] i64 (-1 where masked)
      delta  [L]         bound on |fp32 coordinate - q| (the same for x and y and for the 25 positions of a cell); inf where wild
      wild   [L]   bool  no usable bound: |w| below the floor, delta > DELTA_WILD, or magnitudes outside fp32's safe range
      band   [L,ww] bool entries that a correct fp32 evaluation may decide differently (every entry of a wild cell is one)
      nonfinite [L] bool a non-finite reference coordinate (non-finite matrix): masked by contract, outside band and wild

    delta.  The kernel evaluates, in fp32, X = h0 x + h1 y + h2 (same for Y and w), p = X / w, q = p + k * s.
      * X-hat = X + eX: every term goes through at most 3 roundings (its product and two sums), with or without FMA contraction:
        |eX| <= g3 * Xabs, Xabs = |h0 x| + |h1 y| + |h2|, g3 = 3u / (1 - 3u) < 4u.  Likewise |ew| < 4u * Wabs.
      * the floor on w: |w| >= 2 * 4u * Wabs, so |w-hat| >= |w| / 2 and
        |X-hat / w-hat - X / w| <= (|eX| + |p| |ew|) / |w-hat| <= 8u * (Xabs / |w| + |p| Wabs / |w|).
        (When every partial result of w is exactly representable, ew = 0 and the floor is not needed: that keeps the exact w == 0
        case, where the guard fires, inside the comparison.)
      * the division rounds once (u |p|), the step s = fl(scale * wscale) once, k * s once (|k| <= 2: 2u * 2s together), the final
        sum once (u (|p| + 2s)): below 2u |p| + 6u s, bounded here by 4u * (max(|p|, 1) + 2 s).
    delta = 8u (Xabs / |w| + |p| Wabs / |w|) + 4u (max(|p|, 1) + 2 s), the larger of the x and y values.

    The band is narrower than "any coordinate within delta of an integer" in one respect: an entry with a coordinate out of the
    image by MORE than delta is masked whatever the rounding does, so it is compared even if another coordinate is near an integer."""
    H = np.asarray(H32, np.float32).astype(np.float64).reshape(3, 3)
    hq, wq = grid_hw
    Hi, Wi = img_hw
    wk = Wi // scale
    ys, xs = np.meshgrid(np.arange(hq, dtype=np.float64) * scale, np.arange(wq, dtype=np.float64) * scale, indexing='ij')
    x, y = xs.reshape(-1), ys.reshape(-1)
    with np.errstate(all='ignore'):
        t = [(H[r, 0] * x, H[r, 1] * y, np.full_like(x, H[r, 2])) for r in range(3)]
        X, Y, w = [(a + b) + c for a, b, c in t]
        Xabs, Yabs, Wabs = [np.abs(a) + np.abs(b) + np.abs(c) for a, b, c in t]
        a, b, c = t[2]
        w_exact = _f32_exact(a) & _f32_exact(b) & _f32_exact(a + b) & _f32_exact(w)
        wg = np.where(w == 0, W_GUARD, w)
        px, py = X / wg, Y / wg
        if wscale is None:
            sx = sy = float(scale)
        else:
            sx, sy = [float(scale) * float(np.float32(v)) for v in wscale]
        half = window // 2
        k = np.arange(window * window)
        q = np.stack([px[:, None] + (k % window - half)[None] * sx, py[:, None] + (k // window - half)[None] * sy], -1)
        aw = np.abs(wg)
        s = max(sx, sy)
        dx = 8 * U * (Xabs / aw + np.abs(px) * Wabs / aw) + 4 * U * (np.maximum(np.abs(px), 1) + 2 * s)
        dy = 8 * U * (Yabs / aw + np.abs(py) * Wabs / aw) + 4 * U * (np.maximum(np.abs(py), 1) + 2 * s)
        delta = np.maximum(dx, dy)
        nonfinite = ~(np.isfinite(px) & np.isfinite(py))
        below_floor = ~w_exact & ~(np.abs(w) >= W_FLOOR_FACTOR * Wabs)
        big = np.max([Xabs, Yabs, Wabs, np.abs(px), np.abs(py)], 0)
        unsafe = ~(big < F32_SAFE[1]) | ((aw < F32_SAFE[0]))
        wild = (below_floor | unsafe | ~(delta <= DELTA_WILD)) & ~nonfinite
        delta = np.where(wild, np.inf, delta)
        oob = (q[..., 0] < 0) | (q[..., 1] < 0) | (q[..., 0] >= Wi) | (q[..., 1] >= Hi) | nonfinite[:, None]
        qz = np.where(oob[..., None], 0.0, q)
        kps = np.floor(qz).astype(np.int64)
        cell = np.where(oob, -1, (kps[..., 1] // scale) * wk + kps[..., 0] // scale)
        d = delta[:, None, None]
        lim = np.array([Wi, Hi], np.float64)
        surely_oob = ((q < -d) | (q >= lim + d)).any(-1)                  # decided whatever the rounding
        near = (np.abs(q - np.round(q)) <= d).any(-1)                     # 0, W and H are integers: the borders are included
        band = ((near & ~surely_oob) | wild[:, None]) & ~nonfinite[:, None]
    return {'warped': np.stack([px, py], -1), 'w': w, 'q': q, 'kps': kps, 'mask': ~oob, 'cell': cell, 'delta': delta, 'wild': wild,
            'band': band, 'nonfinite': nonfinite, 'wk': wk, 'img_hw': (Hi, Wi), 'scale': scale}


def band_rule_violations(ref, kps, win):
    """The entries of a result (kps [L,ww,2] or None, win [L,ww]) that the reference does not allow.  Outside the band: kps, mask
    and cell equal the reference.  Inside it: an in-bounds entry holds, per coordinate, floor(q - delta), floor(q) or
    floor(q + delta) - the reference's integer or its neighbour - inside the image, and its cell is the cell of those integers; a
    masked entry needs a coordinate within delta of the border it left through.  Entries of wild cells only have to respect the
    contract (win == -1 with kps 0, or kps inside the image and win their cell).  Without kps (the production call returns the
    table alone) the same rules are applied to the cells of those integers.  Returns (violations, differs), bool [L,ww]."""
    win = np.asarray(win, np.int64)
    Hi, Wi = ref['img_hw']
    scale, wk = ref['scale'], ref['wk']
    lim = np.array([Wi, Hi])
    ncell = -(-Hi // scale) * wk
    inb = win >= 0
    with np.errstate(all='ignore'):
        d = np.where(np.isfinite(ref['delta']), ref['delta'], 0.0)[:, None, None]
        q = np.where(np.isfinite(ref['q']), ref['q'], 0.0)
        cand = [np.floor(q - d), np.floor(q), np.floor(q + d)]
        at_border = ((q - d < 0) | (q + d >= lim)).any(-1)
    if kps is None:
        differs = win != ref['cell']
        contract = np.where(inb, win < ncell, win == -1)
        neighbour = np.zeros(win.shape, bool)
        for cx in cand:
            for cy in cand:
                x, y = cx[..., 0], cy[..., 1]
                inside = (x >= 0) & (x < Wi) & (y >= 0) & (y < Hi)
                neighbour |= inside & (win == (y // scale) * wk + x // scale)
    else:
        kps = np.asarray(kps, np.int64)
        differs = (kps != ref['kps']).any(-1) | (win != ref['cell'])
        in_image = ((kps >= 0) & (kps < lim)).all(-1)
        own_cell = (kps[..., 1] // scale) * wk + kps[..., 0] // scale
        contract = np.where(inb, in_image & (win == own_cell) & (win < ncell), (win == -1) & (kps == 0).all(-1))
        neighbour = ((kps == cand[0]) | (kps == cand[1]) | (kps == cand[2])).all(-1)
    banded_ok = contract & np.where(inb, neighbour, at_border)
    ok = np.where(ref['wild'][:, None], contract, np.where(ref['band'], banded_ok, ~differs & contract))
    return ~ok, differs


def window_contract_violations(win, ncell):
    """Entries of a window table that are neither -1 nor a cell of the key grid."""
    win = np.asarray(win, np.int64)
    return ~((win == -1) | ((win >= 0) & (win < ncell)))


# ----------------------------------------------------------------------------------------------------------------- keypoint rescale
def keypoint_rescale_reference(kp, scale, s):
    """The reference's expression, in fp32 on the CPU: (kp.long() / (scale * s) * scale).long() with kp [n,2] (any dtype), `scale`
    the Python int coarse scale and s [2] the image's fp32 (x, y) scale.  THIS is the specification: an int64 tensor divided by an
    fp32 tensor is an fp32 division (correctly rounded), the product with the Python int is an fp32 product."""
    k = torch.as_tensor(kp).long()
    s = torch.as_tensor(s, dtype=torch.float32)
    return (k / (scale * s) * scale).long()


def rescale_exact_floor(coords, scale, s):
    """floor of the exact rational value of the same expression on the same fp32 input (only to count knife edges)."""
    sv = Fraction(float(np.float32(s)))
    return np.array([(Fraction(int(c)) / (scale * sv) * scale).__floor__() for c in coords], np.int64)


def rescale_knife_edges(scale, s, top=1280):
    """Number of integer coordinates 0..top where the fp32 expression differs from the exact floor."""
    c = np.arange(top + 1)
    got = keypoint_rescale_reference(np.stack([c, c], 1), scale, [s, s])[:, 0].numpy()
    return int((got != rescale_exact_floor(c, scale, s)).sum())


def rescale_case():
    """Match lists for the rescale test: per sample every multiple of 8 in 0..1280 on both axes (x ascending, y descending, so that
    both images see the whole range on both axes) followed by every integer 0..1280 on x against 1280 - i on y, those with a
    fraction (.5, .75) that the first .long() drops.  Sample b takes
    the x / y scales of image 0 and image 1 from four different places of RESCALE_SCALES.
    -> (mk0 [cap,2] f32, mk1 [cap,2] f32, counts int32 [1+N], scale0 [N,2] f32, scale1 [N,2] f32)"""
    S = RESCALE_SCALES
    N = len(S)
    m8 = np.arange(0, 1281, 8)
    ii = np.arange(0, 1281)
    one0 = np.concatenate([np.stack([m8, m8[::-1]], 1), np.stack([ii + 0.5, 1280.75 - ii], 1)]).astype(np.float32)
    one1 = one0[:, ::-1].copy()
    n = len(one0)
    scale0 = np.array([[S[b], S[(b + 1) % N]] for b in range(N)], np.float32)
    scale1 = np.array([[S[(b + 2) % N], S[(b + 3) % N]] for b in range(N)], np.float32)
    counts = np.array([N * n] + [n] * N, np.int32)
    return np.tile(one0, (N, 1)), np.tile(one1, (N, 1)), counts, scale0, scale1


# ----------------------------------------------------------------------------------------------------------------- inlier index
def inlier_reference(kp0, kp1, keep, counts, L, S, w0, w1, scale=8):
    """Occupancy maps and ascending index lists of the kept matches.  kp [cap,2] integer-valued, keep [cap], counts [1+N] (total,
    then per sample).  -> dict(map0 bool [N,L], map1 bool [N,S], idx0 / idx1: lists of int arrays, nidx int [N,2])."""
    kp0, kp1 = np.asarray(kp0).astype(np.int64), np.asarray(kp1).astype(np.int64)
    keep = np.asarray(keep).astype(bool)
    cnt = [int(c) for c in np.asarray(counts)[1:]]
    N = len(cnt)
    map0, map1 = np.zeros((N, L), bool), np.zeros((N, S), bool)
    off = 0
    for b, c in enumerate(cnt):
        sel = keep[off:off + c]
        a, bb = kp0[off:off + c][sel], kp1[off:off + c][sel]
        map0[b, (a[:, 1] // scale) * w0 + a[:, 0] // scale] = True
        map1[b, (bb[:, 1] // scale) * w1 + bb[:, 0] // scale] = True
        off += c
    idx0, idx1 = [np.nonzero(m)[0] for m in map0], [np.nonzero(m)[0] for m in map1]
    nidx = np.array([[len(a), len(b)] for a, b in zip(idx0, idx1)], np.int64)
    return {'map0': map0, 'map1': map1, 'idx0': idx0, 'idx1': idx1, 'nidx': nidx}


def inlier_cases():
    """[(name, dict(kp0, kp1, keep, counts, L, S, w0, w1))]: the chunked compaction at one chunk exactly, one cell more, the full
    grid and an unequal pair; all / no / first-only / last-only cells set; an empty sample; a sample of more than 6400 matches
    with duplicates."""
    rng = np.random.default_rng(77)

    def cells_to_kp(cells, w):
        cells = np.asarray(cells, np.int64)
        return np.stack([(cells % w) * 8 + rng.integers(0, 8, len(cells)), (cells // w) * 8 + rng.integers(0, 8, len(cells))], 1)

    out = []
    for name, (h0, w0), (h1, w1) in [('6400x6400', (80, 80), (80, 80)), ('4800x4560', (60, 80), (60, 76)),
                                     ('1024x1025', (32, 32), (25, 41)), ('1x3', (1, 1), (1, 3))]:
        L, S = h0 * w0, h1 * w1
        per = []                                                          # (cells0, cells1, keep) per sample
        m = max(L, S)
        allc = np.arange(m)
        per.append((allc % L, allc % S, np.ones(m, np.uint8)))            # every cell of both sides set: nidx == (L, S)
        per.append((allc % L, allc % S, np.zeros(m, np.uint8)))           # keep all 0: nidx == 0
        per.append((np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint8)))     # count 0
        per.append((np.array([0, 0, 0]), np.array([0, 0, 0]), np.array([1, 0, 1], np.uint8)))            # only the first cell
        per.append((np.array([L - 1, 0, L - 1]), np.array([S - 1, 0, S - 1]), np.array([1, 0, 1], np.uint8)))   # only the last
        big = 7000 if L >= 6400 else 3 * m + 5                            # more matches than cells: duplicates
        per.append((rng.integers(0, L, big), rng.integers(0, S, big), (rng.random(big) > 0.4).astype(np.uint8)))
        k = min(40, m)
        per.append((rng.integers(0, L, k), rng.integers(0, S, k), (rng.random(k) > 0.3).astype(np.uint8)))
        kp0 = np.concatenate([cells_to_kp(p[0], w0) for p in per]).astype(np.float32)
        kp1 = np.concatenate([cells_to_kp(p[1], w1) for p in per]).astype(np.float32)
        keep = np.concatenate([p[2] for p in per])
        cnts = [len(p[0]) for p in per]
        out.append((name, dict(kp0=kp0, kp1=kp1, keep=keep, counts=np.array([sum(cnts)] + cnts, np.int32), L=L, S=S, w0=w0, w1=w1)))
    return out


# ----------------------------------------------------------------------------------------------------------------- degenerate models
def degenerate_match_sets():
    """[(name, kp0 int64 [60,2], kp1 int64 [60,2])]: match sets whose best homography is singular or nearly so, and a control."""
    rng = np.random.default_rng(5)
    n = 60
    p0 = np.stack([rng.permutation(80)[:n] * 8, rng.integers(0, 80, n) * 8], 1).astype(np.int64)     # distinct x
    line0 = np.stack([np.arange(n) * 8, np.arange(n) * 8 + 40], 1).astype(np.int64)
    line1 = np.stack([np.arange(n) * 8 + 16, 560 - np.arange(n) * 8], 1).astype(np.int64)
    col3_0, col3_1 = line0.copy(), line1.copy()
    col3_0[-3:] = [[600, 16], [40, 480], [320, 8]]
    col3_1[-3:] = [[560, 80], [96, 400], [300, 40]]
    rows0 = np.stack([np.arange(n) % 30 * 16, np.where(np.arange(n) < 30, 80, 400)], 1).astype(np.int64)
    return [('one_row', p0, np.stack([p0[:, 0], np.full(n, 200)], 1)),
            ('one_column', p0, np.stack([np.full(n, 304), p0[:, 1]], 1)),
            ('one_point', p0, np.tile(np.array([[320, 240]], np.int64), (n, 1))),
            ('both_collinear', line0, line1),
            ('collinear_plus3', col3_0, col3_1),
            ('two_rows', rows0, rows0 + np.array([24, -16]))]


def adjugate_inverse(M):
    """fp64 inverse as adjugate / determinant (defined, possibly inf / nan, for any matrix; numpy.linalg.inv may refuse)."""
    g = np.asarray(M, np.float64).reshape(-1)
    det = g[0] * (g[4] * g[8] - g[5] * g[7]) - g[1] * (g[3] * g[8] - g[5] * g[6]) + g[2] * (g[3] * g[7] - g[4] * g[6])
    adj = np.array([g[4] * g[8] - g[5] * g[7], g[2] * g[7] - g[1] * g[8], g[1] * g[5] - g[2] * g[4],
                    g[5] * g[6] - g[3] * g[8], g[0] * g[8] - g[2] * g[6], g[2] * g[3] - g[0] * g[5],
                    g[3] * g[7] - g[4] * g[6], g[1] * g[6] - g[0] * g[7], g[0] * g[4] - g[1] * g[3]])
    with np.errstate(all='ignore'):
        return (adj / det).reshape(3, 3)


def minv_f32_tolerance(M):
    """Relative tolerance (of the largest entry of the inverse) for the fp32 cast of an fp64 inverse of M: an fp64 inversion is
    backward stable to a few cond(M) * 2^-53 - taken as cond(M) * 2^-52 for the two implementations compared - plus the one fp32
    rounding of the cast, 2^-24."""
    return float(np.linalg.cond(M)) * 2.0 ** -52 + 2.0 ** -24


def planted_matches(n, n_out, H, hw0, hw1, seed):
    """n matches on the coarse grids (multiples of 8) of images hw0 / hw1 following H, n_out of them replaced by random ones."""
    rng = np.random.default_rng(seed)
    p0 = np.zeros((0, 2), np.int64)
    p1 = np.zeros((0, 2), np.int64)
    while len(p0) < n:
        a = np.stack([rng.integers(0, hw0[1] // 8, 4 * n) * 8, rng.integers(0, hw0[0] // 8, 4 * n) * 8], 1).astype(np.int64)
        qh = np.c_[a, np.ones(len(a))] @ H.T
        b = np.floor(qh[:, :2] / qh[:, 2:3] / 8).astype(np.int64) * 8
        ok = (b[:, 0] >= 0) & (b[:, 0] < hw1[1]) & (b[:, 1] >= 0) & (b[:, 1] < hw1[0])
        p0, p1 = np.concatenate([p0, a[ok]]), np.concatenate([p1, b[ok]])
    p0, p1 = p0[:n].copy(), p1[:n].copy()
    out = rng.choice(n, n_out, replace=False)
    p1[out] = np.stack([rng.integers(0, hw1[1] // 8, n_out) * 8, rng.integers(0, hw1[0] // 8, n_out) * 8], 1)
    return p0, p1
