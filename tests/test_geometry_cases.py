"""CPU checks of geometry_cases.py: the generators are deterministic; the derived `delta` really bounds an fp32 evaluation (the
oracle's torch fp32 warp_points + make_windows never differs from the float64 reference outside the band); the input classes keep
the shares the GPU test relies on; the non-dyadic scales contain knife edges; the degenerate match sets behave as the GPU test
assumes under the C RANSAC oracle."""
import numpy as np
import pytest
import torch

import geoformer_oracle as O
import geometry_cases as GC
import ransac_oracle as RO


def oracle_windows(H32, grid_hw, img_hw, wscale, scale=8, window=5):
    """The oracle's fp32 path as geo_module calls it -> (warped [L,2] f32, kps [L,ww,2] i64, cell [L,ww] i64 with -1 where masked)."""
    p = O.warp_points(O.map_keypoints(grid_hw[0] * scale, grid_hw[1] * scale, scale), torch.from_numpy(np.asarray(H32, np.float32)))
    step = scale if wscale is None else scale * torch.tensor(wscale, dtype=torch.float32)
    k, m = O.make_windows(p, img_hw, window, step)
    k, m = k.numpy(), m.numpy()
    return p.numpy(), k, np.where(m, (k[..., 1] // scale) * (img_hw[1] // scale) + k[..., 0] // scale, -1)


def test_generators_deterministic():
    for kind in ('exact', 'generic', 'horizon'):
        a, b = GC.homographies(kind), GC.homographies(kind)
        assert [n for n, _ in a] == [n for n, _ in b] and all(np.array_equal(x[1], y[1]) for x, y in zip(a, b))
    assert len(GC.homographies('generic')) >= 24
    assert len({n for k in ('exact', 'generic', 'horizon') for n, _ in GC.homographies(k)}) == sum(
        len(GC.homographies(k)) for k in ('exact', 'generic', 'horizon'))
    for a, b in zip(GC.rescale_case(), GC.rescale_case()):
        assert np.array_equal(a, b)
    for (na, a), (nb, b) in zip(GC.inlier_cases(), GC.inlier_cases()):
        assert na == nb and all(np.array_equal(a[k], b[k]) for k in a)
    for a, b in zip(GC.degenerate_match_sets(), GC.degenerate_match_sets()):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # the horizon class is what it says: w changes sign inside the 80 x 80 grid, except the all-negative one
    for name, H in GC.homographies('horizon'):
        w = GC.window_reference(H.astype(np.float32), (80, 80), (640, 640))['w']
        assert (w.max() < 0) if name == 'w_negative' else (w.min() < 0 < w.max()), name
    w = GC.window_reference(GC.homographies('horizon')[0][1].astype(np.float32), (80, 80), (640, 640))['w'].reshape(80, 80)
    assert (w[:, 32] == 0).all() and (w != 0).sum() == 80 * 79           # w == 0 exactly on the column x = 256


@pytest.mark.parametrize('grid,img', GC.SHAPES)
def test_exact_class_needs_no_band(grid, img):
    """Integer, half- and quarter-integer coordinates: the fp32 oracle equals the float64 reference EVERYWHERE (no band consulted), and the
    class really puts window positions on decision boundaries (integers; the borders 0 / W / H for some)."""
    on_border = 0
    for name, H in GC.homographies('exact'):
        H32 = H.astype(np.float32)
        assert np.array_equal(H32.astype(np.float64), H), name
        ref = GC.window_reference(H32, grid, img)
        p, k, cell = oracle_windows(H32, grid, img, None)
        assert np.array_equal(p.astype(np.float64), ref['warped']), name
        assert np.array_equal(k, ref['kps']) and np.array_equal(cell, ref['cell']), name
        assert np.array_equal(ref['q'] * 4, np.round(ref['q'] * 4)), name         # multiples of 1/4: exact in fp32
        on_border += int(((ref['q'] == 0) | (ref['q'] == np.array([img[1], img[0]]))).sum())
    assert on_border > 10000


@pytest.mark.parametrize('wscale', GC.WSCALES, ids=str)
@pytest.mark.parametrize('grid,img', GC.SHAPES)
def test_delta_bounds_the_fp32_oracle(grid, img, wscale):
    """THE test that delta is a bound: an independent fp32 evaluation (torch on the CPU) differs from the float64 reference only
    inside the band, there only by the band rule, and its warped coordinates stay within delta.  Also the conditions on the
    inputs: band share of every generic homography <= 1 %, comparable share of every horizon homography >= 50 %."""
    for kind in ('generic', 'horizon'):
        n_all = n_band = n_diff = n_diff_out = 0
        for name, H in GC.homographies(kind):
            H32 = H.astype(np.float32)
            ref = GC.window_reference(H32, grid, img, wscale=wscale)
            p, k, cell = oracle_windows(H32, grid, img, wscale)
            viol, differs = GC.band_rule_violations(ref, k, cell)
            assert not viol.any(), (name, int(viol.sum()))
            assert not (differs & ~ref['band']).any(), name
            ok = ~ref['wild']
            assert (np.abs(p.astype(np.float64) - ref['warped'])[ok].max(-1) <= ref['delta'][ok]).all(), name
            share = float(ref['band'].mean())
            if kind == 'generic':
                assert share <= GC.BAND_SHARE_CAP, (name, share)
                assert not ref['wild'].any(), name
            else:
                assert 1.0 - share >= GC.HORIZON_COMPARABLE_MIN, (name, share)
            n_all += viol.size; n_band += int(ref['band'].sum()); n_diff += int(differs.sum())
            n_diff_out += int((differs & ~ref['band']).sum())
        print(f'{kind} {grid}->{img} wscale {wscale}: {n_all} entries, {n_band} in the band, {n_diff} differ (all inside), {n_diff_out} outside')
        assert n_diff > 0 or kind == 'horizon'       # the band is not idle: fp32 does decide some banded entries differently


def test_band_rule_rejects_wrong_tables():
    """The comparison has teeth: a shifted table, a wrong cell width, a flipped mask and an out-of-range cell are all reported."""
    name, H = GC.homographies('generic')[3]
    grid, img = GC.SHAPES[1]
    ref = GC.window_reference(H.astype(np.float32), grid, img, wscale=(1.2, 0.8))
    kps, cell = ref['kps'], ref['cell']
    assert not GC.band_rule_violations(ref, kps, cell)[0].any()
    inb = cell >= 0
    assert inb.sum() > 1000 and (~inb).sum() > 1000
    shifted = kps + np.where(inb, 1, 0)[..., None] * np.array([1, 0])
    sc = np.where(inb, (shifted[..., 1] // 8) * ref['wk'] + shifted[..., 0] // 8, -1)
    assert GC.band_rule_violations(ref, shifted, sc)[0].sum() >= 0.98 * inb.sum()
    wrong_w = np.where(inb, (kps[..., 1] // 8) * (ref['wk'] + 4) + kps[..., 0] // 8, -1)       # the other image's grid width
    assert GC.band_rule_violations(ref, kps, wrong_w)[0].sum() >= 0.9 * (inb & (kps[..., 1] >= 8)).sum()
    masked = np.where(inb, -1, cell)
    assert GC.band_rule_violations(ref, np.zeros_like(kps), masked)[0].sum() >= 0.98 * inb.sum()
    assert GC.window_contract_violations(np.array([-1, 0, 4559, 4560, -2, 1 << 30]), 4560).tolist() == [False, False, False, True, True, True]
    # a reference built with the other scale pair is a different table
    other = GC.window_reference(H.astype(np.float32), grid, img, wscale=(0.8, 1.2))
    assert GC.band_rule_violations(ref, other['kps'], other['cell'])[0].sum() > 1000


def test_nonfinite_matrices_are_masked_by_the_reference():
    for row in range(3):
        for bad in (np.inf, np.nan):
            H = np.eye(3); H[row, :] = bad
            ref = GC.window_reference(H.astype(np.float32), (60, 80), (480, 608))
            if row == 2 and bad == np.inf:       # x / inf == 0 is a finite coordinate (inf * 0 on the first row / column is not)
                assert (ref['nonfinite'] | ref['wild']).all() and ref['nonfinite'].sum() == 60 + 80 - 1
            else:
                assert ref['nonfinite'].all() and (ref['cell'] == -1).all() and not ref['band'].any()
            assert (ref['cell'][ref['nonfinite']] == -1).all() and not (ref['nonfinite'] & ref['wild']).any()
    H = np.eye(3); H[0, 0] = 1e34
    ref = GC.window_reference(H.astype(np.float32), (60, 80), (480, 608))
    assert not ref['nonfinite'].any()


def test_rescale_scales_contain_knife_edges():
    """The fp32 expression is the specification; it differs from the exact floor at >= 50 integer coordinates for each scale
    (none for the dyadic scales the other tests use), so a device division that is not correctly rounded cannot pass."""
    counts = {s: GC.rescale_knife_edges(8, s) for s in GC.RESCALE_SCALES}
    print(counts)
    assert len(counts) >= 5 and all(c >= 50 for c in counts.values()), counts
    assert [GC.rescale_knife_edges(8, s) for s in (1.0, 1.25, 1.5)] == [0, 0, 0]
    mk0, mk1, cnt, s0, s1 = GC.rescale_case()
    assert cnt[0] == len(mk0) == len(mk1) == cnt[1:].sum() and len(cnt) - 1 == len(s0) == len(s1) == len(GC.RESCALE_SCALES)
    n = int(cnt[1])
    assert set(range(0, 1281, 8)) <= set(mk0[:n, 0].astype(int)) and set(range(0, 1281, 8)) <= set(mk0[:n, 1].astype(int))
    assert set(range(1281)) <= set(mk0[:n, 0].astype(int)) and set(range(1281)) <= set(mk1[:n, 1].astype(int))
    assert (s0[:, 0] != s0[:, 1]).all() and (s1[:, 0] != s1[:, 1]).all() and (s0 != s1).all()
    # every scale of the list reaches both axes of both images
    for col in (s0[:, 0], s0[:, 1], s1[:, 0], s1[:, 1]):
        assert sorted(col.tolist()) == sorted(np.float32(GC.RESCALE_SCALES).tolist())


def test_inlier_reference_and_cases():
    names = [n for n, _ in GC.inlier_cases()]
    assert names == ['6400x6400', '4800x4560', '1024x1025', '1x3']
    for name, c in GC.inlier_cases():
        r = GC.inlier_reference(**c)
        L, S = c['L'], c['S']
        assert r['nidx'][0].tolist() == [L, S] and r['nidx'][1].tolist() == [0, 0] and r['nidx'][2].tolist() == [0, 0], name
        assert r['idx0'][3].tolist() == [0] and r['idx1'][3].tolist() == [0], name
        assert r['idx0'][4].tolist() == [L - 1] and r['idx1'][4].tolist() == [S - 1], name
        assert int(c['counts'][1 + 2]) == 0 and int(c['counts'][1 + 5]) > max(L, S), name
        assert all((np.diff(i) > 0).all() for i in r['idx0'] + r['idx1']), name
    assert int(GC.inlier_cases()[0][1]['counts'][1 + 5]) > 6400


EXPECT_MODEL = {'one_row': True, 'one_column': True, 'one_point': True, 'both_collinear': False, 'collinear_plus3': True,
                'two_rows': True}


def test_degenerate_sets_under_the_ransac_oracle():
    """Which sets give a model: only 'both_collinear' finds no hypothesis.  'one_row', 'one_column' and 'one_point' give models that
    are singular to working precision (cond(M) > 1e12; for 'one_column' the determinant of the CPU statement's M is 0 or next to
    it, so an adjugate inverse is non-finite or above 1e30): the RANSAC as stated does return them, which is why the GPU test
    asserts finiteness under valid == 1 and the window contract for whatever comes out."""
    conds = {}
    for b, (name, p0, p1) in enumerate(GC.degenerate_match_sets()):
        M, mask = RO.find_homography(p0, p1, sample=b)
        assert (M is not None) == EXPECT_MODEL[name], name
        if M is None:
            assert not mask.any(), name
            continue
        conds[name] = float(np.linalg.cond(M))
        assert np.isfinite(M.astype(np.float32)).all() and mask.sum() >= 58, name
        inv = GC.adjugate_inverse(M)
        print(name, 'cond %.3g' % conds[name], 'max |adjugate inverse| %.3g' % np.abs(inv).max())
        if name in ('one_row', 'one_column'):
            assert not np.abs(inv).max() < 1e30, name                   # (nan / inf included)
        if name in ('collinear_plus3', 'two_rows'):
            assert np.abs(inv.astype(np.float32)).max() < 1e5, name
    assert conds['one_row'] > 1e12 and conds['one_column'] > 1e12 and conds['one_point'] > 1e12
    assert 1e5 < conds['collinear_plus3'] < 1e8 and conds['two_rows'] < 1e4
