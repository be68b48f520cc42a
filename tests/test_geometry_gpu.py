"""The geometry stage on the GPU (window_geometry, inlier_index, the RANSAC keypoint rescale, model validity, GeoModule.geometry)
through geoformer_amd.ops - the C ABI - against the float64 / fp32-specification references of tests/geometry_cases.py.  No kernel
is compared with another kernel; the only self-comparisons are the stated repeat-call and with / without-flags equalities.

Two contracts are pinned here:
  * every entry of a window table is -1 or a cell of the key grid, for ANY matrix (inf, nan, 1e34, the inverse of a singular
    model): the tables are read back on the host - none of them is handed to an attention kernel;
  * valid == 1 implies that M, M_f32 and Minv_f32 are finite.

Measured on one MI355X (every figure is printed by the tests; run with -s):
  * window_geometry, exact class: 12 matrices x 2 shapes, 0 differences anywhere.
  * generic class (28 matrices), entries compared exactly / in the band / differing (all inside the band), per window-scale mode
    none, (1.25, 1.5), (1.2, 0.8):  80 x 80 -> 640 x 640: 4 473 410 / 6 590 / 75,  4 473 405 / 6 595 / 75,  4 473 344 / 6 656 / 116;
    60 x 80 -> 480 x 608: 3 355 615 / 4 385 / 75,  3 355 655 / 4 345 / 75,  3 355 874 / 4 126 / 80.  None differs outside the band.
  * horizon class (5 matrices): 80 x 80: 762 039 / 37 961 / 600,  762 115 / 37 885 / 595,  765 628 / 34 372 / 731;
    60 x 80: 569 107 / 30 893 / 445,  569 174 / 30 826 / 434,  571 716 / 28 284 / 556.  None outside the band.
    (The CPU's torch fp32 path differs from float64 at 100 / 100 / 109 and 75 / 75 / 80 generic entries: the device contracts to FMA.)
  * contract for any matrix: 1 607 950 (80 x 80) and 1 206 950 (60 x 80) entries with a non-finite reference coordinate, all -1.
    BEFORE the bounds test was made NaN-proof this test failed with
        AssertionError: ('row0_inf', 'non-finite reference coordinate not masked', [-1, 0, 80, 160, 240, 320, ...])
    gfx950 converts NaN to 0, so the old predicate left such entries UNMASKED and in range: an all-nan matrix gave cell 0 for all
    160 000 entries, a nan x coordinate gave cells 0, 80, 160, ... (row of the finite y, column 0).  No entry was ever out of range.
  * keypoint rescale: 40 376 coordinates, 13 572 of them knife edges (fp32 expression != exact floor), all exact.
  * singular models: one_row valid, cond 5e18, max |Minv_f32| 1.6e34; one_column valid, cond 1.7e36, 4.9e34; one_point valid,
    cond 6.9e21, 7.3; both_collinear no model; collinear_plus3 cond 3.0e6, Minv error 5.3e-9 (tolerance 6.0e-8); two_rows cond 834.
    No valid sample had a non-finite matrix, so ransac_final was left as it is.  The CPU statement's M for one_column has
    determinant exactly 0 (adjugate inverse inf / nan); the device's block sums run in another order and its M (equal to 1e-9)
    has a tiny non-zero one: finiteness there is measured, not constructed.
  * wiring: win1 / win0 of the two valid samples 119 854 / 113 883 and 119 805 / 113 747 compared exactly, 146 / 117 and 195 / 253
    in the band, 0 differing; each swap on the reference side gives 39 753 ... 116 924 violations.
"""
import numpy as np
import pytest
import torch

import geometry_cases as GC
import ransac_oracle as RO

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _mats(kinds):
    out = [(k, n, H) for k in kinds for n, H in GC.homographies(k)]
    return out, _t(np.stack([H for _, _, H in out]), torch.float32)


def _wscale_arg(ws, N):
    return None if ws is None else _t(np.tile(np.float32(ws), (N, 1)))


# ------------------------------------------------------------------------------------------------ 1. window_geometry, exact class
@pytest.mark.parametrize('grid,img', GC.SHAPES)
def test_window_geometry_exact_class(grid, img):
    """Integer / half-integer coordinates, every window position on a decision boundary: kps, mask and win equal the float64
    reference everywhere, no band."""
    from geoformer_amd import ops
    mats, Hm = _mats(['exact'])
    win, kps, warped = ops.window_geometry(Hm, None, grid, img, img[1] // 8, 8, 5, debug=True)
    win, kps, warped = win.cpu().numpy(), kps.cpu().numpy(), warped.cpu().numpy()
    for b, (_, name, H) in enumerate(mats):
        ref = GC.window_reference(H.astype(np.float32), grid, img)
        np.testing.assert_array_equal(warped[b].astype(np.float64), ref['warped'], err_msg=name)
        np.testing.assert_array_equal(kps[b], ref['kps'], err_msg=name)
        np.testing.assert_array_equal(win[b] >= 0, ref['mask'], err_msg=name)
        np.testing.assert_array_equal(win[b], ref['cell'], err_msg=name)


# ------------------------------------------------------------------------------------------------ 2. generic and horizon classes
@pytest.mark.parametrize('wscale', GC.WSCALES, ids=str)
@pytest.mark.parametrize('grid,img', GC.SHAPES)
def test_window_geometry_generic_and_horizon(grid, img, wscale):
    """Outside the band kps, mask and win equal the float64 reference; inside it only the neighbouring integer or the mask flip at
    the border the entry sits on; `warped` within delta wherever |w| is above the helper's floor.  The share caps are re-asserted
    on what was actually compared."""
    from geoformer_amd import ops
    mats, Hm = _mats(['generic', 'horizon'])
    N = len(mats)
    win, kps, warped = ops.window_geometry(Hm, None, grid, img, img[1] // 8, 8, 5, window_scale=_wscale_arg(wscale, N), debug=True)
    win, kps, warped = win.cpu().numpy(), kps.cpu().numpy(), warped.cpu().numpy()
    tot = {k: np.zeros(5, np.int64) for k in ('generic', 'horizon')}       # compared, band, differs, differs outside, violations
    for b, (kind, name, H) in enumerate(mats):
        ref = GC.window_reference(H.astype(np.float32), grid, img, wscale=wscale)
        viol, differs = GC.band_rule_violations(ref, kps[b], win[b])
        ok = ~ref['wild']
        werr = np.abs(warped[b].astype(np.float64) - ref['warped'])[ok].max(-1)
        assert (werr <= ref['delta'][ok]).all(), (name, float((werr / ref['delta'][ok]).max()))
        share = float(ref['band'].mean())
        if kind == 'generic':
            assert share <= GC.BAND_SHARE_CAP and not ref['wild'].any(), (name, share)
        else:
            assert 1.0 - share >= GC.HORIZON_COMPARABLE_MIN, (name, share)
        out = int((differs & ~ref['band']).sum())
        tot[kind] += [int((~ref['band']).sum()), int(ref['band'].sum()), int(differs.sum()), out, int(viol.sum())]
        assert out == 0 and not viol.any(), (name, out, int(viol.sum()), np.argwhere(viol)[:5].tolist())
    for kind, t in tot.items():
        print(f'window_geometry {kind} {grid}->{img} wscale {wscale}: {t[0]} compared exactly, {t[1]} in the band, {t[2]} differ '
              f'(inside the band), {t[3]} differ outside, {t[4]} violations')
        assert t[0] > 100 * t[1] if kind == 'generic' else t[0] > t[1]


# ------------------------------------------------------------------------------------------------ 3. the contract for any matrix
def _singular_inverse_f32():
    """fp32 adjugate inverse of the 'one_row' model (60 inliers, det ~ 1e-32, entries up to ~3e34) as the C oracle finds it."""
    name, p0, p1 = GC.degenerate_match_sets()[0]
    M, _ = RO.find_homography(p0, p1, sample=0)
    assert name == 'one_row' and M is not None
    inv = GC.adjugate_inverse(M).astype(np.float32)
    assert np.isfinite(inv).all() and np.abs(inv).max() > 1e30
    return inv


def _hostile_matrices():
    eye = np.eye(3, dtype=np.float32)
    out = []
    for row in range(3):
        for bad in (np.inf, -np.inf, np.nan):
            H = eye.copy(); H[row, :] = bad
            out.append((f'row{row}_{bad}', H))
    H = eye.copy(); H[0, 2] = np.nan
    out.append(('nan_tx', H))
    H = eye.copy(); H[2, 2] = np.inf
    out.append(('inf_h33', H))
    out.append(('all_nan', np.full((3, 3), np.nan, np.float32)))
    out.append(('adjugate_over_zero', np.array([[np.inf, np.nan, -np.inf], [-np.inf, np.nan, np.inf], [-np.inf, np.nan, np.inf]], np.float32)))
    for row in range(3):
        H = eye.copy(); H[row, :] = [1e34, -1e34, 1e34]
        out.append((f'row{row}_1e34', H))
    out.append(('all_1e34', np.full((3, 3), 1e34, np.float32)))
    out.append(('singular_model_inverse', _singular_inverse_f32()))
    out.append(('zeros', np.zeros((3, 3), np.float32)))
    return out


def _check_contract(name, win, ref, ncell):
    bad = GC.window_contract_violations(win, ncell)
    assert not bad.any(), (name, int(bad.sum()), np.unique(win[bad])[:8].tolist())
    nf = ref['nonfinite']
    assert (win[nf] == -1).all(), (name, 'non-finite reference coordinate not masked', np.unique(win[nf])[:8].tolist())


@pytest.mark.parametrize('wscale', [None, (1.2, 0.8)], ids=str)
@pytest.mark.parametrize('grid,img', GC.SHAPES)
def test_window_geometry_contract_any_matrix(grid, img, wscale):
    """Finite matrices mixed with rows of inf / nan, entries of 1e34 and the fp32 inverse of a singular RANSAC model: every entry is
    -1 or a cell of the key grid, a non-finite reference coordinate gives -1, and the finite samples are what they are alone.
    The tables are only read back on the host."""
    from geoformer_amd import ops
    finite = [(n, H.astype(np.float32)) for n, H in GC.homographies('generic')[:4] + GC.homographies('horizon')[:2]]
    hostile = _hostile_matrices()
    mixed = []
    for i, h in enumerate(hostile):                      # interleaved: a finite sample between hostile ones
        mixed.append(h)
        if i < len(finite):
            mixed.append(finite[i])
    N = len(mixed)
    ncell = -(-img[0] // 8) * (img[1] // 8)
    Hm = _t(np.stack([H for _, H in mixed]))
    win, kps, _ = ops.window_geometry(Hm, None, grid, img, img[1] // 8, 8, 5, window_scale=_wscale_arg(wscale, N), debug=True)
    alone = ops.window_geometry(_t(np.stack([H for _, H in finite])), None, grid, img, img[1] // 8, 8, 5,
                                window_scale=_wscale_arg(wscale, len(finite)))
    win, kps, alone = win.cpu().numpy(), kps.cpu().numpy(), alone.cpu().numpy()
    names = [n for n, _ in mixed]
    n_nf = 0
    for b, (name, H) in enumerate(mixed):
        ref = GC.window_reference(H, grid, img, wscale=wscale)
        _check_contract(name, win[b], ref, ncell)
        viol, _ = GC.band_rule_violations(ref, kps[b], win[b])
        assert not viol.any(), (name, int(viol.sum()), np.argwhere(viol)[:5].tolist())
        n_nf += int(ref['nonfinite'].sum()) * 25
    for i, (name, _) in enumerate(finite):
        np.testing.assert_array_equal(win[names.index(name)], alone[i], err_msg=name)
    print(f'contract {grid}->{img} wscale {wscale}: {N} matrices, {n_nf} entries with a non-finite reference coordinate, all -1')
    assert n_nf > 25 * grid[0] * grid[1] * 8


# ------------------------------------------------------------------------------------------------ 4. valid flags + window_scale
def test_window_geometry_valid_flags_with_window_scale():
    from geoformer_amd import ops
    grid, img = GC.SHAPES[1]
    mats, Hm = _mats(['horizon', 'exact'])
    N = len(mats)
    rng = np.random.default_rng(3)
    ws = _t(rng.choice(np.float32(GC.RESCALE_SCALES + [1.25, 1.5]), (N, 2)))
    flags = np.arange(N) % 3 != 1
    flags[0], flags[-1] = False, True
    plain = ops.window_geometry(Hm, None, grid, img, img[1] // 8, 8, 5, window_scale=ws)
    w2, k2, _ = ops.window_geometry(Hm, _t(flags.astype(np.int32)), grid, img, img[1] // 8, 8, 5, window_scale=ws, debug=True)
    for b in range(N):
        if flags[b]:
            assert torch.equal(w2[b], plain[b]), b
        else:
            assert bool((w2[b] == -1).all()), b
    # the per-sample scales really are per sample: each table equals the reference of ITS pair
    w2 = w2.cpu().numpy(); k2 = k2.cpu().numpy(); wsn = ws.cpu().numpy()
    for b in np.nonzero(flags)[0]:
        ref = GC.window_reference(mats[b][2].astype(np.float32), grid, img, wscale=tuple(wsn[b]))
        viol, differs = GC.band_rule_violations(ref, k2[b], w2[b])
        assert not viol.any() and not (differs & ~ref['band']).any(), mats[b][1]


# ------------------------------------------------------------------------------------------------ 5. inlier_index
@pytest.mark.parametrize('case', [c for _, c in GC.inlier_cases()], ids=[n for n, _ in GC.inlier_cases()])
def test_inlier_index_chunks_and_edges(case):
    """(L, S) at one 1024-cell chunk exactly, one more, 6400 and an unequal pair; all cells, no cell, only the first, only the last;
    an empty sample; more matches than cells.  Maps, nidx and idx[:nidx] exact; a second call is bit-identical."""
    from geoformer_amd import ops
    ref = GC.inlier_reference(**case)
    N = len(case['counts']) - 1
    args = (_t(case['kp0']), _t(case['kp1']), _t(case['keep']), _t(case['counts']), N, case['L'], case['S'], case['w0'], case['w1'])
    g = ops.inlier_index(*args)
    h = ops.inlier_index(*args)
    nidx = g['nidx'].cpu().numpy()
    np.testing.assert_array_equal(nidx, ref['nidx'])
    np.testing.assert_array_equal(g['map0'].cpu().numpy() != 0, ref['map0'])
    np.testing.assert_array_equal(g['map1'].cpu().numpy() != 0, ref['map1'])
    assert set(np.unique(g['map0'].cpu().numpy())) <= {0, 1} and set(np.unique(g['map1'].cpu().numpy())) <= {0, 1}
    for b in range(N):
        np.testing.assert_array_equal(g['idx0'][b, :nidx[b, 0]].cpu().numpy(), ref['idx0'][b], err_msg=str(b))
        np.testing.assert_array_equal(g['idx1'][b, :nidx[b, 1]].cpu().numpy(), ref['idx1'][b], err_msg=str(b))
        assert torch.equal(g['idx0'][b, :nidx[b, 0]], h['idx0'][b, :nidx[b, 0]]) and torch.equal(g['idx1'][b, :nidx[b, 1]], h['idx1'][b, :nidx[b, 1]])
    assert torch.equal(g['map0'], h['map0']) and torch.equal(g['map1'], h['map1']) and torch.equal(g['nidx'], h['nidx'])


# ------------------------------------------------------------------------------------------------ 6. keypoint rescale
def test_ransac_keypoint_rescale_knife_edges():
    """kp / (scale * scale0[b]) * scale in fp32, then .long(): every multiple of 8 in 0..1280 on both axes and every integer on one,
    at non-dyadic scales where the fp32 expression differs from the exact floor at 75 ... 1280 coordinates.  An integer keypoint
    is right or wrong: exact equality."""
    from geoformer_amd import ops
    mk0, mk1, counts, s0, s1 = GC.rescale_case()
    N = len(s0)
    rs = ops.ransac_homography(_t(mk0), _t(mk1), _t(counts), N, 8, _t(s0), _t(s1), integer_keypoints=True)
    kp0, kp1 = rs['kp0'].cpu().numpy(), rs['kp1'].cpu().numpy()
    n = int(counts[1])
    edges = 0
    for b in range(N):
        sl = slice(b * n, (b + 1) * n)
        for got, mk, s in ((kp0[sl], mk0[sl], s0[b]), (kp1[sl], mk1[sl], s1[b])):
            want = GC.keypoint_rescale_reference(mk, 8, s).numpy()
            np.testing.assert_array_equal(got.astype(np.int64), want, err_msg=f'sample {b} scales {s}')
            assert (got == np.floor(got)).all()
            for c in range(2):
                edges += int((want[:, c] != GC.rescale_exact_floor(mk[:, c].astype(np.int64), 8, s[c])).sum())
    print(f'keypoint rescale: {2 * N * n * 2} coordinates exact, {edges} of them knife edges (fp32 expression != exact floor)')
    assert edges > 1000
    # without per-image scales: only the first .long()
    r0 = ops.ransac_homography(_t(mk0), _t(mk1), _t(counts), N, 8)
    np.testing.assert_array_equal(r0['kp0'].cpu().numpy(), np.floor(mk0))
    np.testing.assert_array_equal(r0['kp1'].cpu().numpy(), np.floor(mk1))


# ------------------------------------------------------------------------------------------------ 7. singular models
def test_ransac_singular_models_and_their_windows():
    """Match sets whose best model is singular or nearly so.  valid / keep / M agree with the C oracle as in
    test_ransac_matches_c_oracle_bit_exact_mask; valid == 1 implies finite M, M_f32, Minv_f32 and Minv_f32 == fp32(inv(M)) to a
    tolerance derived from cond(M); valid == 0 gives keep all ones and zero matrices.  The returned matrices then go through
    window_geometry, whose tables are checked on the host against the contract (never handed to attention)."""
    from geoformer_amd import ops
    sets = GC.degenerate_match_sets()
    N = len(sets)
    counts = np.array([sum(len(s[1]) for s in sets)] + [len(s[1]) for s in sets], np.int32)
    mk0 = np.concatenate([s[1] for s in sets]).astype(np.float32)
    mk1 = np.concatenate([s[2] for s in sets]).astype(np.float32)
    rs = ops.ransac_homography(_t(mk0), _t(mk1), _t(counts), N, 8)
    valid = rs['valid'].cpu().numpy()
    M, Mf, Mi, keep = rs['M'].cpu().numpy(), rs['M_f32'].cpu().numpy(), rs['Minv_f32'].cpu().numpy(), rs['keep'].cpu().numpy()
    off = 0
    conds = {}
    for b, (name, p0, p1) in enumerate(sets):
        n = len(p0)
        Mo, mask = RO.find_homography(p0, p1, sample=b)
        print(f'{name}: valid {valid[b]} oracle {Mo is not None} max|Minv_f32| {np.abs(Mi[b]).max():.3g} finite '
              f'{bool(np.isfinite(M[b]).all() and np.isfinite(Mf[b]).all() and np.isfinite(Mi[b]).all())}')
        if valid[b]:
            assert np.isfinite(M[b]).all() and np.isfinite(Mf[b]).all() and np.isfinite(Mi[b]).all(), \
                (name, 'valid == 1 with a non-finite matrix', Mi[b].tolist())
        assert int(valid[b]) == int(Mo is not None), name
        if Mo is not None:
            np.testing.assert_array_equal(keep[off:off + n], mask[:, 0], err_msg=name)
            np.testing.assert_allclose(M[b], Mo, rtol=1e-9, atol=1e-9, err_msg=name)
            np.testing.assert_array_equal(Mf[b], M[b].astype(np.float32), err_msg=name)
            conds[name] = float(np.linalg.cond(M[b]))
            tol = GC.minv_f32_tolerance(M[b])
            if tol < 1.0:
                inv = np.linalg.inv(M[b])
                err = np.abs(Mi[b].astype(np.float64) - inv).max() / np.abs(inv).max()
                print(f'    cond {conds[name]:.3g} tolerance {tol:.3g} error {err:.3g}')
                assert err <= tol, (name, err, tol)
            else:           # cond(M) >= 2^52: an fp64 inverse has no correct digit (numpy may refuse it as singular); finiteness is the claim
                print(f'    cond {conds[name]:.3g}: no digit of an fp64 inverse is determined, only finiteness is asserted')
        else:
            np.testing.assert_array_equal(keep[off:off + n], np.ones(n, np.uint8), err_msg=name)
            assert not M[b].any() and not Mf[b].any() and not Mi[b].any(), name
        off += n
    assert max(conds.values()) > 1e12 and conds['two_rows'] < 1e4          # a near-singular valid model and the control
    for (grid, img), mat in ((((60, 80), (480, 608)), rs['M_f32']), (((60, 76), (480, 640)), rs['Minv_f32'])):
        win = ops.window_geometry(mat, rs['valid'], grid, img, img[1] // 8, 8, 5).cpu().numpy()
        ncell = (img[0] // 8) * (img[1] // 8)
        for b, (name, _, _) in enumerate(sets):
            ref = GC.window_reference(mat[b].cpu().numpy(), grid, img)
            _check_contract(name, win[b], ref, ncell)
            if valid[b]:
                viol, _ = GC.band_rule_violations(ref, None, win[b])
                assert not viol.any(), (name, int(viol.sum()))
            else:
                assert (win[b] == -1).all(), name


# ------------------------------------------------------------------------------------------------ 8. GeoModule.geometry wiring
def test_geomodule_geometry_wiring():
    """An unequal pair (480 x 640 against 480 x 608), per-image scales that differ between the images and between x and y, one
    sample without a model.  Everything GeoModule.geometry derives from its RANSAC result is rebuilt in numpy from that result.

    Which assertion catches which swap:
      * s0 <-> s1 in the ransac call: the kp0 / kp1 comparison with keypoint_rescale_reference (each image's own scale);
      * s0 <-> s1 in the two window_geometry calls: the band rule on win1 (image 1's scale) and win0 (image 0's scale) - the
        negative control below rebuilds the reference with the pair swapped and requires violations;
      * hw0c <-> hw1c: the shapes of win0 / win1 / idx0 / idx1 (4800 against 4560 cells) and the cell indices of the tables (key
        grid width 80 against 76) - negative control: the reference with the other grid width is violated;
      * M <-> M^-1: the band rule on both tables - negative control with the matrices swapped."""
    from geoformer_amd.model.geo_config import get_cfg_model
    from geoformer_amd.model.modules import GeoModule
    hw0, hw1 = (480, 640), (480, 608)
    hw0c, hw1c = (60, 80), (60, 76)
    N = 3
    Hs = [np.array([[0.93, -0.11, 44.3], [0.08, 0.97, -9.6], [1e-4, -5e-5, 1]]), None,
          np.array([[1.12, 0.08, -21.0], [-0.05, 0.9, 37.5], [2e-4, -1.3e-4, 1]])]
    sets = [GC.planted_matches(700, 210, Hs[0], hw0, hw1, 1), GC.planted_matches(5, 0, Hs[0], hw0, hw1, 2),
            GC.planted_matches(500, 150, Hs[2], hw0, hw1, 3)]
    scale0 = np.float32([[1.2, 1.6], [1.1, 1.25], [1.5, 1.7]])
    scale1 = np.float32([[1.6, 1.1], [1.7, 1.2], [1.25, 1.5]])
    mk0 = np.concatenate([s[0] for s in sets]).astype(np.float32)
    mk1 = np.concatenate([s[1] for s in sets]).astype(np.float32)
    cnt = [len(s[0]) for s in sets]
    batch = {'image0': torch.empty(N, 1, *hw0), 'image1': torch.empty(N, 1, *hw1), 'hw0_i': hw0, 'hw0_c': hw0c,
             'm_bids': _t(np.repeat(np.arange(N), cnt)), 'mkpts0_c': _t(mk0), 'mkpts1_c': _t(mk1),
             'scale0': _t(scale0), 'scale1': _t(scale1)}
    geo = GeoModule(get_cfg_model(), 256).geometry(batch, N, hw0c, hw1c, torch.device(DEV))
    rs = geo['ransac']
    valid = rs['valid'].cpu().numpy()
    assert valid.tolist() == [1, 0, 1] and torch.equal(geo['valid'], rs['valid'])
    L, S = hw0c[0] * hw0c[1], hw1c[0] * hw1c[1]
    assert tuple(geo['win1'].shape) == (N, L, 25) and tuple(geo['win0'].shape) == (N, S, 25)
    assert tuple(geo['idx0'].shape) == (N, L) and tuple(geo['idx1'].shape) == (N, S) and 'idx_both' not in geo and 'nidx_both' not in geo
    assert geo['hw0'] == hw0c and geo['hw1'] == hw1c
    # the keypoints: each image's own scale
    kp0, kp1, keep = rs['kp0'].cpu().numpy(), rs['kp1'].cpu().numpy(), rs['keep'].cpu().numpy()
    off = 0
    for b in range(N):
        sl = slice(off, off + cnt[b])
        np.testing.assert_array_equal(kp0[sl].astype(np.int64), GC.keypoint_rescale_reference(mk0[sl], 8, scale0[b]).numpy())
        np.testing.assert_array_equal(kp1[sl].astype(np.int64), GC.keypoint_rescale_reference(mk1[sl], 8, scale1[b]).numpy())
        assert (GC.keypoint_rescale_reference(mk0[sl], 8, scale1[b]).numpy() != kp0[sl]).any()       # the swap would show
        off += cnt[b]
    assert keep[cnt[0]:cnt[0] + cnt[1]].all() and 0.5 * cnt[0] < keep[:cnt[0]].sum() < 0.8 * cnt[0]
    # maps and index lists from ITS kp0, kp1, keep: exact
    counts = np.array([sum(cnt)] + cnt, np.int32)
    ref = GC.inlier_reference(kp0, kp1, keep[:sum(cnt)], counts, L, S, hw0c[1], hw1c[1])
    nidx = geo['nidx'].cpu().numpy()
    np.testing.assert_array_equal(nidx, ref['nidx'])
    np.testing.assert_array_equal(geo['nidx_t'].cpu().numpy(), ref['nidx'].T)
    assert geo['nidx_t'].is_contiguous()
    np.testing.assert_array_equal(geo['map0'].cpu().numpy() != 0, ref['map0'])
    np.testing.assert_array_equal(geo['map1'].cpu().numpy() != 0, ref['map1'])
    for b in range(N):
        np.testing.assert_array_equal(geo['idx0'][b, :nidx[b, 0]].cpu().numpy(), ref['idx0'][b])
        np.testing.assert_array_equal(geo['idx1'][b, :nidx[b, 1]].cpu().numpy(), ref['idx1'][b])
    # the window tables from ITS M
    M = rs['M'].cpu().numpy()
    win0, win1 = geo['win0'].cpu().numpy(), geo['win1'].cpu().numpy()
    for b in range(N):
        if not valid[b]:
            assert (win0[b] == -1).all() and (win1[b] == -1).all()
            continue
        Mf, Mi = M[b].astype(np.float32), np.linalg.inv(M[b]).astype(np.float32)
        np.testing.assert_array_equal(rs['M_f32'][b].cpu().numpy(), Mf)
        r1 = GC.window_reference(Mf, hw0c, hw1, wscale=tuple(scale1[b]))          # image-0 grid into image 1, image 1's scale
        r0 = GC.window_reference(Mi, hw1c, hw0, wscale=tuple(scale0[b]))          # image-1 grid into image 0, image 0's scale
        for tag, r, w in (('win1', r1, win1[b]), ('win0', r0, win0[b])):
            viol, differs = GC.band_rule_violations(r, None, w)
            print(f'wiring sample {b} {tag}: {int((~r["band"]).sum())} compared exactly, {int(r["band"].sum())} in the band, '
                  f'{int(differs.sum())} differ, {int(viol.sum())} violations')
            assert not viol.any() and not (differs & ~r['band']).any(), (b, tag, int(viol.sum()))
            assert r['band'].mean() <= GC.BAND_SHARE_CAP and (r['cell'] >= 0).mean() > 0.3, (b, tag)
        # negative controls (the swaps, made on the reference side): each is violated
        wrong = {'scales swapped': (GC.window_reference(Mf, hw0c, hw1, wscale=tuple(scale0[b])), win1[b]),
                 'scales swapped (win0)': (GC.window_reference(Mi, hw1c, hw0, wscale=tuple(scale1[b])), win0[b]),
                 'M and inverse swapped': (GC.window_reference(Mi, hw0c, hw1, wscale=tuple(scale1[b])), win1[b]),
                 'images swapped': (GC.window_reference(Mf, hw0c, hw0, wscale=tuple(scale1[b])), win1[b])}
        for what, (r, w) in wrong.items():
            v = int(GC.band_rule_violations(r, None, w)[0].sum())
            print(f'    control, {what}: {v} violations')
            assert v > 1000, what
