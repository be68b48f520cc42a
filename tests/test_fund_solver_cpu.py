"""The fundamental-matrix RANSAC as stated in geoformer_amd/csrc/fund_solver.h, through its host build (csrc/host/fund_host.cpp: the
serial form of what k_fundamental.hip runs on the device).  No GPU.  Scenes and the independent numpy solver: tests/fund_cases.py."""
import numpy as np
import pytest

import fund_cases as C

# Bounds of the minimal-solver tests.  Basis: the independent numpy solver of fund_cases.py (SVD null space, cubic through four sampled
# determinants, numpy.roots) over the same 1000 scenes has the worst values on the left; each bound is ~300x that, which leaves room for
# another elimination order and root finder, while a wrong solver misses the held-out points by more than 0.1 px.
#   largest held-out Sampson distance of the best root     numpy 6.5e-9 px    (host build: 3.5e-9)     bound 2e-6
#   largest Sampson distance of the seven points, any root  numpy 1.5e-11 px   (host build: 1.8e-11)    bound 5e-9
#   largest |det F| of any root (Frobenius norm 1, pixels)  numpy 8.2e-18      (host build: 1.4e-17)    bound 3e-15
HELD_OUT_BOUND = 2e-6
SEVEN_BOUND = 5e-9
DET_BOUND = 3e-15


# ------------------------------------------------------------------------------------------------------------ minimal solver
@pytest.fixture(scope='module')
def minimal_runs():
    out = []
    for seed in range(1000):
        p0, p1, norm, F = C.minimal_scene(seed)
        out.append((p0, p1, norm, C.host_seven_point(p0[:7], p1[:7], norm), C.numpy_seven_point(p0[:7], p1[:7], norm)))
    return out


def test_best_root_fits_the_held_out_points(minimal_runs):
    """1000 seeded scenes of seven exact fp64 correspondences plus 50 held-out ones (the box over all 57): for the best root the largest
    held-out Sampson distance is below HELD_OUT_BOUND.  numpy's worst on this generator: 6.5e-9 px; bound 2e-6 px (~300x)."""
    worst, worst_np = 0.0, 0.0
    for p0, p1, norm, Fs, Fn in minimal_runs:
        assert len(Fs) > 0
        worst = max(worst, min(C.sampson_px(F, p0[7:], p1[7:]).max() for F in Fs))
        worst_np = max(worst_np, min(C.sampson_px(F, p0[7:], p1[7:]).max() for F in Fn))
    print(f'worst held-out Sampson distance over 1000 scenes: host build {worst:.3e} px, numpy solver {worst_np:.3e} px')
    assert worst_np < HELD_OUT_BOUND / 100 and worst < HELD_OUT_BOUND


def test_every_root_is_singular_of_norm_one_and_fits_its_seven_points(minimal_runs):
    wd, ws, wd_np, ws_np = 0.0, 0.0, 0.0, 0.0
    for p0, p1, norm, Fs, Fn in minimal_runs:
        for F in Fs:
            assert abs(np.linalg.norm(F) - 1) < 1e-12
            wd = max(wd, abs(np.linalg.det(F)))
            ws = max(ws, C.sampson_px(F, p0[:7], p1[:7]).max())
        for F in Fn:
            wd_np = max(wd_np, abs(np.linalg.det(F)))
            ws_np = max(ws_np, C.sampson_px(F, p0[:7], p1[:7]).max())
    print(f'worst |det F|: host build {wd:.3e}, numpy {wd_np:.3e}; worst Sampson distance of the seven: host build {ws:.3e} px, numpy {ws_np:.3e} px')
    assert wd_np < DET_BOUND / 100 and ws_np < SEVEN_BOUND / 100
    assert wd < DET_BOUND and ws < SEVEN_BOUND


def test_root_counts_are_one_or_three_and_agree_with_numpy(minimal_runs):
    counts = [len(Fs) for _, _, _, Fs, _ in minimal_runs]
    assert set(counts) == {1, 3}, sorted(set(counts))
    assert counts == [len(Fn) for _, _, _, _, Fn in minimal_runs]
    print(f'{counts.count(3)} scenes with 3 roots, {counts.count(1)} with 1')


def test_seven_point_fails_cleanly_on_non_finite_and_degenerate_input():
    p0, p1, norm, _ = C.minimal_scene(0)
    p0, p1 = p0[:7], p1[:7]
    for v in (np.nan, np.inf, -np.inf):
        bad = p0.copy(); bad[2, 1] = v
        assert len(C.host_seven_point(bad, p1, norm)) == 0
        bad = p1.copy(); bad[6, 0] = v
        assert len(C.host_seven_point(p0, bad, norm)) == 0
    unit = np.array([0.0, 0, 1, 0, 0, 1])
    assert len(C.host_seven_point(np.zeros((7, 2)), np.zeros((7, 2)), unit)) == 0           # rank 1: the pivot search fails
    assert len(C.host_seven_point(np.repeat(p0[:1], 7, 0), np.repeat(p1[:1], 7, 0), norm)) == 0     # seven copies of one match
    assert len(C.host_seven_point(p0, p1, np.array([0.0, 0, 0, 0, 0, 1]))) == 0              # a box without extent: division by zero
    assert len(C.host_seven_point(p0, p1, np.full(6, np.nan))) == 0


def test_vanishing_leading_coefficient():
    """det(x F1 + F2) with det F1 == 0 to the last bit (a zero row): the cubic's leading coefficient vanishes.  The pencil is then read
    from its other end, where F1 itself is the root 0: finite solutions, F1 among them."""
    F1 = np.array([[1.0, 2, 3], [4, 5, 6], [0, 0, 0]])
    F2 = np.array([[2.0, -1, 0], [1, 3, -2], [0, 1, 4]])
    assert np.linalg.det(F2) != 0
    for a, b in ((F1, F2), (F2, F1)):
        Fs = C.host_pencil(a, b)
        assert len(Fs) in (1, 3) and np.isfinite(Fs).all()
        assert all(abs(np.linalg.norm(F) - 1) < 1e-12 and abs(np.linalg.det(F)) < 1e-14 for F in Fs)
        assert min(min(np.abs(F - F1 / np.linalg.norm(F1)).max(), np.abs(F + F1 / np.linalg.norm(F1)).max()) for F in Fs) < 1e-12
    both = C.host_pencil(F1, F1[[2, 0, 1]])                          # both ends singular to the last bit: no leading coefficient at all
    assert len(both) == 0
    assert np.isfinite(C.host_pencil(np.zeros((3, 3)), np.zeros((3, 3)))).all()


# ------------------------------------------------------------------------------------------------------------ RANSAC, serial form
# Scene seeds.  The selection rule has no refit, so the winner is ONE seven-point model; away from its inliers' support it can differ
# from the planted F and accept a far outlier (scanned scene seeds 100 .. 115 at 30 %: 101, 104 and 112 accept rows 1.8 .. 69 px from the
# planted line, in the numpy RANSAC exactly as in the host build).  The scenes below are those of 100 .. 109 where the NUMPY RANSAC over the
# same draws (fund_cases.numpy_ransac) meets the check; the tests assert that it does, then ask the same of the host build.
SEEDS_30 = (100, 102, 103, 105, 106, 107, 108, 109)
SEEDS_50 = (100, 102, 103, 104, 106, 107, 108, 109)              # of 100 .. 109: not 101 (numpy misses 13 of 150) and 105 (115 of 150)
THR = 1.0


def outcome_30(sc, mask):
    """30 % outliers: no planted inlier missed; every extra accepted row within 1.5 thr of the planted F's epipolar line"""
    inl = ~sc['outlier']
    extra = mask & ~inl
    d = C.line_distance_px(sc['F'], sc['m'][:, :2].astype(np.float64), sc['m'][:, 2:].astype(np.float64))
    return int((inl & ~mask).sum()) == 0 and bool((d[extra] < 1.5 * THR).all()), int((inl & ~mask).sum()), int(extra.sum())


def outcome_50(sc, mask):
    """50 % outliers: at most 1 % of the planted inliers missed"""
    inl = ~sc['outlier']
    missed = int((inl & ~mask).sum())
    return missed <= 0.01 * inl.sum(), missed, int((mask & ~inl).sum())


@pytest.mark.parametrize('seed', SEEDS_30)
def test_ransac_30_percent_outliers(seed):
    sc = C.scene(seed, 300, 0.3)
    ok_np, _, _ = outcome_30(sc, C.numpy_ransac(sc['m'], THR, 256, seed - 100))
    assert ok_np, 'the numpy RANSAC itself misses the check: not a scene for this test'
    r = C.host_ransac(sc['m'], thr=THR, iters=256, seed=seed - 100)
    ok, missed, extra = outcome_30(sc, r['inliers'])
    print(f'scene {seed}: {missed} planted inliers missed, {extra} extra rows accepted, hypothesis {tuple(r["hyp"])}')
    assert r['valid'] == 1 and ok and r['n_inliers'] == int(r['inliers'].sum())
    assert abs(np.linalg.norm(r['F']) - 1) < 1e-12


@pytest.mark.parametrize('seed', SEEDS_50)
def test_ransac_50_percent_outliers(seed):
    sc = C.scene(seed, 300, 0.5)
    ok_np, _, _ = outcome_50(sc, C.numpy_ransac(sc['m'], THR, 256, seed - 100))
    assert ok_np, 'the numpy RANSAC itself is outside the cap: not a scene for this test'
    r = C.host_ransac(sc['m'], thr=THR, iters=256, seed=seed - 100)
    ok, missed, extra = outcome_50(sc, r['inliers'])
    print(f'scene {seed}: {missed} planted inliers missed, {extra} extra rows accepted')
    assert r['valid'] == 1 and ok


def filtered_case():
    """a 300-row scene with a score array that filters rows (some below the threshold, one NaN) and non-finite coordinates in others"""
    sc = C.scene(120, 300, 0.3)
    m = sc['m'].copy()
    rng = np.random.default_rng(5)
    scores = rng.uniform(0.3, 1.0, 300).astype(np.float32)
    scores[[3, 70, 71, 72, 100, 130, 131, 190, 299]] = 0.1
    scores[150] = np.nan
    m[17, 0] = np.nan; m[66, 3] = np.inf; m[200, 2] = -np.inf
    keep = (scores >= 0.25) & np.isfinite(m).all(1)
    return m, scores, keep


def test_score_filter_and_non_finite_rows():
    m, scores, keep = filtered_case()
    assert keep.sum() == 300 - 13
    a = C.host_ransac(m, scores, sc_thres=0.25)
    b = C.host_ransac(m[keep], None)
    c = C.host_ransac(m[keep], scores[keep], sc_thres=0.25)
    assert a['valid'] == 1 and not a['inliers'][~keep].any()
    for other in (b, c):
        assert np.array_equal(a['inliers'][keep], other['inliers']) and a['n_inliers'] == other['n_inliers']
        assert np.array_equal(a['F'].view(np.int64), other['F'].view(np.int64)) and tuple(a['hyp']) == tuple(other['hyp'])


def test_row_counts():
    sc = C.scene(121, 40, 0.0)
    for n in (6, 0):
        r = C.host_ransac(sc['m'][:n])
        assert r['status'] == 0 and r['valid'] == 0 and not r['inliers'].any() and tuple(r['hyp']) == (-1, -1) and not r['F'].any()
    scores = np.full(40, 0.1, np.float32)
    scores[:6] = 1.0                                                 # 40 rows, six survive
    r = C.host_ransac(sc['m'], scores)
    assert r['valid'] == 0 and not r['inliers'].any()
    r = C.host_ransac(sc['m'][:7])
    assert r['valid'] == 1 and r['n_inliers'] == 7 and r['inliers'].all()
    r = C.host_ransac(np.repeat(sc['m'][:1], 20, 0))                 # twenty copies of one match: no box, no draw
    assert r['valid'] == 0 and not r['inliers'].any()


def test_deterministic_and_keyed_by_seed_and_pair_index():
    sc = C.scene(122, 300, 0.3)
    a, b = C.host_ransac(sc['m'], seed=1), C.host_ransac(sc['m'], seed=1)
    assert all(np.array_equal(a[k], b[k]) for k in ('F', 'hyp', 'inliers'))
    assert tuple(a['hyp']) != tuple(C.host_ransac(sc['m'], seed=2)['hyp'])
    assert tuple(a['hyp']) != tuple(C.host_ransac(sc['m'], seed=1, sample=3)['hyp'])


@pytest.mark.parametrize('iters', [0, -64, 100, C.HYP_PER_WG + 1])
def test_bad_iteration_count_is_an_invalid_argument(iters):
    sc = C.scene(123, 50, 0.3)
    assert C.host_ransac(sc['m'], iters=iters)['status'] == -1       # GF_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------------------ the offsets clamp
def host_offsets_range(offsets, n, M):
    import ctypes
    off = np.ascontiguousarray(offsets, np.int32)
    out = np.full(2, -7, np.int32)
    f = C.host_lib().gf_fund_host_offsets_range
    f.restype, f.argtypes = None, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    f(off.ctypes.data, n, M, out.ctypes.data)
    return int(out[0]), int(out[1])


def test_offsets_clamp():
    """gs_offsets_range of solver_common.h, which every stage that reads a device-side offsets array applies (fundamental matrix, absolute
    pose, triangulation), through the host build: o = clamp(offsets[n], 0, M), e = clamp(max(offsets[n + 1], o), 0, M) -> (o, e - o).
    Out-of-range offsets are tested here and only here: on the device they would be indexed with."""
    M = 200

    def rule(a, b):
        o = min(max(a, 0), M)
        e = min(max(max(b, o), 0), M)
        return o, e - o

    offsets = [0, 0, 7, 64, 199, 200]                                  # in range, ascending (an empty and a one-row slice among them)
    for n in range(len(offsets) - 1):
        assert host_offsets_range(offsets, n, M) == rule(offsets[n], offsets[n + 1]) == (offsets[n], offsets[n + 1] - offsets[n])
    for a, b in ((-5, 30), (-2 ** 31, 200), (-1, -1), (-9, 0)):        # a negative start
        assert host_offsets_range([a, b], 0, M) == rule(a, b)
    assert host_offsets_range([-5, 30], 0, M) == (0, 30)
    for a, b in ((150, 201), (0, 2 ** 31 - 1), (199, 1000)):           # an end past M
        assert host_offsets_range([a, b], 0, M) == rule(a, b)
    assert host_offsets_range([150, 201], 0, M) == (150, 50)
    for a, b in ((120, 40), (200, 0), (1, 0), (50, -3)):               # a descending pair: empty, at the clamped start
        assert host_offsets_range([a, b], 0, M) == rule(a, b) == (a, 0)
    for a, b in ((201, 300), (300, 201), (2 ** 31 - 1, 2 ** 31 - 1)):  # both past M
        assert host_offsets_range([a, b], 0, M) == rule(a, b) == (M, 0)
    assert host_offsets_range([9, 9, 120, 40, 77], 2, M) == (120, 0)   # entry n of a longer array
    assert host_offsets_range([3, 5], 0, 0) == (0, 0)                  # an empty list
