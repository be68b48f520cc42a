"""The triangulation rule of csrc/tri_solver.h on the host build (csrc/host/tri_host.cpp): the two-view midpoint and each of its
rejections, the hypothesis pairs, the selection, the refit's invariants and the component labelling.  No GPU."""
import itertools
import math

import numpy as np
import pytest

import triangulate_cases as C


@pytest.fixture(scope='module')
def cams():
    return C.make_cameras(12, 3)


def _uv(K, R, t, i, X):
    return C.project(K[i], R[i], t[i], X).astype(np.float32)


def test_two_view_recovery_without_noise(cams):
    K, R, t = cams
    X = np.array([0.3, -0.4, 7.0])
    ok, got = C.host_midpoint(K[0], R[0], t[0], _uv(K, R, t, 0, X), K[7], R[7], t[7], _uv(K, R, t, 7, X))
    # the pixels are rounded to fp32 (2^-14 px at 800 px) at a depth of 7 units and a focal length of 800 px: 7 / 800 * 6e-5 = 5e-7 units,
    # over a baseline a third of the depth
    assert ok == 1 and np.linalg.norm(got - X) < 1e-5


def test_rejections_of_the_two_view_solver(cams):
    K, R, t = cams
    X = np.array([0.3, -0.4, 7.0])
    a, b = _uv(K, R, t, 0, X), _uv(K, R, t, 7, X)
    # equal camera centres: the same camera twice gives parallel rays (1 - c^2 = 0)
    ok, got = C.host_midpoint(K[0], R[0], t[0], a, K[0], R[0], t[0], a)
    assert ok == 0 and np.all(got == 0)
    # equal centres, different pixels: the rays meet at the centre, lambda = mu = 0 is not > 0
    assert C.host_midpoint(K[0], R[0], t[0], a, K[0], R[0], t[0], a + np.float32(50))[0] == 0
    # the point behind one camera: camera 7 turned by half a turn about its y axis sees the pixel's ray point away from the scene
    flip = np.diag([-1.0, 1.0, -1.0])
    assert C.host_midpoint(K[0], R[0], t[0], a, K[7], flip @ R[7], flip @ t[7], b)[0] == 0
    # the angle test on both sides of the cosine
    da = R[0].T @ np.array([(a[0] - 800) / 800, (a[1] - 600) / 808, 1.0])
    db = R[7].T @ np.array([(b[0] - 800) / 800, (b[1] - 600) / 808, 1.0])
    c = float(da @ db / np.linalg.norm(da) / np.linalg.norm(db))
    assert C.host_midpoint(K[0], R[0], t[0], a, K[7], R[7], t[7], b, cos_min=c + 1e-9)[0] == 1
    assert C.host_midpoint(K[0], R[0], t[0], a, K[7], R[7], t[7], b, cos_min=c - 1e-9)[0] == 0
    # a NaN pose, a NaN pixel
    tn = t[7].copy()
    tn[1] = np.nan
    assert C.host_midpoint(K[0], R[0], t[0], a, K[7], R[7], tn, b)[0] == 0
    assert C.host_midpoint(K[0], R[0], t[0], a, K[7], R[7], t[7], np.array([np.nan, b[1]], np.float32))[0] == 0
    assert C.host_midpoint(K[0], R[0], t[0], np.array([a[0], np.inf], np.float32), K[7], R[7], t[7], b)[0] == 0


def test_pairs_are_lexicographic_up_to_11_and_drawn_from_12():
    h = C.host_lib()
    for L in range(2, C.TR_LEX_MAX + 1):
        want = list(itertools.combinations(range(L), 2))
        assert h.gf_tri_host_hyp_count(L) == len(want)
        assert [C.host_pair(5, t, L) for t in range(len(want))] == [(1, p) for p in want]
        assert C.host_pair(5, len(want), L)[0] == 0 and C.host_pair(5, -1, L)[0] == 0
    assert h.gf_tri_host_hyp_count(0) == 0 and h.gf_tri_host_hyp_count(1) == 0
    for L in (12, 13, 40, 100000):
        assert h.gf_tri_host_hyp_count(L) == C.TR_MAX_HYP
        got = [C.host_pair(5, t, L) for t in range(C.TR_MAX_HYP)]
        assert all(ok == 1 and 0 <= a < L and 0 <= b < L and a != b for ok, (a, b) in got)
        assert [p for _, p in got] != list(itertools.islice(itertools.combinations(range(L), 2), C.TR_MAX_HYP))   # draws, not the first 64 pairs
        assert [C.host_pair(6, t, L) for t in range(C.TR_MAX_HYP)] != got                               # keyed by the track
        assert C.host_pair(5, C.TR_MAX_HYP, L)[0] == 0


def test_selection_tie_goes_to_the_smaller_hypothesis(cams):
    K, R, t = cams
    tr = C.planted_tracks(K, R, t, [4], seed=1, noise=0.0)
    rc, out = C.host_triangulate(tr['track_off'], tr['obs_image'], tr['obs_uv'], K, R, t)
    assert rc == 0 and out['valid'][0] == 1 and out['n_inliers'][0] == 4 and out['hypothesis'][0] == 0       # all six pairs see four inliers
    # observation 0 made an outlier: the pairs without it are hypotheses 3, 4, 5 and see three inliers each
    uv = tr['obs_uv'].copy()
    uv[0] += 300
    rc, out = C.host_triangulate(tr['track_off'], tr['obs_image'], uv, K, R, t)
    assert out['n_inliers'][0] == 3 and out['hypothesis'][0] == 3 and out['inliers'].tolist() == [0, 1, 1, 1]


def test_refit_0_is_the_midpoint_and_inliers_never_decrease(cams):
    K, R, t = cams
    lengths = [2, 3, 5, 8, 12] * 12
    tr = C.planted_tracks(K, R, t, lengths, seed=2, noise=0.5, outlier_frac=0.2)
    outs = [C.host_triangulate(tr['track_off'], tr['obs_image'], tr['obs_uv'], K, R, t, refit=r)[1] for r in range(9)]
    o0 = outs[0]
    assert np.all(o0['rounds'] == 0) and o0['valid'].sum() >= 55
    for k in np.flatnonzero(o0['valid']):                               # refit 0: the midpoint of the pair the hypothesis names
        b, e = tr['track_off'][k], tr['track_off'][k + 1]
        ok, (pa, pb) = C.host_pair(int(k), int(o0['hypothesis'][k]), int(e - b))
        ia, ib = b + pa, b + pb
        ca, cb = tr['obs_image'][ia], tr['obs_image'][ib]
        ok2, X = C.host_midpoint(K[ca], R[ca], t[ca], tr['obs_uv'][ia], K[cb], R[cb], t[cb], tr['obs_uv'][ib])
        assert ok == 1 and ok2 == 1 and X.tobytes() == o0['X'][k].tobytes()
    for prev, cur in zip(outs, outs[1:]):
        assert np.all(cur['n_inliers'] >= prev['n_inliers']) and np.all(cur['rounds'] >= prev['rounds'])
        assert np.array_equal(cur['hypothesis'], o0['hypothesis'])
    for r, o in enumerate(outs):
        assert o['rounds'].max() <= r
        same = o['rounds'] == 0
        assert o['X'][same].tobytes() == o0['X'][same].tobytes()        # rounds = 0 means the midpoint's bits
        assert np.array_equal(np.add.reduceat(o['inliers'].astype(int), tr['track_off'][:-1]) * o['valid'], o['n_inliers'] * o['valid'])
    assert outs[2]['rounds'].max() >= 1


def test_conflict_poseless_and_short_tracks(cams):
    K, R, t = cams
    tr = C.planted_tracks(K, R, t, [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10]], seed=4, noise=0.2)
    img = tr['obs_image'].copy()
    img[1] = img[0]                                                      # track 0: an image twice
    Rn = R.copy()
    Rn[4] = np.nan                                                       # track 1's middle observation loses its pose
    Rn[10] = np.nan                                                      # track 3 (length 2) is left with one effective observation
    rc, out = C.host_triangulate(tr['track_off'], img, tr['obs_uv'], K, Rn, t)
    assert rc == 0
    assert out['conflict'].tolist() == [1, 0, 0, 0] and out['valid'].tolist() == [0, 1, 1, 0]
    assert out['hypothesis'].tolist() == [-1, 0, 0, -1] and out['n_inliers'].tolist() == [0, 2, 3, 0]
    assert out['inliers'].tolist() == [0, 0, 0, 1, 0, 1, 1, 1, 1, 0, 0] and np.all(out['X'][[0, 3]] == 0)
    # exactly as if the pose-less observation were absent
    keep = np.array([3, 5])
    rc, two = C.host_triangulate(np.array([0, 2], np.int32), img[keep], tr['obs_uv'][keep], K, R, t)
    assert two['X'][0].tobytes() == out['X'][1].tobytes() and two['err2'][0] == out['err2'][1]


def test_argument_errors():
    z = np.zeros(1, np.int32)
    K, R, t = C.make_cameras(2, 0)
    for kw in (dict(pixel_thr=0.0), dict(pixel_thr=float('inf')), dict(min_obs=1), dict(refit=-1), dict(refit=9), dict(cos_min=float('nan'))):
        assert C.host_triangulate(np.array([0, 2], np.int32), np.array([0, 1], np.int32), np.zeros((2, 2), np.float32), K, R, t, **kw)[0] == -1
    assert C.host_triangulate(z, np.zeros(0, np.int32), np.zeros((0, 2), np.float32), K, R, t)[0] == 0                # zero tracks


def test_labelling_against_scipy():
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    rng = np.random.default_rng(11)
    for n_img, per, n_pairs, rows in ((5, 6, 4, 5), (20, 30, 25, 12), (50, 100, 60, 50), (8, 1, 20, 1)):
        e = []
        for _ in range(n_pairs):
            i, j = sorted(rng.choice(n_img, 2, replace=False).tolist())
            e += [(i, int(a), j, int(b)) for a, b in zip(rng.integers(0, per, rows), rng.integers(0, per, rows))]
        g = C.graph([per] * n_img, e)
        st, parent, toff, oimg, okp, onode = C.host_tracks(g)
        n = g['n_nodes']
        u = np.array([g['kp_off'][a] + k for a, k, _, _ in e])
        v = np.array([g['kp_off'][b] + l for _, _, b, l in e])
        ncomp, lab = connected_components(sp.coo_matrix((np.ones(len(u)), (u, v)), shape=(n, n)), directed=False)
        assert st == 0
        mins = np.full(ncomp, n)
        np.minimum.at(mins, lab, np.arange(n))
        assert np.array_equal(parent, mins[lab])                         # the root is the component's smallest node
        sizes = np.bincount(lab)
        roots = np.sort(mins[sizes >= 2])
        assert len(toff) == len(roots) + 1 and np.array_equal(onode[toff[:-1]], roots)
        for k in range(len(roots)):
            seg = onode[toff[k]:toff[k + 1]]
            assert np.array_equal(seg, np.flatnonzero(parent == roots[k]))
        assert np.array_equal(g['kp_off'][oimg] + okp, onode)


def test_edge_out_of_range_is_reported_and_skipped():
    g = C.graph([2, 2], [(0, 1, 1, 0), (0, 5, 1, 1), (0, 0, 1, -1)])
    st, parent = C.host_label(g)
    assert st == 1 and parent.tolist() == [0, 1, 1, 3]
