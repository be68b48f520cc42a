"""Shared by test_keypoint_quantize_cpu.py and test_keypoint_quantize_gpu.py: the ctypes wrapper of the serial host build of the
keypoint consolidation (csrc/host/keypoint_host.cpp over csrc/keypoint_spec.h), the golden fixture's cases and the synthetic inputs."""
import ctypes
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g19_keypoint_quantize.npz')
MAX_COORD = np.float32(4194304.0)            # keypoint_spec.h KP_MAX_COORD

_host = None


def host_lib():
    global _host
    if _host is None:
        from geoformer_amd import build
        if not os.path.exists(build.KEYPOINT_HOST_LIB):
            build.build_keypoint_host(verbose=False)
        h = ctypes.CDLL(build.KEYPOINT_HOST_LIB)
        h.gf_keypoint_host_cell.restype = ctypes.c_float
        h.gf_keypoint_host_cell.argtypes = [ctypes.c_float, ctypes.c_float]
        h.gf_keypoint_host_filter.restype = ctypes.c_int
        h.gf_keypoint_host_filter.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        h.gf_keypoint_host_consolidate.restype = ctypes.c_int
        h.gf_keypoint_host_consolidate.argtypes = ([ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                                                           ctypes.c_int] + [ctypes.c_void_p] * 5)
        _host = h
    return _host


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_consolidate(matches, scores, pair_offsets, pair_images, n_images, sc_thres=0.25, psize=48.0, dthres=4.0, unique=True):
    """-> (keypoints [K,2] f32, kp_offsets [n_images+1] i32, ids [M',2] i32, ids_offsets [P+1] i32, stats dict)."""
    matches = np.ascontiguousarray(matches, np.float32).reshape(-1, 4)
    scores = np.ascontiguousarray(scores, np.float32)
    pair_offsets = np.ascontiguousarray(pair_offsets, np.int32)
    pair_images = np.ascontiguousarray(pair_images, np.int32).reshape(-1, 2)
    P, M = len(pair_offsets) - 1, len(matches)
    assert pair_offsets[-1] == M == len(scores) and len(pair_images) == P
    kp, kpo = np.zeros((2 * M + 1, 2), np.float32), np.zeros(n_images + 1, np.int32)
    ids, ido = np.zeros((M + 1, 2), np.int32), np.zeros(P + 1, np.int32)
    st = np.zeros(8, np.int64)
    rc = host_lib().gf_keypoint_host_consolidate(_p(matches), _p(scores), _p(pair_offsets), _p(pair_images), P, n_images, sc_thres, psize, dthres,
                                                 int(unique), _p(kp), _p(kpo), _p(ids), _p(ido), _p(st))
    if rc != 0:
        raise ValueError(f'gf_keypoint_host_consolidate returned {rc}')
    stats = dict(zip(('flags', 'points', 'groups', 'longest_group', 'most_centres', 'dropped', 'K', 'rows'), (int(v) for v in st)))
    return kp[:stats['K']].copy(), kpo, ids[:stats['rows']].copy(), ido, stats


def host_filter(ids, scores):
    ids, scores = np.ascontiguousarray(ids, np.int32).reshape(-1, 2), np.ascontiguousarray(scores, np.float32)
    keep = np.zeros(len(ids), np.uint8)
    assert host_lib().gf_keypoint_host_filter(_p(ids), _p(scores), len(ids), _p(keep)) == 0
    return keep.astype(bool)


def golden_cases():
    """-> (inputs dict, [(psize, dthres, unique, expected dict)])."""
    g = np.load(GOLDEN)
    inputs = {k: g[k] for k in ('matches', 'scores', 'pair_offsets', 'pair_images')}
    inputs['n_images'] = int(g['pair_images'].max()) + 1
    inputs['sc_thres'] = float(g['sc_thres'])
    cases = []
    for c, (psize, dthres, unique) in enumerate(g['cases']):
        cases.append((float(psize), float(dthres), bool(unique),
                      {k: g[f'c{c}_{k}'] for k in ('keypoints', 'kp_offsets', 'ids', 'ids_offsets', 'most_centres')}))
    return inputs, cases


def sort_rows_per_pair(ids, offsets):
    out = ids.copy()
    for q in range(len(offsets) - 1):
        r = ids[offsets[q]:offsets[q + 1]]
        out[offsets[q]:offsets[q + 1]] = r[np.lexsort((r[:, 1], r[:, 0]))]
    return out


def check_against_golden(result, psize, dthres, unique, exp):
    """result = (keypoints, kp_offsets, ids, ids_offsets, ...): keypoints bit-equal through uint32 views; id rows equal in order with the
    filter off (and in the exact mode), equal as lexicographically sorted rows per pair with it on."""
    kp, kpo, ids, ido = (np.asarray(a) for a in result[:4])
    assert kp.dtype == np.float32 and np.array_equal(kpo, exp['kp_offsets'])
    assert np.array_equal(kp.view(np.uint32), exp['keypoints'].view(np.uint32))
    assert np.array_equal(ido, exp['ids_offsets'])
    if unique and psize > 0 and dthres > 0:
        assert np.array_equal(sort_rows_per_pair(ids, ido), exp['ids'])
    else:
        assert np.array_equal(ids, exp['ids'])


def assert_same(a, b):
    """Two results (keypoints, kp_offsets, ids, ids_offsets, ...) bit for bit, order included."""
    for x, y, name in zip(a[:4], b[:4], ('keypoints', 'kp_offsets', 'ids', 'ids_offsets')):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape, (name, x.dtype, y.dtype, x.shape, y.shape)
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), name


def boundary_values():
    """k * psize and one ulp on either side for psize in {16, 48}, k = 0 .. 200, both signs, plus the largest supported coordinate."""
    vals = [np.float32(0.0), np.float32(-0.0), MAX_COORD, -MAX_COORD, np.nextafter(MAX_COORD, np.float32(0))]
    for p in (16, 48):
        k = np.arange(0, 201, dtype=np.float32) * np.float32(p)
        for v in (k, -k):
            vals += [v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))]
    return np.unique(np.concatenate([np.atleast_1d(v) for v in vals]).astype(np.float32))


def boundary_case():
    """One pair over two images whose coordinates walk the cell boundaries (boundary_values in both coordinates, shuffled against each other)."""
    v = boundary_values()
    rng = np.random.RandomState(5)
    m = np.stack([v, rng.permutation(v), rng.permutation(v), v[::-1]], axis=1).astype(np.float32)
    sc = (np.float32(0.3) + np.float32(0.6) * rng.permutation(len(v)).astype(np.float32) / np.float32(len(v))).astype(np.float32)
    return m, sc, np.array([0, len(v)], np.int32), np.array([[0, 1]], np.int32), 2


def lattice_case():
    """One cell (psize 48): all 2304 points of the 1-pixel lattice in shuffled order plus 500 points jittered by 0.25 - under dthres 0.5
    far more than 256 centres, and merges into them, in one group.  Side 1 repeats the points in another order inside cell (2, 0)."""
    rng = np.random.RandomState(7)
    j = rng.permutation(2304)
    x, y = (j % 48).astype(np.float32), (j // 48).astype(np.float32)
    pick = rng.randint(0, 2304, 500)
    jx = (pick % 48).astype(np.float32) + rng.choice(np.array([0.25, 0.0], np.float32), 500)
    jy = (pick // 48).astype(np.float32) + rng.choice(np.array([0.25, 0.0], np.float32), 500)
    p0 = np.stack([np.concatenate([x, jx]), np.concatenate([y, jy])], axis=1)
    p1 = p0[rng.permutation(len(p0))] + np.array([96.0, 0.0], np.float32)
    m = np.concatenate([p0, p1], axis=1).astype(np.float32)
    sc = (np.float32(0.3) + np.float32(0.6) * rng.permutation(len(m)).astype(np.float32) / np.float32(len(m))).astype(np.float32)
    return m, sc, np.array([0, len(m)], np.int32), np.array([[0, 1]], np.int32), 2


def long_groups_case():
    """One image pair whose points all fall into 3 cells of 2000 points each (psize 48, dthres 4)."""
    rng = np.random.RandomState(11)
    cell = np.repeat(np.arange(3), 2000)[rng.permutation(6000)]
    p0 = np.stack([48.0 * cell + rng.randint(0, 192, 6000) / 4.0, 96.0 + rng.randint(0, 192, 6000) / 4.0], axis=1)
    p1 = np.stack([48.0 * cell[::-1] + rng.randint(0, 192, 6000) / 4.0, rng.randint(0, 192, 6000) / 4.0], axis=1)
    m = np.concatenate([p0, p1], axis=1).astype(np.float32)
    sc = (np.float32(0.3) + np.float32(0.6) * rng.permutation(6000).astype(np.float32) / np.float32(6000)).astype(np.float32)
    return m, sc, np.array([0, 6000], np.int32), np.array([[0, 1]], np.int32), 2


def interleaved_case():
    """5 images, 10 pairs (every i < j) in shuffled order and orientation with 0 to 300 rows each; a quarter of the scores below 0.25."""
    rng = np.random.RandomState(13)
    pairs = [(i, j) for i in range(5) for j in range(i + 1, 5)]
    pairs = [pairs[k] if rng.rand() < 0.5 else pairs[k][::-1] for k in rng.permutation(10)]
    rows = [0, 300, 1, 17, 150, 64, 65, 299, 128, 33]
    ms, ss = [], []
    for n in rows:
        ms.append((rng.randint(0, 4 * 160, (n, 4)) / 4.0).astype(np.float32))
        ss.append(rng.permutation(n).astype(np.float32) / np.float32(max(n, 1)))
    return (np.concatenate(ms), np.concatenate(ss).astype(np.float32), np.concatenate([[0], np.cumsum(rows)]).astype(np.int32),
            np.array(pairs, np.int32), 5)


def exact_case():
    """Exact mode: repeated points within and across pairs, +0.0 against -0.0."""
    rng = np.random.RandomState(17)
    base = (rng.randint(0, 40, (60, 2)) / 2.0).astype(np.float32)
    base[0], base[1], base[2], base[3] = (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)
    rows = [90, 0, 70]
    m = np.concatenate([base[rng.randint(0, 60, sum(rows))], base[rng.randint(0, 60, sum(rows))]], axis=1).astype(np.float32)
    m[:4, :2] = base[:4]
    sc = rng.rand(sum(rows)).astype(np.float32)
    return m, sc, np.concatenate([[0], np.cumsum(rows)]).astype(np.int32), np.array([[0, 1], [1, 2], [1, 0]], np.int32), 3


def equal_scores_case():
    """Every score equal: the filter's winners are decided by the row index alone."""
    rng = np.random.RandomState(23)
    rows = [200, 180]
    m = (rng.randint(0, 4 * 96, (sum(rows), 4)) / 4.0).astype(np.float32)
    sc = np.full(sum(rows), 0.5, np.float32)
    sc[::7] = np.float32(0.75)
    return m, sc, np.concatenate([[0], np.cumsum(rows)]).astype(np.int32), np.array([[0, 1], [1, 0]], np.int32), 2
