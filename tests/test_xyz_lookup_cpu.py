"""The 3-D map lookup of csrc/abs_solver.h (as_xyz_sample) on the CPU: the host build against numpy fp64 written in the same expression
order, bit for bit.  Maps and points: tests/abspose_cases.py (the GPU test uses the same)."""
import numpy as np

import abspose_cases as C


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    """bit-equal, any NaN equal to any NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(_bits(a)[~np.isnan(a)], _bits(b)[~np.isnan(b)])


def test_host_lookup_equals_numpy_bit_for_bit():
    for k, m in enumerate(C.lookup_maps()):
        Hm, Wm = m.shape[:2]
        pts = C.lookup_points(Hm, Wm, 5 + k)
        got = C.host_xyz_lookup([m], [0, len(pts)], pts)
        want = np.array([C.numpy_lookup(m, x, y) for x, y in pts])
        assert _same(got, want), np.flatnonzero(~(np.isnan(got) == np.isnan(want)).all(1))
        assert np.isfinite(got).all(1).sum() > 30 and np.isnan(got).all(1).sum() >= 9
        assert (np.isnan(got).all(1) | np.isfinite(got).all(1)).all()         # a row is all NaN or all finite


def test_integer_coordinates_and_edges():
    a, b = C.lookup_maps()
    got = C.host_xyz_lookup([a], [0, 6], np.array([[0, 0], [6, 4], [6, 0], [0, 4], [7, 0], [0, 5]], np.float32))
    for row, (y, x) in zip(got[:4], ((0, 0), (4, 6), (0, 6), (4, 0))):
        assert np.array_equal(_bits(row), _bits(a[y, x]))                     # integer coordinates are the pixel's own value
    assert np.isnan(got[4:]).all()                                            # one past the last column / row
    # next to a hole: NaN; the hole's own pixel: NaN
    got = C.host_xyz_lookup([a], [0, 3], np.array([[3, 2], [2.5, 2], [3.5, 1.5]], np.float32))
    assert np.isnan(got).all()


def test_two_pair_table_with_maps_of_different_sizes_and_rows_outside_every_pair():
    a, b = C.lookup_maps()
    pa, pb = C.lookup_points(5, 7, 1), C.lookup_points(33, 65, 2)
    pts = np.concatenate([pa, pb, pb[:4]])
    off = [0, len(pa), len(pa) + len(pb)]                                    # the last four rows belong to no pair
    got = C.host_xyz_lookup([a, b], off, pts)
    want = np.array([C.numpy_lookup(a, x, y) for x, y in pa] + [C.numpy_lookup(b, x, y) for x, y in pb])
    assert _same(got[:len(want)], want) and np.isnan(got[len(want):]).all()
