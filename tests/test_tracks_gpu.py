"""Track building on the GPU: gf_track_link and gf_track_flatten (csrc/k_triangulate.hip behind ops.build_tracks) against the serial
union-find and track list of the host build (csrc/host/tri_host.cpp), exactly.  Graphs: tests/triangulate_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

import triangulate_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CASES = C.graph_cases()


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32, device=DEV)


def device_tracks(g):
    from geoformer_amd import ops
    out = ops.build_tracks(_t(g['ids']), _t(g['id_off']), _t(g['pair_images']), _t(g['kp_off']), n_nodes=g['n_nodes'])
    assert all(x.dtype == torch.int32 and x.is_cuda for x in out)
    return [x.cpu().numpy() for x in out]


def device_parent(g):
    from geoformer_amd import _lib, ops
    parent = torch.full((max(g['n_nodes'], 1),), -7, dtype=torch.int32, device=DEV)
    status = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    a = [_t(g[k]) for k in ('ids', 'id_off', 'pair_images', 'kp_off')]
    h = _lib.lib()
    assert h.gf_track_link(ops._p(a[0]), ops._p(a[1]), ops._p(a[2]), len(g['pair_images']), len(g['ids']), ops._p(a[3]), len(g['kp_off']) - 1,
                           g['n_nodes'], ops._p(parent), ops._p(status), ops._stream()) == 0
    assert h.gf_track_flatten(ops._p(parent), g['n_nodes'], ops._stream()) == 0
    return int(status.cpu()[0]), parent.cpu().numpy()[:g['n_nodes']]


@pytest.mark.parametrize('name', list(CASES))
def test_build_tracks_equals_the_host_build(name):
    g = CASES[name]
    st, parent, toff, oimg, okp, onode = C.host_tracks(g)
    assert st == 0
    dst, dparent = device_parent(g)
    assert dst == 0 and np.array_equal(dparent, parent)
    first = device_tracks(g)
    for got, want in zip(first, (toff, oimg, okp, onode)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    for got, again in zip(first, device_tracks(g)):                     # two runs: equal bits
        assert got.tobytes() == again.tobytes()
    assert np.array_equal(device_parent(g)[1], dparent)


def test_expected_shapes_of_the_small_cases():
    assert device_tracks(CASES['no_edges'])[0].tolist() == [0]
    assert [x.tolist() for x in device_tracks(CASES['one_edge'])] == [[0, 2], [0, 2], [1, 3], [1, 8]]
    assert device_tracks(CASES['path_200_reversed'])[0].tolist() == [0, 200]
    assert device_tracks(CASES['star'])[3].tolist() == list(range(70))
    toff, oimg, okp, onode = device_tracks(CASES['joined_by_last_edge'])
    assert toff.tolist() == [0, 6] and onode.tolist() == [0, 3, 4, 9, 10, 15]
    assert oimg.tolist() == [0, 0, 1, 2, 2, 3] and okp.tolist() == [0, 3, 0, 1, 2, 3]


def test_row_out_of_range_is_reported_not_followed():
    from geoformer_amd import _lib, ops
    g = C.graph([2, 2], [(0, 1, 1, 0), (0, 5, 1, 1), (0, 0, 1, -1)])
    st, parent = C.host_label(g)
    dst, dparent = device_parent(g)
    assert st == dst == 1 and np.array_equal(parent, dparent)
    with pytest.raises(_lib.GeoFormerHipError, match='does not exist'):
        ops.build_tracks(_t(g['ids']), _t(g['id_off']), _t(g['pair_images']), _t(g['kp_off']))


def test_argument_errors_come_back_as_status_codes():
    from geoformer_amd import _lib
    h = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert h.gf_track_link(p, None, p, 1, 1, p, 1, 1, p, p, None) == -1 and b'null pointer' in h.gf_last_error()
    assert h.gf_track_link(p, p, p, 1, -1, p, 1, 1, p, p, None) == -1 and h.gf_track_link(p, p, p, 1, 1, p, 1, -1, p, p, None) == -1
    assert h.gf_track_flatten(None, 4, None) == -1 and h.gf_track_flatten(p, -1, None) == -1
