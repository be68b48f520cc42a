"""Padded batches of unequal image sizes, the parts that need no device: the ragged map batch's description of its maps and its refusals,
the padded pair grouping and its waste bound, the command line's new flags, and the argument errors of the two ragged entries (status codes,
no launch)."""
import ctypes
import os
import random

import pytest
import torch


def _nhwc(c, h, w, dtype=torch.float32):
    return torch.zeros(h, w, c, dtype=dtype).permute(2, 0, 1)


def test_ragged_map_batch_describes_its_maps_and_refuses_maps_that_disagree():
    from geoformer_amd.ops import RaggedMapBatch
    a, b, c = _nhwc(16, 5, 7), _nhwc(16, 3, 7), _nhwc(16, 5, 4)
    rb = RaggedMapBatch([c, a, c, b])                                                  # extents differ, one entry twice
    assert rb.shape == torch.Size([4, 16, 5, 7]) and rb.dtype == torch.float32 and rb.device == a.device and len(rb) == 4
    assert rb.size() == rb.shape and rb.size(2) == 5 and rb.layout == 'nhwc'
    assert rb.extents == [(5, 4), (5, 7), (5, 4), (3, 7)] and rb.addresses == [m.data_ptr() for m in (c, a, c, b)]
    assert rb.align >= 4 and all(ad % rb.align == 0 for ad in rb.addresses)
    # one gf_map_record per sample: base, sc, sh, sw, h | w << 32 - each map with its OWN row stride
    assert rb.records() == [[c.data_ptr(), 1, 4 * 16, 16, 5 | (4 << 32)], [a.data_ptr(), 1, 7 * 16, 16, 5 | (7 << 32)],
                            [c.data_ptr(), 1, 4 * 16, 16, 5 | (4 << 32)], [b.data_ptr(), 1, 7 * 16, 16, 3 | (7 << 32)]]
    assert RaggedMapBatch([b, c]).shape == torch.Size([2, 16, 5, 7])                   # the per-axis maximum, no map has it
    assert RaggedMapBatch([a, b], canvas=(6, 8)).shape == torch.Size([2, 16, 6, 8])
    nchw = RaggedMapBatch([torch.zeros(16, 5, 7), torch.zeros(16, 2, 3)])
    assert nchw.layout == 'nchw' and nchw.records()[1][1:] == [6, 3, 1, 2 | (3 << 32)]
    off = torch.zeros(5 * 7 * 16 + 1)[1:].view(5, 7, 16).permute(2, 0, 1)              # starts one element into its allocation
    assert RaggedMapBatch([a, off]).align == 4
    with pytest.raises(ValueError, match='agree in C'):
        RaggedMapBatch([a, _nhwc(8, 5, 7)])
    with pytest.raises(ValueError, match='dtype'):
        RaggedMapBatch([a, b.half()])
    with pytest.raises(ValueError, match='layout'):
        RaggedMapBatch([a, torch.zeros(16, 3, 7)])                                     # channels-last and contiguous in one batch
    with pytest.raises(ValueError, match='channels-last'):
        RaggedMapBatch([torch.zeros(16, 5, 14)[:, :, ::2]])                            # neither kind
    with pytest.raises(ValueError, match='no maps'):
        RaggedMapBatch([])
    with pytest.raises(ValueError, match='canvas'):
        RaggedMapBatch([a, b], canvas=(5, 6))
    with pytest.raises(ValueError, match='canvas'):
        RaggedMapBatch([a, b], canvas=(4, 7))


def _waste_ok(shapes, idx, max_waste):
    for side in (0, 1):
        hs, ws = [shapes[k][side][0] for k in idx], [shapes[k][side][1] for k in idx]
        own = sum(h * w for h, w in zip(hs, ws))
        if len(idx) * max(hs) * max(ws) > max_waste * own:
            return False
    return True


def test_group_pairs_padded_covers_every_pair_within_batch_and_waste_bounds():
    from geoformer_amd.matcher import group_pairs, group_pairs_padded
    rng = random.Random(5)
    sizes = [(480, 512 + 32 * k) for k in range(8)] + [(640, 480), (320, 640)]
    shapes = [(rng.choice(sizes), rng.choice(sizes)) for _ in range(61)]
    for batch in (1, 3, 8):
        for max_waste in (1.0, 1.1, 1.25, 2.0, 100.0):
            batches = group_pairs_padded(shapes, batch, max_waste)
            assert sorted(k for b in batches for k in b) == list(range(len(shapes)))          # every pair once
            assert all(1 <= len(b) <= batch and b == sorted(b) for b in batches)
            assert all(_waste_ok(shapes, b, max_waste) for b in batches)
            out = [None] * len(shapes)                # scattering per-batch results back by index gives the input order
            for b in batches:
                for k in b:
                    out[k] = k
            assert out == list(range(len(shapes)))
        if batch > 1:
            # the bound bites: a looser one needs no more batches, and without one the batches are simply full
            counts = [len(group_pairs_padded(shapes, batch, r)) for r in (1.0, 1.25, 100.0)]
            assert counts[0] >= counts[1] >= counts[2] == -(-len(shapes) // batch) and counts[0] > counts[2]
    assert all(len({shapes[k] for k in b}) == 1 for b in group_pairs_padded(shapes, 8, 1.0))  # waste 1: equal shapes only
    # pairs are taken in order of area: the two small pairs share a batch, not the first two of the list
    A, B = ((160, 184), (160, 184)), ((320, 368), (320, 368))
    assert group_pairs_padded([A, B, A, B], 2, 1.5) == [[0, 2], [1, 3]]
    # a portrait and a landscape image of one area: the canvas is the per-axis maximum, twice either's area
    P, Q = ((100, 200), (100, 200)), ((200, 100), (100, 200))
    assert group_pairs_padded([P, Q], 2, 1.9) == [[0], [1]] and group_pairs_padded([P, Q], 2, 2.0) == [[0, 1]]
    # one shape throughout: group_pairs' batches
    one = [A] * 11
    assert group_pairs_padded(one, 4, 1.0) == group_pairs(one, 4) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10]]
    assert group_pairs_padded([], 8, 1.5) == [] and group_pairs_padded([A], 8, 1.5) == [[0]]
    with pytest.raises(ValueError, match='batch'):
        group_pairs_padded(shapes, 0, 1.5)
    with pytest.raises(ValueError, match='max_waste'):
        group_pairs_padded(shapes, 4, 0.99)
    with pytest.raises(ValueError, match='max_waste'):
        group_pairs_padded(shapes, 4, float('nan'))


def test_parser_knows_pad_on_pairs_only():
    from geoformer_amd.matcher import build_parser
    ap = build_parser()
    a = ap.parse_args(['pairs', 'list.txt', '--pad', '--pad-waste', '1.5'])
    assert (a.cmd, a.list, a.pad, a.pad_waste, a.batch) == ('pairs', 'list.txt', True, 1.5, 8)
    a = ap.parse_args(['pairs', 'list.txt'])
    assert (a.pad, a.pad_waste) == (False, None)
    a = ap.parse_args(['pairs', '--all-pairs', 'dir', '--pad'])
    assert (a.pad, a.pad_waste) == (True, None)
    with pytest.raises(SystemExit):
        ap.parse_args(['match', 'x.png', 'y.png', '--pad'])
    with pytest.raises(SystemExit):
        ap.parse_args(['hpatches', 'root', '--pad'])
    assert not hasattr(ap.parse_args(['match', 'x.png', 'y.png']), 'pad')


@pytest.fixture(scope='module')
def lib():
    from geoformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_ragged_entries_report_argument_errors_as_status_codes(lib):
    """A null table, N <= 0, N > 65535, a bad dtype or an alignment that is no power of two is GF_ERR_INVALID_ARGUMENT (-1) before
    anything touches a device."""
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def pe(table, n, dt=1, odt=1, align=32):
        return lib.gf_pos_encode_ragged(table, dt, align, p, p, odt, n, 8, 1, 1, None, None)
    assert pe(None, 1) == -1 and b'gf_pos_encode_ragged' in lib.gf_last_error() and b'null pointer' in lib.gf_last_error()
    assert pe(p, 0) == -1 and b'empty' in lib.gf_last_error()
    assert pe(p, -3) == -1 and b'empty' in lib.gf_last_error()
    assert pe(p, 65536) == -1 and b'65535' in lib.gf_last_error()
    assert pe(p, 1, dt=7) == -1 and b'dtype' in lib.gf_last_error()
    assert pe(p, 1, odt=-1) == -1 and b'dtype' in lib.gf_last_error()
    assert pe(p, 1, align=24) == -1 and b'power of two' in lib.gf_last_error()
    assert pe(p, 1, align=0) == -1 and b'power of two' in lib.gf_last_error()

    def fg(t0, t1, n, dt=1, odt=1, align=16):
        return lib.gf_fine_gather_ragged(t0, t1, n, dt, align, 8, p, p, odt, 1, 1, 8, p, p, p, 1, 1, 1, 4, 5, p, p, None)
    assert fg(None, p, 1) == -1 and b'gf_fine_gather_ragged' in lib.gf_last_error() and b'null pointer' in lib.gf_last_error()
    assert fg(p, None, 1) == -1 and b'null pointer' in lib.gf_last_error()
    assert fg(p, p, 0) == -1 and b'empty' in lib.gf_last_error()
    assert fg(p, p, -1) == -1 and b'empty' in lib.gf_last_error()
    assert fg(p, p, 65536) == -1 and b'65535' in lib.gf_last_error()
    assert fg(p, p, 1, dt=-1) == -1 and b'dtype' in lib.gf_last_error()
    assert fg(p, p, 1, odt=3) == -1 and b'dtype' in lib.gf_last_error()
    assert fg(p, p, 1, align=48) == -1 and b'power of two' in lib.gf_last_error()


def test_record_layout_in_the_header_is_what_the_binding_writes():
    """gf_map_record is declared once, in the header: five 8-byte words - base, sc, sh, sw and h | w << 32 - as RaggedMapBatch.records() packs."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'geoformer_hip.h')).read()
    body = re.search(r'typedef struct gf_map_record \{(.*?)\} gf_map_record;', hdr, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = [' '.join(f.split()) for f in body.split(';') if f.strip()]
    assert fields == ['const void* base', 'long sc, sh, sw', 'int h, w']

    class Record(ctypes.Structure):
        _fields_ = [('base', ctypes.c_void_p), ('sc', ctypes.c_long), ('sh', ctypes.c_long), ('sw', ctypes.c_long), ('h', ctypes.c_int), ('w', ctypes.c_int)]
    assert ctypes.sizeof(Record) == 40
    from geoformer_amd.ops import RaggedMapBatch
    m = torch.zeros(3, 7, 16).permute(2, 0, 1)
    words = torch.tensor(RaggedMapBatch([m]).records(), dtype=torch.int64)
    rec = Record.from_buffer_copy(words.numpy().tobytes())
    assert (rec.base, rec.sc, rec.sh, rec.sw, rec.h, rec.w) == (m.data_ptr(), 1, 7 * 16, 16, 3, 7)


def test_mask_out_and_mixed_batch_kinds_are_refused_before_any_launch():
    from geoformer_amd import ops
    a = _nhwc(16, 5, 7)
    ids = torch.zeros(1, dtype=torch.int64)
    c = torch.zeros(1, 4, 8)
    with pytest.raises(TypeError, match='both'):
        ops.fine_gather(ops.RaggedMapBatch([a]), ops.MapBatch([a]), c, c, ids, ids, ids, 2, 2, 4, 5, torch.float32)
    with pytest.raises(TypeError, match='both'):
        ops.fine_gather(a[None], ops.RaggedMapBatch([a]), c, c, ids, ids, ids, 2, 2, 4, 5, torch.float32)
