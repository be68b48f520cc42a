"""Feature store and many-pair matching, the parts that need no device: the store's LRU order, byte accounting and counters on stand-in
records, pair grouping, pair-list parsing, the command line's parser, the argument errors of the two address-table entries (status codes,
no launch) and the map batch's refusal of maps that do not agree."""
import ctypes
import os
import threading

import pytest
import torch


class Rec:
    """Stand-in record: only its size matters to the store."""

    def __init__(self, name, nbytes):
        self.name, self.nbytes = name, nbytes


def test_store_lru_order_bytes_and_counters():
    from geoformer_amd.matcher import FeatureStore
    st = FeatureStore(max_bytes=250)
    made = []

    def make(name, nbytes=100):
        def f():
            made.append(name)
            return Rec(name, nbytes)
        return f
    a = st.get_or_extract('a', make('a'))
    b = st.get_or_extract('b', make('b'))
    assert (st.extractions, st.hits, st.nbytes, st.keys()) == (2, 0, 200, ['a', 'b'])
    assert st.get_or_extract('a', make('a')) is a                     # a hit: no extraction, 'a' becomes the most recently used
    assert (st.extractions, st.hits, st.keys(), made) == (2, 1, ['b', 'a'], ['a', 'b'])
    st.get_or_extract('c', make('c'))                                 # 300 > 250: the least recently used entry ('b') goes
    assert (st.extractions, st.hits, st.nbytes, st.keys(), st.evictions) == (3, 1, 200, ['a', 'c'], 1)
    assert 'b' not in st and st.get('b') is None and st.hits == 1     # a miss counts nothing
    assert st.get_or_extract('b', make('b')) is not b                 # extracted again; 'a' is the oldest now
    assert (st.extractions, st.keys(), made) == (4, ['c', 'b'], ['a', 'b', 'c', 'b'])
    st.get_or_extract('big', make('big', 1000))                       # larger than the whole budget: stays alone
    assert (st.keys(), st.nbytes, len(st)) == (['big'], 1000, 1)
    st.clear()
    assert (len(st), st.nbytes) == (0, 0)


def test_store_unbounded_explicit_size_and_duplicate_insert():
    from geoformer_amd.matcher import FeatureStore
    st = FeatureStore()                                               # max_bytes=None: nothing is ever evicted
    for k in range(50):
        st.put(k, object(), nbytes=1 << 30)
    assert (len(st), st.nbytes, st.evictions, st.extractions) == (50, 50 << 30, 0, 50)
    first = st.get(7)
    assert st.put(7, object(), nbytes=5) is first and st.nbytes == 50 << 30        # the entry that was there first is kept
    with pytest.raises(ValueError):
        FeatureStore(max_bytes=-1)


def test_store_is_consistent_under_two_threads():
    from geoformer_amd.matcher import FeatureStore
    st = FeatureStore(max_bytes=10 * 8)

    def work(seed):
        for k in range(2000):
            st.get_or_extract((k * (seed + 3)) % 37, lambda: Rec('x', 8))
    ts = [threading.Thread(target=work, args=(s,)) for s in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert len(st) <= 10 and st.nbytes == 8 * len(st)
    assert st.extractions + st.hits == 4000 and st.extractions - st.evictions >= len(st)      # (> only if both missed one key at once)


def test_group_pairs_keeps_input_order_across_shape_groups_and_short_batches():
    from geoformer_amd.matcher import group_pairs
    A, B = ((160, 184), (160, 208)), ((160, 208), (160, 208))
    shapes = [A, B, A, A, B, A, A, A]                                  # 6 of A (batches of 4 and 2), 2 of B
    batches = group_pairs(shapes, 4)
    assert batches == [[0, 2, 3, 5], [6, 7], [1, 4]]
    assert all(len({shapes[k] for k in b}) == 1 for b in batches)
    # scattering per-batch results back by index gives the input order
    out = [None] * len(shapes)
    for b in batches:
        for k in b:
            out[k] = k
    assert out == list(range(len(shapes)))
    assert group_pairs([], 8) == [] and group_pairs([A], 8) == [[0]]
    with pytest.raises(ValueError):
        group_pairs(shapes, 0)


def test_pair_list_parsing(tmp_path):
    from geoformer_amd.matcher import all_pairs, read_pair_list
    d = tmp_path / 'lists'
    d.mkdir()
    lst = d / 'pairs.txt'
    lst.write_text('\n# a comment\nimgs/a.png  imgs/b.png\n\n   \n/abs/c.png\t../d.png\n')
    assert read_pair_list(str(lst)) == [(str(d / 'imgs' / 'a.png'), str(d / 'imgs' / 'b.png')), ('/abs/c.png', str(tmp_path / 'd.png'))]
    bad = d / 'bad.txt'
    bad.write_text('only_one.png\n')
    with pytest.raises(ValueError, match='bad.txt:1'):
        read_pair_list(str(bad))
    for n in ('b.png', 'a.ppm', 'c.JPG', 'notes.txt'):
        (d / n).write_bytes(b'')
    names = [(os.path.basename(p), os.path.basename(q)) for p, q in all_pairs(str(d))]
    assert names == [('a.ppm', 'b.png'), ('a.ppm', 'c.JPG'), ('b.png', 'c.JPG')]


def test_parser_knows_the_new_arguments_and_parses_the_old_ones_as_before():
    from geoformer_amd.matcher import build_parser
    ap = build_parser()
    a = ap.parse_args(['pairs', 'list.txt', '--out', 'o', '--batch', '4', '--cache-gb', '1.5'])
    assert (a.cmd, a.list, a.all_pairs, a.out, a.batch, a.cache_gb, a.imsize, a.precision) == ('pairs', 'list.txt', None, 'o', 4, 1.5, 640, 'fp16')
    a = ap.parse_args(['pairs', '--all-pairs', 'dir'])
    assert (a.list, a.all_pairs, a.batch, a.cache_gb, a.no_match_upscale) == (None, 'dir', 8, None, False)
    a = ap.parse_args(['hpatches', 'root', '--reuse-features'])
    assert a.reuse_features is True
    a = ap.parse_args(['hpatches', 'root', '--max-seqs', '2'])
    assert (a.cmd, a.root, a.max_seqs, a.reuse_features, a.imsize, a.no_match_upscale, a.ransac_thres, a.match_threshold, a.precision,
            a.preprocess, a.ckpt) == ('hpatches', 'root', 2, False, 480, True, 3.0, 0.2, 'fp16', 'host', None)
    a = ap.parse_args(['match', 'x.png', 'y.png', '--out', 'm.npz', '--preprocess', 'device'])
    assert (a.cmd, a.im1, a.im2, a.out, a.imsize, a.no_match_upscale, a.preprocess) == ('match', 'x.png', 'y.png', 'm.npz', 640, False, 'device')
    assert not hasattr(a, 'reuse_features') and not hasattr(a, 'batch')
    with pytest.raises(SystemExit):
        ap.parse_args(['match', 'x.png', 'y.png', '--reuse-features'])


@pytest.fixture(scope='module')
def lib():
    from geoformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_address_table_entries_report_argument_errors_as_status_codes(lib):
    """A null table, N <= 0 or a bad dtype is GF_ERR_INVALID_ARGUMENT (-1) before anything touches a device."""
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    pe = lambda table, n, dt=1: lib.gf_pos_encode_ptrs(table, dt, 1, 8, 8, 32, p, p, 1, n, 8, 1, 1, None)          # noqa: E731
    assert pe(None, 1) == -1 and b'gf_pos_encode_ptrs' in lib.gf_last_error() and b'null pointer' in lib.gf_last_error()
    assert pe(p, 0) == -1 and b'empty' in lib.gf_last_error()
    assert pe(p, -3) == -1
    assert pe(p, 1, dt=7) == -1 and b'dtype' in lib.gf_last_error()
    assert lib.gf_pos_encode_ptrs(p, 1, 1, 8, 8, 24, p, p, 1, 1, 8, 1, 1, None) == -1 and b'power of two' in lib.gf_last_error()

    def fg(t0, t1, n, dt=1):
        return lib.gf_fine_gather_ptrs(t0, t1, n, dt, 16, p, p, 4, 4, 4, 4, 8, p, p, 1, 1, 1, 8, p, p, p, 1, 1, 1, 4, 5, p, p, None)
    assert fg(None, p, 1) == -1 and b'gf_fine_gather_ptrs' in lib.gf_last_error() and b'null pointer' in lib.gf_last_error()
    assert fg(p, None, 1) == -1
    assert fg(p, p, 0) == -1 and b'empty' in lib.gf_last_error()
    assert fg(p, p, 1, dt=-1) == -1 and b'dtype' in lib.gf_last_error()


def test_map_batch_describes_its_maps_and_refuses_maps_that_disagree():
    from geoformer_amd.ops import MapBatch
    maps = [torch.zeros(5, 7, 16).permute(2, 0, 1) for _ in range(3)]
    mb = MapBatch([maps[2], maps[0], maps[2]])
    assert mb.shape == torch.Size([3, 16, 5, 7]) and mb.dtype == torch.float32 and mb.device == maps[0].device and len(mb) == 3
    assert mb.map_stride == (1, 7 * 16, 16) and mb.addresses == [maps[2].data_ptr(), maps[0].data_ptr(), maps[2].data_ptr()]
    assert mb.align >= 4 and all(a % mb.align == 0 for a in mb.addresses)
    off = torch.zeros(5 * 7 * 16 + 1)[1:].view(5, 7, 16).permute(2, 0, 1)              # starts one element into its allocation
    assert MapBatch([maps[0], off]).align == 4
    with pytest.raises(ValueError, match='shape'):
        MapBatch([maps[0], torch.zeros(5, 8, 16).permute(2, 0, 1)])
    with pytest.raises(ValueError, match='strides'):
        MapBatch([maps[0], torch.zeros(16, 5, 7)])                                     # same shape, NCHW strides
    with pytest.raises(ValueError, match='dtype'):
        MapBatch([maps[0], maps[1].half()])
    with pytest.raises(ValueError):
        MapBatch([])


def test_kept_features_are_an_inference_interface():
    from geoformer_amd.model.cvpr_ds_config import get_default_cfg
    from geoformer_amd.model.full_model import GeoFormer
    from geoformer_amd.model.geo_config import get_cfg_model
    m = GeoFormer(get_default_cfg(), get_cfg_model())
    m.train()
    with pytest.raises(RuntimeError, match='eval'):
        m.extract_features(torch.zeros(1, 1, 64, 64))
    with pytest.raises(RuntimeError, match='eval'):
        m.match_features([], [])
    m.eval()
    with pytest.raises(RuntimeError, match='no CPU path'):
        m.extract_features(torch.zeros(1, 1, 64, 64))
    with pytest.raises(ValueError):
        m.match_features([], [])
