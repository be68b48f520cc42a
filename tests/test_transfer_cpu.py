"""The packed transfer of the SfM stages (sfm._upload / sfm._download) and the row preamble of the pair stages (sfm._pair_rows), on device
'cpu': layout, alignment, zero sizes, dtypes - what every stage used to compute by hand."""
import numpy as np
import pytest
import torch


def _arrays(seed=0):
    rng = np.random.default_rng(seed)
    return {'f64': rng.standard_normal((5, 3)), 'i64': rng.integers(-2 ** 40, 2 ** 40, (4, 2)), 'f32': rng.standard_normal((7, 4)).astype(np.float32),
            'i32': rng.integers(-2 ** 30, 2 ** 30, 3).astype(np.int32), 'odd': rng.standard_normal(5).astype(np.float32)}


def _block_words(monkeypatch):
    """Records the length, in 32-bit words, of every block that goes through torch.from_numpy."""
    seen, real = [], torch.from_numpy

    def from_numpy(block):
        assert block.dtype == np.int32 and block.ndim == 1
        seen.append(block.size)
        return real(block)
    monkeypatch.setattr(torch, 'from_numpy', from_numpy)
    return seen


def _round_trip(sfm, arrays):
    views = sfm._upload('cpu', *arrays)
    assert len(views) == len(arrays)
    for v, a in zip(views, arrays):
        assert isinstance(v, torch.Tensor) and tuple(v.shape) == a.shape and v.dtype == sfm._DEVICE_DTYPE[a.dtype]
    back = sfm._download(*views)
    assert len(back) == len(arrays)
    for b, a in zip(back, arrays):
        assert b.dtype == a.dtype and b.shape == a.shape and b.tobytes() == np.ascontiguousarray(a).tobytes()
    return views


def test_round_trip_of_mixed_dtypes_is_bit_equal(monkeypatch):
    from geoformer_amd import sfm
    a, seen = _arrays(), _block_words(monkeypatch)
    _round_trip(sfm, [a['f32'], a['f64'], a['i32'], a['odd'], a['i64']])
    assert len(seen) == 1                                              # one block, one torch.from_numpy


def test_an_eight_byte_item_after_an_odd_number_of_words_is_padded(monkeypatch):
    from geoformer_amd import sfm
    a, seen = _arrays(1), _block_words(monkeypatch)
    items = [a['odd'], a['f64'], a['i32'], a['i64']]                   # 5 words, then fp64; 3 more words (5 + 1 + 30 + 3 = 39), then int64
    views = _round_trip(sfm, items)
    assert seen == [5 + 1 + 30 + 3 + 1 + 16]
    base = views[0].data_ptr()
    assert views[1].data_ptr() - base == 4 * 6 and views[3].data_ptr() - base == 4 * 40          # both on even words


def test_eight_byte_items_first_need_no_padding(monkeypatch):
    from geoformer_amd import sfm
    a, seen = _arrays(2), _block_words(monkeypatch)
    items = [a['f64'], a['i64'], a['f32'], a['odd'], a['i32']]
    _round_trip(sfm, items)
    assert seen == [sum(x.nbytes for x in items) // 4]                 # the block is the inputs, nothing else: the layout the stages had


@pytest.mark.parametrize('position', ['alone', 'first', 'middle', 'last'])
@pytest.mark.parametrize('empty', [np.zeros((0, 4), np.float32), np.zeros((0, 3)), np.zeros(0, np.int64), np.zeros((2, 0), np.int32)],
                         ids=['f32', 'f64', 'i64', 'i32'])
def test_zero_size_arrays(position, empty):
    from geoformer_amd import sfm
    a = _arrays(3)
    items = {'alone': [empty], 'first': [empty, a['odd'], a['f64']], 'middle': [a['odd'], empty, a['f64']],
             'last': [a['f64'], a['odd'], empty]}[position]
    _round_trip(sfm, items)


def test_non_contiguous_inputs_are_made_contiguous():
    from geoformer_amd import sfm
    a = _arrays(4)
    rows, pim = a['f32'], np.arange(12, dtype=np.int32).reshape(6, 2)
    views = _round_trip(sfm, [a['f64'].T, rows[:, :2], rows[:, 2:], pim.T, pim[:, 1], a['f64'][::2]])
    assert np.array_equal(views[3].numpy(), pim.T) and np.array_equal(views[1].numpy(), rows[:, :2])


def test_a_list_is_one_item_joined_along_the_first_axis(monkeypatch):
    from geoformer_amd import sfm
    rng, seen = np.random.default_rng(5), _block_words(monkeypatch)
    ms = [rng.standard_normal((n, 4)).astype(np.float32) for n in (3, 0, 1)]
    m, xy, off = sfm._upload('cpu', ms, [x[:, 2:] for x in ms], np.array([0, 3, 3, 4], np.int32))
    assert seen == [16 + 8 + 4]
    assert tuple(m.shape) == (4, 4) and np.array_equal(m.numpy(), np.concatenate(ms))
    assert tuple(xy.shape) == (4, 2) and np.array_equal(xy.numpy(), np.concatenate(ms)[:, 2:])
    (none,) = sfm._upload('cpu', [np.zeros((0, 4), np.float32)])
    assert tuple(none.shape) == (0, 4) and none.dtype == torch.float32


@pytest.mark.parametrize('bad', [np.zeros(3, np.uint8), np.zeros(3, bool), np.zeros(3, np.float16), np.zeros(3, np.int16),
                                 [np.zeros(3, np.float32), np.zeros(3, np.int32)]], ids=['u8', 'bool', 'f16', 'i16', 'mixed list'])
def test_an_unsupported_dtype_is_a_type_error(bad):
    from geoformer_amd import sfm
    with pytest.raises(TypeError, match='_upload: float32, int32, float64 or int64'):
        sfm._upload('cpu', np.zeros(2, np.float32), bad)


def test_download_keeps_bytes_flags_and_shapes():
    from geoformer_amd import sfm
    rng = np.random.default_rng(6)
    F, inl, ok = rng.standard_normal((2, 3, 3)), rng.integers(0, 2, 5).astype(np.uint8), np.array([True, False, True])
    nin = np.array([7, 0], np.int32)
    got = sfm._download(torch.from_numpy(F), torch.from_numpy(inl), torch.from_numpy(nin), torch.from_numpy(ok), torch.from_numpy(F)[:, 0])
    for g, want in zip(got, (F, inl, nin, ok, F[:, 0])):                  # (F after 5 bytes of flags: unaligned in the block, still exact)
        assert g.dtype == want.dtype and g.shape == want.shape and np.array_equal(g, want)


# -- _pair_rows
STAGES = ('consolidate_matches', 'verify_matches', 'relative_poses', 'localize_queries')


def _result(n, dtype=np.float32, seed=0):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, 4)).astype(dtype)
    return m, m[:, :2], m[:, 2:], rng.random(n).astype(dtype)


def test_pair_rows_without_pairs():
    from geoformer_amd import sfm
    ms, ss, off = sfm._pair_rows('verify_matches', [], [])
    assert ms == [] and ss == [] and off.dtype == np.int32 and off.tolist() == [0]


@pytest.mark.parametrize('n', [0, 1])
def test_pair_rows_of_one_pair(n):
    from geoformer_amd import sfm
    r = _result(n)
    ms, ss, off = sfm._pair_rows('verify_matches', [('a', 'b')], [r])
    assert len(ms) == len(ss) == 1 and ms[0].shape == (n, 4) and ss[0].shape == (n,) and ms[0].dtype == ss[0].dtype == np.float32
    assert off.dtype == np.int32 and off.tolist() == [0, n] and np.array_equal(ms[0], r[0]) and np.array_equal(ss[0], r[3])


def test_pair_rows_casts_float64_matches_once():
    from geoformer_amd import sfm
    rs = [_result(3, np.float64, 1), _result(0, np.float64, 2), _result(2, np.float64, 3)]
    ms, ss, off = sfm._pair_rows('relative_poses', [('a', 'b')] * 3, rs)
    assert off.tolist() == [0, 3, 3, 5] and all(m.dtype == np.float32 and s.dtype == np.float32 for m, s in zip(ms, ss))
    assert all(np.array_equal(m, r[0].astype(np.float32)) and np.array_equal(s, r[3].astype(np.float32)) for m, s, r in zip(ms, ss, rs))


@pytest.mark.parametrize('what', STAGES)
def test_pair_rows_errors_name_the_stage(what):
    from geoformer_amd import sfm
    good, bad = _result(3), _result(3)[:3] + (np.zeros(2, np.float32),)
    with pytest.raises(ValueError) as e:
        sfm._pair_rows(what, [('a', 'b'), ('a', 'c')], [good, bad])
    assert str(e.value) == f'{what}: a result whose matches and scores differ in length'
    with pytest.raises(ValueError) as e:
        sfm._pair_rows(what, [('a', 'b'), ('a', 'c')], [good])
    assert str(e.value) == f'{what}: 2 pairs but 1 results'


@pytest.mark.parametrize('what', STAGES)
def test_the_stages_raise_those_errors_before_any_upload(what, monkeypatch):
    """Through matcher.<stage>, as callers reach them: the texts are the ones the stages raised before they shared _pair_rows."""
    from geoformer_amd import matcher
    monkeypatch.setattr(torch, 'from_numpy', lambda *a, **k: pytest.fail('an upload was prepared'))
    good, bad = _result(3), _result(3)[:3] + (np.zeros(2, np.float32),)
    pairs = [('a', 'b'), ('a', 'c')]
    extra = {'consolidate_matches': (), 'verify_matches': (), 'relative_poses': ({n: np.eye(3) for n in 'abc'},),
             'localize_queries': ({'a': np.eye(3)}, {})}[what]
    with pytest.raises(ValueError) as e:
        getattr(matcher, what)(pairs, [good, bad], *extra, device='cpu')
    assert str(e.value) == f'{what}: a result whose matches and scores differ in length'
    with pytest.raises(ValueError) as e:
        getattr(matcher, what)(pairs, [good], *extra, device='cpu')
    assert str(e.value) == f'{what}: 2 pairs but 1 results'


def test_matcher_still_resolves_the_moved_names():
    from geoformer_amd import matcher, sfm
    for name in ('consolidate_matches', 'verify_matches', 'relative_poses', 'localize_queries', 'undistort_results', 'triangulate', 'refine',
                 'localize_queries_sparse', '_refine_device', '_device_rows', '_sparse_rows', '_covis_tables', '_original_pixel_rows',
                 '_triangulation_inputs', '_assemble_tracks', '_refine_inputs', 'Camera', 'read_triangulated', 'write_triangulated'):
        assert getattr(matcher, name) is getattr(sfm, name), name
    assert not hasattr(sfm, 'matcher')
