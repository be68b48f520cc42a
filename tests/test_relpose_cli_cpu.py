"""The host-side pieces of `python -m geoformer_amd.matcher pairs ... --verify-pose`: the parser, its two restrictions, and the files of
a run with a stubbed matcher and the host build of the rule in place of the device (tests/relpose_cases.py)."""
import io
import os

import numpy as np
import pytest

import pose_cases as P
import relpose_cases as C

KEYS = ['kpts1', 'kpts2', 'matches', 'scores']


class _Store:
    extractions = hits = 0


class _Matcher:
    """match_many of planted scenes: pair k = scene 60 + k, 80 rows"""
    device, name, store = 'cpu', 'stub', _Store()

    def match_many(self, pairs, **kw):
        out = []
        for k in range(len(pairs)):
            m = C.rows(P.scene(60 + k, 80, 0.3, 0.3)).astype(np.float64)
            out.append((m, m[:, :2].copy(), m[:, 2:].copy(), np.full(len(m), 0.9, np.float32)))
        return out


def _host_relative_poses(pairs, results, intrinsics, thr=1.0, min_inliers=15, sc_thres=0.25, iters=None, device='cuda', refit=0):
    from geoformer_amd import matcher
    rs = [C.host_ransac(r[0], r[3], intrinsics[a], intrinsics[b], pixel_thr=thr, sc_thres=sc_thres, iters=512, sample=k, refit=refit)
          for k, ((a, b), r) in enumerate(zip(pairs, results))]
    ver = np.array([r['valid'] == 1 and r['n_inliers'] >= min_inliers for r in rs])
    return matcher.RelativePoses(np.stack([r['E'] for r in rs]), np.stack([r['R'] for r in rs]), np.stack([r['t'] for r in rs]),
                                 np.array([r['n_inliers'] for r in rs], np.int32), ver,
                                 [r['inliers'] if v else np.zeros(len(r['inliers']), bool) for r, v in zip(rs, ver)],
                                 np.array([r['rounds'] for r in rs], np.int32))


@pytest.fixture
def cli(tmp_path, monkeypatch):
    from geoformer_amd import matcher
    monkeypatch.setattr(matcher, 'GeoFormerMatcher', lambda *a, **k: _Matcher())
    monkeypatch.setattr(matcher, 'relative_poses', _host_relative_poses)
    names = [str(tmp_path / f'{c}.png') for c in 'abc']
    lst = tmp_path / 'pairs.txt'
    lst.write_text(f'{names[0]} {names[1]}\n{names[1]} {names[2]}\n')
    intr = tmp_path / 'k.txt'
    intr.write_text(''.join(f'{os.path.basename(n)} 500 500 320 240\n' for n in names))
    return matcher, str(lst), str(intr), tmp_path


def _npz(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def test_parser_and_its_two_restrictions(cli, capsys):
    matcher, lst, intr, tmp = cli
    a = matcher.build_parser().parse_args(['pairs', lst, '--verify-pose', '--intrinsics', intr, '--verify-refit'])
    assert a.verify_pose and a.intrinsics == intr and a.verify_refit == 4 and not a.verify and a.verify_thr == 1.0 and a.min_inliers == 15
    assert not matcher.build_parser().parse_args(['pairs', lst]).verify_pose
    for bad in (['--verify-pose'], ['--verify-pose', '--intrinsics', intr, '--verify'],
                ['--verify-pose', '--intrinsics', intr, '--cameras', intr], ['--verify-pose', '--intrinsics', intr, '--verify-refit', '9']):
        with pytest.raises(SystemExit) as e:
            matcher.main(['pairs', lst, *bad])
        assert e.value.code == 2 and '--verify-pose' in capsys.readouterr().err


def test_files_of_a_run_with_the_flag(cli, monkeypatch):
    matcher, lst, intr, tmp = cli
    monkey_cm = matcher.ConsolidatedMatches(['a', 'b', 'c'], [np.zeros((0, 2), np.float32)] * 3, np.array([[0, 1], [1, 2]], np.int32),
                                            [np.zeros((0, 2), np.int32)] * 2)
    kept = {}

    def consolidate(pairs, results, *a, keep=None, **k):
        kept['keep'] = keep
        return monkey_cm
    monkeypatch.setattr(matcher, 'consolidate_matches', consolidate)
    monkeypatch.setattr(matcher, 'write_consolidated', lambda d, cm: os.makedirs(d, exist_ok=True))
    matcher.main(['pairs', lst, '--verify-pose', '--intrinsics', intr, '--verify-refit', '2', '--out', str(tmp / 'm'), '--keypoints', str(tmp / 'k')])
    pairs = matcher.read_pair_list(lst)
    want = _host_relative_poses(pairs, _Matcher().match_many(pairs), matcher._intrinsics_for(intr, pairs), refit=2)
    assert want.verified.all() and (want.rounds > 0).any()
    files = sorted(os.listdir(tmp / 'm'))
    assert len(files) == 2
    for k, f in enumerate(files):
        z = _npz(tmp / 'm' / f)
        assert sorted(z) == sorted(KEYS + ['E', 'R', 't', 'inliers', 'verified', 'refit_rounds'])
        assert np.array_equal(z['E'], want.E[k]) and np.array_equal(z['R'], want.R[k]) and np.array_equal(z['t'], want.t[k])
        assert np.array_equal(z['inliers'], want.masks[k]) and bool(z['verified']) and int(z['refit_rounds']) == int(want.rounds[k])
        assert abs(np.linalg.norm(z['E']) - 1) < 1e-12 and abs(np.linalg.det(z['R']) - 1) < 1e-12
    tv = _npz(tmp / 'k' / 'two_view.npz')
    assert sorted(tv) == sorted(['pairs', 'E', 'R', 't', 'n_inliers', 'verified', 'refit_rounds'])
    assert np.array_equal(tv['pairs'], [[0, 1], [1, 2]]) and np.array_equal(tv['R'], want.R) and np.array_equal(tv['n_inliers'], want.n_inliers)
    assert all(np.array_equal(a, b) for a, b in zip(kept['keep'], want.masks))         # only verified inliers are consolidated
    assert not os.path.exists(tmp / 'k' / 'intrinsics.txt')                             # (--cameras writes it, --intrinsics does not)
    # without the refit there is no refit_rounds
    matcher.main(['pairs', lst, '--verify-pose', '--intrinsics', intr, '--out', str(tmp / 'm0')])
    assert sorted(_npz(tmp / 'm0' / sorted(os.listdir(tmp / 'm0'))[0])) == sorted(KEYS + ['E', 'R', 't', 'inliers', 'verified'])


def test_a_missing_image_in_the_intrinsics_file_names_it(cli):
    matcher, lst, intr, tmp = cli
    with open(intr, 'w') as f:
        f.write('a.png 500 500 320 240\nb.png 500 500 320 240\n')
    with pytest.raises(SystemExit, match='c.png'):
        matcher.main(['pairs', lst, '--verify-pose', '--intrinsics', intr, '--out', str(tmp / 'm')])


def test_a_run_without_the_flag_writes_what_it_wrote_before(cli):
    """the key set is pinned, and every file holds the members of np.savez on the four arrays, in their order and with their bytes - what
    the command wrote before the flag existed (a zip member's time stamp is the one thing that differs between two writes)"""
    import zipfile
    matcher, lst, intr, tmp = cli
    matcher.main(['pairs', lst, '--out', str(tmp / 'm')])
    pairs = matcher.read_pair_list(lst)
    files = sorted(os.listdir(tmp / 'm'))
    assert files == ['00000_a_b.npz', '00001_b_c.npz']
    for f, res in zip(files, _Matcher().match_many(pairs)):
        assert sorted(_npz(tmp / 'm' / f)) == KEYS
        buf = io.BytesIO()
        np.savez(buf, matches=res[0], kpts1=res[1], kpts2=res[2], scores=res[3])
        with zipfile.ZipFile(tmp / 'm' / f) as got, zipfile.ZipFile(buf) as want:
            assert got.namelist() == want.namelist() == ['matches.npy', 'kpts1.npy', 'kpts2.npy', 'scores.npy']
            assert all(got.read(n) == want.read(n) for n in want.namelist())
            assert [i.compress_type for i in got.infolist()] == [i.compress_type for i in want.infolist()]
