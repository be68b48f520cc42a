"""The refit of the fundamental matrix on its inliers (the `refit` rule of geoformer_amd/csrc/fund_solver.h) through its host build
(csrc/host/fund_host.cpp: gf_fund_host_ransac_lo, gf_fund_host_refit_once).  No GPU.  Scenes, the independent numpy restatement (SVD for
the null vector and for the rank-2 step, not Jacobi) and the ctypes front end: tests/fund_refit_cases.py."""
import numpy as np
import pytest

import fund_cases as C
import fund_refit_cases as R

# One refit, host build (Jacobi on the normal matrix, FS_JACOBI9_SWEEPS = 10, FS_JACOBI3_SWEEPS = 8) against numpy_fit (SVD of the rows): the
# largest entry difference of the unit-norm F in pixels, up to sign, over the first 8, 9, 20 and all planted inliers of the 12 scenes
# 2000 .. 2011 measured 1.41e-10 (the 8- and 9-row fits carry it: the normal matrix squares the condition number the SVD sees).  The gate is
# 10 x that, the room for other seeds' conditioning.
ONE_REFIT_MEASURED = 1.41e-10
ONE_REFIT_BOUND = 10 * ONE_REFIT_MEASURED
DET_BOUND = 1e-15                 # |det| of the max-abs-normalised refit; measured 1.7e-19 on the same fits
OUTCOME_SEEDS = range(1000, 1024)
WORDS = ('status', 'valid', 'n_inliers')


def same_outputs(a, b):
    return (all(a[k] == b[k] for k in WORDS) and tuple(a['hyp']) == tuple(b['hyp']) and np.array_equal(a['inliers'], b['inliers'])
            and np.array_equal(a['F'].view(np.int64), b['F'].view(np.int64)))


@pytest.fixture(scope='module')
def outcome_runs():
    """seeds 1000 .. 1023, n = 300, 30 % outliers, sigma = 0.5 px; 128 hypotheses, thr = 1, R = 4, sample = 0"""
    out = []
    for seed in OUTCOME_SEEDS:
        sc = R.noisy_scene(seed, 300, 0.3, 0.5)
        plain = C.host_ransac(sc['m'], thr=1.0, iters=128)
        seven = R.host_ransac_lo(sc['m'], thr=1.0, iters=128, refit=0)
        refit = R.host_ransac_lo(sc['m'], thr=1.0, iters=128, refit=4)
        norm = C.box_norm(sc['m'][:, :2], sc['m'][:, 2:])
        Fn, mask_n, rounds_n = R.numpy_refit(sc['m'], seven['F'], seven['inliers'], norm, 1.0, 4)
        out.append((sc, plain, seven, refit, Fn))
    return out


def test_zero_rounds_is_the_seven_point_ransac_on_every_output_word(outcome_runs):
    for sc, plain, seven, refit, _ in outcome_runs:
        assert seven['rounds'] == 0 and same_outputs({**plain, 'rounds': 0}, seven)
        assert tuple(refit['hyp']) == tuple(seven['hyp'])               # `best` keeps naming the seed of the result
    for seed in (120, 121):                                            # exact scenes: the winner already holds every planted inlier
        m = C.scene(seed, 300, 0.3)['m']
        for iters in (64, 256):
            assert same_outputs(C.host_ransac(m, iters=iters), R.host_ransac_lo(m, iters=iters, refit=0))


def test_rounds_zero_means_the_winners_bits_and_inliers_never_decrease(outcome_runs):
    zero = 0
    runs = [(sc['m'], seven, refit) for sc, _, seven, refit, _ in outcome_runs]
    for seed in range(30, 50):                                         # small and exact scenes, where a refit is often rejected or not tried
        m = (C.scene(seed, 7 + seed % 9, 0.0) if seed % 2 else R.noisy_scene(seed, 12 + seed % 9, 0.4, 1.0))['m']
        runs.append((m, R.host_ransac_lo(m, iters=64, refit=0), R.host_ransac_lo(m, iters=64, refit=8)))
    for m, seven, refit in runs:
        assert refit['status'] == seven['status'] and 0 <= refit['rounds'] <= 8
        assert refit['n_inliers'] >= seven['n_inliers'] and refit['n_inliers'] == int(refit['inliers'].sum())
        if refit['rounds'] == 0:
            zero += 1
            assert same_outputs(seven, {**refit, 'rounds': 0})
        elif refit['valid']:
            assert abs(np.linalg.norm(refit['F']) - 1) < 1e-12
    assert zero > 0
    # more rounds never give fewer inliers than fewer rounds: round r + 1 starts from round r's result
    sc = outcome_runs[0][0]
    counts = [R.host_ransac_lo(sc['m'], thr=1.0, iters=128, refit=r)['n_inliers'] for r in range(9)]
    assert counts == sorted(counts)


def test_fewer_than_eight_inliers_are_not_refitted():
    sc = R.noisy_scene(7, 40, 0.0, 0.5)
    r = R.host_ransac_lo(sc['m'][:7], iters=64, refit=8)
    assert r['valid'] == 1 and r['n_inliers'] == 7 and r['rounds'] == 0
    assert same_outputs(C.host_ransac(sc['m'][:7], iters=64), r)
    for n in (6, 0):
        r = R.host_ransac_lo(sc['m'][:n], iters=64, refit=8)
        assert r['status'] == 0 and r['rounds'] == 0 and not r['inliers'].any() and not r['F'].any()
    junk = np.random.default_rng(1).uniform(0, 480, (60, 4)).astype(np.float32)         # pure outliers: whatever happens, the rule holds
    a, b = R.host_ransac_lo(junk, iters=64, refit=0), R.host_ransac_lo(junk, iters=64, refit=8)
    assert b['n_inliers'] >= a['n_inliers'] and (b['rounds'] > 0 or same_outputs(a, b))


def test_filtered_and_non_finite_rows_never_enter_the_fit():
    sc = R.noisy_scene(120, 300, 0.3, 0.5)
    m = sc['m'].copy()
    rng = np.random.default_rng(5)
    scores = rng.uniform(0.3, 1.0, 300).astype(np.float32)
    scores[[3, 70, 71, 72, 100, 130, 131, 190, 299]] = 0.1
    scores[150] = np.nan
    m[17, 0] = np.nan; m[66, 3] = np.inf; m[200, 2] = -np.inf
    keep = (scores >= 0.25) & np.isfinite(m).all(1)
    a = R.host_ransac_lo(m, scores, sc_thres=0.25, iters=128, refit=4)
    b = R.host_ransac_lo(m[keep], None, iters=128, refit=4)
    assert a['valid'] == 1 and a['rounds'] > 0 and not a['inliers'][~keep].any()
    assert np.array_equal(a['inliers'][keep], b['inliers']) and a['n_inliers'] == b['n_inliers'] and a['rounds'] == b['rounds']
    assert np.array_equal(a['F'].view(np.int64), b['F'].view(np.int64)) and np.isfinite(a['F']).all()


def test_one_refit_against_numpy_svd():
    worst, worst_det = 0.0, 0.0
    for seed in range(2000, 2012):
        sc = R.noisy_scene(seed, 300, 0.3, 0.5)
        norm = C.box_norm(sc['m'][:, :2], sc['m'][:, 2:])
        inl = np.flatnonzero(~sc['outlier'])
        for k in (8, 9, 20, len(inl)):
            mask = np.zeros(300, np.uint8)
            mask[inl[:k]] = 1
            Fh, Fn = R.host_refit_once(sc['m'], mask, norm), R.numpy_fit(sc['m'], mask, norm)
            assert Fh is not None and abs(np.linalg.norm(Fh) - 1) < 1e-12
            worst = max(worst, min(np.abs(Fh - Fn).max(), np.abs(Fh + Fn).max()))
            worst_det = max(worst_det, abs(np.linalg.det(Fh / np.abs(Fh).max())))
    print(f'one refit, host build against numpy SVD: largest entry difference {worst:.3e} (gate {ONE_REFIT_BOUND:.2e}), '
          f'largest |det| of the max-abs-normalised F {worst_det:.3e}')
    assert worst <= ONE_REFIT_BOUND
    assert worst_det <= DET_BOUND


def test_outcome_on_noisy_scenes(outcome_runs):
    """Host build: median held-out error 0.480 px for the seven-point winner, 0.130 px after the refit (ratio 0.271), better in 24 of 24
    scenes (worst per-scene ratio 0.517); mean inliers 171.8 -> 200.5 of 210 planted.  The numpy restatement from the same winners: 0.130 px,
    24 of 24."""
    e7, er, en = [], [], []
    for sc, _, seven, refit, Fn in outcome_runs:
        e7.append(R.heldout_error(seven['F'], sc['h0'], sc['h1']))
        er.append(R.heldout_error(refit['F'], sc['h0'], sc['h1']))
        en.append(R.heldout_error(Fn, sc['h0'], sc['h1']))
    e7, er, en = np.array(e7), np.array(er), np.array(en)
    print(f'median held-out error: seven-point {np.median(e7):.3f} px, host refit {np.median(er):.3f} px, numpy refit {np.median(en):.3f} px; '
          f'host better in {int((er < e7).sum())}, numpy in {int((en < e7).sum())} of {len(e7)}; worst host ratio {(er / e7).max():.3f}; mean '
          f'inliers {np.mean([r[2]["n_inliers"] for r in outcome_runs]):.1f} -> {np.mean([r[3]["n_inliers"] for r in outcome_runs]):.1f}')
    lowered = en < e7
    assert (~lowered).sum() <= 2                                       # the scenes the condition may exempt
    assert (er[lowered] < e7[lowered]).all()
    assert np.median(er) <= 0.5 * np.median(e7)


def test_argument_errors():
    m = R.noisy_scene(3, 50, 0.3, 0.5)['m']
    for refit in (-1, 9, 100):
        assert R.host_ransac_lo(m, iters=64, refit=refit)['status'] == -1
    for iters in (0, 100, -64):
        assert R.host_ransac_lo(m, iters=iters, refit=4)['status'] == -1
    assert R.host_ransac_lo(m, iters=64, thr=0.0, refit=4)['status'] == -1
    h = R.host_lib()
    F, hyp, nin, mask = np.zeros(9), np.zeros(2, np.int32), np.zeros(1, np.int32), np.zeros(50, np.uint8)
    args = (m.ctypes.data, None, 50, 0.25, 1.0, 64, 1, 0)
    assert h.gf_fund_host_ransac_lo(*args, 4, F.ctypes.data, hyp.ctypes.data, nin.ctypes.data, mask.ctypes.data, None) == -1     # rounds missing
    assert h.gf_fund_host_ransac_lo(*args, 0, F.ctypes.data, hyp.ctypes.data, nin.ctypes.data, mask.ctypes.data, None) == 1
