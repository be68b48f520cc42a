"""The aggregation half of geoformer_amd/train/metrics.py (pure numpy, no GPU) against values stated here in plain numpy."""
import numpy as np

import pose_cases as P
from geoformer_amd.train import metrics as MT


def _T(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def test_relative_pose_error_angles_fold_and_ignore_threshold():
    R_gt = P.rodrigues(np.array([0.0, 0.2, 0.0]))
    t_gt = np.array([1.0, 0.0, 0.0])
    T = _T(R_gt, t_gt)
    # R off by a rotation of 3 degrees about z (applied on the left), t off by 10 degrees in the x-y plane
    R = P.rodrigues(np.array([0, 0, np.deg2rad(3.0)])) @ R_gt
    t = np.array([np.cos(np.deg2rad(10.0)), np.sin(np.deg2rad(10.0)), 0.0]) * 2.5            # the length does not matter
    t_err, R_err = MT.relative_pose_error(T, R, t)
    assert abs(R_err - 3.0) < 1e-9 and abs(t_err - 10.0) < 1e-9
    # the sign ambiguity of E: -t is the same answer, 170 degrees folds to 10
    t_err, _ = MT.relative_pose_error(T, R, -t)
    assert abs(t_err - 10.0) < 1e-9
    # exact answer, numerical noise outside [-1, 1] is clipped
    t_err, R_err = MT.relative_pose_error(T, R_gt, t_gt * (1 + 1e-16))
    assert t_err == 0.0 and R_err < 1e-6
    # pure rotation: a ground-truth translation shorter than ignore_gt_t_thr is not scored
    T0 = _T(R_gt, np.array([1e-3, 0, 0]))
    assert MT.relative_pose_error(T0, R, np.array([0, 1.0, 0]), ignore_gt_t_thr=0.01)[0] == 0
    assert abs(MT.relative_pose_error(T0, R, np.array([0, 1.0, 0]), ignore_gt_t_thr=0.0)[0] - 90.0) < 1e-9


def _auc_by_hand(errors, thr):
    """Area under the step-free recall curve through (0, 0), (e_1, 1/n), .. (e_n, 1) up to thr, over thr; recall held flat from
    the last error below thr."""
    e = np.sort(np.asarray(errors, float))
    n = len(e)
    xs, ys = [0.0], [0.0]
    for i, v in enumerate(e):
        if v < thr:
            xs.append(v); ys.append((i + 1) / n)
    xs.append(thr); ys.append(ys[-1])
    area = sum((xs[i + 1] - xs[i]) * (ys[i + 1] + ys[i]) / 2 for i in range(len(xs) - 1))
    return area / thr


def test_error_auc_hand_values_and_ignored_thresholds():
    errs = [1.0, 3.0, 7.0, 15.0, np.inf]
    out = MT.error_auc(errs, [1, 2, 3])                       # the argument is ignored: [5, 10, 20] as in the reference
    assert list(out) == ['auc@5', 'auc@10', 'auc@20']
    # auc@5: points (0,0) (1,.2) (3,.4) (5,.4): 0.1 + 0.6 + 0.8 = 1.5 -> 0.3
    assert abs(out['auc@5'] - 0.3) < 1e-12
    # auc@10: + (7,.6) (10,.6): 1.5 - 0.8 + (3..7: 4 * 0.5 = 2.0) + 3 * 0.6 = 1.8 -> (0.1 + 0.6 + 2.0 + 1.8) / 10 = 0.45
    assert abs(out['auc@10'] - 0.45) < 1e-12
    for thr in (5, 10, 20):
        assert abs(out[f'auc@{thr}'] - _auc_by_hand(errs, thr)) < 1e-12
    assert MT.error_auc([np.inf, np.inf], None) == {'auc@5': 0.0, 'auc@10': 0.0, 'auc@20': 0.0}
    assert abs(MT.error_auc([0.0, 0.0], None)['auc@5'] - 1.0) < 1e-12


def test_epidist_prec_with_an_empty_pair():
    errs = np.empty(3, dtype=object)
    errs[0] = np.array([1e-5, 2e-4, 6e-4, 1e-3])                # 2 of 4 below 5e-4
    errs[1] = np.array([])                                      # no matches: precision 0, the pair still counts
    errs[2] = np.array([1e-6])
    assert MT.epidist_prec(errs, [5e-4]) == [(0.5 + 0 + 1.0) / 3]
    d = MT.epidist_prec(errs, [5e-4, 1e-4], ret_dict=True)
    assert list(d) == ['prec@5e-04', 'prec@1e-04'] and abs(d['prec@1e-04'] - (0.25 + 0 + 1.0) / 3) < 1e-15
    assert MT.epidist_prec([], [5e-4]) == [0]


def test_aggregate_metrics_drops_duplicates_and_handles_inf():
    m = {'identifiers': ['a#b', 'c#d', 'a#b', 'e#f'],
         'R_errs': [50.0, 2.0, 1.0, np.inf],
         't_errs': [60.0, 4.0, 3.0, np.inf],
         'epi_errs': [np.array([1.0, 1.0]), np.array([1e-5, 1e-3]), np.array([1e-5]), np.array([])],
         'inliers': [np.array([]), np.array([True, False]), np.array([True]), np.array([])]}
    out = MT.aggregate_metrics(m, epi_err_thr=5e-4)
    # 'a#b' appears twice: the LATER entry is the one kept (the OrderedDict of the reference), so the pose errors are
    # max(R, t) of items 2, 1, 3 = [3, 4, inf] and the precisions [1, 0.5, 0]
    want = MT.error_auc([3.0, 4.0, np.inf], None)
    assert out['auc@5'] == want['auc@5'] and out['auc@10'] == want['auc@10'] and out['auc@20'] == want['auc@20']
    # by hand: points (0,0) (3,1/3) (4,2/3) (5,2/3): 0.5 + 0.5 + 2/3 = 5/3 -> 1/3
    assert abs(out['auc@5'] - 1 / 3) < 1e-12
    assert abs(out['prec@5e-04'] - 0.5) < 1e-15
    assert set(out) == {'auc@5', 'auc@10', 'auc@20', 'prec@5e-04'}


def test_trainer_config_carries_the_validation_keys():
    from geoformer_amd.train.trainer import DEFAULT_TRAINER_CFG, scale_trainer_cfg
    cfg = scale_trainer_cfg(None, 1, 8)
    assert cfg['epi_err_thr'] == 5e-4 and cfg['ransac_pixel_thr'] == 0.5 and cfg['ransac_conf'] == 0.99999
    assert set(DEFAULT_TRAINER_CFG) >= {'epi_err_thr', 'ransac_pixel_thr', 'ransac_conf'}
