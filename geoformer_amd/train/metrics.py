"""Relative-pose validation metrics: the counterpart of model/loftr_src/utils/metrics.py with the reference's names and return
conventions.  The two per-match / per-pair computations run on the device (ops.epipolar_errors, ops.ransac_essential: the
cv2.findEssentialMat + cv2.recoverPose host round trip per pair becomes two kernel launches per batch); the aggregation is the
reference's numpy.

OpenCV parity of the estimated pose is unpinned (geoformer_amd/csrc/pose_solver.h states the algorithm): the iteration count is
fixed (ops.POSE_RANSAC_ITERS), so `ransac_conf` is accepted and unused.
"""
import logging

import numpy as np
import torch

from .. import ops

logger = logging.getLogger(__name__)
_trapz = getattr(np, 'trapezoid', None) or np.trapz


POSE_THRESHOLDS = (5, 10, 20)          # degrees; the only thresholds the pose AUC is reported at


def _angle_deg(cosine):
    return float(np.degrees(np.arccos(min(1.0, max(-1.0, float(cosine))))))


def relative_pose_error(T_0to1, R, t, ignore_gt_t_thr=0.0):
    """-> (t_err, R_err) in degrees against the ground-truth transform T_0to1 [4,4].
    t_err is the angle between the two translation DIRECTIONS, folded to [0, 90] because E fixes t only up to sign, and 0 when the
    ground-truth translation is shorter than `ignore_gt_t_thr` (a pure rotation has no direction to score).  R_err is the angle of
    the rotation that takes R to the ground truth."""
    gt_R, gt_t = np.asarray(T_0to1)[:3, :3], np.asarray(T_0to1)[:3, 3]
    gt_len = float(np.linalg.norm(gt_t))
    t_err = _angle_deg(np.dot(t, gt_t) / (float(np.linalg.norm(t)) * gt_len))
    if t_err > 90.0:
        t_err = 180.0 - t_err
    if gt_len < ignore_gt_t_thr:
        t_err = 0
    R_err = _angle_deg((np.trace(np.asarray(R).T @ gt_R) - 1.0) * 0.5)
    return t_err, R_err


def compute_symmetrical_epipolar_errors(data):
    """Update: data['epi_errs'] fp32 [M], the squared symmetric epipolar distance of every fine match under its pair's T_0to1
    (metrics.py:50-69), on the device."""
    data.update({'epi_errs': ops.epipolar_errors(data['mkpts0_f'], data['mkpts1_f'], data['m_bids'], data['T_0to1'], data['K0'], data['K1'])})


def _cfg_get(config, key, default):
    """TRAINER.RANSAC_PIXEL_THR of a yacs-style config, or the lower-case key of the trainer dict."""
    tr = getattr(config, 'TRAINER', None)
    if tr is not None:
        return getattr(tr, key.upper(), default)
    if config is None:
        return default
    return config.get(key, default)


def match_counts(m_bids, N):
    """int32 [1+N] (total, per pair) on the device, without a host synchronisation."""
    per = torch.zeros(N, dtype=torch.int32, device=m_bids.device)
    per.index_add_(0, m_bids.to(torch.int64), torch.ones(m_bids.shape[0], dtype=torch.int32, device=m_bids.device))
    return torch.cat([per.sum(0, keepdim=True, dtype=torch.int32), per])


def compute_pose_errors(data, config=None):
    """Update: data['R_errs'], data['t_errs'] (List[float], [N]) and data['inliers'] (List[np.ndarray], [N]) - metrics.py:101-134.
    A pair without a pose gets inf errors and an empty mask.  `m_bids` must be sorted by pair (the matcher emits it so).  One
    download per batch."""
    pixel_thr = _cfg_get(config, 'ransac_pixel_thr', 0.5)
    _ = _cfg_get(config, 'ransac_conf', 0.99999)            # unused: the number of hypotheses is fixed
    data.update({'R_errs': [], 't_errs': [], 'inliers': []})
    N = data['K0'].shape[0]
    m_bids = data['m_bids']
    M = m_bids.shape[0]
    rs = ops.ransac_essential(data['mkpts0_f'], data['mkpts1_f'], match_counts(m_bids, N), N, data['K0'], data['K1'], pixel_thr=pixel_thr)
    dev = m_bids.device
    packed = torch.cat([rs['R'].reshape(-1), rs['t'].reshape(-1), rs['valid'].double(), data['T_0to1'].to(dev).double().reshape(-1),
                        m_bids.double(), rs['inliers'].double()]).cpu().numpy()
    R, t, valid, T = (packed[:9 * N].reshape(N, 3, 3), packed[9 * N:12 * N].reshape(N, 3), packed[12 * N:13 * N],
                      packed[13 * N:29 * N].reshape(N, 4, 4))
    bids, inl = packed[29 * N:29 * N + M].astype(np.int64), packed[29 * N + M:] > 0
    no_mask = np.zeros(0, dtype=bool)
    for pair in range(N):
        R_err = t_err = np.inf                               # a pair without a pose: inf errors, empty mask
        mask = no_mask
        if valid[pair]:
            t_err, R_err = relative_pose_error(T[pair], R[pair], t[pair], ignore_gt_t_thr=0.0)
            mask = inl[bids == pair]
        data['R_errs'].append(R_err)
        data['t_errs'].append(t_err)
        data['inliers'].append(mask)


def error_auc(errors, thresholds):
    """{'auc@5', 'auc@10', 'auc@20'}: area under the recall-over-error curve up to each threshold, divided by the threshold.
    The curve passes through (0, 0) and (e_k, k / n) for the sorted errors and is held flat from the last error below the threshold.
    `thresholds` is accepted and ignored - the reference reports at 5 / 10 / 20 degrees whatever it is given."""
    curve_x = np.concatenate([[0.0], np.sort(np.asarray(list(errors), dtype=np.float64))])
    curve_y = np.linspace(0.0, 1.0, len(curve_x))
    out = {}
    for limit in POSE_THRESHOLDS:
        k = int(np.searchsorted(curve_x, limit))          # points strictly below the threshold
        xs = np.append(curve_x[:k], limit)
        ys = np.append(curve_y[:k], curve_y[k - 1])
        out[f'auc@{limit}'] = float(_trapz(ys, xs)) / limit
    return out


def epidist_prec(errors, thresholds, ret_dict=False):
    """Matching precision per threshold: per pair the share of matches whose epipolar error is below it (0 for a pair without
    matches), averaged over the pairs (0 without pairs).  A list, or {'prec@<thr>': value} with ret_dict."""
    values = []
    for limit in thresholds:
        shares = [float(np.mean(np.asarray(e) < limit)) if len(e) else 0 for e in errors]
        values.append(sum(shares) / len(shares) if shares else 0)
    if ret_dict:
        return {f'prec@{limit:.0e}': v for limit, v in zip(thresholds, values)}
    return values


def aggregate_metrics(metrics, epi_err_thr=5e-4):
    """Dataset-level numbers from the concatenated per-step 'metrics' dicts: pose AUC@5/10/20 of max(R_err, t_err) and the mean
    matching precision at `epi_err_thr`.  An identifier that occurs more than once (a distributed sampler pads the last batch) is
    counted once: its LAST occurrence, at the position of its first."""
    last_seen = {}
    for pos, name in enumerate(metrics['identifiers']):
        last_seen[name] = pos                              # dicts keep first-insertion order; the value is overwritten
    rows = list(last_seen.values())
    logger.info('aggregating %d unique pairs of %d', len(rows), len(metrics['identifiers']))
    worst = np.maximum(np.asarray(metrics['R_errs'], dtype=np.float64), np.asarray(metrics['t_errs'], dtype=np.float64))
    out = error_auc(worst[rows], POSE_THRESHOLDS)
    out.update(epidist_prec([metrics['epi_errs'][r] for r in rows], [epi_err_thr], ret_dict=True))
    return out
