"""Outcome-level parity of the 'bf16_fp16' mode (bf16 backbone, fp16 matching path): the 260-pair synthetic HPatches-protocol comparison
of tests/test_outcome_parity_gpu.py::test_hpatches_protocol_auc_260_pairs (same pairs, same committed fp32-oracle fixture
tests/golden/g18_outcome_oracle_260.npz, same evaluation arithmetic, same printed block, same failed-pair condition), with the product
side = the mode's forward_features fed the planted maps as BF16 - what its backbone hands over.

MI355X, the printed block as committed in profiles/mixed_precision_outcome_260.txt (failed pairs 2 / 2, 168 / 168 matches per pair):
  dAUC@1/3/5/10 = -1.63e-3 / -3.4e-4 / -2.2e-4 / -1.1e-4, paired standard error 1.22e-3 / 4.6e-4 / 2.8e-4 / 1.4e-4
  (the fp16 mode on the same pairs: +1.8e-3 / +3.4e-4 / +1.9e-4 / +0.9e-4; the bf16 mode: -2.0e-3 / -1.5e-3 / -2.4e-3 / -3.1e-3).
|dAUC@3| is a third of north_star's 1e-3 and within one standard error of zero: the bar is met."""
import os

import numpy as np
import pytest
import torch

import golden_inputs as GI
from test_outcome_parity_gpu import DEV, GATE_260, PAIRS, THRES, _auc_terms

pytestmark = pytest.mark.gpu

# |dAUC@3| and max over the thresholds |dAUC@t|.  The rule: north_star's 1e-3 on |dAUC@3| when the MI355X measurement is inside it, otherwise the bf16
# mode's gate (GATE_260['bf16']) - never looser than the mode this one improves on; the maximum over the thresholds is gated at the bf16 mode's 9e-3
# unless the measurement supports the fp16 mode's 4e-3.  Measured (above): |dAUC@3| = 3.4e-4 -> 1e-3; the maximum is |dAUC@1| = 1.63e-3, below the fp16
# mode's own 1.8e-3 at that threshold, which the 4e-3 gate was set for -> 4e-3.
GATE_AUC3 = 1e-3
GATE_MAX = 4e-3
assert GATE_AUC3 <= GATE_260['bf16']          # never looser than the mode it improves on


def _product_side(seqs):
    from geoformer_amd import matcher as MT
    from test_e2e_gpu import build, to_dev
    m = build(0.2, 0.1, 'bf16_fp16')
    m.geo_module.homography_fn = None      # device RANSAC
    assert m.compute_dtype == torch.float16 and m.backbone_dtype == torch.bfloat16
    data = to_dev({'image0': torch.zeros(1, 1, 480, 640), 'image1': torch.zeros(1, 1, 480, 608)})
    rows = {}
    for s in range(seqs):
        for k in range(1, PAIRS + 1):
            (c0, f0), (c1, f1), H = GI.hpatches_like_features(s, k)
            with torch.no_grad():
                # bf16 and channels-last, as the backbone emits them: the vector form of gf_pos_encode, the row form of gf_fine_gather
                out = m.forward_features(dict(data), *(t.to(DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
                                                       for t in (c0, f0, c1, f1)))
            assert out['_feat_dev']['geo_f0'].dtype == torch.float16
            matches = torch.cat([out['mkpts0_f'], out['mkpts1_f']], 1).float().cpu().numpy()
            Hp = None
            if len(matches) >= 4:
                Hp, _ = MT.estimate_homography(matches, 3.0, DEV)
            rows[(s, k)] = (MT.corner_error(Hp, H, 640, 480) if Hp is not None else float('inf'), len(matches))
    return rows


def test_hpatches_protocol_auc_260_pairs_bf16_fp16():
    from geoformer_amd import matcher as MT
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g18_outcome_oracle_260.npz'))
    assert len(G['err']) == 260
    got = _product_side(52)
    keys = [(int(s), int(k)) for s, k in zip(G['seq'], G['pair'])]
    er, nr = G['err'].astype(float), G['nmatch']
    eg = np.array([got[k][0] for k in keys]); ng = np.array([got[k][1] for k in keys])
    auc_r, auc_g = MT.cal_error_auc(er, THRES), MT.cal_error_auc(eg, THRES)
    both = np.isfinite(er) & np.isfinite(eg)
    d = eg[both] - er[both]
    se = [float(np.std(_auc_terms(eg, t) - _auc_terms(er, t), ddof=1) / np.sqrt(len(er))) for t in THRES]
    print(f'HPatches-protocol outcome parity at 260 pairs, bf16_fp16 product vs the fp32 oracle fixture: failed pairs oracle {int((~np.isfinite(er)).sum())} / '
          f'product {int((~np.isfinite(eg)).sum())}; matches per pair {nr.mean():.0f} / {ng.mean():.0f}')
    print(f'  AUC@1/3/5/10 oracle  {np.round(auc_r, 5).tolist()}')
    print(f'  AUC@1/3/5/10 product {np.round(auc_g, 5).tolist()}')
    print(f'  dAUC                 {np.round(auc_g - auc_r, 5).tolist()}   paired standard error {np.round(se, 5).tolist()}')
    print(f'  corner-error difference over {int(both.sum())} pairs: mean {d.mean():+.2e} px (standard error {d.std(ddof=1) / np.sqrt(len(d)):.1e}), '
          f'mean |d| {np.abs(d).mean():.2e}, max |d| {np.abs(d).max():.2e}, pairs with |d| > 0.01 px: {int((np.abs(d) > 0.01).sum())}')
    assert int((~np.isfinite(er)).sum()) <= 2 and int((~np.isfinite(eg)).sum()) <= int((~np.isfinite(er)).sum()) + 1
    assert abs(auc_g[1] - auc_r[1]) <= GATE_AUC3, ('bf16_fp16', 'dAUC@3', float(auc_g[1] - auc_r[1]))
    assert np.abs(auc_g - auc_r).max() <= GATE_MAX, ('bf16_fp16', (auc_g - auc_r).tolist())
