"""The validation step of the depth-supervised configuration: lightning/lightning_depth_geoformer.py `_compute_metrics`,
`validation_step` and `validation_epoch_end` without Lightning.  An eval-mode forward under no_grad, then the two device metric
calls of train/metrics.py; no per-pair host trip (one download of the batch's poses at the end)."""
import numpy as np
import torch

from .metrics import aggregate_metrics, compute_pose_errors, compute_symmetrical_epipolar_errors
from .trainer import DEFAULT_TRAINER_CFG


class ValidationStep:
    """`step(batch)` -> {'metrics': {identifiers, epi_errs (one array per pair), R_errs, t_errs, inliers}}, the dict the reference's
    `validation_step` returns under 'metrics'; `aggregate(outputs)` -> auc@5/10/20 and prec@<epi_err_thr> over everything collected
    (duplicates by identifier dropped)."""

    def __init__(self, model, trainer_cfg=None):
        self.model = model
        self.cfg = dict(DEFAULT_TRAINER_CFG, **(trainer_cfg or {}))

    @torch.no_grad()
    def __call__(self, batch):
        was_training = self.model.training
        self.model.eval()
        try:
            self.model(batch)
        finally:
            self.model.train(was_training)
        compute_symmetrical_epipolar_errors(batch)
        compute_pose_errors(batch, self.cfg)
        names = batch['pair_names']
        rel_pair_names = list(zip(*names)) if names and isinstance(names[0], (list, tuple)) else [(n, i) for i, n in enumerate(names)]
        bs = batch['image0'].size(0)
        packed = torch.stack([batch['m_bids'].float(), batch['epi_errs']]).cpu().numpy()         # one download
        bids, epi = packed[0].astype(np.int64), packed[1]
        metrics = {'identifiers': ['#'.join(str(x) for x in rel_pair_names[b]) for b in range(bs)],
                   'epi_errs': [epi[bids == b] for b in range(bs)],
                   'R_errs': batch['R_errs'], 't_errs': batch['t_errs'], 'inliers': batch['inliers']}
        return {'metrics': metrics}

    def aggregate(self, outputs):
        keys = ('identifiers', 'epi_errs', 'R_errs', 't_errs', 'inliers')
        merged = {k: [x for o in outputs for x in o['metrics'][k]] for k in keys}
        return aggregate_metrics(merged, self.cfg['epi_err_thr'])
