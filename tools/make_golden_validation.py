"""Generates tests/golden/validation_metrics.npz from the REAL reference functions (development machine only: needs the reference tree,
imported through oracle.ref_loader): utils/se3_torch.se3_compare on seeded (L = 2, B = 5) poses of two validation steps -- what
GenericRegModel._compute_metrics returns per step -- and GenericRegModel._aggregate_metrics over the two steps, with pairs on either
side of both success thresholds.  tests/test_metrics_host.py pins tests/metrics_ref.py to it.

    python tools/make_golden_validation.py
"""
import logging
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THRESH_ROT, THRESH_TRANS = 10.0, 0.1
L, B = 2, 5


def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def _pose(R, t):
    return np.concatenate([R, np.asarray(t, np.float64).reshape(3, 1)], 1)


def make_step(rng, errors):
    """errors: per layer a list (B) of (rotation error in degrees, translation error norm) -> gt (B, 3, 4), pred (L, B, 3, 4) float32."""
    gt = np.stack([_pose(_rot(rng.standard_normal(3), rng.uniform(0, 45)), rng.uniform(-0.5, 0.5, 3)) for _ in range(B)])
    pred = np.empty((L, B, 3, 4))
    for l in range(L):
        for b in range(B):
            r_deg, t_len = errors[l][b]
            d = rng.standard_normal(3)
            E = _pose(_rot(rng.standard_normal(3), r_deg), t_len * d / np.linalg.norm(d))      # pred = E o gt
            pred[l, b] = np.concatenate([E[:, :3] @ gt[b][:, :3], E[:, :3] @ gt[b][:, 3:] + E[:, 3:]], 1)
    return gt.astype(np.float32), pred.astype(np.float32)


def main():
    from oracle import ref_loader
    ref = ref_loader.load()
    with ref_loader.chdir(ref_loader.REF_SRC):
        import models.generic_reg_model as grm
    rng = np.random.default_rng(20240917)
    # (rotation error, translation error): either side of 10 degrees and of 0.1, and one pair with each single failure
    steps = [make_step(rng, [[(2.0, 0.02), (9.5, 0.09), (10.5, 0.05), (3.0, 0.105), (25.0, 0.4)],
                             [(1.0, 0.01), (9.9, 0.099), (10.1, 0.02), (0.5, 0.11), (179.0, 0.3)]]),
             make_step(rng, [[(0.3, 0.004), (12.0, 0.2), (9.0, 0.095), (45.0, 0.03), (5.0, 0.15)],
                             [(0.1, 0.001), (11.0, 0.12), (8.0, 0.08), (90.0, 0.05), (4.0, 0.2)]])]
    out = {'thresh_rot': THRESH_ROT, 'thresh_trans': THRESH_TRANS, 'n_steps': len(steps)}
    per_step = []
    for s, (gt, pred) in enumerate(steps):
        err = ref.se3_torch.se3_compare(torch.from_numpy(pred), torch.from_numpy(gt)[None, :])      # _compute_metrics, :205
        m = {'rot_err_deg': err['rot_deg'], 'trans_err': err['trans']}
        per_step.append(m)
        out[f'gt_{s}'], out[f'pred_{s}'] = gt, pred
        out[f'rot_err_deg_{s}'], out[f'trans_err_{s}'] = m['rot_err_deg'].numpy(), m['trans_err'].numpy()
    self = types.SimpleNamespace(logger=logging.getLogger('golden'), reg_success_thresh_rot=THRESH_ROT, reg_success_thresh_trans=THRESH_TRANS)
    agg = grm.GenericRegModel._aggregate_metrics(self, per_step)
    for k, v in agg.items():
        out['agg_' + k] = v.numpy()
    out['agg_keys'] = np.array(sorted(agg))
    path = os.path.join(ROOT, 'tests', 'golden', 'validation_metrics.npz')
    np.savez(path, **out)
    print(path, {k: np.asarray(v).shape for k, v in out.items()})
    print({k: v.numpy() for k, v in agg.items() if not k.endswith('hist')})


if __name__ == '__main__':
    main()
