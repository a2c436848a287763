"""Validation and test metrics on the device (csrc/metrics.hip): the registration errors the reference's trainer validates on
(models/generic_reg_model.py:197-250: se3_compare per decoder layer, _aggregate_metrics, reg_success_final) and the RPMNet / DCP metrics
of its ModelNet test (benchmark/benchmark_modelnet.py:33-105), the modified Chamfer distance included.  The host counterparts are
regtr_amd.evaluation.modelnet_metrics / summarize_metrics (scipy KD-trees, one pair at a time).

Nothing here waits for the device: every function enqueues launches on the current stream and returns device tensors.
"""
import torch

from . import _lib, ops

MODELNET_KEYS = ('r_mse', 'r_mae', 't_mse', 't_mae', 'err_r_deg', 'err_t', 'chamfer_dist')
_POSE_COLUMNS = {'rot_err_deg': 0, 'trans_err': 1, 'err_r_deg': 2, 'err_t': 3, 't_mse': 4, 't_mae': 5, 'r_mse': 6, 'r_mae': 7}


def _poses(p, what):
    if isinstance(p, (list, tuple)):
        p = torch.stack(list(p))
    if not isinstance(p, torch.Tensor) or p.device.type != 'cuda':
        raise RuntimeError(f'{what} must be a GPU tensor; there is no CPU fallback')
    return p.to(torch.float32).contiguous()


def pose_errors(pred, gt):
    """pred (L, B, 3, 4) or (B, 3, 4), gt (B, 3, 4) or (B, 4, 4) -> ({name: float64 tensor of pred's leading shape} for rot_err_deg,
    trans_err, err_r_deg, err_t, t_mse, t_mae, r_mse, r_mae; composed = pred o gt^-1 in float32).  `trans_err` is se3_compare's
    || t_p - R_p R_g^T t_g ||, not harness.pose_errors' || t_p - t_g || (docs/PARITY.md)."""
    with _lib.on_device(pred.device):
        out, comp = ops.pose_metrics(_poses(pred, 'pose_errors: pred'), _poses(gt, 'pose_errors: gt'))
    return {k: out[..., c] for k, c in _POSE_COLUMNS.items()}, comp


def chamfer(src, ref, raw, pred, gt):
    """The reference's modified Chamfer distance (benchmark_modelnet.py:69-76) of B pairs:
        mean_i min_j |pred src_i - raw_j|^2 + mean_i min_j |ref_i - (pred o gt^-1) raw_j|^2
    src, ref, raw: lists (B) of device float32 (n, 3) clouds of any lengths; pred, gt (B, 3, 4) or (B, 4, 4) -> (B,) float32.
    One regtr_nearest launch over 2B query clouds (the B source clouds under pred against the raw clouds, the B reference clouds against
    the raw clouds under pred o gt^-1) and one regtr_segment_mean; distances in float32 as the reference's, means in float64."""
    B = len(src)
    if not (len(ref) == len(raw) == B) or B == 0:
        raise RuntimeError(f'chamfer: src, ref and raw must be non-empty lists of one length, got {len(src)}, {len(ref)}, {len(raw)}')
    pred, gt = _poses(pred, 'chamfer: pred'), _poses(gt, 'chamfer: gt')
    with _lib.on_device(pred.device):
        _, comp = ops.pose_metrics(pred[:, :3, :], gt)
        return _chamfer(list(src), list(ref), list(raw), pred[:, :3, :], comp)


def _chamfer(src, ref, raw, pred34, comp34):
    B = len(src)
    dev = pred34.device
    queries = src + ref
    q_off, s_off = [0], [0]
    for c in queries:
        q_off.append(q_off[-1] + int(c.shape[0]))
    for c in raw + raw:
        s_off.append(s_off[-1] + int(c.shape[0]))
    q_xyz = torch.cat([c[:, :3] for c in queries])
    s_one = torch.cat([c[:, :3] for c in raw])
    s_xyz = torch.cat([s_one, s_one])                      # query cloud c searches support cloud c: the raw clouds once per direction
    eye = torch.eye(3, 4, dtype=torch.float32, device=dev).expand(B, 3, 4)       # (1 x + 0 y) + 0 z + 0 = x exactly
    q_pose = torch.cat([pred34, eye])
    s_pose = torch.cat([eye, comp34])
    d2, _, offs = ops.nearest(q_xyz, q_off, s_xyz, s_off, q_pose=q_pose, s_pose=s_pose, return_idx=False, return_offsets=True)
    m = ops.segment_mean(d2, offs[0])                      # (the offsets go up once, for both launches)
    return (m[:B] + m[B:]).to(torch.float32)


def modelnet_metrics(pred_pose, batch):
    """benchmark_modelnet.compute_metrics on the device: pred_pose (B, 3, 4), batch with 'src_xyz', 'tgt_xyz', 'tgt_raw' (lists (B) of
    device clouds) and 'pose' (B, 3, 4) or (B, 4, 4) -> {'r_mse', 'r_mae', 't_mse', 't_mae', 'err_r_deg', 'err_t' (float64),
    'chamfer_dist' (float32)}, each (B,) on the device.  With augment.modelnet_train_batch(points, ...) pass tgt_raw=points: the chain
    leaves the reference cloud in the raw frame.  KeyError names a missing key.  Euler angles at gimbal lock do not follow scipy."""
    for k in ('src_xyz', 'tgt_xyz', 'tgt_raw', 'pose'):
        if k not in batch:
            raise KeyError(f"modelnet_metrics: batch[{k!r}] is missing" + (' (the clean cloud of every pair; with modelnet_train_batch(points, ...) '
                                                                             'pass tgt_raw=points)' if k == 'tgt_raw' else ''))
    pred, gt = _poses(pred_pose, 'modelnet_metrics: pred_pose'), _poses(batch['pose'], "modelnet_metrics: batch['pose']")
    with _lib.on_device(pred.device):
        out, comp = ops.pose_metrics(pred[:, :3, :], gt)
        m = {k: out[:, _POSE_COLUMNS[k]] for k in MODELNET_KEYS[:-1]}
        m['chamfer_dist'] = _chamfer(list(batch['src_xyz']), list(batch['tgt_xyz']), list(batch['tgt_raw']), pred[:, :3, :], comp)
    return m


def summarize(metrics):
    """benchmark_modelnet.summarize_metrics (:93-105) on device tensors (evaluation.summarize_metrics' counterpart) -> 0-dim float64
    device tensors."""
    out = {}
    for k, v in metrics.items():
        v = v.to(torch.float64)
        if k.endswith('mse'):
            out[k[:-3] + 'rmse'] = v.mean().sqrt()
        elif k.startswith('err'):
            out[k + '_mean'] = v.mean()
            out[k + '_rmse'] = (v * v).mean().sqrt()
        else:
            out[k] = v.mean()
    return out


def aggregate(step_metrics, thresh_rot, thresh_trans):
    """The reference's _aggregate_metrics (generic_reg_model.py:211-250) without corr_err: step_metrics a list of per-step dicts of
    (L, B_step) tensors -> for every layer p (suffix '{p}', 'final' for the last) rot_err_deg_{s} / trans_err_{s} (means),
    rot_err_{s}_hist / trans_err_{s}_hist (the values; the reference's key has no `_deg` there) and reg_success_{s} (the share of
    pairs under both thresholds, strictly).  Device tensors; no host wait."""
    if not step_metrics or len(step_metrics[0]) == 0:
        return {}
    cat = {k: torch.cat([m[k] for m in step_metrics], dim=1) for k in step_metrics[0]}
    n = next(iter(cat.values())).shape[1]
    if any(v.shape[1] != n for v in cat.values()):
        raise RuntimeError('aggregate: the metrics disagree on the number of instances (dimension 1 is the batch)')
    rot_keys = [k for k in cat if k.startswith('rot_err_deg')]
    out = {}
    if not rot_keys:
        return out
    num_pred = cat[rot_keys[0]].shape[0]
    for p in range(num_pred):
        s = f'{p}' if p < num_pred - 1 else 'final'
        for rk in rot_keys:
            kind = rk[11:]
            tk = 'trans_err' + kind
            out[f'rot_err_deg{kind}_{s}'] = cat[rk][p].mean()
            out[f'rot_err{kind}_{s}_hist'] = cat[rk][p]
            out[f'{tk}_{s}'] = cat[tk][p].mean()
            out[f'{tk}_{s}_hist'] = cat[tk][p]
            ok = torch.logical_and(cat[rk][p] < thresh_rot, cat[tk][p] < thresh_trans)
            out[f'reg_success{kind}_{s}'] = ok.float().mean()
    return out
