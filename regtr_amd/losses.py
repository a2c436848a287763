"""Differentiable drop-ins for the reference's training losses: InfoNCELossFull (models/losses/feature_loss.py:246-314),
CircleLossFull (feature_loss.py:160-243, dist_type 'euclidean'; csrc/circle_loss.hip: regtr_circle_rows / regtr_circle_bwd),
CorrCriterion (models/losses/corr_loss.py:9-40) and OverlapCriterion (nn.BCEWithLogitsLoss, models/regtr.py:84,250-252), with the same
constructors, parameter names and forward signatures, so that

    model.feature_criterion = InfoNCELossFull(cfg.d_embed, cfg.r_p, cfg.r_n)
    model.feature_criterion_un = InfoNCELossFull(cfg.d_embed, cfg.r_p, cfg.r_n)
    model.corr_criterion = CorrCriterion(metric='mae')
    model.overlap_criterion = OverlapCriterion()

drop into the reference model's training step ("Training-loss drop-in").  Forward and backward run on the HIP kernels
of csrc/losses.hip (regtr_infonce_rows / regtr_infonce_bwd / regtr_gemm_tn, regtr_loss_terms / regtr_corr_l1_bwd), csrc/head_bwd.hip
(regtr_bce_logits_bwd) and the exact-f32 GEMM; torch only packs the per-pair lists and forms the scalar means.  Nothing here synchronises with the host.

Reference semantics are kept: a pair without an anchor inside r_p gives NaN (0 / 0), and its gradient contributions are exactly 0.
PoseCriterion is this project's own opt-in pose term (cfg.wt_pose), a few torch ops, not a reference loss.
Refused: metric='mse', overlap_weights=None, CircleLossFull's dist_type other than 'euclidean', coordinates / poses / weights that require grad, double backward, tensors off the GPU.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import context, ops

_EPS = 1e-6     # corr_loss.py:6


def _on_gpu(name, ts):
    for t in ts:
        if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
            raise RuntimeError(f'{name}: every tensor must be on the GPU (got {getattr(t, "device", type(t))})')


def _no_grad_inputs(name, ts):
    if any(t.requires_grad for t in ts):
        raise RuntimeError(f'{name}: coordinates, poses and weights take no gradient here (only features, W and the warped points do)')


def _offsets(lens, dev):
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    return torch.tensor(off, dtype=torch.int32).to(dev, non_blocking=True)


class _InfoNCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, G, W, ax, px, a_off, p_off, max_anc, max_pos, r_p, r_n):
        with context.forward(A.device, f16_pair=False, status=None):
            Wt = torch.triu(W)
            w_sym = (Wt + Wt.t()).contiguous()                                        # feature_loss.py:295-296
            P = ops.gemm(G, w_sym)                                                    # P' = G W_sym, exact-f32 MFMA
            saved = ops.infonce_rows(A, P, ax, px, a_off, p_off, max_anc, r_p, r_n)
        out = saved[0]
        ctx.save_for_backward(A, G, P, w_sym, ax, px, a_off, p_off, *saved)
        ctx.meta = (max_anc, max_pos, r_n, out.shape[0])
        return (out[:, 0] / out[:, 1]).mean()                                         # feature_loss.py:312-314

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        A, G, P, w_sym, ax, px, a_off, p_off, *saved = ctx.saved_tensors
        max_anc, max_pos, r_n, B = ctx.meta
        g = g.detach().to(torch.float32).contiguous()
        with context.forward(A.device, f16_pair=False, status=None):
            dA, dP = ops.infonce_bwd(A, P, ax, px, a_off, p_off, max_anc, max_pos, r_n, saved, g, float(B))
            dG = ops.gemm(dP, w_sym) if ctx.needs_input_grad[1] else None            # W_sym is symmetric
            dW = ops.gemm_tn(G, dP, fold=True) if ctx.needs_input_grad[2] else None   # G^T dP', folded onto triu(W)
        return dA, dG, dW, None, None, None, None, None, None, None, None


class InfoNCELossFull(nn.Module):
    """feature_loss.py:246-314 on the HIP kernels.  Parameter `W` (d_embed x d_embed, N(0, 0.1) init) and `n_sample` as the reference,
    so state_dict keys match.  forward(src_feat, tgt_feat, src_xyz, tgt_xyz): lists of per-pair (N, D) float32 features and (N, 3)
    coordinates on the GPU (src_xyz already in the target frame, as RegTR.compute_loss passes them) -> the mean over pairs of the
    masked mean InfoNCE loss.  Gradients go to the features and to W."""

    def __init__(self, d_embed, r_p, r_n):
        super().__init__()
        self.r_p = r_p
        self.r_n = r_n
        self.n_sample = 256
        self.W = nn.Parameter(torch.zeros(d_embed, d_embed), requires_grad=True)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.normal_(self.W, std=0.1)

    def forward(self, src_feat, tgt_feat, src_xyz, tgt_xyz):
        B = len(src_feat)
        if B == 0 or not (len(tgt_feat) == len(src_xyz) == len(tgt_xyz) == B):
            raise RuntimeError(f'InfoNCELossFull: need the same number (>= 1) of src / tgt features and coordinates, got '
                               f'{len(src_feat)}, {len(tgt_feat)}, {len(src_xyz)}, {len(tgt_xyz)}')
        _no_grad_inputs('InfoNCELossFull', [*src_xyz, *tgt_xyz])
        _on_gpu('InfoNCELossFull', [self.W, *src_feat, *tgt_feat, *src_xyz, *tgt_xyz])
        if any(f.dtype != torch.float32 for f in [self.W, *src_feat, *tgt_feat, *src_xyz, *tgt_xyz]):
            raise RuntimeError('InfoNCELossFull: float32 features, coordinates and W only')
        n_src = [int(f.shape[0]) for f in src_feat]
        n_tgt = [int(f.shape[0]) for f in tgt_feat]
        if min(n_src) < 1 or min(n_tgt) < 1:
            raise RuntimeError('InfoNCELossFull: every cloud needs at least one point (the reference\'s topk needs one too)')
        dev = src_feat[0].device
        A = torch.cat(list(src_feat)).contiguous()
        G = torch.cat(list(tgt_feat)).contiguous()
        ax = torch.cat(list(src_xyz)).contiguous()
        px = torch.cat(list(tgt_xyz)).contiguous()
        return _InfoNCE.apply(A, G, self.W, ax, px, _offsets(n_src, dev), _offsets(n_tgt, dev), max(n_src), max(n_tgt),
                              float(self.r_p), float(self.r_n))


class _Circle(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, G, ax, px, a_off, p_off, max_anc, max_pos, r_p, r_n, params):
        with context.forward(A.device, f16_pair=False, status=None):
            saved = ops.circle_rows(A, G, ax, px, a_off, p_off, max_anc, max_pos, r_p, r_n, params)
        out = saved[0]
        ctx.save_for_backward(A, G, ax, px, a_off, p_off, *saved)
        ctx.meta = (max_anc, max_pos, r_p, r_n, params, out.shape[0])
        return ((out[:, 0] / out[:, 1] + out[:, 2] / out[:, 3]) / 2).mean()           # feature_loss.py:229, 243

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        A, G, ax, px, a_off, p_off, *saved = ctx.saved_tensors
        max_anc, max_pos, r_p, r_n, params, B = ctx.meta
        g = g.detach().to(torch.float32).contiguous()
        with context.forward(A.device, f16_pair=False, status=None):
            dA, dG = ops.circle_bwd(A, G, ax, px, a_off, p_off, max_anc, max_pos, r_p, r_n, saved, g, float(B), params)
        return dA, dG, None, None, None, None, None, None, None, None, None


class CircleLossFull(nn.Module):
    """feature_loss.py:160-243 on the HIP kernels of csrc/circle_loss.hip, with the reference's constructor and attributes and, like it,
    no parameters (an empty state_dict).  forward(anchor_feat, positive_feat, anchor_xyz, positive_xyz): lists of per-pair (N, D) float32
    features and (N, 3) coordinates on the GPU (anchor_xyz already in the positives' frame) -> the mean over pairs of
    (mean of the selected row losses + mean of the selected column losses) / 2.  Gradients go to the features.  dist_type: only
    'euclidean', what the reference model constructs; any other is refused when called.  A pair without a selected row or column gives NaN,
    as the reference's mean of nothing, and contributes exactly zero gradient (the reference's autograd would still pass the gradient of
    the half that is not empty).  log_scale, the margins and the radii are read at every call."""

    def __init__(self, dist_type='cosine', log_scale=10, r_p=0.125, r_n=0.25, pos_margin=0.1, neg_margin=1.4):
        super().__init__()
        self.log_scale = log_scale
        self.pos_margin = pos_margin
        self.neg_margin = neg_margin
        self.pos_optimal = pos_margin
        self.neg_optimal = neg_margin
        self.dist_type = dist_type
        self.r_p = r_p
        self.r_n = r_n

    def params(self):
        """The kernels' scalar arguments, from the attributes as they are now."""
        return dict(log_scale=float(self.log_scale), pos_margin=float(self.pos_margin), pos_optimal=float(self.pos_optimal),
                    neg_margin=float(self.neg_margin), neg_optimal=float(self.neg_optimal))

    def forward(self, anchor_feat, positive_feat, anchor_xyz, positive_xyz):
        if self.dist_type != 'euclidean':
            raise NotImplementedError(f"CircleLossFull: dist_type {self.dist_type!r} is not implemented (only 'euclidean', what RegTR uses)")
        B = len(anchor_feat)
        if B == 0 or not (len(positive_feat) == len(anchor_xyz) == len(positive_xyz) == B):
            raise RuntimeError(f'CircleLossFull: need the same number (>= 1) of anchor / positive features and coordinates, got '
                               f'{len(anchor_feat)}, {len(positive_feat)}, {len(anchor_xyz)}, {len(positive_xyz)}')
        _no_grad_inputs('CircleLossFull', [*anchor_xyz, *positive_xyz])
        _on_gpu('CircleLossFull', [*anchor_feat, *positive_feat, *anchor_xyz, *positive_xyz])
        if any(f.dtype != torch.float32 for f in [*anchor_feat, *positive_feat, *anchor_xyz, *positive_xyz]):
            raise RuntimeError('CircleLossFull: float32 features and coordinates only')
        n_anc = [int(f.shape[0]) for f in anchor_feat]
        n_pos = [int(f.shape[0]) for f in positive_feat]
        if min(n_anc) < 1 or min(n_pos) < 1:
            raise RuntimeError('CircleLossFull: every cloud needs at least one point')
        if [int(x.shape[0]) for x in anchor_xyz] != n_anc or [int(x.shape[0]) for x in positive_xyz] != n_pos:
            raise RuntimeError('CircleLossFull: one coordinate per feature row (feature_loss.py:235-236)')
        dev = anchor_feat[0].device
        A = torch.cat(list(anchor_feat)).contiguous()
        G = torch.cat(list(positive_feat)).contiguous()
        ax = torch.cat(list(anchor_xyz)).contiguous()
        px = torch.cat(list(positive_xyz)).contiguous()
        return _Circle.apply(A, G, ax, px, _offsets(n_anc, dev), _offsets(n_pos, dev), max(n_anc), max(n_pos), float(self.r_p),
                             float(self.r_n), self.params())


class _CorrL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, warped, kp, w, seg, seg2, pose):
        with context.forward(warped.device, f16_pair=False, status=None):
            terms = ops.loss_terms(w, w, kp, warped, seg2, pose)                      # (B, 5): columns 1, 2 = sum w |e|_1, sum w
        den = terms[:, 2].sum().clamp_min(_EPS)
        ctx.save_for_backward(kp, warped, w, seg, pose, den)
        return terms[:, 1].sum() / den

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        kp, warped, w, seg, pose, den = ctx.saved_tensors
        g = g.detach().to(torch.float32).contiguous()
        with context.forward(kp.device, f16_pair=False, status=None):
            d = ops.corr_l1_bwd(kp, warped, w, seg, pose, g, den)
        return d, None, None, None, None, None


class CorrCriterion(nn.Module):
    """corr_loss.py:9-40 with metric 'mae' on the HIP kernels.  forward(kp_before, kp_warped_pred, pose_gt, overlap_weights): lists of
    per-pair (N, 3) points and (N,) weights, pose_gt (B, 3, 4) or (B, 4, 4) -> sum w |warped - T kp|_1 / max(sum w, 1e-6) over all
    pairs.  Gradients go to kp_warped_pred."""

    def __init__(self, metric='mae'):
        super().__init__()
        if metric != 'mae':
            raise NotImplementedError(f"CorrCriterion: metric {metric!r} is not implemented (only 'mae', what RegTR uses)")
        self.metric = metric

    def forward(self, kp_before, kp_warped_pred, pose_gt, overlap_weights=None):
        if overlap_weights is None:
            raise NotImplementedError('CorrCriterion: overlap_weights=None (the per-point mean of corr_loss.py:37) is not implemented')
        B = int(pose_gt.shape[0])
        if not (len(kp_before) == len(kp_warped_pred) == len(overlap_weights) == B) or B == 0:
            raise RuntimeError(f'CorrCriterion: need one key-point set, warped set and weight vector per pose, got {len(kp_before)}, '
                               f'{len(kp_warped_pred)}, {len(overlap_weights)} for {B} poses')
        _no_grad_inputs('CorrCriterion', [pose_gt, *kp_before, *overlap_weights])
        _on_gpu('CorrCriterion', [pose_gt, *kp_before, *kp_warped_pred, *overlap_weights])
        if any(t.dtype != torch.float32 for t in [pose_gt, *kp_before, *kp_warped_pred, *overlap_weights]):
            raise RuntimeError('CorrCriterion: float32 points, weights and poses only')
        if pose_gt.dim() != 3 or tuple(pose_gt.shape[1:]) not in ((3, 4), (4, 4)):
            raise RuntimeError(f'CorrCriterion: pose_gt must be (B, 3, 4) or (B, 4, 4), got {tuple(pose_gt.shape)}')
        lens = [int(k.shape[0]) for k in kp_before]
        dev = pose_gt.device
        seg2 = _offsets(lens + [0] * B, dev)          # regtr_loss_terms' (src clouds, tgt clouds) layout with empty tgt clouds
        seg = seg2[:B + 1]
        kp = torch.cat(list(kp_before)).contiguous()
        warped = torch.cat(list(kp_warped_pred)).contiguous()
        w = torch.cat([x.reshape(-1) for x in overlap_weights]).contiguous()
        return _CorrL1.apply(warped, kp, w, seg, seg2, pose_gt.contiguous())


class _OverlapBCE(torch.autograd.Function):
    """mean_i BCEWithLogits(logit_i, gt_i): the BCE sums of regtr_loss_terms (per pair, float64 inside), added and divided as
    RegTR.compute_loss does -- the same bits on the same tensors.  kp, warped, pose only feed that kernel's other columns."""

    @staticmethod
    def forward(ctx, logit, gt, seg2, kp, warped, pose):
        with context.forward(logit.device, f16_pair=False, status=None):
            terms = ops.loss_terms(logit, gt, kp, warped, seg2, pose)
        ctx.save_for_backward(logit, gt)
        return terms[:, 0].sum() / logit.shape[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        logit, gt = ctx.saved_tensors
        g = g.detach().to(torch.float32).contiguous()
        with context.forward(logit.device, f16_pair=False, status=None):
            d = ops.bce_logits_bwd(logit, gt, g)
        return d, None, None, None, None, None


def overlap_bce(logit, gt, seg2, kp, warped, pose):
    """_OverlapBCE on the tensors RegTR.compute_loss hands regtr_loss_terms (seg2 (2B+1,): src clouds, then tgt clouds)."""
    return _OverlapBCE.apply(logit, gt, seg2, kp, warped, pose)


class OverlapCriterion(nn.Module):
    """nn.BCEWithLogitsLoss() (mean reduction, no weights) on packed (N,) logits and float targets in [0, 1], forward and backward on
    the HIP kernels.  forward(logit, target, seg_off=None): seg_off (2B+1,) int32 on the GPU, the (src clouds, tgt clouds) offsets of a
    pair batch -- the sum is then taken pair by pair as RegTR.compute_loss takes it (bit-equal to its overlap term); None: one sum over
    all points.  Gradients go to logit."""

    def forward(self, logit, target, seg_off=None):
        _on_gpu('OverlapCriterion', [logit, target] + ([] if seg_off is None else [seg_off]))
        _no_grad_inputs('OverlapCriterion', [target])
        if logit.dtype != torch.float32 or target.dtype != torch.float32:
            raise RuntimeError('OverlapCriterion: float32 logits and targets only')
        if logit.dim() != 1 or target.shape != logit.shape or logit.shape[0] < 1:
            raise RuntimeError(f'OverlapCriterion: logit and target must be (N,) with N >= 1, got {tuple(logit.shape)}, {tuple(target.shape)}')
        n, dev = logit.shape[0], logit.device
        if seg_off is None:
            seg_off = torch.tensor([0, n, n], dtype=torch.int32).to(dev, non_blocking=True)
        B = seg_off.numel() // 2
        zeros = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        pose = torch.eye(3, 4, dtype=torch.float32, device=dev).expand(B, 3, 4).contiguous()
        return _OverlapBCE.apply(logit.contiguous(), target.contiguous(), seg_off, zeros, zeros, pose)


class PoseCriterion(nn.Module):
    """mean over pairs of ||R_pred - R_gt||_F^2 + ||t_pred - t_gt||^2: the opt-in pose term of RegTR.compute_loss / compute_loss_grad
    (cfg.wt_pose > 0).  NOT a loss of the reference (its RegTR.compute_loss never reads pred['pose']): the simplest supervision of the
    pose that regtr_weighted_procrustes_bwd makes trainable.  A few plain torch ops on (B, 3, 4) tensors, no kernel.
    forward(pose_pred (B, 3, 4), pose_gt (B, 3, 4) or (B, 4, 4), per_pair=False) -> 0-dim, or (B,) with per_pair=True.  Gradients go to
    pose_pred."""

    def forward(self, pose_pred, pose_gt, per_pair=False):
        _on_gpu('PoseCriterion', [pose_pred, pose_gt])
        _no_grad_inputs('PoseCriterion', [pose_gt])
        if pose_pred.dim() != 3 or tuple(pose_pred.shape[1:]) != (3, 4) or pose_gt.dim() != 3 or pose_gt.shape[0] != pose_pred.shape[0] or \
                tuple(pose_gt.shape[1:]) not in ((3, 4), (4, 4)):
            raise RuntimeError(f'PoseCriterion: pose_pred (B, 3, 4) and pose_gt (B, 3, 4) or (B, 4, 4) expected, got {tuple(pose_pred.shape)}, '
                               f'{tuple(pose_gt.shape)}')
        per = ((pose_pred.as_subclass(torch.Tensor) - pose_gt[:, :3, :].to(torch.float32)) ** 2).sum(dim=(1, 2))
        return per if per_pair else per.mean()
