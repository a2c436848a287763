"""compute_rigid_transform drop-in (/root/reference/src/utils/se3_torch.py:108-154) on the fused Procrustes kernel, differentiable in
a, b and weights like the reference's (whose gradient comes from autograd through ~20 torch ops and torch.svd): the backward is
regtr_weighted_procrustes_bwd, the closed form of csrc/procrustes.hip."""
import torch
from torch.autograd.function import once_differentiable

from . import context, ops


class _RigidTransform(torch.autograd.Function):
    """(a (P N, 3), b (1, P N, 3), w (P, N), seg) -> pose (1, P, 3, 4): P pure-source pairs of one layer.  Backward: d_kp is a's gradient,
    d_corr b's, d_weight w's -- the gradient with respect to the weight itself, finite at weights of exactly 0 and 1, where the logit
    the kernel reads is infinite."""

    @staticmethod
    def forward(ctx, a, b, w, seg, P):
        logit = (torch.log(w) - torch.log1p(-w)).view(1, -1).contiguous()
        ctx.save_for_backward(a, b, logit, seg)
        ctx.P, ctx.w_shape = P, w.shape
        return ops.weighted_procrustes(a, b, logit, seg, P)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_pose):
        a, b, logit, seg = ctx.saved_tensors
        need = ctx.needs_input_grad
        with context.ForwardContext(a.device):
            d_b, _, d_a, d_w = ops.weighted_procrustes_bwd(a, b, logit, seg, ctx.P, d_pose.detach().to(torch.float32).contiguous(),
                                                           want_logit=False, want_kp=need[0], want_weight=need[2])
        return (d_a[0] if need[0] else None, d_b if need[1] else None, d_w.view(ctx.w_shape) if need[2] else None, None, None)


def compute_rigid_transform(a: torch.Tensor, b: torch.Tensor, weights: torch.Tensor = None):
    """a, b ([*,] N, 3), weights ([*,] N) in [0, 1] -> ([*,] 3, 4) with T a = b (weighted Kabsch).

    The kernel consumes the model's native layout (key points, predicted coordinates, overlap LOGITS); this generic
    entry point re-expresses its arguments in that layout: a is passed as the 'key points' of a pure-source pair,
    b as its predicted coordinates, and logit = log(w / (1 - w)).
    Differentiable in a, b and weights (once; GPU tensors).  A batch entry whose transform is no differentiable function of its inputs
    (coincident or collinear points, a weight sum below 1e-6: docs/PARITY.md) gets zero gradients where the reference returns inf / NaN."""
    assert a.shape == b.shape and a.shape[-1] == 3
    if a.device.type != 'cuda' or b.device != a.device or (weights is not None and weights.device != a.device):
        raise RuntimeError(f'compute_rigid_transform: a, b and weights must be on one GPU (got {a.device}, {b.device}); there is no CPU fallback')
    batch_shape = a.shape[:-2]
    N = a.shape[-2]
    a2 = a.reshape(-1, N, 3).to(torch.float32).contiguous()
    b2 = b.reshape(-1, N, 3).to(torch.float32).contiguous()
    P = a2.shape[0]
    if weights is None:
        w = torch.full((P, N), 0.5, dtype=torch.float32, device=a.device)
    else:
        assert a.shape[:-1] == weights.shape
        w = weights.reshape(P, N).to(torch.float32)
    # P independent "pairs", each with N source rows and 0 target rows, one "layer"
    seg = torch.cat([torch.arange(P + 1, dtype=torch.int32) * N,
                     torch.full((P,), P * N, dtype=torch.int32)]).to(a.device)
    pose = _RigidTransform.apply(a2.view(P * N, 3), b2.view(1, P * N, 3), w, seg, P)
    return pose[0].reshape(*batch_shape, 3, 4)
