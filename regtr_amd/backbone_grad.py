"""The differentiable InstanceNorm (+ LeakyReLU, + shortcut) and max-pool operators of the KPConv backbone: the plain forward's launches
with a HIP backward (csrc/norm_pool_bwd.hip), the counterpart of regtr_amd/kpconv_grad.py for the two operators between the convolutions.

    y = backbone_grad.instance_norm(x, seg_off, max_len, residual=r, residual_normed=True, lrelu=True)
        # bit-identical to ops.instnorm_apply(x, seg_off, max_len, ops.instnorm_stats(x, ...), r, ops.instnorm_stats(r, ...), lrelu=True)
    p = backbone_grad.max_pool(x, pool_inds)                 # bit-identical to ops.maxpool(x, pool_inds)
    loss(y, p).backward()                                    # x.grad, r.grad

instance_norm is the reference's BatchNormBlock with nn.InstanceNorm1d (per cloud, per channel, biased variance, no affine:
kpconv_blocks.py:489,510-519), the blocks' LeakyReLU(0.1) (:556-561) and the bottleneck's shortcut sum (:741), in the three forms the
blocks use: no shortcut, a plain one (y = act(norm(x) + r)) and a normalised one (y = act(norm(x) + norm(r))).  The gradient flows
through the statistics.  x, the shortcut and the (n_clouds, C, 2) statistics are saved, y is not: the backward recomputes the
activation's argument with the forward's own arithmetic, so every element's LeakyReLU side is the forward's.

max_pool is kpconv_blocks.py:127-143: the maximum over the rows a neighbour table lists, a zero shadow row for indices outside the
supports.  Like torch.max(dim), the whole gradient of an output element goes to ONE row -- on equal values the lowest column of the
table -- and none to the shadow row.  The forward stores that column per (query, channel) as int16 in the pass that takes the maximum
(ops.maxpool_fwd_argmax: ops.maxpool's and ops.maxpool_argmax's results from one gather of the rows; 2 bytes per output element
instead of recomputing the maximum once per table entry in backward); the backward walks the table by support (ops.nbr_transpose) and
adds, in ascending entry order, the gradients of the entries that won.

Both backward passes have one owner per output element, no atomics, and are bit-reproducible.  Nothing here synchronises.
Refused: CPU tensors, double backward."""
import torch
from torch.autograd.function import once_differentiable

from . import context, ops
from .transformer_grad import _rows


def _on_gpu(name, **tensors):
    for what, t in tensors.items():
        if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
            raise RuntimeError(f'{name}: {what} must be a GPU tensor (got {getattr(t, "device", type(t))}); there is no CPU fallback')


class _InstanceNorm(torch.autograd.Function):
    """(x, residual | None) -> y by the ops.instnorm_stats / ops.instnorm_apply calls of the plain path."""

    @staticmethod
    def forward(ctx, x, residual, seg_off, max_len, residual_normed, lrelu, slope, eps):
        stats = ops.instnorm_stats(x, seg_off, max_len, eps)
        res_stats = ops.instnorm_stats(residual, seg_off, max_len, eps) if residual_normed else None
        y = ops.instnorm_apply(x, seg_off, max_len, stats, residual, res_stats, lrelu=lrelu, slope=slope)
        ctx.save_for_backward(x, residual, seg_off, stats, res_stats)
        ctx.max_len, ctx.lrelu, ctx.slope = max_len, lrelu, slope
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, residual, seg_off, stats, res_stats = ctx.saved_tensors
        need_x, need_r = ctx.needs_input_grad[0], residual is not None and ctx.needs_input_grad[1]
        with context.ForwardContext(x.device):
            dx, dres = ops.instnorm_bwd(x, seg_off, ctx.max_len, stats, _rows(dy), residual, res_stats, ctx.lrelu, ctx.slope,
                                        want_dx=need_x, want_dres=need_r)
        return (dx, dres) + (None,) * 6


def instance_norm(x, seg_off, max_len, residual=None, residual_normed=False, lrelu=False, slope=0.1, eps=1e-5):
    """act(norm(x) [+ residual | + norm(residual)]) per cloud segment and channel, differentiable in x and residual.
    x (N, C) float32, C a multiple of 4 with C / 4 a power of two <= 256; seg_off (n_clouds + 1,) int32 on the device; max_len >= every
    cloud's length (a host int); residual (N, C) or None; residual_normed: the shortcut is normalised with its own statistics; lrelu:
    LeakyReLU(slope) on the sum.  The result is bit-identical to ops.instnorm_apply on ops.instnorm_stats (the same launches)."""
    _on_gpu('instance_norm', x=x, seg_off=seg_off, **({} if residual is None else {'residual': residual}))
    if residual is None and residual_normed:
        raise RuntimeError('instance_norm: residual_normed needs a residual')
    if residual is not None and residual.shape != x.shape:
        raise RuntimeError(f'instance_norm: residual must be {tuple(x.shape)} like x, got {tuple(residual.shape)}')
    return _InstanceNorm.apply(x, residual, seg_off, int(max_len), bool(residual_normed), bool(lrelu), float(slope), float(eps))


class _MaxPool(torch.autograd.Function):
    """x (Ns, C) -> (Nq, C), the bits of the plain path's ops.maxpool, and the winning columns from the same pass over the rows."""

    @staticmethod
    def forward(ctx, x, nbr, width, transposed):
        out, arg = ops.maxpool_fwd_argmax(x, nbr, width)
        ctx.save_for_backward(nbr, arg)
        ctx.ns, ctx.width, ctx.transposed = x.shape[0], width, transposed
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        nbr, arg = ctx.saved_tensors
        H = nbr.shape[1] if ctx.width is None else ctx.width
        with context.ForwardContext(dy.device):
            table = ctx.transposed
            if table is None:
                table = ops.nbr_transpose(nbr if H == nbr.shape[1] else nbr[:, :H].contiguous(), ctx.ns)
            dx = ops.maxpool_bwd(_rows(dy), arg, H, table)
        return dx, None, None, None


def max_pool(x, nbr, width=None, transposed=None):
    """max over the rows of x (Ns, C) that nbr (Nq, H) int32 lists (indices outside [0, Ns): a zero row), differentiable in x; bit-identical
    to ops.maxpool(x, nbr, width).  width: pool over the first `width` columns only.
    transposed: ops.nbr_transpose of the table pooled through, built earlier -- a block may share ONE table between its convolution
    (KPConv.forward_grad) and its pool.  That is legal exactly when both walk the same nbr with the same H and the same Ns: the table
    lists entries q H + h, so a pool over `width` < H columns, or a convolution over another table of the level, needs its own.  Without
    it the backward builds the table (with `width`, from the contiguous first `width` columns)."""
    _on_gpu('max_pool', x=x, nbr=nbr)
    if nbr.dtype is not torch.int32:
        raise NotImplementedError(f'max_pool: nbr must be int32 (the tables the preprocessor builds), got {nbr.dtype}')
    if width is not None and not 1 <= int(width) <= nbr.shape[1]:
        raise RuntimeError(f'max_pool: width must be in 1 ... {nbr.shape[1]}, got {width}')
    width = None if width is None else int(width)
    H = nbr.shape[1] if width is None else width
    if transposed is not None and (len(transposed) != 2 or transposed[0].numel() != x.shape[0] + 1 or transposed[1].numel() < nbr.shape[0] * H):
        raise RuntimeError('max_pool: `transposed` must be ops.nbr_transpose of the (Nq, H) table pooled through, over Ns supports')
    return _MaxPool.apply(x, nbr, width, transposed)
