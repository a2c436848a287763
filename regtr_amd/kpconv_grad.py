"""The differentiable KPConv operator: KPConv.forward_grad (regtr_amd/kpconv.py) -- the plain forward's launches with a HIP backward.

    conv.load_state_dict(reference_kpconv.state_dict())
    out = conv.forward_grad(q_pts, s_pts, neighb_inds, x)          # bit-identical to conv(q_pts, s_pts, neighb_inds, x)
    loss(out).backward()                                           # conv.weights.grad and x.grad

Rigid KPConv, linear influence, sum aggregation (kpconv_blocks.py:269-414 of the reference).  The forward is a gather
wf[q, k Cin + c] = sum_h infl[q, h, k] x[nbr[q, h], c] followed by out = (wf W) / num[q]; with g = dOut / num (ops.row_div):
    dW  = wf^T g       ops.gemm_tn where both widths are multiples of 64, else ops.gemm_tn_any (KP Cin = 480, Cout = 32, the 15-wide wf
                       of the first block); viewed as the parameter's (KP, Cin, Cout)
    dWF = g W^T        ops.gemm on a transposed SplitWeight of the same parameter (cached per parameter version), always in the bf16x3
                       split -- gradients are routinely far below f16's normal range (regtr_amd/transformer_grad.py)
    dX  = the scatter of infl x dWF over the neighbour table, by support-row owners walking the TRANSPOSED table (ops.nbr_transpose,
          ops.kpconv_gather_bwd): no atomics, bit-reproducible.
num is an integer count (kpconv_blocks.py:409-411) and carries no gradient; kernel_points has requires_grad=False; the coordinates
receive none.  Influences are recomputed from the coordinates, never stored.

wf is RECOMPUTED in backward (ops.kpconv_wf: the forward's own gather launch, which also returns num), not saved.  A 64-pair level-0
call (Nq = 2.4 M rows, Cin = 32: Nq x 15 Cin floats) would keep 4.6 GB alive per convolution between forward and backward if it were
saved -- two such convolutions at level 0 alone; recomputing costs one more gather launch (the forward's ~2 ms there) and holds the
4.6 GB only while this Function's backward runs, beside the equally large dWF.  Nothing here synchronises.
Refused: CPU tensors, double backward; the fused forms of KPConv.forward (NotImplementedError in KPConv.forward_grad).
"""
import torch
from torch.autograd.function import once_differentiable

from . import context, ops
from .kpconv import _prepared
from .transformer_grad import _rows


class _KPConv(torch.autograd.Function):
    """(x (Ns, Cin), weights (KP, Cin, Cout)) -> (Nq, Cout) by the ops.kpconv call of a plain KPConv.forward on the prepared weight `sw`."""

    @staticmethod
    def forward(ctx, x, weights, q_pts, s_pts, nbr, kernel_points, extent, sw, cache, transposed):
        out = ops.kpconv(q_pts, s_pts, nbr, x, sw, kernel_points, extent)
        ctx.save_for_backward(x, weights, q_pts, s_pts, nbr, kernel_points)
        ctx.extent, ctx.cache, ctx.transposed = extent, cache, transposed
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out):
        x, weights, q_pts, s_pts, nbr, kernel_points = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        KP, Cin, Cout = weights.shape
        dx = dw = None
        with context.ForwardContext(x.device):
            wf, num = ops.kpconv_wf(q_pts, s_pts, nbr, x, kernel_points, ctx.extent)
            g = ops.row_div(_rows(d_out), num)
            if need_w:
                tn = ops.gemm_tn if (KP * Cin) % 64 == 0 and Cout % 64 == 0 else ops.gemm_tn_any
                dw = tn(wf, g).view(KP, Cin, Cout)
            del wf
            if need_x:
                wt = _prepared(ctx.cache, 'wT', weights, lambda p: ops.SplitWeight(p.view(KP * Cin, Cout), 'nk'))
                dwf = ops.gemm(g, wt, planes=3)
                table = ctx.transposed if ctx.transposed is not None else ops.nbr_transpose(nbr, x.shape[0])
                dx = ops.kpconv_gather_bwd(dwf, q_pts, s_pts, nbr.shape[1], kernel_points, ctx.extent, table)
        return (dx, dw) + (None,) * 8


def forward_grad(conv, q_pts, s_pts, neighb_inds, x, transposed=None):
    for name, t in (('q_pts', q_pts), ('s_pts', s_pts), ('neighb_inds', neighb_inds), ('x', x), ('weights', conv.weights)):
        if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
            raise RuntimeError(f'forward_grad: {name} must be a GPU tensor (got {getattr(t, "device", type(t))}); there is no CPU fallback')
    if neighb_inds.dtype is not torch.int32:
        raise NotImplementedError(f'forward_grad: neighb_inds must be int32 (the tables the preprocessor builds), got {neighb_inds.dtype}')
    if x.dim() != 2 or x.shape[1] != conv.in_channels or conv.in_channels > 256:
        raise NotImplementedError(f'forward_grad: x must be (Ns, {conv.in_channels}) with at most 256 channels, got {tuple(x.shape)}')
    if q_pts.requires_grad or s_pts.requires_grad:
        raise NotImplementedError('forward_grad: gradients of the coordinates are not implemented')
    if transposed is not None and (len(transposed) != 2 or transposed[0].numel() != x.shape[0] + 1):
        raise RuntimeError('forward_grad: `transposed` must be ops.nbr_transpose(neighb_inds, Ns) of this table')
    sw = _prepared(conv._cache, 'w', conv.weights, lambda p: ops.SplitWeight(p.view(conv.K * conv.in_channels, conv.out_channels), 'kn'))
    return _KPConv.apply(x, conv.weights, q_pts, s_pts, neighb_inds, conv.kernel_points.detach(), conv.KP_extent, sw, conv._cache,
                         transposed)
