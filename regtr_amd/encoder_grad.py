"""The differentiable KPConv blocks and encoder: UnaryBlock / SimpleBlock / ResnetBottleneckBlock / KPFEncoder .forward_grad
(regtr_amd/kpconv.py) -- the plain composition of the operators that have a HIP backward.

    enc.load_state_dict(reference_encoder.state_dict())
    out = enc.forward_grad(ones, kpconv_meta)                  # (N_coarse, C)
    loss(out).backward()                                       # every weight of the 11 blocks receives .grad

Per block (kpconv_blocks.py:533-567, 590-646, 649-741 of the reference):
    unary        Linear (no bias) -> backbone_grad.instance_norm(lrelu = not no_relu)
    simple       KPConv.forward_grad -> instance_norm(lrelu)
    bottleneck   unary1 | identity -> KPConv.forward_grad -> instance_norm(lrelu) -> unary2's Linear;
                 shortcut = [backbone_grad.max_pool(width = pool_width)] [shortcut Linear];
                 instance_norm(y2, residual = shortcut, residual_normed = <the shortcut has a Linear>, lrelu)
This is NOT the arithmetic of the fused inference routes (block_tail, kpconv_norm_lrelu, regtr_encoder_fwd, statistics from GEMM epilogues,
xyzf records, x_stats folds): every InstanceNorm here takes its statistics from a pass over the stored float32 rows, so a block's output
differs from the inference forward's in the last bits.  It IS bit-equal to the same ops.* calls made without autograd.

The Linears run in the six-term bf16x3 split (ops.gemm, planes = 3), forward and backward; dW through ops.gemm_tn / ops.gemm_tn_any
(transformer_grad.linear_bwd).  A block's input feeds two consumers (unary1 and the shortcut): the Linear hands its input on as a second
output (transformer_grad._LayerNorm's device), the other consumer reads that, and its gradient arrives in the Linear's backward, where
the dX GEMM's epilogue adds it -- autograd adds nothing there.  Where neither consumer is a Linear autograd adds the two.

Transposed neighbour tables (ops.nbr_transpose) are built once per step and shared through `Tables`: one per level's conv table, one
per strided block's pool table, one more where a pool reads fewer columns than its table has.  A block whose input does not require a
gradient (the first one: RegTR's ones) asks for none and launches nothing for dX.

No floating-point atomics, no host wait, bit-reproducible: all of it the operators' own.
Refused: CPU tensors, double backward (the operators); deformable blocks and use_batch_norm: false (the constructors, kpconv.py);
coordinate gradients.
"""
import torch
from torch.autograd.function import once_differentiable

from . import context, ops
from .backbone_grad import instance_norm, max_pool
from .kpconv import ResnetBottleneckBlock, SimpleBlock, UnaryBlock, _LevelView, _prepared
from .transformer_grad import _rows, linear_bwd


class Tables:
    """The transposed neighbour tables of one step, keyed by (level, 'conv' | 'pool', columns walked)."""

    def __init__(self):
        self._t = {}

    def get(self, level, which, nbr, ns, width=None):
        H = nbr.shape[1] if width is None else int(width)
        key = (int(level), which, H)
        t = self._t.get(key)
        if t is None:
            with torch.no_grad():
                t = self._t[key] = ops.nbr_transpose(nbr if H == nbr.shape[1] else nbr[:, :H].contiguous(), ns)
        return t

    def __len__(self):
        return len(self._t)


class _Linear(torch.autograd.Function):
    """(a, weight (out, in)) -> (a W^T, a handed on) by ops.gemm on the prepared weight `sw` in the bf16x3 split."""

    @staticmethod
    def forward(ctx, a, weight, sw, cache):
        y = ops.gemm(a, sw, planes=3)
        ctx.save_for_backward(a, weight)
        ctx.cache = cache
        ctx.set_materialize_grads(False)
        handed = a.detach()
        if not ctx.needs_input_grad[0]:                 # (the output of a Function with a trainable weight would otherwise require grad)
            ctx.mark_non_differentiable(handed)
        return y, handed

    @staticmethod
    @once_differentiable
    def backward(ctx, dy, dres):
        a, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        if dy is None:                                  # only the handed-on input was used
            return dres if need[0] else None, None, None, None
        with context.ForwardContext(a.device):
            da, dw, _ = linear_bwd(a, weight, ctx.cache, ('w', 'kn'), _rows(dy), None, (need[0], need[1], False),
                                   residual=None if dres is None or not need[0] else _rows(dres))
        return da, dw, None, None


def _check(name, x, *others):
    for what, t in (('x', x),) + tuple(('meta', o) for o in others):
        if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
            raise RuntimeError(f'{name}: {what} must be a GPU tensor (got {getattr(t, "device", type(t))}); there is no CPU fallback')
    if x.dim() != 2 or x.dtype is not torch.float32:
        raise RuntimeError(f'{name}: x must be (N, C) float32, got {tuple(x.shape)} {x.dtype}')


def _linear(unary, a):
    """unary.mlp on rows a -> (y, a handed on)."""
    w = unary.mlp.weight
    if w.device != a.device:
        raise RuntimeError(f'forward_grad: the weights ({w.device}) and the rows ({a.device}) must live on one GPU')
    sw = _prepared(unary._cache, 'w', w, lambda p: ops.SplitWeight(p, 'nk'))
    return _Linear.apply(a, w, sw, unary._cache)


def _level(blk, meta):
    v = _LevelView(meta, blk.layer_ind, 'strided' in blk.block_name)
    if v.q_pts.requires_grad or v.s_pts.requires_grad:
        raise NotImplementedError('forward_grad: gradients of the coordinates are not implemented')
    return v


def _conv(blk, v, x, tables):
    """blk.KPConv over the block's table; the transposed table only where dX will be wanted."""
    strided = 'strided' in blk.block_name
    table = None
    if x.requires_grad and torch.is_grad_enabled():
        table = tables.get(blk.layer_ind, 'pool' if strided else 'conv', v.inds, v.s_pts.shape[0])
    return blk.KPConv.forward_grad(v.q_pts, v.s_pts, v.inds, x, transposed=table)


def unary_forward_grad(blk, x, seg_off, max_len):
    _check('UnaryBlock.forward_grad', x, seg_off)
    y, _ = _linear(blk, x)
    return instance_norm(y, seg_off, max_len, lrelu=not blk.no_relu)


def simple_forward_grad(blk, x, meta, tables=None, taps=None):
    _check('SimpleBlock.forward_grad', x)
    tables = Tables() if tables is None else tables
    v = _level(blk, meta)
    out = instance_norm(_conv(blk, v, x, tables), v.seg_post, v.max_post, lrelu=True)
    if taps is not None:
        taps.append({'norms': [out.detach()], 'pools': []})
    return out


def bottleneck_forward_grad(blk, features, meta, tables=None, taps=None):
    _check('ResnetBottleneckBlock.forward_grad', features)
    tables = Tables() if tables is None else tables
    strided = 'strided' in blk.block_name
    v = _level(blk, meta)
    tap = {'norms': [], 'pools': []} if taps is not None else None
    has_u1, has_sc = isinstance(blk.unary1, UnaryBlock), isinstance(blk.unary_shortcut, UnaryBlock)
    # the block's input has two consumers: a Linear among them hands it on and takes the other's gradient into its dX epilogue
    sc_in = features
    sc_lin = None
    if has_u1:
        y1, sc_in = _linear(blk.unary1, features)
        x = instance_norm(y1, v.seg_pre, v.max_pre, lrelu=True)
        if tap is not None:
            tap['norms'].append(x.detach())
    elif has_sc and not strided:
        sc_lin, x = _linear(blk.unary_shortcut, features)
    else:
        x = features
    y = instance_norm(_conv(blk, v, x, tables), v.seg_post, v.max_post, lrelu=True)
    if tap is not None:
        tap['norms'].append(y.detach())
    y2, _ = _linear(blk.unary2, y)
    if strided:
        if tap is not None:
            tap['pools'].append(sc_in.detach())
        table = None
        if sc_in.requires_grad and torch.is_grad_enabled():
            table = tables.get(blk.layer_ind, 'pool', v.inds, v.s_pts.shape[0], v.pool_width)
        sc_in = max_pool(sc_in, v.inds, width=v.pool_width, transposed=table)
    shortcut = sc_in
    if has_sc:
        shortcut = sc_lin if sc_lin is not None else _linear(blk.unary_shortcut, sc_in)[0]
    out = instance_norm(y2, v.seg_post, v.max_post, residual=shortcut, residual_normed=has_sc, lrelu=True)
    if tap is not None:
        tap['norms'].append(out.detach())
        taps.append(tap)
    return out


def encoder_forward_grad(enc, x, meta, taps=None):
    _check('KPFEncoder.forward_grad', x)
    for blk in enc.encoder_blocks:
        if not isinstance(blk, (SimpleBlock, ResnetBottleneckBlock)):
            raise NotImplementedError(f'KPFEncoder.forward_grad: block {type(blk).__name__} is not differentiable')
    tables = Tables()
    for blk in enc.encoder_blocks:
        x = blk.forward_grad(x, meta, tables, taps)
    return x
