"""The differentiable cross-encoder: TransformerCrossEncoderLayer.forward_grad / TransformerCrossEncoder.forward_grad
(regtr_amd/transformer.py) on the packed tokens, parameters and launches of the inference path, with a HIP backward.

    enc.load_state_dict(reference_encoder.state_dict())
    out = enc.forward_grad(x, pe, seg_off, kv_self, kv_cross, max_len)        # (L | 1, N, D), bit-identical to enc(...)
    loss(out).backward()                                                     # every parameter of enc, x and pe receive .grad

Three autograd Functions (and a view splitter) make a pre-norm layer (forward_pre, transformers.py:183-244 of the reference):
  * _LayerNorm   ops.layernorm (+ pe) forward, ops.layernorm_bwd backward.  It hands its input on as a second output, which the block's
                 residual add (and, between layers, the next layer) consumes instead of the input itself: the gradient of that branch
                 then arrives in this Function's backward and is added INSIDE the kernel (`dres`) -- autograd adds nothing per block.
  * _Linear      the very ops.gemm call of the inference path (same SplitWeight, planes, bias / relu / residual epilogue).  Backward:
                 dX = dY W through ops.gemm on a (K, N)-layout SplitWeight of the same parameter, dW = dY^T X through ops.gemm_tn, db and
                 the ReLU mask through ops.bias_relu_bwd; the residual input gets dY unchanged.
  * the attention core: regtr_amd.attention.packed_mha as it is; its (N, 3E) dq | dk | dv buffer is the in-projection's dY, which
                 _SplitQKV hands on without a copy.
The backward contractions always run float32-grade in the bf16x3 split (float32's operand range), whatever format the forward took:
gradients are routinely far below f16's normal range, where the f16 pair split loses its low plane.  Nothing here synchronises.
Refused: CPU tensors, double backward; post-norm layers, a value without the positional embedding, dropout (NotImplementedError).
"""
import torch
from torch.autograd.function import once_differentiable

from . import context, ops
from .attention import packed_mha
from .kpconv import _prepared


def _rows(g):
    """The upstream gradient as the kernels read it: float32, contiguous, 16-byte aligned."""
    g = g.detach().to(torch.float32)
    if not g.is_contiguous() or g.data_ptr() % 16:
        g = g.contiguous()
    return g


class _LayerNorm(torch.autograd.Function):
    """(x, gamma, beta, pe | None, eps) -> (LN(x) gamma + beta [+ pe], x handed on)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, pe, eps):
        y = ops.layernorm(x, gamma, beta, add=pe, eps=eps)
        ctx.save_for_backward(x, gamma)
        ctx.eps = eps
        ctx.set_materialize_grads(False)
        return y, x.detach()

    @staticmethod
    @once_differentiable
    def backward(ctx, dy, dres):
        x, gamma = ctx.saved_tensors
        need = ctx.needs_input_grad
        if dy is None:                                  # only the handed-on input was used
            return dres if need[0] else None, None, None, None, None
        dy = _rows(dy)
        with context.ForwardContext(x.device):
            dx, dgamma, dbeta = ops.layernorm_bwd(x, gamma, dy, dres=None if dres is None else _rows(dres), eps=ctx.eps)
        return (dx if need[0] else None, dgamma if need[1] else None, dbeta if need[2] else None, dy if need[3] else None, None)


def linear_bwd(a, weight, cache, key, dy, h=None, need=(True, True, True), residual=None):
    """Backward of one Linear y = act(a W^T + b) of this module's kind, on float32 rows: dy (M, N) the gradient of its output, h the
    activation it stored after its ReLU (None: no ReLU, or dy already carries the mask) -> (da, dw, db) for need = (a, weight, bias).
    residual (M, K): added to da inside the dX GEMM's epilogue (a gradient that reached `a` by another branch).  dW takes ops.gemm_tn
    where both widths are multiples of 64 (every Linear of the cross-encoder and the head), ops.gemm_tn_any otherwise (the backbone's
    32-wide unaries).  The caller holds the launch context."""
    da = dw = db = None
    g = dy
    if h is not None:
        g, db = ops.bias_relu_bwd(dy, h)
    elif need[2]:
        db = ops.bias_relu_bwd(dy)
    if need[0]:
        da = ops.gemm(g, _prepared(cache, key, weight, lambda w: ops.SplitWeight(w, 'kn')), planes=3, residual=residual)
    if need[1]:
        tn = ops.gemm_tn if g.shape[1] % 64 == 0 and a.shape[1] % 64 == 0 else ops.gemm_tn_any
        dw = tn(g, a)
    return da, dw, db if need[2] else None


class _Linear(torch.autograd.Function):
    """(a, weight (out, in), bias, residual | None) -> act(a W^T + bias) [+ residual] by ops.gemm on the prepared weight `sw`."""

    @staticmethod
    def forward(ctx, a, weight, bias, residual, sw, cache, key, planes, relu):
        out = ops.gemm(a, sw, planes=planes, bias=bias, relu=relu, residual=residual)
        ctx.save_for_backward(a, weight, out if relu else None)
        ctx.prep = (cache, key)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        a, weight, h = ctx.saved_tensors
        cache, key = ctx.prep
        need = ctx.needs_input_grad
        dy = _rows(dy)
        with context.ForwardContext(a.device):
            da, dw, db = linear_bwd(a, weight, cache, key, dy, h, need[:3])
        return da, dw, db, dy if need[3] else None, None, None, None, None, None


class _SplitQKV(torch.autograd.Function):
    """(N, 3E) packed projection -> its q, k, v column views.  Backward: ops.mha_bwd wrote dq | dk | dv as the column blocks of ONE (N, 3E)
    buffer, which is the in-projection's dY as it stands -- handed on without a copy (anything else is concatenated)."""

    @staticmethod
    def forward(ctx, qkv, E):
        return qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]

    @staticmethod
    @once_differentiable
    def backward(ctx, dq, dk, dv):
        base, E = dq._base, dq.shape[1]
        if (base is not None and dk._base is base and dv._base is base and tuple(base.shape) == (dq.shape[0], 3 * E) and base.is_contiguous()
                and dq.data_ptr() == base.data_ptr() and dk.data_ptr() == base.data_ptr() + 4 * E and dv.data_ptr() == base.data_ptr() + 8 * E):
            return base, None
        return torch.cat([dq, dk, dv], 1), None


def _check(layer, x, pe, seg_off, kv_self, kv_cross):
    """Everything forward_grad refuses, before any launch."""
    if not layer.normalize_before:
        raise NotImplementedError('forward_grad: normalize_before=False (post-norm layers) is not implemented')
    if pe is not None:
        for flag in ('sa_val_has_pos_emb', 'ca_val_has_pos_emb'):
            if not getattr(layer, flag):
                raise NotImplementedError(f'forward_grad: {flag}=False (a value projection without the positional embedding) is not implemented')
    if layer.self_attn.dropout != 0.0 or layer.multihead_attn.dropout != 0.0:
        raise NotImplementedError('forward_grad: dropout != 0 is not implemented')
    D, F = layer.d_model, layer.linear1.out_features
    if D % 64 or F % 64:
        raise NotImplementedError(f'forward_grad: d_model and dim_feedforward must be multiples of 64 (regtr_gemm_tn), got {D}, {F}')
    for name, t in (('x', x), ('pe', pe), ('seg_off', seg_off), ('kv_self', kv_self), ('kv_cross', kv_cross)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.device.type != 'cuda'):
            raise RuntimeError(f'forward_grad: {name} must be a GPU tensor (got {getattr(t, "device", type(t))}); there is no CPU fallback')


def _linear(layer, tag, a, weight, bias, residual=None, relu=False):
    return _Linear.apply(a, weight, bias, residual, layer._wt(tag, weight), layer._cache, (tag, 'kn'), layer.gemm_planes, relu)


def _attention(layer, attn, tag, x, norm, pe, seg_off, kv_of, max_len):
    """TransformerCrossEncoderLayer._attention, differentiable: x + out_proj(MHA(q = k = v = LN(x) + pe))."""
    D = layer.d_model
    x2p, x = _LayerNorm.apply(x, norm.weight, norm.bias, pe, norm.eps)
    qkv = _linear(layer, tag + '_in', x2p, attn.in_proj_weight, attn.in_proj_bias)
    q, k, v = _SplitQKV.apply(qkv, D)
    att = packed_mha(q, k, v, seg_off, kv_of, max_len, layer.nhead, layer.attn_precision)
    return _linear(layer, tag + '_out', att, attn.out_proj.weight, attn.out_proj.bias, residual=x)


def _layer(layer, x, pe, seg_off, kv_self, kv_cross, max_len):
    x = _attention(layer, layer.self_attn, 'sa', x, layer.norm1, pe, seg_off, kv_self, max_len)
    x = _attention(layer, layer.multihead_attn, 'ca', x, layer.norm2, pe, seg_off, kv_cross, max_len)
    x2, x = _LayerNorm.apply(x, layer.norm3.weight, layer.norm3.bias, None, layer.norm3.eps)
    h = _linear(layer, 'l1', x2, layer.linear1.weight, layer.linear1.bias, relu=True)
    return _linear(layer, 'l2', h, layer.linear2.weight, layer.linear2.bias, residual=x)


def layer_forward_grad(layer, x, pe, seg_off, kv_self, kv_cross, max_len):
    _check(layer, x, pe, seg_off, kv_self, kv_cross)
    return _layer(layer, x, pe, seg_off, kv_self, kv_cross, max_len)


def encoder_forward_grad(enc, x, pe, seg_off, kv_self, kv_cross, max_len):
    for layer in enc.layers:
        _check(layer, x, pe, seg_off, kv_self, kv_cross)
    outs = []
    for li, layer in enumerate(enc.layers):
        x = _layer(layer, x, pe, seg_off, kv_self, kv_cross, max_len)
        if enc.return_intermediate or li == enc.num_layers - 1:
            if enc.norm is None:
                outs.append(x)
            else:                       # the next layer reads the handed-on x: its gradient joins the final norm's inside the kernel
                y, x = _LayerNorm.apply(x, enc.norm.weight, enc.norm.bias, None, enc.norm.eps)
                outs.append(y)
    return torch.stack(outs)
