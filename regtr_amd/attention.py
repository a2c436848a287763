"""Differentiable packed multi-head attention: the attention core of the cross-encoder (ops.mha, transformers.py:197-226 of the
reference) with a HIP backward (csrc/attention_bwd.hip, regtr_mha_bwd), and an nn.Module around it that carries
nn.MultiheadAttention's parameters.

    attn = PackedMultiheadAttention(256, 8).cuda()
    attn.load_state_dict(reference_layer.self_attn.state_dict())
    y = attn(x, x, x, seg_off, kv_self, max_len)          # x (N, 256): the clouds' tokens stacked, no padding, no mask

Tokens are PACKED: rows [seg_off[c], seg_off[c + 1]) are cloud c, and cloud c attends cloud kv_of[c] (self: kv_of[c] = c; cross: the
partner cloud of the pair; any map is legal).  The forward is ops.mha unchanged; the backward recomputes the probabilities from q, k, v
(flash style), so only those three are saved and the gradients do not depend on the forward's precision.  Nothing here synchronises.
Refused: CPU tensors, double backward.  TransformerCrossEncoderLayer.forward_grad (regtr_amd/transformer_grad.py) is built on it; the
model's forward stays inference only.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import context, ops


class _PackedMHA(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, seg_off, kv_of, max_len, n_heads, precision):
        with context.on_device(q.device):
            out = ops.mha(q, k, v, seg_off, kv_of, max_len, n_heads, precision)
        ctx.save_for_backward(q, k, v, seg_off, kv_of)
        ctx.meta = (int(max_len), int(n_heads))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        q, k, v, seg_off, kv_of = ctx.saved_tensors
        max_len, n_heads = ctx.meta
        g = g.detach().to(torch.float32)
        if g.dim() != 2 or (g.shape[1] > 1 and g.stride(1) != 1) or g.stride(0) % 4 or g.stride(0) < g.shape[1] or g.data_ptr() % 16:
            g = g.contiguous()
        with context.on_device(q.device):
            dq, dk, dv = ops.mha_bwd(q, k, v, g, seg_off, kv_of, max_len, n_heads)
        need = ctx.needs_input_grad
        return (dq if need[0] else None, dk if need[1] else None, dv if need[2] else None, None, None, None, None, None)


def packed_mha(q, k, v, seg_off, kv_of, max_len, n_heads, precision=0):
    """softmax(q k^T / sqrt(32)) v per head on packed clouds, differentiable in q, k, v.  q, k, v: (N, E) float32 GPU tensors or
    row-strided column views of a packed projection (E = 32 n_heads); seg_off (C + 1,) and kv_of (C,) int32 on the GPU; max_len >= the
    longest cloud.  The output is bit-identical to ops.mha(..., precision) whether or not anything requires grad."""
    for name, t in (('q', q), ('k', k), ('v', v), ('seg_off', seg_off), ('kv_of', kv_of)):
        if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
            raise RuntimeError(f'packed_mha: {name} must be a GPU tensor (got {getattr(t, "device", type(t))}); there is no CPU fallback')
    return _PackedMHA.apply(q, k, v, seg_off, kv_of, max_len, n_heads, precision)


class PackedMultiheadAttention(nn.Module):
    """nn.MultiheadAttention (bias, no dropout, no mask beyond the cloud structure) on packed tokens.  Parameters carry
    nn.MultiheadAttention's names and shapes -- in_proj_weight (3E, E), in_proj_bias (3E,), out_proj.weight (E, E), out_proj.bias (E,)
    -- and its initialisation, so a reference state_dict loads.  forward(query, key, value, seg_off, kv_of, max_len): (N, E) packed
    tokens -> (N, E); differentiable end to end: the projections are torch's linear, the core is packed_mha."""

    def __init__(self, embed_dim, num_heads, precision=0):
        super().__init__()
        if embed_dim != 32 * num_heads:
            raise NotImplementedError(f'PackedMultiheadAttention: head_dim must be 32, got embed_dim {embed_dim} / num_heads {num_heads}')
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.precision = precision
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * embed_dim))
        self.out_proj = nn.modules.linear.NonDynamicallyQuantizableLinear(embed_dim, embed_dim, bias=True)
        self._reset_parameters()

    def _reset_parameters(self):       # nn.MultiheadAttention._reset_parameters
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.constant_(self.in_proj_bias, 0.)
        nn.init.constant_(self.out_proj.bias, 0.)

    def forward(self, query, key, value, seg_off, kv_of, max_len):
        E = self.embed_dim
        w, b = self.in_proj_weight, self.in_proj_bias
        if query is key and key is value:
            qkv = F.linear(query, w, b)                   # one packed (N, 3E) projection; q, k, v are its column views
            q, k, v = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
        else:
            q = F.linear(query, w[:E], b[:E])
            k = F.linear(key, w[E:2 * E], b[E:2 * E])
            v = F.linear(value, w[2 * E:], b[2 * E:])
        o = packed_mha(q, k, v, seg_off, kv_of, max_len, self.num_heads, self.precision)
        return self.out_proj(o)
