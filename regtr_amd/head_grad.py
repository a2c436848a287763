"""Everything above the KPConv backbone as differentiable calls with a HIP backward: the correspondence head
(CorrespondenceRegressor.forward_grad) and the stack feat_proj -> positional embedding -> cross-encoder -> head on packed tokens
(stack_forward_grad), which RegTR.forward_grad / RegTR.training_step run above a frozen backbone.

    corr, logit = head.forward_grad(feats)                       # (L', N, 3), (L', N): bit-identical to head(feats)
    (w_c * corr_loss(corr) + w_o * overlap_loss(logit)).backward()

The regressor (regtr.py:399-443 of the reference) is
    h1 = relu(f W0^T + b0),  h2 = relu(h1 W2^T + b2),  corr = h2 W4^T + b4 (M, 3),  logit = f wc^T + bc (M,)
and its forward here is CorrespondenceRegressor._mlp, the four ops.gemm calls of the inference path on the same prepared weights.
Backward: the two narrow outputs go through ONE pass over the rows, ops.head_tail_bwd (csrc/head_bwd.hip): g2, the gradient in front
of coor_mlp[2]'s ReLU, with its column sums db2; r = dlogit wc, the logit branch's share of df; dW4, db4, dwc, dbc.  The two D x D Linears
then go through transformer_grad.linear_bwd, the machinery of transformer_grad._Linear: dX by ops.gemm on a (K, N)-layout SplitWeight of
the same parameter, dW by ops.gemm_tn, the bias sum and the ReLU mask by ops.bias_relu_bwd; r is the `residual` of the last dX GEMM, so
df = g1 W0 + r takes no pass of its own.  The backward contractions run float32-grade in the bf16x3 split whatever format the forward
took, as transformer_grad.py explains.  Nothing here synchronises.
Refused: CPU tensors, double backward, d_embed not a multiple of 64, the attention-valued head CorrespondenceDecoder
(NotImplementedError: regtr_attn_xyz has no backward).
"""
import torch
from torch.autograd.function import once_differentiable

from . import context, ops
from .kpconv import _prepared
from .transformer_grad import _Linear, _rows, linear_bwd

# A-B switch of the head's narrow tail: ops.head_tail_bwd (one pass), or the same backward composed from ops.gemm, ops.gemm_tn_any and
# ops.bias_relu_bwd (tools/head_grad_bench.py measures both; docs/KERNELS.md)
use_fused_tail = True


def tail_bwd_composed(dcorr, dlogit, h2, f, w4, wc):
    """ops.head_tail_bwd's results from the generic ops: two thin GEMMs for g2 (+ the ReLU pass) and r, two transposed GEMMs for dW4 and
    dwc; the 3- and 1-wide bias sums, below ops.bias_relu_bwd's width, by torch."""
    M, D = h2.shape
    dev = h2.device
    zeros = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    if dcorr is not None:
        g2, db2 = ops.bias_relu_bwd(ops.gemm(dcorr, w4.detach().contiguous()), h2, inplace=True)
        dw4, db4 = ops.gemm_tn_any(dcorr, h2), dcorr.sum(0)
    else:
        g2, db2, dw4, db4 = zeros(M, D), zeros(D), zeros(3, D), zeros(3)
    if dlogit is not None:
        dl = dlogit.reshape(M, 1)
        r = ops.gemm(dl, wc.detach().reshape(1, D).contiguous())
        dwc, dbc = ops.gemm_tn_any(dl, f).reshape(D), dl.sum(0)
    else:
        r, dwc, dbc = zeros(M, D), zeros(D), zeros(1)
    return g2, r, dw4, db4, dwc, dbc, db2


class _Regressor(torch.autograd.Function):
    """(f (M, D), W0, b0, W2, b2, W4, b4, wc, bc) -> (corr (M, 3), logit (M, 1)) by CorrespondenceRegressor._mlp."""

    @staticmethod
    def forward(ctx, f, w0, b0, w2, b2, w4, b4, wc, bc, head):
        h1, h2, corr, logit = head._mlp(f)
        ctx.save_for_backward(f, h1, h2, w0, w2, w4, wc)
        ctx.cache = head._cache
        ctx.set_materialize_grads(False)
        return corr, logit

    @staticmethod
    @once_differentiable
    def backward(ctx, dcorr, dlogit):
        f, h1, h2, w0, w2, w4, wc = ctx.saved_tensors
        need = ctx.needs_input_grad
        if dcorr is None and dlogit is None:
            return (None,) * 10
        dcorr = None if dcorr is None else _rows(dcorr)
        dlogit = None if dlogit is None else _rows(dlogit)
        with context.ForwardContext(f.device):
            tail = ops.head_tail_bwd if use_fused_tail else tail_bwd_composed
            g2, r, dw4, db4, dwc, dbc, db2 = tail(dcorr, dlogit, h2, f, w4.detach(), wc.detach())
            if dcorr is None:                       # only the overlap logit was used: df is the logit branch alone
                return r if need[0] else None, None, None, None, None, None, None, dwc.view(1, -1), dbc, None
            dh1, dw2, _ = linear_bwd(h1, w2, ctx.cache, ('2', 'kn'), g2, None, (True, need[3], False))
            df, dw0, db0 = linear_bwd(f, w0, ctx.cache, ('0', 'kn'), dh1, h1, (need[0], need[1], True),
                                      residual=None if dlogit is None else r)
        if dlogit is None:
            dwc = dbc = None
        return df, dw0, db0, dw2, db2, dw4, db4, None if dwc is None else dwc.view(1, -1), dbc, None


def regressor_forward_grad(head, feats):
    """CorrespondenceRegressor.forward_grad: feats (L', N, D) -> corr (L', N, 3), logit (L', N)."""
    if not isinstance(feats, torch.Tensor) or feats.device.type != 'cuda':
        raise RuntimeError(f'forward_grad: feats must be a GPU tensor (got {getattr(feats, "device", type(feats))}); there is no CPU fallback')
    Lyr, N, D = feats.shape
    if D % 64:
        raise NotImplementedError(f'forward_grad: d_embed must be a multiple of 64 (regtr_gemm_tn, regtr_head_tail_bwd), got {D}')
    m, c = head.coor_mlp, head.conf_logits_decoder
    f = feats.reshape(Lyr * N, D)
    corr, logit = _Regressor.apply(f, m[0].weight, m[0].bias, m[2].weight, m[2].bias, m[4].weight, m[4].bias, c.weight, c.bias, head)
    return corr.view(Lyr, N, 3), logit.view(Lyr, N)


class _Procrustes(torch.autograd.Function):
    """(kp (N, 3), corr (L, N, 3), logit (L, N), seg_off (2B + 1,)) -> pose (L, B, 3, 4) by ops.weighted_procrustes.  Backward:
    ops.weighted_procrustes_bwd, the closed form of csrc/procrustes.hip, which recomputes the forward from the saved INPUTS (the
    forward launch saves nothing).  Gradients go to corr and logit."""

    @staticmethod
    def forward(ctx, kp, corr, logit, seg_off, n_pairs):
        pose = ops.weighted_procrustes(kp, corr, logit, seg_off, n_pairs)
        ctx.save_for_backward(kp, corr, logit, seg_off)
        ctx.n_pairs = n_pairs
        return pose

    @staticmethod
    @once_differentiable
    def backward(ctx, d_pose):
        kp, corr, logit, seg_off = ctx.saved_tensors
        need = ctx.needs_input_grad
        with context.ForwardContext(kp.device):
            d_corr, d_logit, _, _ = ops.weighted_procrustes_bwd(kp, corr, logit, seg_off, ctx.n_pairs,
                                                                d_pose.detach().to(torch.float32).contiguous(), want_logit=need[2])
        return None, d_corr if need[1] else None, d_logit, None, None


class PoseTensor(torch.Tensor):
    """What RegTR.forward_grad returns as pred['pose'].  Until the pose solve had a backward that entry was a gradient-free tensor, and
    callers read it as one -- `pred['pose'][0].cpu().numpy()` in logging and in comparisons with a recorded pose.  It now carries a
    grad_fn, on which torch.Tensor.numpy() raises; this subclass keeps those callers working: numpy() (and with it np.asarray) detaches
    first.  Everything else, autograd included, is torch.Tensor's."""

    def numpy(self, *args, **kwargs):
        return self.detach().as_subclass(torch.Tensor).numpy(*args, **kwargs)


def procrustes_forward_grad(kp, corr, logit, seg_off, n_pairs):
    """ops.weighted_procrustes(kp, corr, logit, seg_off, n_pairs) -- the very call, the same bits -- as a differentiable call: pose
    (L, B, 3, 4) carries a gradient to corr (L, N, 3) and logit (L, N), none to kp.  A pair whose pose is no differentiable function of
    its inputs (docs/PARITY.md) contributes exactly zero."""
    for name, t in (('kp', kp), ('corr', corr), ('logit', logit), ('seg_off', seg_off)):
        if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
            raise RuntimeError(f'procrustes_forward_grad: {name} must be a GPU tensor (got {getattr(t, "device", type(t))}); there is no CPU fallback')
    if kp.requires_grad:
        raise NotImplementedError('procrustes_forward_grad: kp.requires_grad (a gradient with respect to the key points) is not implemented '
                                  'here; regtr_amd.se3.compute_rigid_transform differentiates both point sets')
    return _Procrustes.apply(kp, corr.contiguous(), logit.contiguous(), seg_off, int(n_pairs))


class _PosembMLP(torch.autograd.Function):
    """(xyz (n, 3), the five Linears' weight and bias) -> pe (n, d_model) by ops.posemb_mlp with save=True: one launch, the four
    activations after their ReLUs kept as one (n, 480) buffer.  Backward: transformer_grad.linear_bwd per layer, last to first, on
    column views of that buffer -- the ReLU mask and the bias sums by ops.bias_relu_bwd, dX by ops.gemm on a (K, N)-layout SplitWeight,
    dW by ops.gemm_tn / ops.gemm_tn_any.  No dX for the first layer: xyz takes no gradient."""

    @staticmethod
    def forward(ctx, xyz, w0, b0, w1, b1, w2, b2, w3, b3, w4, b4, module):
        pe, acts = ops.posemb_mlp(xyz, module._weights(), save=True)
        ctx.save_for_backward(xyz, acts, w0, w1, w2, w3, w4)
        ctx.cache = module._cache
        return pe

    @staticmethod
    @once_differentiable
    def backward(ctx, dpe):
        xyz, acts, *w = ctx.saved_tensors
        need = ctx.needs_input_grad
        g = _rows(dpe)
        c = (0, 32, 96, 224, 480)
        h = [acts[:, c[l]:c[l + 1]] for l in range(4)]
        a = [xyz] + h
        grads = [None] * 10
        with context.ForwardContext(xyz.device):
            for l in (4, 3, 2, 1, 0):
                g, grads[2 * l], grads[2 * l + 1] = linear_bwd(a[l], w[l], ctx.cache, (('bwd', l), 'kn'), g, h[l] if l < 4 else None,
                                                               (l > 0, need[1 + 2 * l], need[2 + 2 * l]))
        return (None, *grads, None)


def posemb_forward_grad(module, xyz):
    """PositionEmbeddingLearned.forward_grad: xyz (n, 3) -> pe (n, d_model), the bits of module(xyz)."""
    if not isinstance(xyz, torch.Tensor) or xyz.device.type != 'cuda':
        raise RuntimeError(f'forward_grad: xyz must be a GPU tensor (got {getattr(xyz, "device", type(xyz))}); there is no CPU fallback')
    if xyz.requires_grad:
        raise NotImplementedError('forward_grad: xyz.requires_grad (a gradient with respect to the coordinates) is not implemented')
    lin = module.linears()
    return _PosembMLP.apply(xyz, *[t for m in lin for t in (m.weight, m.bias)], module)


def stack_forward_grad(feat_proj, pos_embed, encoder, head, feats_un, xyz, seg_off, kv_self, kv_cross, max_len, head_layers, cache=None):
    """Everything above the backbone on packed tokens (regtr.py:145-168 of the reference), differentiable in feats_un and in every
    parameter of feat_proj, encoder and head:
        both_feats_un = feat_proj(feats_un)                                 (N, D)      a transformer_grad._Linear
        pe            = pos_embed(xyz)                                      (N, D)      pos_embed None: no embedding; the sine table takes no
                                                                                        gradient, the learned MLP runs pos_embed.forward_grad(xyz)
        feats_cond    = encoder.forward_grad(both_feats_un, pe, ...)        (L, N, D)
        corr, logit   = head.forward_grad(feats_cond[head_layers])          (L', N, 3), (L', N)
    head_layers: the decoder layers a loss reads, ascending; the head runs on those only, so a layer no loss reads costs no head
    backward.  cache: the dict feat_proj's prepared weights live in (RegTR passes its own, so the inference path's planes are shared).
    -> (both_feats_un, feats_cond, corr, logit)."""
    from .regtr import CorrespondenceRegressor
    if not isinstance(head, CorrespondenceRegressor):
        raise NotImplementedError(f'stack_forward_grad: {type(head).__name__} has no backward; only CorrespondenceRegressor '
                                  '(direct_regress_coor: true) is differentiable')
    for name, t in (('feats_un', feats_un), ('xyz', xyz), ('seg_off', seg_off), ('kv_self', kv_self), ('kv_cross', kv_cross)):
        if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
            raise RuntimeError(f'stack_forward_grad: {name} must be a GPU tensor (got {getattr(t, "device", type(t))}); there is no CPU fallback')
    head_layers = sorted(set(int(l) for l in head_layers))
    n_out = encoder.num_layers if encoder.return_intermediate else 1
    if not head_layers or head_layers[0] < 0 or head_layers[-1] >= n_out:
        raise RuntimeError(f'stack_forward_grad: head_layers must name some of the encoder\'s {n_out} outputs, got {head_layers}')
    K, D = feat_proj.in_features, feat_proj.out_features
    if K % 64 or D % 64:
        raise NotImplementedError(f'stack_forward_grad: feat_proj\'s widths must be multiples of 64 (regtr_gemm_tn), got {K}, {D}')
    if cache is None:
        cache = feat_proj.__dict__.setdefault('_regtr_cache', {})
    sw = _prepared(cache, 'feat_proj', feat_proj.weight, lambda w: ops.SplitWeight(w, 'nk'))
    both_feats_un = _Linear.apply(feats_un, feat_proj.weight, feat_proj.bias, None, sw, cache, ('feat_proj', 'kn'), 3, False)
    pe = None
    if pos_embed is not None:
        if isinstance(pos_embed, torch.nn.Module) and next(pos_embed.parameters(), None) is not None:
            # the learned embedding: dpe, summed over the LN(x) + pe sites of the layers, trains it
            pe = pos_embed.forward_grad(xyz)
        else:
            with torch.no_grad():
                pe = pos_embed(xyz)
    feats_cond = encoder.forward_grad(both_feats_un, pe, seg_off, kv_self, kv_cross, max_len)
    lo, hi = head_layers[0], head_layers[-1]
    sel = feats_cond[lo:hi + 1] if hi - lo + 1 == len(head_layers) else torch.stack([feats_cond[l] for l in head_layers])
    corr, logit = head.forward_grad(sel)
    return both_feats_un, feats_cond, corr, logit
