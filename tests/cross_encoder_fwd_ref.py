"""Forward-only restatement of the cross-encoder for EVERY configuration (one layer: forward_post / forward_pre, transformers.py:121-244 of
the reference, with both value flags and with or without a positional embedding; the stack, :27-59, with or without the final norm and
return_intermediate) on PACKED tokens, written from the arithmetic in plain torch and dtype-generic: float64 on the CPU is the yardstick
of tests/test_gpu_cross_encoder_variants.py, the same code in float32 on the GPU is the independent float32 evaluation its documented
fallback reads.  It shares the seeded parameters, the token layout, LayerNorm and the attention core (a cloud attending an empty cloud
gets zero rows) with tests/cross_encoder_grads_ref.py; tests/test_cross_encoder_variants_host.py pins it to the stored float64 outputs
of the real reference module (tools/make_golden_cross_encoder_variants.py).

Tokens: rows [seg[c], seg[c + 1]) are cloud c; the clouds are [src_0 .. src_{B-1}, tgt_0 .. tgt_{B-1}]; self-attention reads cloud c
(kv_self), cross-attention the partner cloud of the pair (kv_cross)."""
import math

import torch

from tests.cross_encoder_grads_ref import draw_params, layout, ln_fwd, mha_fwd, posemb

# ------------------------------------------------------------------------------------------------ the configuration matrix
# (pre_norm, sa_val_has_pos_emb, ca_val_has_pos_emb, with pe): the 8 flag combinations under a positional embedding, and pe None for
# both norm orders -- there the value flags decide nothing (with_pos_embed(t, None) = t, transformers.py:118-119), so the tests set them
# to False: a layer that consulted them without a pe would be caught.
BASES = [(pre, sa, ca, True) for pre in (True, False) for sa in (True, False) for ca in (True, False)] + [(True, False, False, False),
                                                                                                         (False, False, False, False)]
# 'full': return_intermediate with the final norm where RegTR builds one (pre-norm only; post-norm: norm None, the raw layer outputs);
# 'plain': norm None, the last layer's output alone.  Every base in both modes: 20 variants (the 8 + 8 with a pe, 2 + 2 without) ...
MODES = ('full', 'plain')
# ... and one more stack form that those leave out: the final norm WITHOUT return_intermediate ('last').
EXTRA = [((True, True, True, True), 'last'), ((True, False, True, True), 'last')]


def variant_name(base, mode):
    pre, sa, ca, with_pe = base
    return f"{'pre' if pre else 'post'}-{'sa%d-ca%d' % (sa, ca) if with_pe else 'nope'}-{mode}"


VARIANTS = {variant_name(b, m): (b, m) for b in BASES for m in MODES}
VARIANTS.update({variant_name(b, m): (b, m) for b, m in EXTRA})


def stack_form(base, mode):
    """-> (final norm?, return_intermediate?) of a variant."""
    return {'full': (base[0], True), 'plain': (False, False), 'last': (True, False)}[mode]


# name -> D, heads, F, layers, (src lens, tgt lens), seed.  'golden' is the shape the real reference module's outputs are stored for;
# 'ragged' (a one-token cloud, a cloud one past a 128-row tile, two pairs), 'ragged_empty' (the second pair's target cloud is empty: its
# partner's cross-attention rows are zero) and 'wide' (the shipped widths) are the GPU tests'.
CASES = {
    'golden': dict(D=64, H=2, F=128, L=2, src=[5, 12], tgt=[1, 9], seed=41),
    'ragged': dict(D=64, H=2, F=128, L=2, src=[33, 64], tgt=[1, 129], seed=42),
    'ragged_empty': dict(D=64, H=2, F=128, L=2, src=[33, 64], tgt=[1, 0], seed=43),
    'wide': dict(D=256, H=8, F=1024, L=2, src=[410], tgt=[339], seed=44),
}


def draw_case(name):
    """-> dict: the case's fields, 'sd' (state_dict WITH the final norm: a variant without one drops the two keys; the layers' parameters
    are drawn first, so they are the same either way), 'x' (N, D), 'pe' (N, D), 'seg', 'kv_self', 'kv_cross', 'max_len' -- float32 CPU
    tensors / int32 arrays from the case's seed."""
    c = dict(CASES[name])
    gen = torch.Generator().manual_seed(c['seed'])
    N = sum(c['src']) + sum(c['tgt'])
    c['sd'] = draw_params(c['D'], c['F'], c['L'], True, gen)
    c['x'] = torch.randn((N, c['D']), generator=gen)
    c['pe'] = posemb(torch.rand((N, 3), generator=gen) * 2.0, c['D'], scale=2 * math.pi)
    c['seg'], c['kv_self'], c['kv_cross'] = layout(c['src'], c['tgt'])
    c['max_len'] = max(c['src'] + c['tgt'])
    return c


def pair_of(c, b):
    """Pair b of a drawn case as a case of its own (the same parameters, that pair's tokens)."""
    B = len(c['src'])
    rows = torch.cat([torch.arange(int(c['seg'][i]), int(c['seg'][i + 1])) for i in (b, B + b)])
    p = dict(c, src=[c['src'][b]], tgt=[c['tgt'][b]], x=c['x'][rows].contiguous(), pe=c['pe'][rows].contiguous(), rows=rows)
    p['seg'], p['kv_self'], p['kv_cross'] = layout(p['src'], p['tgt'])
    p['max_len'] = max(p['src'] + p['tgt'])
    return p


# ------------------------------------------------------------------------------------------------ the arithmetic
def _attn(sd, p, attn, norm, x, pe, seg, kv_of, H, pre_norm, val_has_pe):
    """One attention block.  Queries and keys are the tokens (normalised first when pre_norm) plus pe; the values carry pe only when
    the flag says so; the residual is the block's input; post-norm layers normalise the sum."""
    D = x.shape[1]
    W, b = sd[p + attn + '.in_proj_weight'], sd[p + attn + '.in_proj_bias']
    t = ln_fwd(x, sd[p + norm + '.weight'], sd[p + norm + '.bias'])[0] if pre_norm else x
    qk_in = t if pe is None else t + pe
    v_in = qk_in if val_has_pe else t
    q = qk_in @ W[:D].T + b[:D]
    k = qk_in @ W[D:2 * D].T + b[D:2 * D]
    v = v_in @ W[2 * D:].T + b[2 * D:]
    o = mha_fwd(q, k, v, seg, kv_of, H)[0]
    y = x + o @ sd[p + attn + '.out_proj.weight'].T + sd[p + attn + '.out_proj.bias']
    return y if pre_norm else ln_fwd(y, sd[p + norm + '.weight'], sd[p + norm + '.bias'])[0]


def layer_fwd(sd, prefix, x, pe, seg, kv_self, kv_cross, H, pre_norm, sa_val, ca_val):
    """One TransformerCrossEncoderLayer on all tokens: self-attention, cross-attention (both directions read the tokens the self-attention
    left), feed-forward.  sd: parameters under prefix + their state_dict names, tensors of x's dtype and device."""
    x = _attn(sd, prefix, 'self_attn', 'norm1', x, pe, seg, kv_self, H, pre_norm, sa_val)
    x = _attn(sd, prefix, 'multihead_attn', 'norm2', x, pe, seg, kv_cross, H, pre_norm, ca_val)
    n3 = lambda t: ln_fwd(t, sd[prefix + 'norm3.weight'], sd[prefix + 'norm3.bias'])[0]
    t = n3(x) if pre_norm else x
    y = x + torch.relu(t @ sd[prefix + 'linear1.weight'].T + sd[prefix + 'linear1.bias']) @ sd[prefix + 'linear2.weight'].T + sd[prefix + 'linear2.bias']
    return y if pre_norm else n3(y)


def stack_fwd(sd, x, pe, seg, kv_self, kv_cross, H, L, pre_norm, sa_val, ca_val, final, return_intermediate):
    """The L-layer encoder -> (L, N, D) with return_intermediate (every layer's output, through the final norm when there is one), else
    (1, N, D) (the last layer's).  final: apply sd['norm.*']."""
    fin = (lambda t: ln_fwd(t, sd['norm.weight'], sd['norm.bias'])[0]) if final else (lambda t: t)
    outs = []
    for li in range(L):
        x = layer_fwd(sd, f'layers.{li}.', x, pe, seg, kv_self, kv_cross, H, pre_norm, sa_val, ca_val)
        if return_intermediate:
            outs.append(fin(x))
    return torch.stack(outs) if return_intermediate else fin(x)[None]


def run_variant(c, vname, dtype=torch.float64, device='cpu', sd=None, layers=None):
    """stack_fwd of a drawn case under a variant, in the given dtype / device.  sd: other parameters than the case's (float32 CPU).
    layers=1: the first layer alone -> (N, D)."""
    (pre, sa, ca, with_pe), mode = VARIANTS[vname]
    final, ri = stack_form((pre, sa, ca, with_pe), mode)
    t = lambda a: a.to(device=device, dtype=dtype)
    P = {k: t(v) for k, v in (c['sd'] if sd is None else sd).items()}
    pe = t(c['pe']) if with_pe else None
    if layers == 1:
        return layer_fwd(P, 'layers.0.', t(c['x']), pe, c['seg'], c['kv_self'], c['kv_cross'], c['H'], pre, sa, ca)
    return stack_fwd(P, t(c['x']), pe, c['seg'], c['kv_self'], c['kv_cross'], c['H'], c['L'], pre, sa, ca, final, ri)
