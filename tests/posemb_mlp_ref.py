"""Restatement of the learned positional embedding (PositionEmbeddingLearned, position_embedding.py:53-72 of the reference): the
five-Linear ReLU MLP 3 -> 32 -> 64 -> 128 -> 256 -> d_model in float64 numpy, forward with a componentwise bound on
|float32 evaluation - float64| and a written-out backward.  Float64 on the CPU is the yardstick of tests/test_gpu_posemb_mlp.py and
tests/test_posemb_mlp_host.py.  Seeds are stored, matrices are not.

The bound (running, first order in U = 2^-24).  A float32 evaluation of layer l, y = h W^T + b with K_l inputs, rounds each product
into its sum once per term (an fmaf chain: K_l roundings) and the bias addition once: at most (K_l + 1) U (|W| |h| + |b|), taken as
(K_l + 2) U.  The error e_{l-1} its input already carries passes through |W|, and the ReLU passes an error on unchanged
(|relu(a) - relu(b)| <= |a - b|, a side flip included).  With e_0 = 0 (xyz is float32 data):
    e_l = |W_l| e_{l-1} + (K_l + 2) U (|W_l| |h_{l-1}| + |b_l|).
"""
import numpy as np
import torch

U = 2.0 ** -24
RELU_MARGIN = 2.0 ** -19          # tests/head_grads_ref.py: relu_margin says why a seeded case keeps its ReLU pre-activations this far from 0
LAYERS = (0, 2, 4, 6, 8)          # the Linears' indices in the reference's nn.Sequential
WIDTHS = (3, 32, 64, 128, 256)    # their input widths; the last one's output is d_model
ACT_COLS = (0, 32, 96, 224, 480)  # h1 | h2 | h3 | h4 in the kernel's (n, 480) saved-activations buffer
KEYS = [f'mlp.{i}.{p}' for i in LAYERS for p in ('weight', 'bias')]


def shapes(d_model):
    w = WIDTHS + (d_model,)
    out = {}
    for l, i in enumerate(LAYERS):
        out[f'mlp.{i}.weight'] = (w[l + 1], w[l])
        out[f'mlp.{i}.bias'] = (w[l + 1],)
    return out


def draw_mlp(d_model, seed, hidden_gain=2.0):
    """state_dict of a PositionEmbeddingLearned (float32 CPU tensors, the reference's key order): hidden weights N(0, hidden_gain / fan_in),
    the last layer N(0, 1 / fan_in), biases N(0, 0.1), so that |pe| stays within a few units for key points of unit scale."""
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for k, s in shapes(d_model).items():
        t = torch.randn(s, generator=gen)
        if len(s) == 2:
            gain = 1.0 if k == 'mlp.8.weight' else hidden_gain
            sd[k] = t * (gain / s[1]) ** 0.5
        else:
            sd[k] = 0.1 * t
    return sd


def _np(sd, dtype=np.float64):
    return [(np.asarray(sd[f'mlp.{i}.weight'], dtype=dtype), np.asarray(sd[f'mlp.{i}.bias'], dtype=dtype)) for i in LAYERS]


def forward(sd, xyz, quant=None):
    """The MLP in float64 -> dict: 'pe' (n, d_model), 'h' [h1 .. h4] after their ReLUs, 'z' [z1 .. z4] the pre-activations, 'acts' (n,
    480) = h1 | h2 | h3 | h4, and the bounds 'b_pe', 'b_h' (list), 'b_acts' on |float32 evaluation - this|.
    quant: a function applied to BOTH operands of every contraction (the layer's input and its weight) before it -- the model of an
    evaluation on reduced-precision operands (bf16, one f16 plane); the bounds are those of the unquantised float32 evaluation."""
    q = (lambda a: a) if quant is None else quant
    h = np.asarray(xyz, dtype=np.float64)
    e = np.zeros_like(h)
    hs, zs, bs = [], [], []
    for l, (W, b) in enumerate(_np(sd)):
        K = W.shape[1]
        e = e @ np.abs(W).T + (K + 2) * U * (np.abs(h) @ np.abs(W).T + np.abs(b))
        z = q(h) @ q(W).T + b
        if l < 4:
            h = np.maximum(z, 0.0)
            hs.append(h); zs.append(z); bs.append(e)
    return {'pe': z, 'b_pe': e, 'h': hs, 'z': zs, 'b_h': bs, 'acts': np.concatenate(hs, 1), 'b_acts': np.concatenate(bs, 1)}


def forward_f32(sd, xyz):
    """The same MLP evaluated in float32 numpy (whatever order the matrix product sums in) -> pe (n, d_model) float32."""
    h = np.asarray(xyz, dtype=np.float32)
    for l, (W, b) in enumerate(_np(sd, np.float32)):
        h = h @ W.T + b
        if l < 4:
            h = np.maximum(h, np.float32(0))
    return h


def round_bf16(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def round_f16(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.float16).to(torch.float64).numpy()


def relu_margin(sd, xyz):
    """The smallest |pre-activation| of the MLP's four ReLUs in float64."""
    return min(float(np.abs(z).min()) for z in forward(sd, xyz)['z'])


def backward(sd, xyz, sides, dpe):
    """The parameter gradients of sum(pe * dpe) in float64, with the ReLU sides it is given: sides = [h1 > 0, .., h4 > 0] (bool arrays,
    or the activations themselves).  The activations are recomputed in float64 UNDER those sides (h_l = z_l where the side says so, else
    0), so a kernel's gradients are compared with the gradient of the function the kernel evaluated.  -> {state_dict key: gradient}."""
    P = _np(sd)
    sides = [np.asarray(s) > 0 for s in sides]
    a = [np.asarray(xyz, dtype=np.float64)]
    for l in range(4):
        W, b = P[l]
        a.append(np.where(sides[l], a[l] @ W.T + b, 0.0))
    g = np.asarray(dpe, dtype=np.float64)
    grads = {}
    for l in (4, 3, 2, 1, 0):
        if l < 4:
            g = np.where(sides[l], g, 0.0)
        grads[f'mlp.{LAYERS[l]}.weight'] = g.T @ a[l]
        grads[f'mlp.{LAYERS[l]}.bias'] = g.sum(0)
        if l > 0:
            g = g @ P[l][0]
    return grads


# ------------------------------------------------------------------------------------------------ the model goldens (tools/make_golden_learned_posemb.py)
MODEL_SEED = 31                   # draw_mlp(cfg.d_embed, MODEL_SEED): the pos_embed.mlp.* of the two model goldens


def learned_state_dict(base_sd, d_model, seed=MODEL_SEED):
    """A RegTR state_dict under pos_emb_type 'learned': base_sd (oracle.seeded_weights.seeded_state_dict of the sine config) with the drawn
    pos_embed.mlp.* inserted at the reference's key position, after feat_proj and before transformer_encoder."""
    out = {}
    for k, v in base_sd.items():
        out[k] = v
        if k == 'feat_proj.bias':
            out.update({'pos_embed.' + mk: mv for mk, mv in draw_mlp(d_model, seed).items()})
    return out


# ------------------------------------------------------------------------------------------------ the chain above the backbone with a learned pe
STACK_CASE = '3dmatch_crop_b2'    # tests/head_grads_ref.py's FULL_CASES entry (452 tokens, D = 64), its pe from the learned MLP
STACK_NOMINAL_SEED = 71
STACK_SEED = 71                   # the first seed from the nominal one whose ReLU pre-activations all keep RELU_MARGIN from 0 (stack_relu_margin)


def draw_stack_case(seed=STACK_SEED):
    """head_grads_ref.draw_full_case(STACK_CASE, seed) plus 'sd_pos' = draw_mlp(D, seed) and 'pe' = None (the chain computes it)."""
    from tests import head_grads_ref as HR
    c = HR.draw_full_case(STACK_CASE, seed)
    c['sd_pos'] = draw_mlp(c['D'], seed)
    c['pe'] = None
    return c


def torch_fwd(sd, xyz):
    """The MLP in xyz's dtype on its device -> (pe, [h1 .. h4])."""
    h, hs = xyz, []
    for l, i in enumerate(LAYERS):
        h = h @ sd[f'mlp.{i}.weight'].to(xyz).T + sd[f'mlp.{i}.bias'].to(xyz)
        if l < 4:
            h = torch.relu(h)
            hs.append(h)
    return h, hs


def torch_bwd(sd, xyz, hs, dpe):
    """-> {key: gradient} of sum(pe * dpe), written out (no autograd), in dpe's dtype."""
    a = [xyz] + hs
    g, grads = dpe, {}
    for l in (4, 3, 2, 1, 0):
        if l < 4:
            g = g * (hs[l] > 0)
        grads[f'mlp.{LAYERS[l]}.weight'] = g.T @ a[l]
        grads[f'mlp.{LAYERS[l]}.bias'] = g.sum(0)
        if l > 0:
            g = g @ sd[f'mlp.{LAYERS[l]}.weight'].to(dpe)
    return grads


def stack_relu_margin(c):
    """The smallest |pre-activation| over the MLP's four ReLUs, the encoder's linear1 and the head's two ReLUs, in float64."""
    from tests import head_grads_ref as HR
    xyz = c['xyz'].double().numpy()
    r = forward(c['sd_pos'], xyz)
    return min(min(float(np.abs(z).min()) for z in r['z']), HR.relu_margin(dict(c, pe=torch.from_numpy(r['pe']))))


def full(c, dtype=torch.float64, device='cpu'):
    """head_grads_ref.full on the case with pe = MLP(xyz) evaluated in `dtype` on `device`, and the MLP's gradients from the dpe the
    cross-encoder restatement returns (the sum over the LN(x) + pe sites) -> head_grads_ref.full's dict, 'grads' with the ten
    'pos_embed.mlp.*' added."""
    from tests import cross_encoder_grads_ref as R
    from tests import head_grads_ref as HR
    xyz = c['xyz'].to(device=device, dtype=dtype)
    pe, hs = torch_fwd(c['sd_pos'], xyz)
    seen = {}
    stack = R.stack

    def spy(*a, **kw):
        seen['dpe'] = (r := stack(*a, **kw))['dpe']
        return r
    R.stack = spy                 # head_grads_ref.full calls it twice: the forward, then the backward with the real d_out (the dpe kept)
    try:
        out = HR.full(dict(c, pe=pe), dtype=dtype, device=device)
    finally:
        R.stack = stack
    out['grads'].update({'pos_embed.' + k: v for k, v in torch_bwd(c['sd_pos'], xyz, hs, seen['dpe']).items()})
    return out
