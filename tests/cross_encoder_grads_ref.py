"""Restatement of the pre-norm cross-encoder (forward_pre of one layer, transformers.py:183-244 of the reference, and the stack with its
final norm, :37-59) on PACKED tokens with a manual backward, written from the arithmetic in plain torch -- float64 on the CPU is the
yardstick of tests/test_gpu_cross_encoder_grads.py and tests/test_cross_encoder_grads_host.py; the same code in float32 on the GPU is
the independent float32 evaluation that test falls back on.  No autograd anywhere: every gradient is written out.

Also here: the two new kernels' arithmetic in float64 with per-element bounds on |float32 kernel - float64| derived from the operation
counts of csrc/layer_bwd.hip as written (first order in U = 2^-24), and the seeded inputs / parameters the golden files and the tests
draw alike (seeds are stored, matrices are not).

Tokens: rows [seg[c], seg[c + 1]) are cloud c; the clouds are [src_0 .. src_{B-1}, tgt_0 .. tgt_{B-1}]; self-attention reads cloud c,
cross-attention the partner cloud of the pair."""
import math

import numpy as np
import torch

U = 2.0 ** -24
HD = 32

# ------------------------------------------------------------------------------------------------ seeded cases
# name -> D, heads, F, layers, (src lens, tgt lens), pe, final norm + return_intermediate, seed.  The golden files
# (tools/make_golden_cross_encoder_grads.py) hold the REAL reference module's results for exactly these.
CASES = {
    'ragged': dict(D=64, H=2, F=128, L=2, src=[33, 64], tgt=[1, 129], pe=False, final=False, seed=31),
    'kitchen': dict(D=256, H=8, F=1024, L=2, src=[410], tgt=[339], pe=True, final=True, seed=32),
}
LAYER_KEYS = [('self_attn.in_proj_weight', lambda D, F: (3 * D, D)), ('self_attn.in_proj_bias', lambda D, F: (3 * D,)),
              ('self_attn.out_proj.weight', lambda D, F: (D, D)), ('self_attn.out_proj.bias', lambda D, F: (D,)),
              ('multihead_attn.in_proj_weight', lambda D, F: (3 * D, D)), ('multihead_attn.in_proj_bias', lambda D, F: (3 * D,)),
              ('multihead_attn.out_proj.weight', lambda D, F: (D, D)), ('multihead_attn.out_proj.bias', lambda D, F: (D,)),
              ('linear1.weight', lambda D, F: (F, D)), ('linear1.bias', lambda D, F: (F,)),
              ('linear2.weight', lambda D, F: (D, F)), ('linear2.bias', lambda D, F: (D,)),
              ('norm1.weight', lambda D, F: (D,)), ('norm1.bias', lambda D, F: (D,)), ('norm2.weight', lambda D, F: (D,)),
              ('norm2.bias', lambda D, F: (D,)), ('norm3.weight', lambda D, F: (D,)), ('norm3.bias', lambda D, F: (D,))]


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def layout(src, tgt):
    """-> (seg_off (C + 1,), kv_self (C,), kv_cross (C,)) int32 arrays of the packed pair batch."""
    B = len(src)
    return offsets(list(src) + list(tgt)), np.arange(2 * B, dtype=np.int32), np.concatenate([np.arange(B, 2 * B), np.arange(B)]).astype(np.int32)


def draw_params(D, F, L, final, gen):
    """state_dict (float32 CPU tensors, the reference's key order) of an L-layer encoder: weights N(0, 1 / fan_in), biases and LayerNorm
    shifts N(0, 0.1), LayerNorm scales 1 + N(0, 0.1)."""
    sd = {}
    for li in range(L):
        for key, shape in LAYER_KEYS:
            s = shape(D, F)
            t = torch.randn(s, generator=gen)
            if len(s) == 2:
                t = t * s[1] ** -0.5
            elif key.startswith('norm') and key.endswith('weight'):
                t = 1.0 + 0.1 * t
            else:
                t = 0.1 * t
            sd[f'layers.{li}.{key}'] = t
    if final:
        sd['norm.weight'] = 1.0 + 0.1 * torch.randn(D, generator=gen)
        sd['norm.bias'] = 0.1 * torch.randn(D, generator=gen)
    return sd


def posemb(xyz, D, scale=1.0, temperature=10000.0):
    """A sine embedding of coordinates (N, 3) -> (N, D) float32 (the layout of position_embedding.py:29-50; here only an input)."""
    npf = D // 3 // 2 * 2
    f = np.arange(npf)
    dim_t = temperature ** (2 * (f // 2) / npf)
    p = xyz.double().numpy()[:, :, None] * scale / dim_t
    e = np.where(f % 2 == 0, np.sin(p), np.cos(p)).reshape(len(xyz), 3 * npf)
    return torch.from_numpy(np.pad(e, ((0, 0), (0, D - 3 * npf))).astype(np.float32))


def draw_case(name):
    """-> dict: cfg fields, 'sd' (state_dict), 'x' (N, D), 'pe' (N, D) | None, 'd_out' (L | 1, N, D) the upstream gradient of the output (the
    loss is sum(out * d_out)), 'seg', 'kv_self', 'kv_cross' -- float32 CPU tensors / int32 arrays from the case's seed."""
    c = dict(CASES[name])
    gen = torch.Generator().manual_seed(c['seed'])
    N = sum(c['src']) + sum(c['tgt'])
    c['sd'] = draw_params(c['D'], c['F'], c['L'], c['final'], gen)
    c['x'] = torch.randn((N, c['D']), generator=gen)
    c['pe'] = posemb(torch.rand((N, 3), generator=gen) * 2.0, c['D'], scale=2 * math.pi) if c['pe'] else None
    c['d_out'] = torch.randn((c['L'] if c['final'] else 1, N, c['D']), generator=gen)
    c['seg'], c['kv_self'], c['kv_cross'] = layout(c['src'], c['tgt'])
    c['max_len'] = max(c['src'] + c['tgt'])
    return c


# ------------------------------------------------------------------------------------------------ the pieces, forward and backward
def ln_fwd(x, gamma, beta, eps=1e-5):
    mean = x.mean(1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(1, keepdim=True) + eps)
    xh = xc * rstd
    return xh * gamma + beta, (xh, rstd)


def ln_bwd(saved, gamma, dy):
    xh, rstd = saved
    g = dy * gamma
    dx = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


def mha_fwd(q, k, v, seg, kv_of, H):
    """softmax(q k^T / sqrt(32)) v per head and cloud; a cloud attending an empty cloud gets zero rows."""
    o = torch.zeros_like(q)
    saved = []
    for c in range(len(kv_of)):
        qs, ks = slice(int(seg[c]), int(seg[c + 1])), slice(int(seg[kv_of[c]]), int(seg[kv_of[c] + 1]))
        if qs.stop == qs.start or ks.stop == ks.start:
            saved.append(None)
            continue
        heads = lambda t, s: t[s].reshape(s.stop - s.start, H, HD).transpose(0, 1)
        Q, K, V = heads(q, qs), heads(k, ks), heads(v, ks)
        P = torch.softmax(Q @ K.transpose(1, 2) * HD ** -0.5, -1)
        o[qs] = (P @ V).transpose(0, 1).reshape(qs.stop - qs.start, H * HD)
        saved.append((qs, ks, Q, K, V, P))
    return o, saved


def mha_bwd(saved, d_o, H):
    dq, dk, dv = torch.zeros_like(d_o), torch.zeros_like(d_o), torch.zeros_like(d_o)
    for ent in saved:
        if ent is None:
            continue
        qs, ks, Q, K, V, P = ent
        nq, nk = qs.stop - qs.start, ks.stop - ks.start
        G = d_o[qs].reshape(nq, H, HD).transpose(0, 1)
        dP = G @ V.transpose(1, 2)
        dS = P * (dP - (P * dP).sum(-1, keepdim=True))
        flat = lambda t, n: t.transpose(0, 1).reshape(n, H * HD)
        dq[qs] = flat(dS @ K, nq) * HD ** -0.5
        dk[ks] += flat(dS.transpose(1, 2) @ Q, nk) * HD ** -0.5
        dv[ks] += flat(P.transpose(1, 2) @ G, nk)
    return dq, dk, dv


def _attn_fwd(P, attn, norm, x, pe, seg, kv_of, H):
    x2, ln = ln_fwd(x, P[norm + '.weight'], P[norm + '.bias'])
    x2p = x2 if pe is None else x2 + pe
    D = x.shape[1]
    qkv = x2p @ P[attn + '.in_proj_weight'].T + P[attn + '.in_proj_bias']
    o, core = mha_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], seg, kv_of, H)
    y = x + o @ P[attn + '.out_proj.weight'].T + P[attn + '.out_proj.bias']
    return y, (ln, x2p, o, core)


def _attn_bwd(P, attn, norm, saved, dy, H, grads, pre):
    ln, x2p, o, core = saved
    grads[pre + attn + '.out_proj.weight'] = dy.T @ o
    grads[pre + attn + '.out_proj.bias'] = dy.sum(0)
    dqkv = torch.cat(mha_bwd(core, dy @ P[attn + '.out_proj.weight'], H), 1)
    grads[pre + attn + '.in_proj_weight'] = dqkv.T @ x2p
    grads[pre + attn + '.in_proj_bias'] = dqkv.sum(0)
    dx2p = dqkv @ P[attn + '.in_proj_weight']
    dx, grads[pre + norm + '.weight'], grads[pre + norm + '.bias'] = ln_bwd(ln, P[norm + '.weight'], dx2p)
    return dy + dx, dx2p


def layer_fwd(P, x, pe, seg, kv_self, kv_cross, H):
    """forward_pre of one layer (value carries pe).  P: the layer's parameters by their state_dict names.  -> (y, saved)."""
    x1, s1 = _attn_fwd(P, 'self_attn', 'norm1', x, pe, seg, kv_self, H)
    x2, s2 = _attn_fwd(P, 'multihead_attn', 'norm2', x1, pe, seg, kv_cross, H)
    x2n, ln3 = ln_fwd(x2, P['norm3.weight'], P['norm3.bias'])
    h = torch.relu(x2n @ P['linear1.weight'].T + P['linear1.bias'])
    y = x2 + h @ P['linear2.weight'].T + P['linear2.bias']
    return y, (s1, s2, ln3, x2n, h)


def layer_bwd(P, saved, dy, H, grads, pre=''):
    """-> (dx, dpe); the parameter gradients go into `grads` under pre + name."""
    s1, s2, ln3, x2n, h = saved
    grads[pre + 'linear2.weight'] = dy.T @ h
    grads[pre + 'linear2.bias'] = dy.sum(0)
    dh = (dy @ P['linear2.weight']) * (h > 0)
    grads[pre + 'linear1.weight'] = dh.T @ x2n
    grads[pre + 'linear1.bias'] = dh.sum(0)
    dx2, grads[pre + 'norm3.weight'], grads[pre + 'norm3.bias'] = ln_bwd(ln3, P['norm3.weight'], dh @ P['linear1.weight'])
    dx1, dpe2 = _attn_bwd(P, 'multihead_attn', 'norm2', s2, dy + dx2, H, grads, pre)
    dx, dpe1 = _attn_bwd(P, 'self_attn', 'norm1', s1, dx1, H, grads, pre)
    return dx, dpe1 + dpe2


def _sub(sd, pre):
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


def stack(sd, x, pe, d_out, seg, kv_self, kv_cross, H, L, return_intermediate):
    """The L-layer encoder and the backward of sum(out * d_out).  sd: state_dict ('layers.<i>.*', optional 'norm.*'), tensors of ONE dtype
    and device, which the whole evaluation keeps.  -> dict: 'out' (L | 1, N, D), 'dx', 'dpe', 'acts' (the layers' outputs), 'grads'
    {state_dict name: gradient}."""
    final = 'norm.weight' in sd
    acts, saved, outs, lns = [], [], [], {}
    for li in range(L):
        x, s = layer_fwd(_sub(sd, f'layers.{li}.'), x, pe, seg, kv_self, kv_cross, H)
        acts.append(x)
        saved.append(s)
        if return_intermediate or li == L - 1:
            if final:
                y, lns[li] = ln_fwd(x, sd['norm.weight'], sd['norm.bias'])
                outs.append(y)
            else:
                outs.append(x)
    out = torch.stack(outs)
    grads = {}
    if final:
        grads['norm.weight'], grads['norm.bias'] = torch.zeros_like(sd['norm.weight']), torch.zeros_like(sd['norm.bias'])
    dx = torch.zeros_like(x)
    dpe = torch.zeros_like(x)
    for li in reversed(range(L)):
        if return_intermediate or li == L - 1:
            g = d_out[li if return_intermediate else 0]
            if final:
                g, dg, db = ln_bwd(lns[li], sd['norm.weight'], g)
                grads['norm.weight'] = grads['norm.weight'] + dg
                grads['norm.bias'] = grads['norm.bias'] + db
            dx = dx + g
        dx, dp = layer_bwd(_sub(sd, f'layers.{li}.'), saved[li], dx, H, grads, f'layers.{li}.')
        dpe = dpe + dp
    return {'out': out, 'dx': dx, 'dpe': dpe, 'acts': acts, 'grads': grads}


def run_case(c, dtype=torch.float64, device='cpu', layers=None):
    """stack() on a drawn case (draw_case) in the given dtype / device; layers: only the first `layers` layers, without the final norm
    when layers == 1 (the single-layer test), d_out's first slice as the upstream gradient."""
    t = lambda a: None if a is None else a.to(device=device, dtype=dtype)
    sd = {k: t(v) for k, v in c['sd'].items()}
    L, ri, d_out = c['L'], c['final'], t(c['d_out'])
    if layers == 1:
        sd = {k: v for k, v in sd.items() if k.startswith('layers.0.')}
        L, ri, d_out = 1, False, d_out[:1]
    return stack(sd, t(c['x']), t(c['pe']), d_out, c['seg'], c['kv_self'], c['kv_cross'], c['H'], L, ri)


# ------------------------------------------------------------------------------------------------ the two kernels, with bounds
def chunk_rows(n):
    """csrc/layer_bwd.hip, bwd_chunk_rows: rows per workgroup of both first passes."""
    return max(32, 4 * -(-max(n, 1) // 4096))


def layernorm_fwd(x, gamma, beta, add=None, eps=1e-5):
    """regtr_layernorm in float64 numpy -> dict 'y' (with add), 'plain' (before it) and the bounds 'b_y', 'b_plain' on |float32 kernel -
    float64|.  The kernel (csrc/norm.hip, k_layernorm: one wave per row, two passes for the moments, a third for the output):
      * a row sum: a lane adds its ceil(D / 256) float4 groups (3 additions each), six shuffle levels follow, then the division by D:
        d = ceil(D / 256) + 9 roundings, each at most gamma_d = d U / (1 - d U) of the sum of magnitudes in all;
      * mean^ = sum / D:                     e_mean = gamma_d mean|x|
      * xc^ = x - mean^ (U):                  e_xc = e_mean + U (|xc| + e_mean)
      * var^ = sum xc^2 / D: the squares of the perturbed xc^ (U each, or none where the compiler fuses), the sum as above:
                                              e_var = mean(2 |xc| e_xc + e_xc^2) + gamma_(d + 1) mean((|xc| + e_xc)^2)
      * rstd^ = 1 / sqrtf(var^ + eps): the addition, the square root and the division are correctly rounded (U each, the radicand's U
        halved by the root: 3 U covers them); the radicand's absolute error e_var moves rstd into [rstd(var + e_var), rstd(max(var - e_var, 0))]
        -- taken exactly, not to first order: the stress case is a constant row, var = 0,
        where rstd = 1 / sqrt(eps) and a first-order quotient e_var / (var + eps) is all there is;
      * y = xc^ rstd^ gamma + beta (+ add): the error of the product xc rstd, |gamma| times it, then one U per operation on the
        magnitude at hand (two products, the addition of beta; the addition of `add` for y).
    The amplification of the mean's error by rstd |gamma| is the term that matters: a row offset by 100 with unit spread loses
    100 d U rstd |gamma| however exact the rest is."""
    x, gamma, beta = (np.asarray(a, dtype=np.float64) for a in (x, gamma, beta))
    n, D = x.shape
    d = -(-D // 256) + 9
    gam = lambda k: k * U / (1 - k * U)
    m = lambda a: a.mean(1, keepdims=True)
    mean = m(x)
    xc = x - mean
    var = m(xc * xc)
    rstd = 1.0 / np.sqrt(var + eps)
    e_mean = gam(d) * m(np.abs(x))
    e_xc = e_mean + U * (np.abs(xc) + e_mean)
    e_var = m(2 * np.abs(xc) * e_xc + e_xc * e_xc) + gam(d + 1) * m((np.abs(xc) + e_xc) ** 2)
    r_hi = 1.0 / np.sqrt(np.maximum(var - e_var, 0.0) + eps)
    r_lo = 1.0 / np.sqrt(var + e_var + eps)
    e_rstd = np.maximum(r_hi - rstd, rstd - r_lo) + 3 * U * r_hi
    t = xc * rstd
    e_t = e_xc * r_hi + np.abs(xc) * e_rstd
    ag = np.abs(gamma)[None, :]
    plain = t * gamma + beta
    e_plain = e_t * ag + 2 * U * (np.abs(t) + e_t) * ag + U * (np.abs(plain) + e_t * ag)
    e_plain = e_plain * (1 + 4 * U)                             # (the second-order products of the three U above)
    out = {'plain': plain, 'b_plain': e_plain, 'rstd': rstd}
    if add is None:
        out['y'], out['b_y'] = plain, e_plain
    else:
        y = plain + np.asarray(add, dtype=np.float64)
        out['y'], out['b_y'] = y, e_plain + U * (np.abs(y) + e_plain)
    return out


def layernorm_bwd(x, gamma, dy, dres=None, eps=1e-5):
    """regtr_layernorm_bwd in float64 numpy -> dict 'dx', 'dgamma', 'dbeta' and the bounds 'b_dx', 'b_dgamma', 'b_dbeta' on
    |float32 kernel - float64|, first order in U.  The kernel, per row (one wave, D / 4 float4 column groups dealt to 64 lanes):
      * every row sum: a lane adds its ceil(D / 256) float4 groups (3 additions each), six shuffle levels follow, then the division by D:
        d = ceil(D / 256) + 9 roundings on the sum of magnitudes;
      * mean^, then xc = x - mean^ (U), var^ = sum xc^2 / D (the square U, the sum d), rstd = 1 / sqrtf(var^ + eps): the addition U, sqrtf
        2 U (1 ulp taken), the division U, half of the radicand's relative error;
      * xh = xc rstd (U); g = dy gamma (U); c1 = sum g / D, c2 = sum g xh / D (the product U, sums d);
      * dx = rstd (g - c1 - xh c2) [+ dres]: the product xh c2 (U), two subtractions, the product with rstd, the addition.
    Columns: a wave adds its rows of the chunk in row order (chunk_rows(n) / 4 of them), the four waves are added in order (3), the
    chunks in float64 with one rounding to float32 (1)."""
    x, gamma, dy = (np.asarray(a, dtype=np.float64) for a in (x, gamma, dy))
    n, D = x.shape
    d = -(-D // 256) + 9
    m = lambda a: a.mean(1, keepdims=True)
    mean = m(x)
    xc = x - mean
    var = m(xc * xc)
    rstd = 1.0 / np.sqrt(var + eps)
    xh = xc * rstd
    g = dy * gamma
    c1, c2 = m(g), m(g * xh)
    dx_ln = rstd * (g - c1 - xh * c2)
    dx = dx_ln + (0 if dres is None else np.asarray(dres, dtype=np.float64))
    e_mean = d * U * m(np.abs(x))
    e_xc = e_mean + U * np.abs(xc)
    e_var = m(2 * np.abs(xc) * e_xc + U * xc * xc) + d * U * var
    r_rstd = 0.5 * e_var / (var + eps) + 4 * U
    e_xh = rstd * e_xc + np.abs(xh) * (r_rstd + U)
    ag = np.abs(g)
    e_c1 = (d + 1) * U * m(ag)
    e_c2 = m(ag * e_xh + 2 * U * ag * np.abs(xh)) + d * U * m(ag * np.abs(xh))
    e_t = (U * ag + e_c1 + e_xh * np.abs(c2) + np.abs(xh) * e_c2 + U * np.abs(xh * c2)
           + 2 * U * (ag + np.abs(c1) + np.abs(xh * c2)))
    b_dx = rstd * e_t + np.abs(dx_ln) * (r_rstd + U) + U * np.abs(dx)
    rpw = -(-chunk_rows(n) // 4)
    ady = np.abs(dy)
    return {'dx': dx, 'dgamma': (dy * xh).sum(0), 'dbeta': dy.sum(0), 'b_dx': b_dx,
            'b_dgamma': (ady * e_xh + U * ady * np.abs(xh)).sum(0) + (rpw + 4) * U * (ady * np.abs(xh)).sum(0),
            'b_dbeta': (rpw + 4) * U * ady.sum(0)}


def bias_relu_bwd(g, h=None):
    """regtr_bias_relu_bwd in float64 numpy -> dict 'dh' (exact in float32: a selection), 'db', 'b_db'.  A thread adds its rows of the
    chunk in row order (chunk_rows(n) / TR of them, TR = 256 / CW row lanes, CW = 64, 32 or 16 float4 columns per workgroup by N), the
    TR lanes are added in order, the chunks in float64 with one rounding."""
    g = np.asarray(g, dtype=np.float64)
    n, N = g.shape
    dh = g if h is None else np.where(np.asarray(h) > 0, g, 0.0)
    TR = 256 // (64 if N // 4 >= 64 else (32 if N // 4 >= 32 else 16))
    return {'dh': dh, 'db': dh.sum(0), 'b_db': (-(-chunk_rows(n) // TR) + TR) * U * np.abs(dh).sum(0)}
