"""Restatement of everything above the KPConv backbone with a manual backward, written from the arithmetic in plain torch -- float64 on
the CPU is the yardstick of tests/test_gpu_head_grads.py and tests/test_head_grads_host.py; the same code in float32 on the GPU is the
independent float32 evaluation that test falls back on.  No autograd anywhere: every gradient is written out.

  * the correspondence regressor (regtr.py:399-443 of the reference): head_fwd / head_bwd;
  * nn.BCEWithLogitsLoss (mean): bce;
  * the whole chain feat_proj -> cross-encoder (tests/cross_encoder_grads_ref.py) -> regressor -> overlap BCE + InfoNCE (conditioned and
    unconditioned features) + CorrCriterion (both directions) -> the weighted total of regtr.py:292-293: full().

Also here: the two new kernels' arithmetic in float64 numpy with per-element bounds on |float32 kernel - float64| derived from the
operation counts of csrc/head_bwd.hip as written (first order in U = 2^-24), and the seeded inputs / parameters the golden files and
the tests draw alike (seeds are stored, matrices are not)."""
import os

import numpy as np
import torch

from tests import cross_encoder_grads_ref as R
from tests import loss_grads_ref as LR

U = 2.0 ** -24
TINY = 2.0 ** -149          # float32's subnormal quantum
NORMAL_MIN = 2.0 ** -126    # float32's smallest normal number
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

HEAD_KEYS = [('coor_mlp.0.weight', lambda D: (D, D)), ('coor_mlp.0.bias', lambda D: (D,)), ('coor_mlp.2.weight', lambda D: (D, D)),
             ('coor_mlp.2.bias', lambda D: (D,)), ('coor_mlp.4.weight', lambda D: (3, D)), ('coor_mlp.4.bias', lambda D: (3,)),
             ('conf_logits_decoder.weight', lambda D: (1, D)), ('conf_logits_decoder.bias', lambda D: (1,))]

# ------------------------------------------------------------------------------------------------ seeded cases
# The head alone: name -> D, cloud lengths (tokens N = their sum), decoder layers L', seed.
HEAD_CASES = {
    'ragged': dict(D=64, lens=[33, 64, 1, 129], L=1, seed=41),
    'kitchen': dict(D=256, lens=[410, 339], L=2, seed=42),
}
# The whole chain: name -> the loss golden whose key points / pose are used, widths, seed, and the loss weights of regtr.py:90-95
# (feature_un is given a weight so that its W receives a gradient).  The golden files (tools/make_golden_head_grads.py) hold the REAL
# reference modules' results for exactly these; every loss sits on the last of the L layers.  The kitchen case's nominal seed is 52; 67 is
# the first from there whose ReLU pre-activations all keep RELU_MARGIN from 0 (relu_margin below; 52 has one at 4.6e-7).
FULL_CASES = {
    '3dmatch_crop_b2': dict(D=64, H=2, F=128, L=2, K=128, pe=False, seed=51, wt=dict(overlap=1.0, feature=0.1, feature_un=0.05, corr=1.0)),
    '3dmatch_kitchen': dict(D=256, H=8, F=1024, L=2, K=128, pe=True, seed=67, wt=dict(overlap=1.0, feature=0.1, feature_un=0.05, corr=1.0)),
}


def draw_head(D, gen):
    """state_dict of a CorrespondenceRegressor (float32 CPU tensors, the reference's key order): weights N(0, 1 / fan_in), biases N(0, 0.1)."""
    sd = {}
    for key, shape in HEAD_KEYS:
        s = shape(D)
        t = torch.randn(s, generator=gen)
        sd[key] = t * s[1] ** -0.5 if len(s) == 2 else 0.1 * t
    return sd


def draw_head_case(name):
    """-> dict: 'sd', 'feats' (L, N, D), 'd_corr' (L, N, 3), 'd_logit' (L, N) the upstream gradients (the loss is sum(corr d_corr) +
    sum(logit d_logit))."""
    c = dict(HEAD_CASES[name])
    gen = torch.Generator().manual_seed(c['seed'])
    N = sum(c['lens'])
    c['sd'] = draw_head(c['D'], gen)
    c['feats'] = torch.randn((c['L'], N, c['D']), generator=gen)
    c['d_corr'] = torch.randn((c['L'], N, 3), generator=gen)
    c['d_logit'] = torch.randn((c['L'], N), generator=gen)
    return c


def draw_full_case(name, seed=None):
    """-> dict: the case's fields, the fixtures of tests/golden/losses_<name>.npz / loss_grads_<name>.npz ('src_kp', 'tgt_kp' lists, 'anc'
    the float32 anchors, 'pose' (B, 3, 4), 'r_p', 'r_n'), and from the seed, in this order: 'sd_proj' (feat_proj), 'sd_enc', 'sd_head',
    'W', 'W_un' (N(0, 0.1)), 'feats_un' (N, K) N(0, 1), 'gt' (N,) U(0, 1) with every fifth entry 0 and every seventh 1, and 'pe' (N, D)
    the sine embedding of the key points (None without).  Float32 CPU tensors."""
    c = dict(FULL_CASES[name])
    if seed is not None:
        c['seed'] = seed
    lg = np.load(os.path.join(GOLD, f'losses_{name}.npz'))
    gg = np.load(os.path.join(GOLD, f'loss_grads_{name}.npz'))
    B = int(lg['n_pairs'])
    c['B'] = B
    c['src_kp'] = [lg[f'src_kp_{b}'] for b in range(B)]
    c['tgt_kp'] = [lg[f'tgt_kp_{b}'] for b in range(B)]
    c['anc'] = [gg[f'anc_xyz_{b}'] for b in range(B)]
    c['pose'] = lg['pose'][:, :3, :].astype(np.float32)
    c['r_p'], c['r_n'] = float(lg['r_p']), float(lg['r_n'])
    c['src'], c['tgt'] = [len(x) for x in c['src_kp']], [len(x) for x in c['tgt_kp']]
    N = sum(c['src']) + sum(c['tgt'])
    D, K = c['D'], c['K']
    gen = torch.Generator().manual_seed(c['seed'])
    c['sd_proj'] = {'weight': torch.randn((D, K), generator=gen) * K ** -0.5, 'bias': 0.1 * torch.randn(D, generator=gen)}
    c['sd_enc'] = R.draw_params(D, c['F'], c['L'], True, gen)
    c['sd_head'] = draw_head(D, gen)
    c['W'] = torch.randn((D, D), generator=gen) * 0.1
    c['W_un'] = torch.randn((D, D), generator=gen) * 0.1
    c['feats_un'] = torch.randn((N, K), generator=gen)
    gt = torch.rand(N, generator=gen)
    gt[::5] = 0.0
    gt[::7] = 1.0
    c['gt'] = gt
    xyz = torch.from_numpy(np.concatenate(c['src_kp'] + c['tgt_kp']))
    c['xyz'] = xyz
    c['pe'] = R.posemb(xyz, D) if c['pe'] else None
    c['seg'], c['kv_self'], c['kv_cross'] = R.layout(c['src'], c['tgt'])
    c['max_len'] = max(c['src'] + c['tgt'])
    return c


# ------------------------------------------------------------------------------------------------ the pieces, forward and backward
def head_fwd(P, f):
    """f (M, D) -> (corr (M, 3), logit (M,), saved).  P: the regressor's parameters by their state_dict names."""
    h1 = torch.relu(f @ P['coor_mlp.0.weight'].T + P['coor_mlp.0.bias'])
    h2 = torch.relu(h1 @ P['coor_mlp.2.weight'].T + P['coor_mlp.2.bias'])
    corr = h2 @ P['coor_mlp.4.weight'].T + P['coor_mlp.4.bias']
    logit = (f @ P['conf_logits_decoder.weight'].T + P['conf_logits_decoder.bias'])[:, 0]
    return corr, logit, (f, h1, h2)


def head_bwd(P, saved, d_corr, d_logit, grads, pre=''):
    """-> df; the parameter gradients go into `grads` under pre + name."""
    f, h1, h2 = saved
    grads[pre + 'coor_mlp.4.weight'] = d_corr.T @ h2
    grads[pre + 'coor_mlp.4.bias'] = d_corr.sum(0)
    g2 = (d_corr @ P['coor_mlp.4.weight']) * (h2 > 0)
    grads[pre + 'coor_mlp.2.weight'] = g2.T @ h1
    grads[pre + 'coor_mlp.2.bias'] = g2.sum(0)
    g1 = (g2 @ P['coor_mlp.2.weight']) * (h1 > 0)
    grads[pre + 'coor_mlp.0.weight'] = g1.T @ f
    grads[pre + 'coor_mlp.0.bias'] = g1.sum(0)
    grads[pre + 'conf_logits_decoder.weight'] = d_logit[None, :] @ f
    grads[pre + 'conf_logits_decoder.bias'] = d_logit.sum().reshape(1)
    return g1 @ P['coor_mlp.0.weight'] + d_logit[:, None] * P['conf_logits_decoder.weight']


def run_head_case(c, dtype=torch.float64, device='cpu'):
    """head_fwd / head_bwd on a drawn case -> dict 'corr' (L, N, 3), 'logit' (L, N), 'df' (L, N, D), 'grads'."""
    t = lambda a: a.to(device=device, dtype=dtype)
    P = {k: t(v) for k, v in c['sd'].items()}
    Lyr, N, D = c['feats'].shape
    corr, logit, saved = head_fwd(P, t(c['feats']).reshape(Lyr * N, D))
    grads = {}
    df = head_bwd(P, saved, t(c['d_corr']).reshape(Lyr * N, 3), t(c['d_logit']).reshape(Lyr * N), grads)
    return {'corr': corr.view(Lyr, N, 3), 'logit': logit.view(Lyr, N), 'df': df.view(Lyr, N, D), 'grads': grads}


def bce(x, y):
    """mean BCEWithLogits(x, y) and its gradient in x, in the stable form max(x, 0) - x y + log1p(exp(-|x|))."""
    val = (torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-x.abs()))).mean()
    return val, (torch.sigmoid(x) - y) / x.numel()


def infonce(A, G, W, dec):
    """InfoNCELossFull (feature_loss.py:281-314) on per-pair lists A (anchors' features), G (positives'), with the decisions dec per pair
    (idx, mask, allowed) as bool / int64 tensors -> (loss, dA list, dG list, dW): tests/loss_grads_ref.py's infonce_grads in torch."""
    B = len(A)
    Wt = torch.triu(W)
    Ws = Wt + Wt.T
    losses, dA, dG = [], [], []
    dWs = torch.zeros_like(W)
    for b in range(B):
        a, g = A[b], G[b]
        idx, mask, allowed = dec[b]
        P = g @ Ws
        l = a @ P.T
        lm = torch.where(allowed, l, torch.full_like(l, -float('inf')))
        lse = torch.logsumexp(lm, 1)
        rows = torch.arange(len(a), device=a.device)
        li = lse - l[rows, idx]
        cnt = mask.sum().to(a.dtype)
        losses.append(li[mask].sum() / cnt)
        s = 1.0 / B / cnt
        dl = s * torch.exp(lm - lse[:, None])
        dl[rows, idx] -= s
        dl = dl * mask[:, None]
        dP = dl.T @ a
        dA.append(dl @ P)
        dG.append(dP @ Ws)
        dWs = dWs + g.T @ dP
    return torch.stack(losses).mean(), dA, dG, torch.triu(dWs + dWs.T)


def corr_l1(kp, warped, T, w):
    """CorrCriterion('mae') (corr_loss.py:18-40) over the concatenated pairs: kp / warped / w per-pair lists, T (B, 3, 4) -> (loss, d warped
    list)."""
    e = [warped[b] - (kp[b] @ T[b, :, :3].T + T[b, :, 3]) for b in range(len(kp))]
    den = torch.clamp(sum(x.sum() for x in w), min=1e-6)
    loss = sum((w[b] * e[b].abs().sum(1)).sum() for b in range(len(kp))) / den
    return loss, [w[b][:, None] * torch.sign(e[b]) / den for b in range(len(kp))]


def se3_inv(T):
    R = T[:, :, :3]
    return torch.cat([R.transpose(1, 2), -(R.transpose(1, 2) @ T[:, :, 3:])], 2)


def decisions(c, device='cpu'):
    """The InfoNCE decisions of the case's float32 anchors against the tgt key points, in the kernels' float32 distance arithmetic."""
    out = []
    for b in range(c['B']):
        idx, mask, allowed = LR.decisions(c['anc'][b], c['tgt_kp'][b], c['r_p'], c['r_n'])
        out.append((torch.from_numpy(idx).to(device), torch.from_numpy(mask).to(device), torch.from_numpy(allowed).to(device)))
    return out


RELU_MARGIN = 2.0 ** -19      # see relu_margin


def relu_margin(c):
    """The smallest |pre-activation| of any ReLU of the chain (the layers' linear1, the regressor's coor_mlp[0] and [2]) in float64.
    ReLU's derivative jumps at 0: a float32 forward and the float64 reference take different sides where |z| is below the forward's
    rounding error, and ONE such element moves every gradient upstream of it by the size of a single row's contribution (~1e-4 of the
    maximum at 750 tokens) -- a property of the input, not of the kernels.  The seeded cases are therefore required to keep every
    pre-activation at least RELU_MARGIN = 2^-19 (32 float32 ulps at |z| ~ 1/8 ... 1/4, several times the forward's observed error at
    these widths) away from 0; a case's seed is the first at or after its nominal one that does (tools/make_golden_head_grads.py stores
    the margin, tests/test_head_grads_host.py asserts it)."""
    t = lambda a: None if a is None else torch.as_tensor(a).double()
    sd = {k: t(v) for k, v in c['sd_enc'].items()}
    Ph = {k: t(v) for k, v in c['sd_head'].items()}
    x = t(c['feats_un']) @ t(c['sd_proj']['weight']).T + t(c['sd_proj']['bias'])
    m = float('inf')
    for li in range(c['L']):
        P = R._sub(sd, f'layers.{li}.')
        x, saved = R.layer_fwd(P, x, t(c['pe']), c['seg'], c['kv_self'], c['kv_cross'], c['H'])
        m = min(m, float((saved[3] @ P['linear1.weight'].T + P['linear1.bias']).abs().min()))
    last, _ = R.ln_fwd(x, sd['norm.weight'], sd['norm.bias'])
    z1 = last @ Ph['coor_mlp.0.weight'].T + Ph['coor_mlp.0.bias']
    z2 = torch.relu(z1) @ Ph['coor_mlp.2.weight'].T + Ph['coor_mlp.2.bias']
    return min(m, float(z1.abs().min()), float(z2.abs().min()))


def full(c, dtype=torch.float64, device='cpu'):
    """The whole chain on a drawn case (draw_full_case) in one dtype on one device -> dict: 'losses' {overlap, feature, feature_un, corr,
    total}, 'corr' (N, 3), 'logit' (N,) of the last layer, 'd_feats_un' (N, K), and 'grads' {name: gradient} under the prefixes
    'feat_proj.', 'transformer_encoder.', 'correspondence_decoder.' plus 'feature_criterion.W', 'feature_criterion_un.W'."""
    t = lambda a: None if a is None else torch.as_tensor(a).to(device=device, dtype=dtype)
    B, L, H, wt = c['B'], c['L'], c['H'], c['wt']
    seg = c['seg']
    n_src = int(seg[B])
    N = int(seg[-1])
    cut = lambda x, lo: [x[int(seg[lo + b]):int(seg[lo + b + 1])] for b in range(B)]
    Wp, bp = t(c['sd_proj']['weight']), t(c['sd_proj']['bias'])
    sd_enc = {k: t(v) for k, v in c['sd_enc'].items()}
    Ph = {k: t(v) for k, v in c['sd_head'].items()}
    W, W_un, gt, pe, fu = t(c['W']), t(c['W_un']), t(c['gt']), t(c['pe']), t(c['feats_un'])
    T = t(c['pose'])
    src_kp, tgt_kp = [t(x) for x in c['src_kp']], [t(x) for x in c['tgt_kp']]
    dec = decisions(c, device)

    x = fu @ Wp.T + bp
    d_zero = torch.zeros((L, N, c['D']), dtype=dtype, device=device)
    out = R.stack(sd_enc, x, pe, d_zero, seg, c['kv_self'], c['kv_cross'], H, L, True)['out']
    last = out[L - 1]
    corr, logit, saved = head_fwd(Ph, last)

    l_ov, d_logit = bce(logit, gt)
    l_f, dA, dG, dW = infonce(cut(last, 0), cut(last, B), W, dec)
    l_fu, dAu, dGu, dWu = infonce(cut(x, 0), cut(x, B), W_un, dec)
    l_cs, dws = corr_l1(src_kp, cut(corr, 0), T, cut(gt, 0))
    l_ct, dwt = corr_l1(tgt_kp, cut(corr, B), se3_inv(T), cut(gt, B))
    losses = {'overlap': l_ov, 'feature': l_f, 'feature_un': l_fu, 'corr': l_cs + l_ct}
    losses['total'] = sum(losses[k] * wt[k] for k in ('overlap', 'feature', 'feature_un', 'corr'))

    grads = {'feature_criterion.W': wt['feature'] * dW, 'feature_criterion_un.W': wt['feature_un'] * dWu}
    hg = {}
    d_last = head_bwd(Ph, saved, wt['corr'] * torch.cat(dws + dwt), wt['overlap'] * d_logit, hg, 'correspondence_decoder.')
    grads.update(hg)
    d_out = torch.zeros_like(d_zero)
    d_out[L - 1] = d_last + wt['feature'] * torch.cat(dA + dG)
    r = R.stack(sd_enc, x, pe, d_out, seg, c['kv_self'], c['kv_cross'], H, L, True)
    grads.update({'transformer_encoder.' + k: v for k, v in r['grads'].items()})
    dx = r['dx'] + wt['feature_un'] * torch.cat(dAu + dGu)
    grads['feat_proj.weight'] = dx.T @ fu
    grads['feat_proj.bias'] = dx.sum(0)
    return {'losses': losses, 'corr': corr, 'logit': logit, 'd_feats_un': dx @ Wp, 'grads': grads}


# ------------------------------------------------------------------------------------------------ the two kernels, with bounds
def head_tail_bwd(dcorr, dlogit, h2, f, w4, wc):
    """regtr_head_tail_bwd in float64 numpy -> dict 'g2', 'r', 'dw4', 'db4', 'dwc', 'dbc', 'db2' and bounds 'b_<name>' on |float32 kernel -
    float64| (first order in U).  dcorr / dlogit None: that side's outputs are exact zeros.  The kernel (csrc/head_bwd.hip):
      * g2 = h2 > 0 ? (dc0 W4[0] + dc1 W4[1]) + dc2 W4[2] : +0: three products and two additions, each rounded at most once (a fused
        multiply-add rounds less): every term passes through at most three roundings -> 3 U sum |dc_k W4[k]|; exact (+0) where h2 <= 0;
      * r = dl wc: ONE product, the correctly rounded float32 product -- 'r32' is that value, and the kernel's must equal it;
      * the column sums: a thread adds its ceil(chunk_rows(m) / TR) rows of a chunk in row order (TR = 256 / CW row lanes, CW = 64 float4
        columns per workgroup for D >= 256, else 16), each term a product rounded once (dW4, dwc), an already rounded g2 (db2, whose own
        error adds) or an input (db4, dbc); the TR lanes are added in order; the chunks in float64 with one rounding to float32."""
    h2, f, w4 = (np.asarray(a, dtype=np.float64) for a in (h2, f, w4))
    wc = np.asarray(wc, dtype=np.float64).reshape(-1)
    m, D = h2.shape
    TR = 256 // (64 if D // 4 >= 64 else 16)
    adds = (-(-R.chunk_rows(m) // TR) + TR) * U
    out = {}
    if dcorr is None:
        for k, s in (('g2', (m, D)), ('dw4', (3, D)), ('db4', (3,)), ('db2', (D,))):
            out[k], out['b_' + k] = np.zeros(s), np.zeros(s)
    else:
        dc = np.asarray(dcorr, dtype=np.float64)
        on = h2 > 0
        out['g2'] = np.where(on, dc @ w4, 0.0)
        out['b_g2'] = np.where(on, 3 * U * (np.abs(dc) @ np.abs(w4)), 0.0)
        out['dw4'] = dc.T @ h2
        out['b_dw4'] = (adds + U) * (np.abs(dc).T @ np.abs(h2))
        out['db4'] = dc.sum(0)
        out['b_db4'] = adds * np.abs(dc).sum(0)
        out['db2'] = out['g2'].sum(0)
        out['b_db2'] = out['b_g2'].sum(0) + adds * np.abs(out['g2']).sum(0)
    if dlogit is None:
        for k, s in (('r', (m, D)), ('dwc', (D,)), ('dbc', (1,))):
            out[k], out['b_' + k] = np.zeros(s), np.zeros(s)
        out['r32'] = np.zeros((m, D), dtype=np.float32)
    else:
        dl = np.asarray(dlogit, dtype=np.float64).reshape(m)
        out['r'] = dl[:, None] * wc[None, :]
        out['r32'] = out['r'].astype(np.float32)
        out['b_r'] = U * np.abs(out['r']) + TINY
        out['dwc'] = dl @ f
        out['b_dwc'] = (adds + U) * (np.abs(dl) @ np.abs(f))
        out['dbc'] = dl.sum().reshape(1)
        out['b_dbc'] = adds * np.abs(dl).sum().reshape(1)
    return out


def bce_logits_bwd(x, y, g):
    """regtr_bce_logits_bwd in float64 numpy -> dict 'd', 'b_d'.  The kernel: c = g / n (one rounding; n is exact in float32), e =
    expf(-|x|) (1 ulp = 2 U relative; below float32's normal range, |x| > 87, the hardware exponential may flush: an error of up to e
    itself), then
      s = 1 / (1 + e) for x >= 0, e / (1 + e) below: the addition (U, on top of e's error, which it sees at most halved) and the division
          (U): at most 5 U s;
      d = c (s - y): the subtraction (U |s - y|, after s's absolute error), the product (U), c's rounding (U); a result below the
          normal range may be flushed as well."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = x.size
    e = np.exp(-np.abs(x))
    s = np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    c = float(g) / n
    d = c * (s - y)
    e_s = 5 * U * s + np.where(e < NORMAL_MIN, e, 0.0)
    return {'d': d, 'b_d': abs(c) * (e_s + U * np.abs(s - y)) + 2 * U * np.abs(d) + np.where(np.abs(d) < NORMAL_MIN, np.abs(d), 0.0) + TINY}
