"""Float64 restatement (stock torch ops with autograd; CPU by default) of the three KPConv block kinds and the encoder (kpconv_blocks.py:533-567, 590-646, 649-741 and
kpconv.py:22-88 of the reference; regtr_amd/encoder_grad.py) for tests/test_gpu_backbone_grads.py and tests/test_backbone_grads_host.py,
and the seeded block cases both draw.

The network is piecewise smooth; its discrete choices are handed in as `sides`, so that the restatement differentiates the very branch
the float32 forward took (a weight gradient cannot mask one element out):
    masks     per LeakyReLU, the side of every element (True: argument > 0)
    winners   per max-pool, the winning column of every (query, channel), -1 where the zero shadow row won
    pos       per convolution, which support rows count in KPConv's neighbour number (feature row sum > 0; an integer, no gradient)
sides=None takes every choice from the float64 values themselves (the host test; the margins of a run are returned as 'margin').

A block is a dict: kind 'unary' | 'simple' | 'resnetb', strided, layer, extent, kp (15, 3), no_relu (unary), and the weights under the
module's parameter names ('mlp.weight' | 'KPConv.weights', 'unary1.mlp.weight', 'unary2.mlp.weight', 'unary_shortcut.mlp.weight').
meta: points[l] (N_l, 3), neighbors[l] / pools[l] (., H) integer tables with shadows >= N_l, lens[l], pool_width[l].
"""
import numpy as np
import torch

from tests import kpconv_grads_ref as KR
from tests.norm_pool_grads_ref import EPS32, SLOPE32

F64 = torch.float64
KP = 15


def t64(a, device='cpu', dtype=F64):
    """a as a tensor of `dtype` on `device`: float64, the yardstick, unless a caller asks for the float32 evaluation of the same code."""
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(device)


def inorm(x, lens, eps=EPS32):
    parts = []
    for seg in torch.split(x, [int(n) for n in lens]):
        if seg.shape[0]:
            m = seg.mean(0, keepdim=True)
            seg = (seg - m) / torch.sqrt(((seg - m) ** 2).mean(0, keepdim=True) + eps)
        parts.append(seg)
    return torch.cat(parts)


class _Sides:
    """Reads the given sides in call order, or records the float64 run's own (and their margins)."""

    def __init__(self, given):
        self.given = given
        self.i = {'masks': 0, 'winners': 0, 'pos': 0}
        self.own = {'masks': [], 'winners': [], 'pos': []}
        self.margin = float('inf')

    def take(self, kind, own):
        self.own[kind].append(own.cpu())
        if self.given is None or self.given.get(kind) is None:
            return own
        v = self.given[kind][self.i[kind]]
        self.i[kind] += 1
        return torch.as_tensor(np.asarray(v)).to(own.device)


def lrelu(z, sides, slope=SLOPE32):
    own = z.detach() > 0
    if z.numel():
        sides.margin = min(sides.margin, float(z.detach().abs().min()))
    mask = sides.take('masks', own).to(torch.bool)
    return z * torch.where(mask, 1.0, slope).to(z.dtype)


def max_pool(x, nbr, width, sides):
    ns, C = x.shape
    idx = nbr[:, :width].long()
    idx = torch.where((idx >= 0) & (idx < ns), idx, ns)
    vals = torch.cat([x, torch.zeros_like(x[:1])])[idx]                         # (Nq, width, C)
    d = vals.detach()
    col = d.argmax(1)
    own = torch.where(torch.gather(idx[:, :, None].expand(-1, -1, C), 1, col[:, None, :])[:, 0] < ns, col, -1)
    if d.shape[0] and width > 1:
        shadow = idx >= ns                                                      # (a row's second, third ... shadow is no rival of its first)
        dup = (shadow & (shadow.cumsum(1) > 1))[:, :, None]
        top = torch.where(dup, torch.full_like(d, -float('inf')), d).topk(2, dim=1).values
        sides.margin = min(sides.margin, float((top[:, 0] - top[:, 1]).min()))
    win = sides.take('winners', own).long()
    out = torch.gather(vals, 1, win.clamp(min=0)[:, None, :])[:, 0]
    return torch.where(win >= 0, out, torch.zeros_like(out))


def kpconv(q_pts, s_pts, nbr, x, W, kp, extent, sides):
    ns = x.shape[0]
    idx = nbr.long()
    real = (idx >= 0) & (idx < ns)
    idx = torch.where(real, idx, ns)
    rel = torch.cat([s_pts, torch.full_like(s_pts[:1], 1e6)])[idx] - q_pts[:, None, :]
    d2 = sum((rel[:, :, None, i] - kp[None, None, :, i]) ** 2 for i in range(3))
    w = torch.clamp(1.0 - torch.sqrt(d2) / extent, min=0.0) * real[:, :, None]  # (Nq, H, KP): KR.influences
    nx = torch.cat([x, torch.zeros_like(x[:1])])[idx]                           # (Nq, H, Cin)
    wf = torch.bmm(w.transpose(1, 2), nx)                                        # (Nq, KP, Cin)
    own = x.detach().sum(1) > 0
    pos = sides.take('pos', own).to(torch.bool)
    num = torch.cat([pos, torch.zeros_like(pos[:1])])[idx].sum(1).clamp(min=1).to(x.dtype)
    return (wf.reshape(wf.shape[0], -1) @ W.reshape(-1, W.shape[2])) / num[:, None]


def _view(blk, meta, device, dtype=F64):
    l, strided = blk['layer'], blk['strided']
    return dict(s_pts=t64(meta['points'][l], device, dtype), q_pts=t64(meta['points'][l + 1 if strided else l], device, dtype),
                inds=torch.as_tensor(np.asarray(meta['pools'][l] if strided else meta['neighbors'][l])).to(device),
                lens_pre=meta['lens'][l], lens_post=meta['lens'][l + 1 if strided else l],
                width=int(meta['pool_width'][l]) if strided else None)


def block_forward(blk, W, x, meta, sides):
    """One block on float64 rows x with the weight dict W (leaf tensors) -> output rows."""
    if blk['kind'] == 'unary':
        z = inorm(x @ W['mlp.weight'].t(), meta['lens'][blk['layer']])
        return z if blk.get('no_relu') else lrelu(z, sides)
    v = _view(blk, meta, x.device, x.dtype)
    kp = t64(blk['kp'], x.device, x.dtype)
    conv = lambda f: kpconv(v['q_pts'], v['s_pts'], v['inds'], f, W['KPConv.weights'], kp, blk['extent'], sides)
    if blk['kind'] == 'simple':
        return lrelu(inorm(conv(x), v['lens_post']), sides)
    f = x
    x1 = lrelu(inorm(f @ W['unary1.mlp.weight'].t(), v['lens_pre']), sides) if 'unary1.mlp.weight' in W else f
    y = lrelu(inorm(conv(x1), v['lens_post']), sides)
    y2 = inorm(y @ W['unary2.mlp.weight'].t(), v['lens_post'])
    sc = max_pool(f, v['inds'], v['width'], sides) if blk['strided'] else f
    if 'unary_shortcut.mlp.weight' in W:
        sc = inorm(sc @ W['unary_shortcut.mlp.weight'].t(), v['lens_post'])
    return lrelu(y2 + sc, sides)


WEIGHT_NAMES = ('mlp.weight', 'KPConv.weights', 'unary1.mlp.weight', 'unary2.mlp.weight', 'unary_shortcut.mlp.weight')


def run(blocks, x, meta, d_out, sides=None, x_grad=False, backward=True, device='cpu', dtype=F64):
    """Forward through `blocks` in order and backward of sum(out * d_out), all in `dtype` (float64).  d_out: an array, or a callable that is handed the
    forward's output (a detached tensor) and returns its upstream gradient -- what a loss computed ON that output needs
    (tests/training_step_ref.py).  dtype: torch.float32 evaluates the same code in float32.  sides: per block a dict (or None) of 'masks',
    'winners', 'pos' lists in call order.  -> dict 'out', 'grads' {(block index, weight name): array}, 'dx' (x_grad), 'margin', and
    'sides': the float64 run's own choices per block (same layout).  backward=False: the forward only ('out', 'margin', 'sides').
    device: where the float64 torch ops run -- 'cpu' (the host test pins this very code to finite differences there), or 'cuda' in the
    GPU tests (stock torch float64 ops; the full crop's encoder takes 12 s on 16 CPU threads)."""
    ws = [{k: t64(b[k], device, dtype).requires_grad_() for k in WEIGHT_NAMES if k in b} for b in blocks]
    x = t64(x, device, dtype)
    if x_grad:
        x.requires_grad_()
    cur, own, margin = x, [], float('inf')
    for i, (b, W) in enumerate(zip(blocks, ws)):
        s = _Sides(None if sides is None else sides[i])
        cur = block_forward(b, W, cur, meta, s)
        own.append({k: [np.asarray(a) for a in v] for k, v in s.own.items()})
        margin = min(margin, s.margin)
    if not backward:
        return {'out': cur.detach().cpu().numpy(), 'margin': margin, 'sides': own}
    d = d_out(cur.detach()).to(cur) if callable(d_out) else t64(d_out, device, dtype)
    (cur * d).sum().backward()
    return {'out': cur.detach().cpu().numpy(), 'grads': {(i, k): w.grad.cpu().numpy() for i, W in enumerate(ws) for k, w in W.items()},
            'dx': x.grad.cpu().numpy() if x_grad else None, 'margin': margin, 'sides': own}


# ------------------------------------------------------------------------------------------------ the encoder's block list
def encoder_blocks(cfg, sd, prefix='kpf_encoder.encoder_blocks.'):
    """The block dicts of KPFEncoder(cfg) (kpconv.py:22-88) with the weights of a state_dict (names under `prefix`)."""
    blocks, layer = [], 0
    r = cfg['first_subsampling_dl'] * cfg['conv_radius']
    for bi, name in enumerate(cfg['architecture']):
        if 'upsample' in name:
            break
        b = dict(kind='simple' if 'simple' in name else 'resnetb', strided='strided' in name, layer=layer,
                 extent=float(np.float32(r * cfg['KP_extent'] / cfg['conv_radius'])))
        for k, v in sd.items():
            if k.startswith(f'{prefix}{bi}.'):
                short = k[len(f'{prefix}{bi}.'):]
                if short == 'KPConv.kernel_points':
                    b['kp'] = np.asarray(v, dtype=np.float32)
                else:
                    b[short] = np.asarray(v, dtype=np.float32)
        blocks.append(b)
        if 'strided' in name or 'pool' in name:
            layer += 1
            r *= 2
    return blocks


def meta_of(kpconv_meta):
    """RegTR's kpconv_meta (device tensors) as the host arrays the restatement reads."""
    h = lambda t: t.detach().cpu().numpy()
    return dict(points=[h(p) for p in kpconv_meta['points']], neighbors=[h(t) for t in kpconv_meta['_neighbors_i32']],
                pools=[h(t) for t in kpconv_meta['_pools_i32']], lens=[list(l) for l in kpconv_meta['_lens_host']],
                pool_width=list(kpconv_meta['_pool_width']))


# ------------------------------------------------------------------------------------------------ seeded block cases
# Two levels of points in the unit cube: level 0 in clouds of lens0, level 1 a subsample (every `stride`-th point) with its own lens.
# `H`: table width; radius: neighbour radius at level 0 (twice that for the pool table).  pool_width < H, an all-shadow pool row (one
# level-1 point moved far away) and an in-degree-0 support (removed from every row) in the strided case.
LENS = [1, 0, 5, 300]
CASES = {
    'unary_lrelu': dict(kind='unary', Cin=64, Cout=32, seed=81, lens=LENS),
    'unary_plain': dict(kind='unary', Cin=32, Cout=128, seed=82, lens=LENS, no_relu=True),
    'simple_c1': dict(kind='simple', Cin=1, Cout=64, seed=83, lens=LENS, H=7, radius=0.22),
    'resnetb_lin': dict(kind='resnetb', Cin=64, Cout=128, seed=84, lens=LENS, H=40, radius=0.22),
    'resnetb_id': dict(kind='resnetb', Cin=128, Cout=128, seed=85, lens=LENS, H=7, radius=0.22),
    # identity unary1 (Cin == Cout / 4): the shortcut Linear hands the input on (plain) / autograd adds the pool's and the convolution's
    # gradients (strided)
    'resnetb_u1id': dict(kind='resnetb', Cin=32, Cout=128, seed=87, lens=LENS, H=7, radius=0.22),
    'resnetb_u1id_strided': dict(kind='resnetb', Cin=32, Cout=128, seed=88, lens=[1, 0, 5, 420], H=7, radius=0.2, strided=True, pool_width=5,
                                 stride=3),
    'resnetb_strided': dict(kind='resnetb', Cin=64, Cout=128, seed=86, lens=[1, 0, 5, 420], H=40, radius=0.2, strided=True, pool_width=33,
                            stride=3),
}
ORPHAN_OFFSET = 11          # the support (counted from the last cloud's start) that no pool row lists


def _tables(pts, lens, qpts, qlens, radius, H):
    """Per-cloud brute-force tables, indices global, shadows = total supports."""
    ns = pts.shape[0]
    nbr = np.full((qpts.shape[0], H), ns, dtype=np.int32)
    so = qo = 0
    for n, m in zip(lens, qlens):
        if n and m:
            t = KR.neighbours(qpts[qo:qo + m], pts[so:so + n], radius, H)
            nbr[qo:qo + m] = np.where(t < n, t + so, ns)
        so += n
        qo += m
    return nbr


def draw_case(name):
    """-> (block dict, meta, x (N, Cin) float32, d_out float32, case dict)."""
    c = dict(CASES[name], name=name)
    rng = np.random.default_rng(c['seed'])
    lens, Cin, Cout = c['lens'], c['Cin'], c['Cout']
    n = sum(lens)
    pts = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    meta = dict(points=[pts], lens=[lens], neighbors=[None], pools=[None], pool_width=[None])
    lin = lambda o, i: rng.uniform(-1, 1, (o, i)).astype(np.float32) * np.float32(i ** -0.5)
    if c['kind'] == 'unary':
        blk = dict(kind='unary', layer=0, strided=False, no_relu=bool(c.get('no_relu')))
        blk['mlp.weight'] = lin(Cout, Cin)
        x = rng.normal(0, 1, (n, Cin)).astype(np.float32)
        return blk, meta, x, rng.normal(0, 1, (n, Cout)).astype(np.float32), c
    H, R = c['H'], c['radius']
    meta['neighbors'][0] = _tables(pts, lens, pts, lens, R, H)
    n_out = n
    strided = bool(c.get('strided'))
    if strided:
        off = np.concatenate([[0], np.cumsum(lens)])
        keep = [np.arange(off[i], off[i + 1])[::c['stride']] for i in range(len(lens))]
        qlens = [len(k) for k in keep]
        qpts = pts[np.concatenate(keep)].copy()
        qpts[-2] += 50.0                                                        # an all-shadow pool row
        pool = _tables(pts, lens, qpts, qlens, 2 * R, H)
        orphan = int(off[-2]) + ORPHAN_OFFSET
        pool = KR._edit_rows(pool, n, drop=orphan)
        assert (pool[:, :c['pool_width']] >= n).all(1).any() and not (pool == orphan).any()
        assert (pool[:, c['pool_width']:] < n).any(), 'pool_width must cut real entries off'
        meta['points'].append(qpts); meta['lens'].append(qlens); meta['pools'][0] = pool; meta['pool_width'][0] = c['pool_width']
        meta['neighbors'].append(None); meta['pools'].append(None); meta['pool_width'].append(None)
        n_out = qpts.shape[0]
    v = rng.normal(0, 1, (KP, 3))
    kp = 0.6 * R * v / np.linalg.norm(v, axis=1, keepdims=True) * (2 if strided else 1)
    kp[0] = 0
    blk = dict(kind=c['kind'], layer=0, strided=strided, kp=kp.astype(np.float32), extent=float(np.float32(0.5 * R * (2 if strided else 1))))
    if c['kind'] == 'simple':
        blk['KPConv.weights'] = rng.normal(0, (KP * Cin) ** -0.5, (KP, Cin, Cout)).astype(np.float32)
        x = np.ones((n, 1), dtype=np.float32)
    else:
        mid = Cout // 4
        if Cin != mid:
            blk['unary1.mlp.weight'] = lin(mid, Cin)
        blk['KPConv.weights'] = rng.normal(0, (KP * mid) ** -0.5, (KP, mid, mid)).astype(np.float32)
        blk['unary2.mlp.weight'] = lin(Cout, mid)
        if Cin != Cout:
            blk['unary_shortcut.mlp.weight'] = lin(Cout, Cin)
        x = rng.normal(0, 1, (n, Cin)).astype(np.float32)
    return blk, meta, x, rng.normal(0, 1, (n_out, Cout)).astype(np.float32), c


def tiny_encoder_case(seed=91):
    """One cloud pair, two levels, C <= 16: simple -> resnetb -> resnetb_strided -> resnetb, for the finite-difference check."""
    rng = np.random.default_rng(seed)
    lens0 = [23, 19]
    n0 = sum(lens0)
    pts0 = rng.uniform(0, 1, (n0, 3)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(lens0)])
    keep = [np.arange(off[i], off[i + 1])[::2] for i in range(2)]
    lens1 = [len(k) for k in keep]
    pts1 = pts0[np.concatenate(keep)].copy()
    H, R = 6, 0.35
    meta = dict(points=[pts0, pts1], lens=[lens0, lens1],
                neighbors=[_tables(pts0, lens0, pts0, lens0, R, H), _tables(pts1, lens1, pts1, lens1, 2 * R, H)],
                pools=[_tables(pts0, lens0, pts1, lens1, R, H), None], pool_width=[5, None])

    def block(kind, strided, layer, cin, cout):
        r = R * (2 if layer else 1)
        v = rng.normal(0, 1, (KP, 3))
        kp = 0.6 * r * v / np.linalg.norm(v, axis=1, keepdims=True)
        kp[0] = 0
        b = dict(kind=kind, strided=strided, layer=layer, kp=kp.astype(np.float32), extent=float(np.float32(0.5 * r)))
        lin = lambda o, i: rng.uniform(-1, 1, (o, i)).astype(np.float32) * np.float32(i ** -0.5)
        if kind == 'simple':
            b['KPConv.weights'] = rng.normal(0, (KP * cin) ** -0.5, (KP, cin, cout)).astype(np.float32)
            return b
        mid = cout // 4
        if cin != mid:
            b['unary1.mlp.weight'] = lin(mid, cin)
        b['KPConv.weights'] = rng.normal(0, (KP * mid) ** -0.5, (KP, mid, mid)).astype(np.float32)
        b['unary2.mlp.weight'] = lin(cout, mid)
        if cin != cout:
            b['unary_shortcut.mlp.weight'] = lin(cout, cin)
        return b
    blocks = [block('simple', False, 0, 1, 4), block('resnetb', False, 0, 4, 8), block('resnetb', True, 0, 8, 8),
              block('resnetb', False, 1, 8, 16)]
    x = np.ones((n0, 1), dtype=np.float32)
    d_out = rng.normal(0, 1, (pts1.shape[0], 16)).astype(np.float32)
    return blocks, meta, x, d_out


# ------------------------------------------------------------------------------------------------ the reference-module golden's draws
INDEX_SEED, D_OUT_SEED, N_SAMPLE = 23, 29, 2048


def sample_indices(param_index, numel):
    """The flat gradient entries tools/make_golden_backbone_grads.py stores of the `param_index`-th trainable encoder parameter: all of
    them up to N_SAMPLE, else a seeded sorted sample without replacement.  Only the generator calls this: the golden stores the indices
    themselves and the test reads them there."""
    if numel <= N_SAMPLE:
        return np.arange(numel)
    return np.sort(np.random.default_rng([INDEX_SEED, param_index]).choice(numel, N_SAMPLE, replace=False))


def golden_d_out(shape):
    return np.random.default_rng(D_OUT_SEED).normal(0, 1, shape).astype(np.float32)
