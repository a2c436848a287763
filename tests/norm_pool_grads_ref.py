"""Float64 restatements of the backbone's InstanceNorm (+ LeakyReLU, + shortcut) and max-pool operators and their backward (BatchNormBlock
with nn.InstanceNorm1d, kpconv_blocks.py:489,510-519,556-561,741 and max_pool, :127-143 of the reference; csrc/norm.hip and kpconv.hip
forward, csrc/norm_pool_bwd.hip backward) for tests/test_gpu_norm_pool_grads.py and tests/test_norm_pool_grads_host.py, with the
per-element bound on |float32 kernels - float64| of the InstanceNorm gradient, a float32 ascending-entry-order restatement of the pool
backward (the kernel must equal it bit for bit), and the seeded cases both tests and tools/make_golden_norm_pool_grads.py draw.

InstanceNorm, per cloud segment (n rows) and channel, means over the segment's rows:
    xh = (x - mean(x)) rstd,  rstd = (var(x) + eps)^-1/2  (biased variance),   z = xh [+ r | + rh],   y = z > 0 ? z : slope z
    g  = dy (z > 0 ? 1 : slope),   dx = rstd (g - mean(g) - xh mean(g xh)),   dr = g  |  rrstd (g - mean(g) - rh mean(g rh)).
Max-pool: out[q, c] = max_h xp[nbr[q, h], c] over the first `width` columns, xp = x with a zero row for every index outside [0, Ns);
arg[q, c] = the lowest column holding the maximum (-1 when its row is the zero row); dx[s, c] = sum over (q, h) with nbr[q, h] = s and
arg[q, c] = h of dy[q, c].
"""
import numpy as np

U = 2.0 ** -24
SLOPE = 0.1
EPS = 1e-5
# what the kernels use (float arguments); the reference module uses the doubles 0.1 and 1e-5
SLOPE32, EPS32 = float(np.float32(SLOPE)), float(np.float32(EPS))

# ---- the InstanceNorm gradient's float32 error bound (first order in U, constants rounded up), from the kernels' operations as written.
# The restatement takes the float32 inputs, float32(slope), float32(eps) and the LeakyReLU mask as given and does everything else in float64; the
# kernels differ from it by these roundings (|float64 effects| of the one-pass variance and the chunk sums are ~1e-16 and not counted):
#   mean, rstd   stored as float32: U |mean|, U rstd
#   xh           (x - mean) rounded, times rstd rounded:            e_xh = U (C_XH |xh| + |mean| rstd)      C_XH = 3 roundings + 1
#   g            dy * slope rounded on the slope side, dy itself elsewhere:                      e_g = U |g|
#   mean(g)      float64 sums of the float32 g, one rounding to float32:                         e_m1 = mean(e_g) + U |m1|
#   mean(g xh)   float64 products and sums of float32 g and xh, one rounding:                    e_m2 = mean(|g| e_xh + e_g |xh|) + U |m2|
#   t = (g - m1) - xh m2    two subtractions and a product, each rounded (contraction is off in the kernel):
#                           e_t = e_g + e_m1 + U |g - m1| + e_xh |m2| + |xh| e_m2 + U |xh m2| + U |t|
#   dx = rstd t             e_dx = rstd e_t + C_RS U |dx|            C_RS = rstd's own rounding + the product's = 2
# and the same with r for a normalised shortcut's gradient; a plain shortcut's is g itself: e_g.
C_XH = 4
C_RS = 2
SECOND_ORDER = 1.001          # the terms dropped by "first order in U"


def in_rows(n_clouds, max_len, C):
    """Rows of one cloud per workgroup of the InstanceNorm launches (csrc/common.h rg_in_rows; tests/dispatch.py mirrors it)."""
    from tests import dispatch
    return dispatch.in_rows(n_clouds, max_len, C)


def edge_lens(C):
    """[1, 0, 5, R + 1]: a one-row cloud, an empty one, a short one and one that straddles a chunk of the R rows the launcher picks."""
    R = in_rows(4, 129, C)
    lens = [1, 0, 5, R + 1]
    assert in_rows(4, max(lens), C) == R
    return lens


# kind 'in': C, lens ('edge': edge_lens(C)), seed; `golden`: (lrelu, shortcut) of the stored reference run (clouds of >= 2 rows: the
# reference's nn.InstanceNorm1d refuses shorter ones).  kind 'pool': x (Ns, C), nbr (Nq, ld), the first `width` columns pooled.
#   orphan: support 5 is in no row.  hub: support 3 is in EVERY row (in-degree Nq > 64: the transposer's long-list regime).  dead: that
#   many query rows are all shadow.  full: no shadow anywhere in the first `width` columns, and x < 0: a negative maximum, the later
#   columns (shadows among them) must not be read.  ties: x drawn from five values, 0 (the shadow row's) among them.  neg_index: one
#   entry is -1, a shadow like Ns.
CASES = {
    'in_c4': dict(kind='in', C=4, lens='edge', seed=61),
    'in_c64': dict(kind='in', C=64, lens='edge', seed=62),
    'in_c256': dict(kind='in', C=256, lens='edge', seed=63),
    'in_c1024': dict(kind='in', C=1024, lens='edge', seed=64),
    'in_chunks': dict(kind='in', C=32, lens=[65 * 128 + 3, 200], seed=65),          # 66 chunks of 128 rows: beyond one wave of chunk lanes
    'in_g64': dict(kind='in', C=64, lens=[37, 2, 150], seed=66, golden=(True, 'none')),
    'in_g32': dict(kind='in', C=32, lens=[90, 61], seed=67, golden=(True, 'plain')),
    'in_g128': dict(kind='in', C=128, lens=[45, 77, 3], seed=68, golden=(True, 'normed')),
    'pool_h1': dict(kind='pool', C=4, Ns=53, Nq=37, ld=1, width=1, seed=71, dead=3),
    'pool_h7': dict(kind='pool', C=64, Ns=101, Nq=83, ld=7, width=7, seed=72, orphan=True, dead=2, golden=True),
    'pool_h40': dict(kind='pool', C=1024, Ns=61, Nq=70, ld=40, width=40, seed=73, hub=True, neg_index=True),
    'pool_width': dict(kind='pool', C=64, Ns=77, Nq=45, ld=9, width=5, seed=74, full=True, golden=True),
    'pool_ties': dict(kind='pool', C=64, Ns=40, Nq=59, ld=7, width=7, seed=75, ties=True, golden=True),
}
IN_CASES = [n for n, c in CASES.items() if c['kind'] == 'in']
POOL_CASES = [n for n, c in CASES.items() if c['kind'] == 'pool']
GOLDEN_CASES = [n for n, c in CASES.items() if c.get('golden')]
VARIANTS = [(lrelu, shortcut) for lrelu in (False, True) for shortcut in ('none', 'plain', 'normed')]
HUB, ORPHAN = 3, 5
TIE_VALUES = (-1.0, -0.5, 0.0, 0.5, 1.0)


def draw_case(name):
    """-> dict of the case's fields plus float32 / int32 numpy arrays.  'in': x, res, dy (N, C), lens, seg_off (n_clouds + 1,), max_len.
    'pool': x (Ns, C), nbr (Nq, ld), dy (Nq, C)."""
    c = dict(CASES[name], name=name)
    rng = np.random.default_rng(c['seed'])
    C = c['C']
    if c['kind'] == 'in':
        lens = edge_lens(C) if c['lens'] == 'edge' else list(c['lens'])
        N = sum(lens)
        # per-channel scales and offsets, so that the means are not small beside the deviations
        x = (rng.normal(0, 1, (N, C)) * rng.uniform(0.5, 1.5, C) + rng.normal(0, 2, C)).astype(np.float32)
        res = (rng.normal(0, 1, (N, C)) * rng.uniform(0.5, 1.5, C) + rng.normal(0, 1, C)).astype(np.float32)
        dy = rng.normal(0, 1, (N, C)).astype(np.float32)
        c.update(lens=lens, seg_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), max_len=max(lens), x=x, res=res, dy=dy)
        return c
    ns, nq, ld, width = c['Ns'], c['Nq'], c['ld'], c['width']
    if c.get('ties'):
        x = rng.choice(np.array(TIE_VALUES, dtype=np.float32), (ns, C))
    elif c.get('full'):
        x = (-np.abs(rng.normal(0, 1, (ns, C))) - 0.1).astype(np.float32)
    else:
        x = rng.normal(0, 1, (ns, C)).astype(np.float32)
    allowed = np.array([s for s in range(ns) if not (c.get('orphan') and s == ORPHAN) and not (c.get('hub') and s == HUB)])
    nbr = np.full((nq, ld), ns, dtype=np.int32)
    for q in range(nq):
        lo = width if c.get('full') else 0
        k = int(rng.integers(lo, ld + 1))
        row = list(rng.choice(allowed, size=min(k, ld - (1 if c.get('hub') else 0)), replace=False))
        if c.get('hub'):
            row.insert(int(rng.integers(0, len(row) + 1)), HUB)
        nbr[q, :len(row)] = row
    for i in range(c.get('dead', 0)):
        nbr[2 + 7 * i] = ns
    if c.get('neg_index'):
        nbr[1, ld - 1] = -1
    dy = rng.normal(0, 1, (nq, C)).astype(np.float32)
    c.update(x=x, nbr=nbr, dy=dy)
    real = (nbr >= 0) & (nbr < ns)
    if c.get('hub'):
        assert np.all((nbr == HUB).sum(1) == 1) and nq > 64
    if c.get('orphan'):
        assert not (nbr == ORPHAN).any()
    if c.get('dead'):
        assert (~real[:, :width]).all(1).sum() >= c['dead']
    if c.get('full'):
        assert real[:, :width].all() and (~real[:, width:]).any() and (x < 0).all()
    return c


# ------------------------------------------------------------------------------------------------ InstanceNorm
def instnorm_run(x, lens, dy, res=None, normed=False, lrelu=False, mask=None, slope=SLOPE, eps=EPS, bounds=False):
    """Forward and backward in float64 from the float32 inputs.  mask (N, C) bool: the LeakyReLU side of every element (True: z > 0) --
    None takes it from the float64 z; the GPU test passes the sign of the forward's own output.  -> dict 'out', 'z', 'dx', 'dres' (None
    without a shortcut); slope and eps are used as given (SLOPE32 / EPS32 to restate the kernels, SLOPE / EPS the reference module);
    bounds=True adds 'b_dx', 'b_dres' (the constants above)."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    r = None if res is None else np.asarray(res, np.float64)
    assert not (normed and r is None)
    out, z_all, dx = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    dres = None if r is None else np.zeros_like(x)
    b_dx, b_dres = np.zeros_like(x), None if r is None else np.zeros_like(x)
    o = 0
    for n in lens:
        sl = slice(o, o + n)
        o += n
        if n == 0:
            continue

        def norm(v):
            m = v.mean(0)
            rs = 1.0 / np.sqrt(((v - m) ** 2).mean(0) + eps)
            return m, rs, (v - m) * rs
        mean, rstd, xh = norm(x[sl])
        z = xh.copy()
        if r is not None:
            rmean, rrstd, rh = norm(r[sl]) if normed else (None, None, None)
            z += rh if normed else r[sl]
        pos = z > 0 if mask is None else np.asarray(mask[sl], bool)
        g = dy[sl] * np.where(pos, 1.0, slope) if lrelu else dy[sl]
        out[sl] = np.where(pos, z, slope * z) if lrelu else z
        z_all[sl] = z

        def grad(h, rs):
            m1, m2 = g.mean(0), (g * h).mean(0)
            return rs * (g - m1 - h * m2), m1, m2
        dx[sl], m1, m2 = grad(xh, rstd)
        if r is not None:
            dres[sl] = grad(rh, rrstd)[0] if normed else g
        if not bounds:
            continue
        e_g = U * np.abs(g) * (~pos if lrelu else np.zeros_like(pos))          # one rounding on the slope side, none elsewhere

        def bound(h, m, rs, d):
            _, m1_, m2_ = grad(h, rs)
            e_h = U * (C_XH * np.abs(h) + np.abs(m) * rs)
            e_m1 = e_g.mean(0) + U * np.abs(m1_)
            e_m2 = (np.abs(g) * e_h + e_g * np.abs(h)).mean(0) + U * np.abs(m2_)
            t = g - m1_ - h * m2_
            e_t = e_g + e_m1 + U * np.abs(g - m1_) + e_h * np.abs(m2_) + np.abs(h) * e_m2 + U * np.abs(h * m2_) + U * np.abs(t)
            return SECOND_ORDER * (rs * e_t + C_RS * U * np.abs(d))
        b_dx[sl] = bound(xh, mean, rstd, dx[sl])
        if r is not None:
            b_dres[sl] = bound(rh, rmean, rrstd, dres[sl]) if normed else SECOND_ORDER * e_g
    res_ = {'out': out, 'z': z_all, 'dx': dx, 'dres': dres}
    if bounds:
        res_.update(b_dx=b_dx, b_dres=b_dres)
    return res_


def torch_instance_norm(x, lens, res=None, normed=False, lrelu=False, slope=SLOPE, eps=EPS):
    """The same forward in stock torch ops (any dtype / device), statistics written out (a one-row cloud is legal here, unlike
    F.instance_norm): what autograd differentiates in the host test."""
    import torch

    def norm(v):
        parts = []
        for seg in torch.split(v, list(lens)):
            if seg.shape[0]:
                m = seg.mean(0, keepdim=True)
                parts.append((seg - m) / torch.sqrt(((seg - m) ** 2).mean(0, keepdim=True) + eps))
        return torch.cat(parts) if parts else v
    z = norm(x)
    if res is not None:
        z = z + (norm(res) if normed else res)
    return torch.nn.functional.leaky_relu(z, slope) if lrelu else z


# ------------------------------------------------------------------------------------------------ max-pool
def pool_run(x, nbr, width, dy):
    """Forward and backward in float64.  -> dict 'out' (Nq, C), 'arg' (Nq, C) int16 (lowest winning column, -1: the zero row won), 'dx'."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    ns, C = x.shape
    idx = np.asarray(nbr)[:, :width]
    real = (idx >= 0) & (idx < ns)
    idx = np.where(real, idx, ns)
    vals = np.concatenate([x, np.zeros((1, C))])[idx]                          # (Nq, width, C)
    col = vals.argmax(1) if len(idx) else np.zeros((0, C), np.int64)           # numpy keeps the FIRST maximum
    out = np.take_along_axis(vals, col[:, None, :], 1)[:, 0, :] if len(idx) else np.zeros((0, C))
    winner = np.take_along_axis(idx, col, 1) if len(idx) else col              # (Nq, C) support index of the winner
    dx = np.zeros((ns + 1, C))
    np.add.at(dx, (winner, np.arange(C)[None, :].repeat(len(idx), 0)), dy)
    return {'out': out, 'arg': np.where(winner < ns, col, -1).astype(np.int16), 'dx': dx[:ns]}


def pool_bwd_f32(dy, arg, nbr, width, ns):
    """The kernel's arithmetic restated: per element of dx a FLOAT32 sum, taken sequentially over the support's entries q width + h in
    ascending order, of (arg[q, c] == h ? dy[q, c] : +0).  -> (ns, C) float32, to be equalled bit for bit."""
    dy = np.asarray(dy, np.float32)
    dx = np.zeros((ns, dy.shape[1]), np.float32)
    idx = np.asarray(nbr)[:, :width]
    for q in range(idx.shape[0]):                                              # q-major, h-minor: ascending entries for every support
        for h in range(width):
            s = idx[q, h]
            if 0 <= s < ns:
                dx[s] = dx[s] + np.where(arg[q] == h, dy[q], np.float32(0))
    return dx


def torch_max_pool(x, nbr):
    """max_pool in stock torch ops (kpconv_blocks.py:127-143 with plain indexing; nbr int64, shadows = Ns)."""
    import torch
    return torch.cat([x, torch.zeros_like(x[:1])])[nbr].max(1)[0]
