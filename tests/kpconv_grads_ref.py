"""Float64 restatement of the KPConv operator and its backward (rigid, linear influence, sum aggregation: kpconv_blocks.py:269-414 of the
reference; regtr_kpconv_gather + the contraction forward, csrc/kpconv_bwd.hip backward) for tests/test_gpu_kpconv_grads.py and
tests/test_kpconv_grads_host.py, with per-element bounds on |float32 kernels - float64| and the seeded cases both tests and
tools/make_golden_kpconv_grads.py draw.

    infl[q,h,k] = max(0, 1 - |s[nbr[q,h]] - q_pts[q] - kp[k]| / extent)          (a shadow entry, nbr >= Ns, sits at 1e6: infl = 0)
    wf[q,k,c]   = sum_h infl[q,h,k] x[nbr[q,h], c]                                (a shadow entry's feature row is 0)
    num[q]      = max(1, #{h : sum_c x[nbr[q,h], c] > 0})                         (an integer count: no gradient)
    out[q,o]    = sum_{k,c} wf[q,k,c] W[k,c,o] / num[q]
With g = d_out / num:  dW[k,c,o] = sum_q wf[q,k,c] g[q,o],  dwf[q,k,c] = sum_o g[q,o] W[k,c,o],
dx[s,c] = sum_{(q,h): nbr[q,h] = s} sum_k infl[q,h,k] dwf[q,k,c].
"""
import numpy as np

U = 2.0 ** -24
KP = 15

# ---- the bounds' constants (first order in U), from the kernels' operation counts as written:
# influences: the forward's documented error of one float32 influence against float64 (csrc/kpconv.hip: uncontracted squared distance,
# 1-ulp hardware square root, precomputed float32 1 / extent) -- absolute, also where one side clamps to 0 and the other does not
E_INFL = 2e-7
# wf: an H-term float32 fma / MFMA chain over the neighbours: (H + 1) U of the sum of magnitudes, plus E_INFL per neighbour feature
# g = d_out / num: one IEEE division, U relative
# dW: MFMA sums over row chunks (at most Nq terms in all), a float64 sum of the chunks, one rounding to float32, and g's own U
C_DW = 4            # (Nq + C_DW) U: Nq chain terms + g + final rounding + the chunk combination, rounded up
# dwf = g W^T: a Cout-term contraction, exact-f32 MFMA or the bf16x3 split (include/regtr_hip.h: operands split exactly, the dropped
# cross terms below one float32 ulp = 2 U of each product; 4 U taken), g's U, the final rounding
C_DWF = 6           # (Cout + C_DWF) U
# dx: one fma per (entry, kernel point) in a chain of 15 deg terms, then a tree of at most 6 additions across lanes
C_DX = 8            # (15 deg + C_DX) U, rounded up

# Seeded cases.  `strided`: the queries are a separate, smaller cloud (Nq < Ns, not a subset of the supports).  `hub`: support 3 is put into
# EVERY query's row (in-degree Nq: beyond one wave's 64 entries, unbounded by H).  `orphan`: support 5 is removed from every row.
# `dead_rows`: that many queries are moved far away, their rows are all shadow.  Nq / Ns are multiples of no tile size (4, 16, 32, 64).
CASES = {
    'c1': dict(Cin=1, Cout=64, Ns=211, Nq=211, H=13, radius=0.30, seed=41),
    'c32': dict(Cin=32, Cout=32, Ns=203, Nq=203, H=40, radius=0.30, seed=42, orphan=True, dead_rows=3),
    'c64': dict(Cin=64, Cout=64, Ns=157, Nq=157, H=37, radius=0.33, seed=43, hub=True),
    'strided': dict(Cin=128, Cout=128, Ns=301, Nq=97, H=23, radius=0.36, seed=44, strided=True, orphan=True),
    'c256': dict(Cin=256, Cout=256, Ns=67, Nq=67, H=11, radius=0.45, seed=45),
}
HUB, ORPHAN = 3, 5


def neighbours(q_pts, s_pts, radius, H):
    """Brute force: per query the supports with d < radius, nearest first (ties by index), the first H of them; rows padded with the
    shadow index Ns.  -> (Nq, H) int32"""
    ns = s_pts.shape[0]
    d2 = ((q_pts[:, None, :].astype(np.float64) - s_pts[None].astype(np.float64)) ** 2).sum(-1)
    nbr = np.full((q_pts.shape[0], H), ns, dtype=np.int32)
    for q in range(q_pts.shape[0]):
        idx = np.nonzero(d2[q] < radius * radius)[0]
        idx = idx[np.argsort(d2[q, idx], kind='stable')][:H]
        nbr[q, :len(idx)] = idx
    return nbr


def _edit_rows(nbr, ns, drop=None, first=None):
    """Rows without `drop`, with `first` in front (once), still H wide and shadow padded."""
    out = np.full_like(nbr, ns)
    for q in range(nbr.shape[0]):
        row = [int(i) for i in nbr[q] if i < ns and i != drop and i != first]
        if first is not None:
            row = [first] + row
        row = row[:nbr.shape[1]]
        out[q, :len(row)] = row
    return out


def draw_case(name):
    """-> dict of the case's fields plus float32 / int32 numpy arrays: q_pts (Nq, 3), s_pts (Ns, 3), nbr (Nq, H), kernel_points (15, 3),
    extent (a float32-representable float), weights (15, Cin, Cout), x (Ns, Cin), d_out (Nq, Cout)."""
    c = dict(CASES[name], name=name)
    rng = np.random.default_rng(c['seed'])
    ns, nq, H, Cin, Cout, R = c['Ns'], c['Nq'], c['H'], c['Cin'], c['Cout'], c['radius']
    s_pts = rng.uniform(0, 1, (ns, 3)).astype(np.float32)
    q_pts = rng.uniform(0, 1, (nq, 3)).astype(np.float32) if c.get('strided') else s_pts.copy()
    for i in range(c.get('dead_rows', 0)):
        q_pts[7 + 11 * i] += 50.0
    nbr = neighbours(q_pts, s_pts, R, H)
    if c.get('orphan') or c.get('hub'):
        nbr = _edit_rows(nbr, ns, drop=ORPHAN if c.get('orphan') else None, first=HUB if c.get('hub') else None)
    # kernel points: the centre and 14 directions at 0.6 R (the layout of the shipped disposition); influence radius 0.5 R, so that most
    # (entry, kernel point) pairs have influence exactly 0 and a few do not
    v = rng.normal(0, 1, (KP, 3))
    kp = (0.6 * R * v / np.linalg.norm(v, axis=1, keepdims=True))
    kp[0] = 0
    kp = kp.astype(np.float32)
    extent = float(np.float32(0.5 * R))
    weights = rng.normal(0, (KP * Cin) ** -0.5, (KP, Cin, Cout)).astype(np.float32)
    # features: N(0, 1) around a per-row shift of +-0.5 (+-1 for one channel), so that row sums of both signs occur and none is within
    # rounding of 0 -- num counts the rows with a POSITIVE sum, and float32 and float64 must agree on that integer
    sign = np.where(rng.uniform(size=(ns, 1)) < 0.6, 1.0, -1.0)
    x = (rng.normal(0, 1, (ns, Cin)) * (0.3 if Cin == 1 else 1.0) + sign * (1.0 if Cin == 1 else 0.5)).astype(np.float32)
    rs, ra = x.astype(np.float64).sum(1), np.abs(x.astype(np.float64)).sum(1)
    assert np.all(np.abs(rs) >= 1e-3 * ra), f'{name}: a feature row sums to ~0; the neighbour count would depend on rounding'
    assert (rs > 0).any() and (rs < 0).any()
    d_out = rng.normal(0, 1, (nq, Cout)).astype(np.float32)
    c.update(q_pts=q_pts, s_pts=s_pts, nbr=nbr, kernel_points=kp, extent=extent, weights=weights, x=x, d_out=d_out)
    if c.get('hub'):
        assert np.all((nbr == HUB).sum(1) == 1)
    if c.get('orphan'):
        assert not (nbr == ORPHAN).any()
    if c.get('dead_rows'):
        assert (nbr == ns).all(1).sum() >= c['dead_rows']
    return c


def transpose_table(nbr, ns):
    """The neighbour table by support: -> (row_off (ns + 1,), entries) int32; support s's incoming entries q H + h (nbr[q, h] == s) are
    entries[row_off[s]:row_off[s + 1]], ascending; entries outside [0, ns) (shadows) are dropped."""
    flat = np.asarray(nbr).reshape(-1).astype(np.int64)
    e = np.nonzero((flat >= 0) & (flat < ns))[0]
    e = e[np.argsort(flat[e], kind='stable')]
    row_off = np.concatenate([[0], np.cumsum(np.bincount(flat[e], minlength=ns))])
    return row_off.astype(np.int32), e.astype(np.int32)


def influences(q_pts, s_pts, nbr, kp, extent):
    """(Nq, H, KP) float64."""
    sp = np.concatenate([np.asarray(s_pts, np.float64), np.full((1, 3), 1e6)])
    rel = sp[nbr] - np.asarray(q_pts, np.float64)[:, None, :]
    d = np.sqrt(((rel[:, :, None, :] - np.asarray(kp, np.float64)[None, None]) ** 2).sum(-1))
    return np.maximum(0.0, 1.0 - d / extent)


def run(q_pts, s_pts, nbr, x, weights, kp, extent, d_out, bounds=False):
    """Forward and backward in float64.  -> dict: 'out' (Nq, Cout), 'num' (Nq,), 'wf' (Nq, KP, Cin), 'dwf' (Nq, KP, Cin), 'dx' (Ns, Cin),
    'dw' (KP, Cin, Cout); bounds=True adds 'b_dwf', 'b_dx', 'b_dw': per-element bounds on |float32 kernels - float64| (module docstring
    of the constants)."""
    x, W, g_out = (np.asarray(a, np.float64) for a in (x, weights, d_out))
    nbr = np.asarray(nbr)
    ns, Cin = x.shape
    nq, H = nbr.shape
    real = (nbr >= 0) & (nbr < ns)
    idx = np.where(real, nbr, ns)
    w = influences(q_pts, s_pts, idx, kp, extent) * real[:, :, None]
    nx = np.concatenate([x, np.zeros((1, Cin))])[idx]                          # (Nq, H, Cin)
    wf = np.einsum('qhk,qhc->qkc', w, nx)
    num = np.maximum(1, (nx.sum(-1) > 0).sum(1)).astype(np.float64)
    out = np.einsum('qkc,kco->qo', wf, W) / num[:, None]
    g = g_out / num[:, None]
    dw = np.einsum('qkc,qo->kco', wf, g)
    dwf = np.einsum('qo,kco->qkc', g, W)
    dnx = np.einsum('qhk,qkc->qhc', w, dwf)
    dx = np.zeros((ns + 1, Cin))
    np.add.at(dx, idx, dnx)
    r = {'out': out, 'num': num, 'wf': wf, 'dwf': dwf, 'dx': dx[:ns], 'dw': dw}
    if not bounds:
        return r
    Cout = W.shape[2]
    a_nx = np.abs(nx)
    b_wf = (H + 1) * U * np.einsum('qhk,qhc->qkc', w, a_nx) + E_INFL * a_nx.sum(1)[:, None, :]
    r['b_dw'] = (nq + C_DW) * U * np.einsum('qkc,qo->kco', np.abs(wf), np.abs(g)) + np.einsum('qkc,qo->kco', b_wf, np.abs(g))
    b_dwf = (Cout + C_DWF) * U * np.einsum('qo,kco->qkc', np.abs(g), np.abs(W))
    r['b_dwf'] = b_dwf
    a_dnx = np.einsum('qhk,qkc->qhc', w, np.abs(dwf))
    e_dnx = (np.einsum('qhk,qkc->qhc', w, b_dwf) + E_INFL * np.abs(dwf).sum(1)[:, None, :]) * real[:, :, None]
    A, E = np.zeros((ns + 1, Cin)), np.zeros((ns + 1, Cin))
    np.add.at(A, idx, a_dnx)
    np.add.at(E, idx, e_dnx)
    deg = np.bincount(idx.reshape(-1), minlength=ns + 1)[:ns]
    r['b_dx'] = (KP * deg[:, None] + C_DX) * U * A[:ns] + E[:ns]
    return r


def gather_bwd(q_pts, s_pts, nbr, kp, extent, dwf, ns):
    """dx (ns, Cin) float64 of a given dwf (Nq, KP, Cin), with its bound for an exact dwf: the entry point alone."""
    nbr = np.asarray(nbr)
    dwf = np.asarray(dwf, np.float64)
    real = (nbr >= 0) & (nbr < ns)
    idx = np.where(real, nbr, ns)
    w = influences(q_pts, s_pts, idx, kp, extent) * real[:, :, None]
    Cin = dwf.shape[2]
    dx, A, E = (np.zeros((ns + 1, Cin)) for _ in range(3))
    np.add.at(dx, idx, np.einsum('qhk,qkc->qhc', w, dwf))
    np.add.at(A, idx, np.einsum('qhk,qkc->qhc', w, np.abs(dwf)))
    np.add.at(E, idx, E_INFL * np.abs(dwf).sum(1)[:, None, :] * real[:, :, None])
    deg = np.bincount(idx.reshape(-1), minlength=ns + 1)[:ns]
    return dx[:ns], (np.asarray(kp).shape[0] * deg[:, None] + C_DX) * U * A[:ns] + E[:ns]


def torch_forward(q_pts, s_pts, nbr, x, weights, kp, extent):
    """The same forward in stock torch ops (any dtype / device; nbr int64), materialising the (Nq, H, KP) influences and the (Nq, H, Cin)
    gathered features as the reference does: what autograd differentiates in the host test and what tools/kpconv_grad_bench.py times."""
    import torch
    sp = torch.cat([s_pts, torch.full_like(s_pts[:1], 1e6)])
    rel = sp[nbr] - q_pts[:, None, :]
    d2 = ((rel[:, :, None, :] - kp) ** 2).sum(-1)
    w = torch.clamp(1 - torch.sqrt(d2) / extent, min=0.0).transpose(1, 2)      # (Nq, KP, H)
    nx = torch.cat([x, torch.zeros_like(x[:1])])[nbr]                          # (Nq, H, Cin)
    wf = torch.matmul(w, nx)                                                   # (Nq, KP, Cin)
    out = torch.matmul(wf.permute(1, 0, 2), weights).sum(0)
    num = torch.gt(nx.sum(-1), 0.0).sum(-1)
    num = torch.max(num, torch.ones_like(num))
    return out / num.unsqueeze(1)
