"""Float64 numpy restatement of the weighted Procrustes backward (csrc/procrustes.hip: k_procrustes_bwd), the zero-gradient rule, and
the float32 error bound the GPU test holds the kernel to.  Shared by tests/test_procrustes_grads_host.py and
tests/test_gpu_procrustes_grads.py; tests/golden/procrustes_grads.npz (tools/make_golden_procrustes_grads.py) holds the reference's
own float64 autograd on the same inputs.

Per (pair, layer), in the kernel's notation: a = [src_kp ; tgt_corr], b = [src_corr ; tgt_kp], w = sigmoid(logit), W = max(sum w, 1e-6),
wn = w / W, ca = sum wn a, cb = sum wn b, a' = a - ca, b' = b - cb, H = sum wn a' b'^T = U S V^T, d = sign det(V U^T),
R = V diag(1, 1, d) U^T, t = cb - R ca.  With G_R | g_t the upstream gradient of R | t:
    G = G_R - g_t ca^T,  dca = -R^T g_t,  dcb = g_t
    A = (G R^T - R G^T) / 2,  A' = V^T A V,  lam = (S0, S1, d S2)
    Y'_ij = -A'_ij / (lam_i + lam_j) (i != j; zero diagonal),  dH = 2 R^T V Y' V^T
    da_i = wn_i (dH b'_i + dca),  db_i = wn_i (dH^T a'_i + dcb)
    dwn_i = a'_i^T dH b'_i + a'_i . dca + b'_i . dcb     (a_i . dca + b_i . dcb less its constant ca . dca + cb . dcb = g_t . t, which the
                                                          next line's mean removes anyway: leaving it out from the start costs no cancellation)
    dw_i = (dwn_i - sum_j wn_j dwn_j) / W,  dlogit_i = dw_i w_i (1 - w_i)
roundings=True restates the float32 steps of the forward exactly as k_procrustes takes them (w, W, wn, the products under the float64
sums, the float32 centroids), so that the only float32 difference left between this file and the device is expf's last bit.

The zero-gradient rule (docs/PARITY.md): the pair's rows are exactly 0 when the pair is empty, when the weight sum hit the 1e-6 clamp,
or when min_{i<j} (lam_i + lam_j) <= 2^-23 lam_0 (R is not a differentiable function of float32 inputs there)."""
import numpy as np

U32 = 2.0 ** -23          # one float32 ulp, relative
EPS_W = np.float32(1e-6)  # se3_torch.py's _EPS


def pair_forward(a, b, logit=None, w=None, roundings=True, w_ulps=None):
    """a, b (n, 3), logit (n,) or w (n,) -> dict of the forward quantities of one pair in float64 (float32-rounded where the kernel
    rounds, with roundings=True)."""
    n = a.shape[0]
    if roundings:
        a32, b32 = a.astype(np.float32), b.astype(np.float32)
        if w is None:
            with np.errstate(over='ignore'):
                w32 = np.float32(1) / (np.float32(1) + np.exp(-logit.astype(np.float32)))
        else:
            w32 = w.astype(np.float32)
        if w_ulps is not None:       # each w_i moved by that many float32 ulps: what the device's expf may do (the bound's term 1)
            w32 = (w32.view(np.int32) + w_ulps.astype(np.int32)).view(np.float32)
        wsum = w32.astype(np.float64).sum()
        clamped = not (np.float32(wsum) > EPS_W)
        W32 = max(np.float32(wsum), EPS_W)
        wn32 = w32 / W32
        ca = np.float32((a32 * wn32[:, None]).astype(np.float64).sum(0)) if n else np.zeros(3, np.float32)
        cb = np.float32((b32 * wn32[:, None]).astype(np.float64).sum(0)) if n else np.zeros(3, np.float32)
        ca, cb = ca.astype(np.float32), cb.astype(np.float32)
        pa = a32 - ca
        pb = (b32 - cb) * wn32[:, None]
        H = (pa[:, :, None] * pb[:, None, :]).astype(np.float64).sum(0)      # float32 products under a float64 sum
        a, b, wv, W, wn = a32.astype(np.float64), b32.astype(np.float64), w32.astype(np.float64), float(W32), wn32.astype(np.float64)
        ca, cb = ca.astype(np.float64), cb.astype(np.float64)
    else:
        a, b = a.astype(np.float64), b.astype(np.float64)
        wv = 1.0 / (1.0 + np.exp(-logit.astype(np.float64))) if w is None else w.astype(np.float64)
        wsum = wv.sum()
        clamped = not (wsum > 1e-6)
        W = max(wsum, 1e-6)
        wn = wv / W
        ca, cb = (a * wn[:, None]).sum(0), (b * wn[:, None]).sum(0)
        H = ((a - ca)[:, :, None] * ((b - cb) * wn[:, None])[:, None, :]).sum(0)
    U, S, Vt = np.linalg.svd(H)
    V = Vt.T
    d = 1.0 if np.linalg.det(V @ U.T) > 0 else -1.0
    R = V @ np.diag([1.0, 1.0, d]) @ U.T
    lam = np.array([S[0], S[1], d * S[2]])
    return dict(a=a, b=b, w=wv, W=W, wn=wn, ca=ca, cb=cb, H=H, U=U, S=S, V=V, d=d, R=R, lam=lam, clamped=clamped, n=n)


def lam_sums(lam):
    return np.array([lam[0] + lam[1], lam[0] + lam[2], lam[1] + lam[2]])


def pair_backward(a, b, d_pose, logit=None, w=None, roundings=True, w_ulps=None):
    """One pair: d_pose (3, 4) -> (da (n, 3), db (n, 3), dlogit (n,), dw (n,), info).  info: kappa = lam_0 / min (lam_i + lam_j), d, S,
    zeroed (the zero-gradient rule applied)."""
    f = pair_forward(a, b, logit, w, roundings, w_ulps)
    n = f['n']
    lam = f['lam']
    sums = lam_sums(lam)
    zeroed = n == 0 or f['clamped'] or not (sums.min() > U32 * lam[0])
    info = dict(kappa=(lam[0] / sums.min() if sums.min() > 0 else np.inf), d=f['d'], S=f['S'], zeroed=zeroed, R=f['R'])
    if zeroed:
        return np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n), np.zeros(n), info
    GR, gt = d_pose[:, :3].astype(np.float64), d_pose[:, 3].astype(np.float64)
    R, V, ca, cb = f['R'], f['V'], f['ca'], f['cb']
    G = GR - np.outer(gt, ca)
    dca, dcb = -R.T @ gt, gt
    A = 0.5 * (G @ R.T - R @ G.T)
    Ap = V.T @ A @ V
    Y = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            if i != j:
                Y[i, j] = -Ap[i, j] / (lam[i] + lam[j])
    dH = 2.0 * R.T @ V @ Y @ V.T
    ap, bp = f['a'] - ca, f['b'] - cb
    wn = f['wn']
    da = wn[:, None] * (bp @ dH.T + dca)
    db = wn[:, None] * (ap @ dH + dcb)
    terms = np.stack([np.einsum('ir,rc,ic->i', ap, dH, bp), ap @ dca, bp @ dcb])
    dwn = terms.sum(0)
    info.update(w=f['w'], dw_terms=np.abs(terms).sum(0).max() / f['W'])
    dw = (dwn - (wn * dwn).sum()) / f['W']
    dlogit = dw * f['w'] * (1.0 - f['w'])
    return da, db, dlogit, dw, info


def model_backward(kp, corr, logit, seg_off, d_pose, roundings=True, w_ulps=None):
    """The operator's layout: kp (N, 3), corr (L, N, 3), logit (L, N), seg_off (2B + 1,), d_pose (L, B, 3, 4) ->
    dict(d_corr (L, N, 3), d_logit (L, N), d_kp (L, N, 3), d_weight (L, N)) float64, and info[l][b]."""
    Lyr, N = logit.shape
    B = (len(seg_off) - 1) // 2
    out = dict(d_corr=np.zeros((Lyr, N, 3)), d_logit=np.zeros((Lyr, N)), d_kp=np.zeros((Lyr, N, 3)), d_weight=np.zeros((Lyr, N)))
    infos = []
    for l in range(Lyr):
        infos.append([])
        for p in range(B):
            s, t = slice(seg_off[p], seg_off[p + 1]), slice(seg_off[B + p], seg_off[B + p + 1])
            ns = s.stop - s.start
            a = np.concatenate([kp[s], corr[l, t]])
            b = np.concatenate([corr[l, s], kp[t]])
            lg = np.concatenate([logit[l, s], logit[l, t]])
            ul = None if w_ulps is None else np.concatenate([w_ulps[l, s], w_ulps[l, t]])
            da, db, dl, dw, info = pair_backward(a, b, d_pose[l, p], logit=lg, roundings=roundings, w_ulps=ul)
            out['d_corr'][l, s], out['d_corr'][l, t] = db[:ns], da[ns:]
            out['d_kp'][l, s], out['d_kp'][l, t] = da[:ns], db[ns:]
            out['d_logit'][l, s], out['d_logit'][l, t] = dl[:ns], dl[ns:]
            out['d_weight'][l, s], out['d_weight'][l, t] = dw[:ns], dw[ns:]
            info['rows'] = (s, t)
            infos[-1].append(info)
    return out, infos


# ---------------------------------------------------------------------------------------------------------------- the float32 error bound
# What separates the device from pair_backward(roundings=True), to first order in u = 2^-23 (one float32 ulp, relative):
#   (1) w_i.  The device's expf may differ from numpy's in its last bit, and the roundings of 1 + e and 1 / (1 + e) may then fall the
#       other way: w_i moves by up to one ulp, |dw_i| <= u w_i.  Every later float32 step of the forward is restated exactly but reads
#       the moved w_i and may round the other way too: wn_i = w_i / W (another u), the float32 products under the float64 sums of ca, cb
#       and H (u each), the float32 centroids (u / 2 each).  So wn_i moves by <= 2u, a centred point a'_i = a_i - ca by <= 3u of the
#       cloud's extent (2u through wn in the centroid, u through its products and rounding), and H, a sum of wn_i a'_i b'_i^T, by
#       <= (2 + 3 + 3) u of sum wn_i |a'_i| |b'_i|.
#   (2) R, and the backward's dH.  Step 3 of the closed form IS the derivative of R with respect to H: a change of H turns R by at most
#       |dH| / min (lam_i + lam_j).  Relative to lam_0 that is the amplification kappa = lam_0 / min_{i<j} (lam_i + lam_j).  The
#       backward's dH = 2 R^T V Y' V^T is linear in R and of degree -1 in lam, so it moves by the rotation's change once more for each:
#       2 * 8u kappa relative to its size.
#   (3) The outputs are products of wn_i (2u), a centred point (3u), and dH (16u kappa) or dca = -R^T g_t (8u kappa); the centroid enters
#       G = G_R - g_t ca^T once more (3u).  Relative to the size of the pair's output:
#           rel = u (8 + 16 kappa)
#   (4) the final float32 rounding of each output, u / 2 of the entry, and the float64 fixed-tree sums, n 2^-53 of the largest term.
# "The size of the pair's output" is the pair's largest entry for d_corr and d_kp.  d_weight subtracts the weighted mean from dwn_i, and
# dwn_i is itself a sum of three terms: its size is T = max_i (|a'_i^T dH b'_i| + |a'_i . dca| + |b'_i . dcb|) / W, the terms before they
# cancel.  d_logit_i = dw_i w_i (1 - w_i) takes
# w_i (1 - w_i) of d_weight's bound, plus u |d_logit_i| for w_i (1 - w_i) itself.
# tests/test_procrustes_grads_host.py moves every w_i by an ulp in the restatement and finds the result inside this bound.
def rel_bound(n, kappa):
    return U32 * (8.0 + 16.0 * kappa) + 0.5 * U32 + n * 2.0 ** -53


def pair_bounds(ref, infos):
    """ref, infos = model_backward(...).  Per output an array like it: the absolute bound of every entry."""
    out = {k: np.zeros_like(v) for k, v in ref.items()}
    for l, row in enumerate(infos):
        for info in row:
            if info['zeroed']:
                continue
            s, t = info['rows']
            ns = s.stop - s.start
            rb = rel_bound(ns + (t.stop - t.start), info['kappa'])
            for k in ('d_corr', 'd_kp'):
                m = max(np.abs(ref[k][l, s]).max(initial=0.0), np.abs(ref[k][l, t]).max(initial=0.0))
                out[k][l, s] = out[k][l, t] = rb * m
            bw = rb * info['dw_terms']
            ww = info['w'] * (1.0 - info['w'])
            out['d_weight'][l, s] = out['d_weight'][l, t] = bw
            out['d_logit'][l, s] = ww[:ns] * bw + U32 * np.abs(ref['d_logit'][l, s])
            out['d_logit'][l, t] = ww[ns:] * bw + U32 * np.abs(ref['d_logit'][l, t])
    return out
