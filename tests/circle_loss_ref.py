"""Float64 restatement of CircleLossFull with dist_type 'euclidean' (feature_loss.py:160-243), forward and backward, in closed form,
for tests/test_circle_loss_host.py and tests/test_gpu_circle_loss.py; the seeded features of the circle_loss_<case> goldens
(tools/make_golden_circle_loss.py draw_features, restated: the tools are not imported by the tests); float32 error bounds.

Closed form per pair (s = log_scale; pm / po = pos_margin / pos_optimal, nm / no = neg_margin / neg_optimal):
    d_ij = sqrt(sum_c (a_ic - b_jc)^2 + 1e-12),   wp = max(d - po, 0) [pos],   wn = max(no - d, 0) [neg]   (0 where masked)
    tp = s (d - pm) wp,   tn = s (nm - d) wn          -- a masked entry is 0: it enters the log-sum-exp as exp(0) = 1
    row_i = softplus(LSE_j tp + LSE_j tn) / s,  selected when row i has a pos and a neg;  col_j the same over i
    pair = (mean_sel row + mean_sel col) / 2 (NaN for an empty selection);  loss = mean over pairs.
Backward (wp, wn detached): g_ij = (k_i Pp^r + k_j Pp^c) wp - (k_i Pn^r + k_j Pn^c) wn with P = exp(t - LSE) the softmax weights,
k_i = g / (2 B n_rows) softplus'(x_i) on selected rows; c = g_ij / d_ij; dA_i = (sum_j c_ij) a_i - sum_j c_ij b_j, dB_j likewise.
A pair with an empty selection contributes exactly zero gradient (the kernels' rule).
softplus is torch's: x itself above the threshold 20 (derivative 1), so that the float64 reference module is met to the last digits.

Error bounds of a float32 evaluation (U = 2^-24), every step a worst case:
    d:     the D-term fused sum of squares of rounded differences: |dd| <= (D / 2 + 6) U d
    tp/tn: two subtractions against a float32 margin (each dd + 2 U (d + |margin|)) and two products
    LSE:   the largest term error of the row + 8 U (|LSE| + log(n + 1))   (expf / logf within a few ulp, n float32 adds)
    P, k:  exp and sigmoid are 1- and 1/4-Lipschitz in their arguments' errors
    c:     the quotient rule on g / d
    dA:    sum_j dc_ij (|a_i| + |b_j|) + (n + 8) U sum_j |c_ij| (|a_i| + |b_j|): the two sums are formed separately, so close features do
           not cancel the rounding of their parts.
"""
import numpy as np
import torch

from tests.loss_grads_ref import dist_f32

F32 = np.float32
U = 2.0 ** -24
DEFAULTS = dict(log_scale=10.0, pos_margin=0.1, pos_optimal=0.1, neg_margin=1.4, neg_optimal=1.4)


def draw_features(n_src, n_tgt, D, seed, anc_xyz, tgt_xyz):
    """Unit directions scaled by s / sqrt(2), s ~ U(0.3, 1.3) (feature distances 0.3 .. 1.3 about both margins), src clouds then tgt
    clouds; then six anchors per pair are copied onto their nearest positive (by coordinates) with 1e-3 noise: positives under
    pos_margin.  float32 tensors from torch's CPU generator."""
    gen = torch.Generator().manual_seed(int(seed))

    def cloud(n):
        v = torch.randn((n, D), generator=gen)
        v = v / v.norm(dim=1, keepdim=True)
        s = torch.rand(n, generator=gen) * 1.0 + 0.3
        return v * (s / np.sqrt(2.0)).unsqueeze(1).float()
    src = [cloud(n) for n in n_src]
    tgt = [cloud(n) for n in n_tgt]
    for b, n in enumerate(n_src):
        idx = np.arange(0, n, max(n // 6, 1))[:6]
        cd = np.linalg.norm(anc_xyz[b][idx].astype(np.float64)[:, None] - tgt_xyz[b].astype(np.float64)[None], axis=-1)
        near = cd.argmin(1)
        noise = torch.randn((len(idx), D), generator=gen) * 1e-3
        src[b][torch.from_numpy(idx)] = tgt[b][torch.from_numpy(near)] + noise
    return src, tgt


def masks(ax, px, r_p, r_n):
    """(pos, neg) in the kernels' float32 coordinate arithmetic, both strict."""
    d = dist_f32(ax, px)
    return d < F32(r_p), d > F32(r_n)


def _lse(t, axis):
    m = t.max(axis)
    return m + np.log(np.exp(t - np.expand_dims(m, axis)).sum(axis))


def _softplus(x):
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def _dsoftplus(x):
    return np.where(x > 20.0, 1.0, 1.0 / (1.0 + np.exp(-x)))


def circle(A, G, msk, params=None, g=1.0, bounds=False):
    """A / G: lists of per-pair float arrays, msk: per pair (pos, neg).  Float64 -> (loss, per-pair losses, dA list, dG list, counts
    [(n_rows, n_cols)]) and, with bounds=True, also (per-pair loss bounds, bA list, bG list)."""
    p = dict(DEFAULTS, **(params or {}))
    s, pm, po, nm, no = (float(p[k]) for k in ('log_scale', 'pos_margin', 'pos_optimal', 'neg_margin', 'neg_optimal'))
    B = len(A)
    per, dA, dG, cnt, bA, bG, bper = [], [], [], [], [], [], []
    for b in range(B):
        a, gg = A[b].astype(np.float64), G[b].astype(np.float64)
        pos, neg = msk[b]
        n_r, n_c = len(a), len(gg)
        D = a.shape[1]
        d = np.sqrt(((a[:, None, :] - gg[None, :, :]) ** 2).sum(-1) + 1e-12)
        wp = np.where(pos, np.maximum(d - po, 0.0), 0.0)
        wn = np.where(neg, np.maximum(no - d, 0.0), 0.0)
        tp, tn = s * (d - pm) * wp, s * (nm - d) * wn
        lp_r, ln_r, lp_c, ln_c = _lse(tp, 1), _lse(tn, 1), _lse(tp, 0), _lse(tn, 0)
        x_r, x_c = lp_r + ln_r, lp_c + ln_c
        row, col = _softplus(x_r) / s, _softplus(x_c) / s
        sel_r = pos.any(1) & neg.any(1)
        sel_c = pos.any(0) & neg.any(0)
        nr, nc = int(sel_r.sum()), int(sel_c.sum())
        cnt.append((nr, nc))
        live = nr > 0 and nc > 0
        per.append((row[sel_r].mean() + col[sel_c].mean()) / 2 if live else np.nan)
        if live:
            k_r = np.where(sel_r, g / (2 * B * nr) * _dsoftplus(x_r), 0.0)
            k_c = np.where(sel_c, g / (2 * B * nc) * _dsoftplus(x_c), 0.0)
        else:
            k_r, k_c = np.zeros(n_r), np.zeros(n_c)
        Pp_r, Pn_r = np.exp(tp - lp_r[:, None]), np.exp(tn - ln_r[:, None])
        Pp_c, Pn_c = np.exp(tp - lp_c[None, :]), np.exp(tn - ln_c[None, :])
        gp = k_r[:, None] * Pp_r + k_c[None, :] * Pp_c
        gn = k_r[:, None] * Pn_r + k_c[None, :] * Pn_c
        c = (gp * wp - gn * wn) / d
        dA.append(c.sum(1)[:, None] * a - c @ gg)
        dG.append(c.sum(0)[:, None] * gg - c.T @ a)
        if not bounds:
            continue
        ed = (D / 2 + 6) * U * d
        e_p = ed + 2 * U * (d + abs(pm) + abs(po))                                   # error of d - margin (a float32 margin)
        e_n = ed + 2 * U * (d + abs(nm) + abs(no))
        etp = np.where(pos, s * (np.abs(d - pm) + wp) * e_p, 0.0) + 4 * U * np.abs(tp)
        etn = np.where(neg, s * (np.abs(nm - d) + wn) * e_n, 0.0) + 4 * U * np.abs(tn)
        ewp, ewn = np.where(pos, e_p, 0.0), np.where(neg, e_n, 0.0)

        def e_lse(et, lse, axis, n):
            return et.max(axis) + 8 * U * (np.abs(lse) + np.log(n + 1.0))
        elp_r, eln_r = e_lse(etp, lp_r, 1, n_c), e_lse(etn, ln_r, 1, n_c)
        elp_c, eln_c = e_lse(etp, lp_c, 0, n_r), e_lse(etn, ln_c, 0, n_r)
        e_row = (elp_r + eln_r + 4 * U * np.abs(x_r)) / s + 6 * U * row
        e_col = (elp_c + eln_c + 4 * U * np.abs(x_c)) / s + 6 * U * col
        bper.append((e_row[sel_r].mean() + e_col[sel_c].mean()) / 2 + 8 * U * abs(per[-1]) if live else 0.0)
        ek_r = np.where(sel_r, np.abs(g) / (2 * B * max(nr, 1)) * 0.25 * (elp_r + eln_r + 4 * U * np.abs(x_r)), 0.0) + 8 * U * np.abs(k_r)
        ek_c = np.where(sel_c, np.abs(g) / (2 * B * max(nc, 1)) * 0.25 * (elp_c + eln_c + 4 * U * np.abs(x_c)), 0.0) + 8 * U * np.abs(k_c)
        rel = lambda et, el, P: np.expm1(et + el + 4 * U * (1.0 - np.log(np.maximum(P, 1e-300))))      # relative error of P = exp(t - LSE)
        eg = (ek_r[:, None] * Pp_r + np.abs(k_r)[:, None] * Pp_r * rel(etp, elp_r[:, None], Pp_r) +
              ek_c[None, :] * Pp_c + np.abs(k_c)[None, :] * Pp_c * rel(etp, elp_c[None, :], Pp_c)) * wp + np.abs(gp) * ewp + \
             (ek_r[:, None] * Pn_r + np.abs(k_r)[:, None] * Pn_r * rel(etn, eln_r[:, None], Pn_r) +
              ek_c[None, :] * Pn_c + np.abs(k_c)[None, :] * Pn_c * rel(etn, eln_c[None, :], Pn_c)) * wn + np.abs(gn) * ewn + \
             8 * U * (np.abs(gp) * wp + np.abs(gn) * wn)
        ac = np.abs(c)
        ec = eg / d + ac * ed / d + 4 * U * ac
        aA, aG = np.abs(a), np.abs(gg)
        bA.append(ec.sum(1)[:, None] * aA + ec @ aG + (n_c + 8) * U * (ac.sum(1)[:, None] * aA + ac @ aG))
        bG.append(ec.sum(0)[:, None] * aG + ec.T @ aA + (n_r + 8) * U * (ac.sum(0)[:, None] * aG + ac.T @ aA))
    loss = float(np.mean(per))
    if not bounds:
        return loss, per, dA, dG, cnt
    return loss, per, dA, dG, cnt, bper, bA, bG
