"""Float64 restatements of InfoNCELossFull / CorrCriterion forward + backward (feature_loss.py:281-314, corr_loss.py:18-40) for
tests/test_gpu_loss_grads.py and tests/test_loss_grads_host.py, and the seeded inputs of the loss_grads_<case> goldens
(tools/make_golden_loss_grads.py draw_inputs, restated: the tools are not imported by the tests)."""
import numpy as np
import torch

F32 = np.float32
U = 2.0 ** -24


def dist_f32(a, p):
    """d_ij = sqrt_rn(((dx^2 + dy^2) + dz^2)) in float32, rounded per operation (the kernels' arithmetic)."""
    d = a[:, None, :].astype(F32) - p[None, :, :].astype(F32)
    sq = d * d
    return np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2]).astype(F32)


def transform_f32(T, x):
    T = T.astype(F32)
    return np.stack([((T[r, 0] * x[:, 0] + T[r, 1] * x[:, 1]) + T[r, 2] * x[:, 2]) + T[r, 3] for r in range(3)], 1).astype(F32)


def draw_inputs(n_src, n_tgt, D, seed):
    gen = torch.Generator().manual_seed(int(seed))
    src = [torch.randn((n, D), generator=gen) * 0.2 for n in n_src]
    tgt = [torch.randn((n, D), generator=gen) * 0.2 for n in n_tgt]
    W = torch.randn((D, D), generator=gen) * 0.1
    w = []
    for n in n_src:
        x = torch.rand(n, generator=gen)
        x[::3] = 0.0
        w.append(x)
    return src, tgt, W, w


def decisions(ax, px, r_p, r_n):
    """(idx (lowest j on ties), mask, allowed) in the kernels' float32 distance arithmetic."""
    d = dist_f32(ax, px)
    idx = np.argmin(d, axis=1)
    rows = np.arange(len(ax))
    mask = d[rows, idx] < F32(r_p)
    allowed = ~(d < F32(r_n))
    allowed[rows, idx] = True
    return idx, mask, allowed


def fold(dws):
    """dW of W from dW_sym (W_sym = triu(W) + triu(W)^T)."""
    return np.triu(dws + dws.T)


def infonce_grads(A, G, W, dec, g=1.0, bounds=False):
    """A / G lists of per-pair float arrays, W (D, D), dec per pair (idx, mask, allowed).  Float64: -> (loss, dA list, dG list, dW) and,
    with bounds=True, per-element error bounds of a float32 evaluation (exact-f32 products, float32 sums, U = 2^-24) of the same."""
    B = len(A)
    D = W.shape[0]
    W = W.astype(np.float64)
    Wt = np.triu(W)
    Ws = Wt + Wt.T
    aWs = np.abs(Ws)
    losses, dA, dG, bA, bG = [], [], [], [], []
    dWs = np.zeros((D, D))
    bWs = np.zeros((D, D))
    aG_all = []
    for b in range(B):
        a, gg = A[b].astype(np.float64), G[b].astype(np.float64)
        idx, mask, allowed = dec[b]
        P = gg @ Ws
        ePm = (D + 4) * U * (np.abs(gg) @ aWs)                        # |P' error| of the float32 GEMM
        l = a @ P.T
        lm = np.where(allowed, l, -np.inf)
        m = lm.max(1)
        lse = m + np.log(np.exp(lm - m[:, None]).sum(1))
        rows = np.arange(len(a))
        li = lse - l[rows, idx]
        cnt = mask.sum()
        losses.append(li[mask].sum() / cnt if cnt else np.nan)
        s = g / B / cnt if cnt else 0.0
        p = np.where(allowed, np.exp(lm - lse[:, None]), 0.0)
        dl = s * p
        dl[rows, idx] -= s
        dl[~mask] = 0.0
        dP = dl.T @ a
        dA.append(dl @ P)
        dG.append(dP @ Ws)
        dWs += gg.T @ dP
        if bounds:
            aA, aP, adl = np.abs(a), np.abs(P), np.abs(dl)
            el = (D + 8) * U * (aA @ aP.T) + aA @ ePm.T                    # logit error
            e_lse = np.where(allowed, el, 0).max(1) + 8 * U * (np.abs(lse) + np.log(allowed.sum(1) + 1.0))
            edl = np.where(mask[:, None], abs(s) * p * (el + e_lse[:, None] + 8 * U) + 4 * U * adl, 0.0)
            n_c, n_r = len(gg), len(a)
            bA.append(edl @ aP + adl @ ePm + (n_c + 8) * U * (adl @ aP))
            bP = edl.T @ aA + (n_r + 8) * U * (adl.T @ aA)
            bG.append(bP @ aWs + (D + 8) * U * (np.abs(dP) @ aWs))
            bWs += np.abs(gg).T @ bP + np.abs(gg).T @ np.abs(dP) * 8 * U
            aG_all.append(np.abs(gg).T @ np.abs(dP))
    loss = float(np.mean(losses))
    dW = np.triu(dWs + dWs.T)
    if not bounds:
        return loss, dA, dG, dW
    n_tot = sum(len(x) for x in G)
    aGdP = sum(aG_all)
    bW = np.triu(bWs + bWs.T + (n_tot + 8) * U * (aGdP + aGdP.T)) + 4 * U * np.abs(dW)
    return loss, dA, dG, dW, bA, bG, bW


def corr_grads(kp, warped, T, w, g=1.0):
    """CorrCriterion('mae') over the concatenated pairs in float64 on float32-rounded T kp: -> (loss, d warped list)."""
    e = [warped[b].astype(np.float64) - transform_f32(T[b], kp[b]).astype(np.float64) for b in range(len(kp))]
    ww = [x.astype(np.float64) for x in w]
    den = max(sum(x.sum() for x in ww), 1e-6)
    loss = sum((ww[b] * np.abs(e[b]).sum(1)).sum() for b in range(len(kp))) / den
    return loss, [g / den * ww[b][:, None] * np.sign(e[b]) for b in range(len(kp))]
